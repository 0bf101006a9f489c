"""CPU: the operand-family sets of tests/zb_family_sets.py through the independent models of the batched AIR-set forms and the
library's host verifiers (docs/boundary_tests.md, "The batched AIR-set forms: operand families").  For every set and family the model
proves; its verifier accepts exactly when every trace passes air.check_trace and, with the bus part, the buses balance (an unbalanced
bus is never accepted); zkhip_airbatch_verify / zkhip_airkey_batch_verify / zkhip_airkey_cached_verify agree with it on the model's
words.  No family is skipped for a zero denominator under the committed seed.  The coverage the sets were built for is asserted: the
degrees and heights of mixed_nobus, a job whose s_a(0) equals its running claim (s_a(1) = 0 from equal operands), a used-up AIR whose
constant is not zero (the halving is invisible on a zero)."""
import pytest

import zb_family_sets as zf
from pymodel import P
from test_airset_cpu import PARAM_SETS, _lp

ERR_VERIFY = -7
SET_CASES = [(name, wb) for name in zf.SETS for wb in zf.fset(name)["with_bus"]]


def _host_verify(name, wb, i, res):
    """the library's host verifier on the model's words: (accepted, root)"""
    import zkvm_prover_amd as z

    S = zf.fset(name)
    prm = _lp(PARAM_SETS[zf.prm_index(name, wb, i)])
    pvs, prefix, words = S["fams"][i][3], zf.prefix_of(name, wb, i), res["words"]
    try:
        if S["form"] == "airbatch":
            out = z.airbatch_verify(prm, prefix, S["airs"], pvs, S["l"], words, wb)
            out = out[0] if wb else out
        elif S["form"] == "keyed":
            out = z.airkey_batch_verify(prm, prefix, S["airs"], res["key_root"], S["lpr"], pvs, S["l"], words, wb)
            out = out[0] if wb else out
        else:
            out = z.airkey_cached_verify(prm, prefix, S["airs"], res["key_root"], S["lpr"], S["lsc"], pvs, S["l"], words, wb)
            assert out[-1].tolist() == res["cached_roots"]
            out = out[0]
    except z.ZkhipError as e:
        assert e.code == ERR_VERIFY, e
        return False, None
    return True, out.tolist()


@pytest.mark.parametrize("name,wb", SET_CASES)
def test_models_and_host_verifiers_on_every_family(name, wb):
    S = zf.fset(name)
    skipped, accepted, eq_claim, const_nonzero = [], 0, [], []
    plans, act, M, D, red, M2 = zf.plans_of(name, wb)
    for i, (fam, traces, preps, pvs) in enumerate(S["fams"]):
        res = zf.model(name, wb, i)
        if res is None:
            skipped.append(fam)
            continue
        want = zf.satisfied(name, i) and res["balanced"]
        assert res["accepted"] == want, fam
        assert not (res["accepted"] and not res["balanced"]), fam
        ok, root = _host_verify(name, wb, i, res)
        assert ok == res["accepted"], fam
        assert root is None or root == res["root"], fam
        accepted += ok
        info = res["info"]
        # s_a(0) + s_a(1) is the running claim: s_a(1) = 0 says s_a(0) equals it
        if any(sa[1] == [0, 0, 0, 0] for sa in info["sa"].values()):
            eq_claim.append(fam)
        if any(info["g_end"][a] != [0, 0, 0, 0] for a in act if plans[a].m < M):
            const_nonzero.append(fam)
    assert skipped == [], "zero denominators under the committed seed: %s" % skipped
    assert accepted >= 1 and accepted < len(S["fams"])   # the honest traces are taken, the others (bar a satisfying constant) are not
    assert eq_claim, "no family makes a job's s_a(0) equal its running claim"
    assert const_nonzero, "no family leaves a used-up AIR a non-zero constant"
    print("%s with_bus=%d: accepted %d of %d; s_a(0) = claim in %d families, non-zero used-up constant in %d"
          % (name, wb, accepted, len(S["fams"]), len(eq_claim), len(const_nonzero)))


def test_mixed_nobus_degrees_and_heights():
    """the shape the extension, the weights and the halved constants need: at least three distinct D_a with D - min D_a >= 2, an AIR at
    m = 1 (it runs out after round 0), AIRs running out in three later rounds, a reduction over several heights and one AIR outside it"""
    plans, act, M, D, red, M2 = zf.plans_of("mixed_nobus", False)
    ds, ms = [plans[a].D for a in act], [plans[a].m for a in act]
    assert len(act) == 5 and len(set(ds)) >= 3 and D - min(ds) >= 2 and D == max(ds)
    assert M == 5 and min(ms) == 1 and len(set(ms)) >= 4 and ms != sorted(ms)
    assert M2 == 5 and 0 < len(red) < len(act) and len({plans[a].m for a in red}) >= 3


def test_mixed_bus_keyed_and_cached_shapes():
    plans, act, M, D, red, M2 = zf.plans_of("mixed_bus", True)
    assert sorted(p.m for p in plans) == [1, 2, 3, 4, 5] and all(p.ints for p in plans)
    for name in ("keyed", "cached"):
        plans, act, M, D, red, M2 = zf.plans_of(name, True)
        classes = {(p.D, bool(p.wp)) for p in plans}
        assert any((d, True) in classes and (d, False) in classes for d, _ in classes)     # PREP and non-PREP classes of one degree
        assert any(w and not w2 and d != d2 for d, w in classes for d2, w2 in classes)   # and of different degrees
        assert {p.m for p in plans} == {1, 2, 3, 4, 5} and M == M2 == 5
        assert any(p.rot_p for p in plans) and any(p.rot for p in plans)
    S = zf.fset("cached")
    assert sorted(S["airs"][a]["log_height"] for a, c in enumerate(S["lsc"]) if c is not None) == [1, 5]


def test_every_case_holds_raw_p_minus_1_cells():
    """the families reach the device as Montgomery words: the constant, alternating and one-hot families hold the word p - 1"""
    from boundary_inputs import raw_words

    v = int(raw_words([P - 1])[0])
    for name in zf.SETS:
        fams = dict((f[0], f) for f in zf.fset(name)["fams"])
        for fam in ("const raw 0x%08x" % (P - 1), "alternate raw p-1/0 period 2", "delta at 0"):
            assert all((t == v).any() for t in fams[fam][1]), (name, fam)
    for name in ("keyed", "cached"):
        f = dict((f[0], f) for f in zf.fset(name)["fams"])["prep const raw 0x%08x" % (P - 1)]
        assert all((p == v).all() for p in f[2] if p is not None)
