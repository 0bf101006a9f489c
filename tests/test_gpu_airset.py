"""GPU: the AIR-set proof (docs/airset.md) -- the device prover's words equal the independent model's (tests/airset_model.py) on the
CPU test's shapes and on the smallest shapes that reach each device path (the GKR in one kernel and with streamed layers, the joint
pass's first rounds and last fold, the rotation reduction's tail in both forms); the root equals Context.stack_commit's; (P, Q) and
every B_a equal what the leaves built from the traces give; the host verifier accepts a device proof of twelve ChipSet chips of mixed
heights and refuses device proofs over tampered traces; runs are deterministic; the other provers' bytes do not change."""
import numpy as np
import pytest

import airset_model as am
import gkr_model as gm
import whir_model as wm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_airset_cpu import _air, _bus_mix, _fib, _lookup, _set
from test_gpu_gkr import _cases, np_mle
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _upload(zk, traces):
    return [zk.upload(np.asarray(t, dtype=np.uint32).reshape(-1)) for t in traces]


def _split(items):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]


def _against_model(zk, prm, airs, traces, pvs, l, prefix):
    root, proof = zk.airset_prove(_lp(prm), airs, _upload(zk, traces), pvs, l, prefix)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words, info = am.prove(ch, prm, airs, traces, pvs, l)
    assert root.tolist() == mroot and len(proof) == len(words) == z.airset_proof_words(_lp(prm), airs, l)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    lroot, pq = z.airset_verify(_lp(prm), prefix, airs, pvs, l, proof)
    assert lroot.tolist() == mroot and pq.tolist()[:4] == [0, 0, 0, 0]
    return info


@pytest.mark.parametrize("name", ["lookup", "limb", "bus_mix", "fib+lookup", "mixed"])
def test_cpu_shapes_words_equal_model(zk, name):
    airs, traces, pvs, l = _set(name)
    _against_model(zk, _params(1, 2, 1), airs, traces, pvs, l, [7, 1])


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_joint_pass_first_rounds_and_last_fold(zk, m):
    """m = 1: round 0 and the last fold both from the base trace; m = 2, 3, 4: the streaming pass 1, 2 and 3 rounds deep.  L = m + 3."""
    airs, traces, pvs = _split([_bus_mix(m)])
    info = _against_model(zk, _params(1, 1, 0), airs, traces, pvs, min(m + 1, 4), [m])
    assert info["L"] == m + 3


@pytest.mark.parametrize("case,L", [("lookup", 11), ("bus_mix", 12)])
def test_streamed_gkr_layers(zk, case, L):
    """L = 11 and 12: the GKR's layers above 2^10 entries stream (L <= 10, the single kernel: every other test here)"""
    items = _lookup(10, 6) if case == "lookup" else [_bus_mix(9)]
    airs, traces, pvs = _split(items)
    info = _against_model(zk, _params(1, 4, 2), airs, traces, pvs, 9, [L])
    assert info["L"] == L


@pytest.mark.parametrize("m", [9, 11])
def test_rotation_tail_beside_a_lookup(zk, m):
    """Fibonacci (the constraint part only) beside a lookup pair: the reduction's tail from F_a, F_b, eq (m = 9) and from folded tables (11)"""
    airs, traces, pvs = _split([_fib(m)] + _lookup(3, 2))
    _against_model(zk, _params(1, 4, 2), airs, traces, pvs, 9, [m])


def _np_mle_ext(vals, point):
    return np_mle(np.asarray(vals, dtype=np.int64), point)


def test_root_leaves_and_leaf_claims(zk):
    """the root is stack_commit's; (P, Q) is the fraction sum of the leaves built from the traces in the sorted layout; rho is the
    point the GKR words lead to; every B_a is the MLE of its leaf blocks at rho's prefix"""
    airs, traces, pvs, l = _set("mixed")
    prm, prefix = _params(1, 2, 1), [5]
    root, proof = zk.airset_prove(_lp(prm), airs, _upload(zk, traces), pvs, l, prefix)
    cols = [zk.upload(np.asarray(c, dtype=np.uint32)) for t in traces for c in t]
    assert zk.stack_commit(_lp(prm), cols, l).root.tolist() == root.tolist() == proof[:8].tolist()
    plans = [am.Plan(a) for a in airs]
    blocks, T, L = am.layout(plans)
    ch = Challenger()
    ch.observe(prefix)
    ch.observe(proof[:8].tolist())
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    gamma, beta = gm.bus_challenges(ch)
    num, den = am.leaves(plans, blocks, L, traces, pvs, gamma, beta)
    top = gm.build_layers(num, den)[0]
    g = gm.proof_words(L)
    assert proof[8:16].tolist() == top[0][0] + top[1][0] and top[0][0] == am.ZERO
    rho, (ps, qs), _ = gm.verify(ch, proof[8:8 + g].tolist(), L)
    n4 = np.zeros((1 << L, 4), dtype=np.int64)
    n4[:, 0] = num
    assert _np_mle_ext(n4, rho) == ps and _np_mle_ext(den, rho) == qs
    kappa = ch.sample_ext()
    eb = am.block_eq(blocks, rho)
    with_ints = [a for a, p in enumerate(plans) if p.ints]
    for i, a in enumerate(with_ints):
        want = am.ZERO
        for (a2, j, m, off), e in zip(blocks, eb):
            if a2 == a:
                n_, d_ = _np_mle_ext(n4[off:off + (1 << m)], rho[:m]), _np_mle_ext(den[off:off + (1 << m)], rho[:m])
                want = am.ext_add(want, am.ext_mul(e, am.ext_add(n_, am.ext_mul(kappa, d_))))
        assert proof[8 + g + 4 * i:8 + g + 4 * i + 4].tolist() == want


def _chipset():
    """twelve ChipSet chips of mixed heights up to 2^14 rows and, in place of the set's preprocessed range table, a two-row table with
    its keys in a main column"""
    chips = air.ChipSet(n_chips=12, log_max=14, log_min=4, total_width=120, seed=2).gen(seed=2)[:-1]
    counts = sum(np.bincount(c["trace"][1].astype(np.int64), minlength=2)[:2] for c in chips)
    tb = air.AirBuilder(2, 0)
    tb.push_interaction(air.ChipSet.RANGE_BUS, [tb.var(0)], tb.var(1), "receive")
    table = dict(_air(tb, 1), trace=np.array([[0, 1], counts % P], dtype=np.uint32), pvs=np.zeros(0, np.uint32))
    return chips[:5] + [table] + chips[5:]


def test_host_verifier_accepts_a_chipset_device_proof(zk):
    airs = _chipset()
    assert len({a["log_height"] for a in airs}) >= 5 and max(a["log_height"] for a in airs) == 14
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    l, prefix = 17, [4, 2]
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    pvs = [a["pvs"] for a in airs]
    root, proof = zk.airset_prove(prm, vairs, _upload(zk, [a["trace"] for a in airs]), pvs, l, prefix)
    lroot, pq = z.airset_verify(prm, prefix, vairs, pvs, l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0] and pq.tolist()[4:] != [0, 0, 0, 0]
    bad = proof.copy()
    bad[len(bad) // 5] = (int(bad[len(bad) // 5]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.airset_verify(prm, prefix, vairs, pvs, l, bad)


def test_device_proofs_over_tampered_traces_are_refused(zk):
    prm = _lp(_params(1, 2, 1))
    airs, traces, pvs, l = _set("lookup")
    z.airset_verify(prm, [1], airs, pvs, l, zk.airset_prove(prm, airs, _upload(zk, traces), pvs, l, [1])[1])
    traces[1][2][1] = (traces[1][2][1] + 1) % P   # one multiplicity: P != 0
    proof = zk.airset_prove(prm, airs, _upload(zk, traces), pvs, l, [1])[1]
    assert proof[8:12].tolist() != [0, 0, 0, 0]
    with pytest.raises(z.ZkhipError):
        z.airset_verify(prm, [1], airs, pvs, l, proof)
    airs, traces, pvs, l = _set("bus_mix")
    traces[0][2][1] = (traces[0][2][1] + 1) % P   # the buses still balance, constraint 0 fails
    proof = zk.airset_prove(prm, airs, _upload(zk, traces), pvs, l, [2])[1]
    assert proof[8:12].tolist() == [0, 0, 0, 0]
    with pytest.raises(z.ZkhipError):
        z.airset_verify(prm, [2], airs, pvs, l, proof)


def test_two_runs_give_identical_words(zk):
    airs, traces, pvs, l = _set("mixed")
    prm = _lp(_params(1, 2, 1))
    d = _upload(zk, traces)
    x = zk.airset_prove(prm, airs, d, pvs, l, [1])
    y = zk.airset_prove(prm, airs, d, pvs, l, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_interleaved_airset_leaves_the_other_provers_unchanged(zk):
    airs = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    prm = _lp(_params(2, 2, 2, pow_bits=4, nq=8))
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]

    def others():
        zc = zk.zerocheck_prove(prm, vairs, d_traces, pvs, 8, [2])
        return pk.prove(d_traces, pvs), zc[0].tolist(), zc[1].tolist(), pk.bus_gkr_prove(d_traces, pvs, [3]).tolist()

    before = others()
    root, proof = zk.airset_prove(prm, vairs, d_traces, pvs, 8, [2])
    assert others() == before
    z.airset_verify(prm, [2], vairs, pvs, 8, proof)
    assert z.verify(params, airs, pvs, before[0]) == 0
