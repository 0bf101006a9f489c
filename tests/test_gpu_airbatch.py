"""GPU: the batched AIR-set proof (docs/airbatch.md) -- the device prover's words equal the independent model's
(tests/airbatch_model.py) on the CPU test's shapes and on the smallest shapes that reach each device path (an AIR whose round 0 and
last fold are both from the base trace beside AIRs that stream on, AIRs running out in consecutive rounds, a job boundary inside the
job search, two degree classes with and without bus parts in one round, D = 1 beside D = 8, 64 jobs, a reduction with M' != M, the
second iteration of the grid-stride loops, boundary operands); the root, v, v' and u against numpy; a ChipSet proof; tampered traces;
determinism; the per-AIR provers' words before and after; the launch count against the document's formula."""
import numpy as np
import pytest

import airbatch_model as bm
import airset_model as am
import zc_edge_shapes as es
import zerocheck_model as zm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_airbatch_cpu import ALL_SETS, _deg1, bset
from test_airset_cpu import _air, _bus_mix, _fib, _limb, _lookup
from test_gpu_airset import _chipset, _lp, _params, _split, _upload
from test_gpu_zerocheck import _np_mle_base
from test_zerocheck_cpu import _synth
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P
PRM = _params(1, 2, 1)


def _against_model(zk, prm, airs, traces, pvs, l, prefix, with_bus=True):
    root, proof = zk.airbatch_prove(_lp(prm), airs, _upload(zk, traces), pvs, l, prefix, with_bus)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words, info = bm.prove(ch, prm, airs, [np.asarray(t).tolist() for t in traces], pvs, l, with_bus)
    assert root.tolist() == mroot and len(proof) == len(words) == z.airbatch_proof_words(_lp(prm), airs, l, with_bus)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    out = z.airbatch_verify(_lp(prm), prefix, airs, pvs, l, proof, with_bus)
    assert (out[0] if with_bus else out).tolist() == mroot
    return info


@pytest.mark.parametrize("with_bus", [True, False])
@pytest.mark.parametrize("name", ALL_SETS)
def test_cpu_shapes_words_equal_model(zk, name, with_bus):
    airs, traces, pvs, l = bset(name)
    _against_model(zk, PRM, airs, traces, pvs, l, [7, 1], with_bus)


@pytest.mark.parametrize("heights", [(1, 2, 3), (1, 4), (2, 2), (3, 1, 2)])
def test_airs_running_out_in_consecutive_rounds(zk, heights):
    """m = 1: round 0 and the last fold both from the base trace, beside AIRs that stream on"""
    items = [_bus_mix(m) for m in heights]
    airs, traces, pvs = _split(items)
    _against_model(zk, _params(1, 1, 0), airs, traces, pvs, 4, list(heights))
    items = [_fib(m) for m in heights]
    airs, traces, pvs = _split(items)
    _against_model(zk, _params(1, 1, 0), airs, traces, pvs, 4, list(heights), with_bus=False)


@pytest.mark.parametrize("order", [(8, 2), (2, 8)])
def test_job_search_at_a_job_boundary(zk, order):
    """m = 8: 128 pairs, two workgroups; m = 2: one pair: the job search meets a boundary after two workgroups and after one"""
    airs, traces, pvs = _split([_bus_mix(m) for m in order])
    _against_model(zk, _params(1, 2, 1), airs, traces, pvs, 8, list(order))


@pytest.mark.parametrize("with_bus", [True, False])
def test_two_degree_classes_in_one_round(zk, with_bus):
    """Fibonacci (D = 3) and SyntheticAir at degree 5 (D = 6), with bus_mix and a lookup pair: with the bus part four classes"""
    items = [_fib(3), _synth(2, 5), _bus_mix(3)] + _lookup(2, 2) + [_synth(4, 5, seed=2)]
    airs, traces, pvs = _split(items)
    _against_model(zk, PRM, airs, traces, pvs, 5, [5], with_bus)


def test_degree_1_beside_degree_8(zk):
    d0, p7 = es.deg0(3), es.prod(7, 2)
    airs, traces, pvs = _split([d0, p7, es.deg0(1), es.prod(7, 3)])
    _against_model(zk, PRM, airs, [np.asarray(t) for t in traces], pvs, 4, [18], with_bus=False)


def test_64_airs(zk):
    kinds = [lambda: _fib(2), lambda: _bus_mix(2), lambda: _limb(2), lambda: _deg1(2)]
    items = [kinds[i % 4]() for i in range(64)]
    airs, traces, pvs = _split(items)
    _against_model(zk, _params(1, 1, 0), airs, traces, pvs, 6, [64])


@pytest.mark.parametrize("ms", [(9, 11), (11, 9)])
def test_batched_reduction_with_other_heights(zk, ms):
    """Fibonacci at m = 9 and 11 beside a lookup pair (sender 2^12: M = 12 != M' = 11) and a non-reducing AIR between them"""
    look = _lookup(12, 3)
    items = [_fib(ms[0]), look[0], _deg1(10), _fib(ms[1]), look[1]]
    airs, traces, pvs = _split(items)
    _against_model(zk, _params(1, 4, 2), airs, traces, pvs, 12, list(ms))


@pytest.mark.parametrize("kind", ["raw p-1", "canonical p-1", "zero"])
def test_boundary_count_columns(zk, kind):
    """two bus_mix AIRs (m = 3 and 1) whose count columns are at raw p - 1, canonical p - 1 and zero"""
    fams3 = {f[0]: f[1][0] for f in es.as_family_case("bus_mix", 3)[2]}
    fams1 = {f[0]: f[1][0] for f in es.as_family_case("bus_mix", 1)[2]}
    a3, a1 = _bus_mix(3)[0], _bus_mix(1)[0]
    traces = [fams3["count " + kind], fams1["count " + kind]]
    pvs = [[es.PV_POOL[1]], [es.PV_POOL[3]]]
    ch = Challenger()
    ch.observe([3])
    try:
        mroot, words, _ = bm.prove(ch, PRM, [a3, a1], [t.tolist() for t in traces], pvs, 4, leaf_hook=es.no_zero_den)
    except es.ZeroDenominator:
        pytest.fail("a zero denominator under the committed seed")
    root, proof = zk.airbatch_prove(_lp(PRM), [a3, a1], _upload(zk, traces), pvs, 4, [3])
    assert root.tolist() == mroot
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))


def _replay(prm, prefix, airs, pvs, l, proof, with_bus, keyed=None):
    """(plans, r, r', offsets) by replaying the transcript up to the points with the model's challenger.  keyed = (the key's root,
    log_stack_prep): the keyed batched form, whose transcript takes the key's root first and whose values are [v | v' | v_p | v_p']"""
    import gkr_model as gm

    ch = Challenger()
    ch.observe(prefix)
    if keyed:
        import keyed_batch_model as kb

        S = kb.Shape(prm, airs, l, keyed[1], with_bus)
        plans, L = S.plans, S.L
        act, M, D, red, M2 = kb.dims(plans)
        n_val = lambda a: plans[a].n_val
        ch.observe([int(x) for x in keyed[0]])
    else:
        plans, _, _, blocks, L = bm.shape(prm, airs, l, with_bus)
        act, M, D, red, M2 = bm.dims(plans)
        n_val = lambda a: plans[a].w + len(plans[a].rot)
    ch.observe(proof[:8].tolist())
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    q = 8
    if with_bus:
        gm.bus_challenges(ch)
        g = gm.proof_words(L)
        gm.verify(ch, proof[8:8 + g].tolist(), L)
        ch.sample_ext()
        nb = 4 * sum(1 for p in plans if p.ints)
        ch.observe(proof[8 + g:8 + g + nb].tolist())
        q = 8 + g + nb
    if any(plans[a].proven for a in act):
        [ch.sample_ext() for _ in range(M + 1)]
    ch.sample_ext()
    r, rp = [], []
    for _ in range(M):
        ch.observe(proof[q:q + 4 * D].tolist())
        r.append(ch.sample_ext())
        q += 4 * D
    o_vals = q
    nv = sum(4 * n_val(a) for a in act)
    ch.observe(proof[q:q + nv].tolist())
    q += nv
    if red:
        ch.sample_ext()
        for _ in range(M2):
            ch.observe(proof[q:q + 8].tolist())
            rp.append(ch.sample_ext())
            q += 8
    return plans, act, red, r, rp, o_vals, q


def test_root_and_values_against_numpy(zk):
    airs, traces, pvs, l = bset("heights")
    prm, prefix = PRM, [5]
    d = _upload(zk, traces)
    root, proof = zk.airbatch_prove(_lp(prm), airs, d, pvs, l, prefix)
    cols = [zk.upload(np.asarray(c, dtype=np.uint32)) for t in traces for c in t]
    assert zk.stack_commit(_lp(prm), cols, l).root.tolist() == root.tolist() == proof[:8].tolist()
    plans, act, red, r, rp, qv, qu = _replay(prm, prefix, airs, pvs, l, proof, True)
    assert red and len(act) > len(red)
    for a in act:
        pl, t = plans[a], np.asarray(traces[a], dtype=np.uint32)
        for j in range(pl.w):
            assert proof[qv + 4 * j:qv + 4 * j + 4].tolist() == _np_mle_base(t[j], np.array(r[:pl.m]))
        for k, j in enumerate(pl.rot):
            at = qv + 4 * (pl.w + k)
            assert proof[at:at + 4].tolist() == _np_mle_base(np.roll(t[j], -1), np.array(r[:pl.m]))
        qv += 4 * (pl.w + len(pl.rot))
        if a in red:
            for j in range(pl.w):
                assert proof[qu + 4 * j:qu + 4 * j + 4].tolist() == _np_mle_base(t[j], np.array(rp[:pl.m]))
            qu += 4 * pl.w


def test_second_iteration_of_the_grid_stride_loops(zk):
    """bus_mix at 2^19 rows (4096 pair groups on 1024 workgroups: four iterations in round 0, two in the first pass) beside
    Fibonacci at 2^3; one cell of the tall AIR changed in a row of a later iteration is refused"""
    m = 19
    tr, pv = air.bus_mix_trace(m, seed=3)
    small = _fib(3)
    airs = [_air(air.bus_mix_air(), m), small[0]]
    pvs = [pv, small[2]]
    prm, l, prefix = _lp(_params(1, 4, 4, pow_bits=8, nq=20)), 19, [m]
    root, proof = zk.airbatch_prove(prm, airs, _upload(zk, [tr, small[1]]), pvs, l, prefix)
    lroot, pq = z.airbatch_verify(prm, prefix, airs, pvs, l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0]
    bad = tr.copy()
    row = (1 << (m - 1)) + 5
    bad[2, row] = (int(bad[2, row]) + 1) % P
    _, proof = zk.airbatch_prove(prm, airs, _upload(zk, [bad, small[1]]), pvs, l, prefix)
    with pytest.raises(z.ZkhipError):
        z.airbatch_verify(prm, prefix, airs, pvs, l, proof)


def test_host_verifier_accepts_a_chipset_device_proof(zk):
    airs = _chipset()
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    l, prefix = 17, [4, 2]
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    pvs = [a["pvs"] for a in airs]
    d = _upload(zk, [a["trace"] for a in airs])
    for with_bus in (True, False):
        root, proof = zk.airbatch_prove(prm, vairs, d, pvs, l, prefix, with_bus)
        out = z.airbatch_verify(prm, prefix, vairs, pvs, l, proof, with_bus)
        assert (out[0] if with_bus else out).tolist() == root.tolist()
        bad = proof.copy()
        bad[len(bad) // 5] = (int(bad[len(bad) // 5]) + 1) % P
        with pytest.raises(z.ZkhipError):
            z.airbatch_verify(prm, prefix, vairs, pvs, l, bad, with_bus)


def test_device_proofs_over_tampered_traces_are_refused(zk):
    prm = _lp(PRM)
    airs, traces, pvs, l = bset("lookup")
    traces[1][2][1] = (traces[1][2][1] + 1) % P   # one multiplicity: P != 0
    proof = zk.airbatch_prove(prm, airs, _upload(zk, traces), pvs, l, [1])[1]
    assert proof[8:12].tolist() != [0, 0, 0, 0]
    with pytest.raises(z.ZkhipError):
        z.airbatch_verify(prm, [1], airs, pvs, l, proof)
    airs, traces, pvs, l = bset("mixed")
    traces[0][0][1] = (traces[0][0][1] + 1) % P   # the shortest AIR's constraint fails
    for with_bus in (True, False):
        proof = zk.airbatch_prove(prm, airs, _upload(zk, traces), pvs, l, [2], with_bus)[1]
        with pytest.raises(z.ZkhipError):
            z.airbatch_verify(prm, [2], airs, pvs, l, proof, with_bus)


def test_two_runs_give_identical_words(zk):
    airs, traces, pvs, l = bset("mixed")
    d = _upload(zk, traces)
    x = zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [1])
    y = zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_the_per_air_provers_are_unchanged_around_a_batched_call(zk):
    airs, traces, pvs, l = bset("mixed")
    d = _upload(zk, traces)

    def others():
        a = zk.airset_prove(_lp(PRM), airs, d, pvs, l, [2])
        b = zk.zerocheck_prove(_lp(PRM), airs, d, pvs, l, [2])
        return a[1].tolist(), b[1].tolist()

    ch = Challenger()
    ch.observe([2])
    want_as = am.prove(ch, PRM, airs, traces, pvs, l)[1]
    ch = Challenger()
    ch.observe([2])
    want_zc = zm.prove(ch, PRM, airs, traces, pvs, l)[1]
    assert others() == (want_as, want_zc)
    zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [2])
    zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [2], with_bus=False)
    assert others() == (want_as, want_zc)


def _zb_launches(zk, airs, traces, pvs, l, with_bus=True):
    d = _upload(zk, traces)
    zk.profile_reset()
    zk.profile_enable(True)
    zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [1], with_bus)
    stats = zk.profile_read()
    zk.profile_enable(False)
    return {n: v[0] for n, v in stats.items() if n.startswith("zb_")}


def test_launch_count_does_not_grow_with_the_number_of_airs(zk):
    """k copies of Fibonacci at m = 5 with one copy of bus_mix at m = 5: docs/airbatch.md's formula with M = M' = 5, two classes
    alive in every round, one height: 1 zb_eq (tau) + 1 zb_pows + 2 (M + 1) passes + M zb_round_tr + 1 zb_emit, and for the reduction
    1 zb_pows + 1 zb_eq + 1 zb_combine + M' zb_rot_pass + M' zb_round_tr + 1 zb_eq + 1 zb_dot"""
    m = 5
    want = {"zb_eq": 3, "zb_pows": 2, "zb_round0": 2, "zb_pass": 2 * m, "zb_round_tr": 2 * m, "zb_emit": 1, "zb_combine": 1, "zb_rot_pass": m, "zb_dot": 1}
    for k in (1, 4, 16):
        items = [_fib(m)] * k + [_bus_mix(m)]
        airs, traces, pvs = _split(items)
        assert _zb_launches(zk, airs, traces, pvs, 7) == want, k
    # without the bus part bus_mix joins no other class than its own degree's: Fibonacci (D = 3) and bus_mix's constraints (D = 3) share one
    want0 = dict(want, zb_round0=1, zb_pass=m)
    airs, traces, pvs = _split([_fib(m)] * 4 + [_bus_mix(m)])
    assert _zb_launches(zk, airs, traces, pvs, 7, with_bus=False) == want0
