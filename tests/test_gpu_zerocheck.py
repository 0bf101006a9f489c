"""GPU: the AIR zero-check (docs/zerocheck.md) -- the device prover's words equal the independent model's (tests/zerocheck_model.py)
on the CPU test's shapes and on shapes that take the streaming constraint pass 1, 2 and 3 rounds deep and the rotation reduction
through both forms of its tail; the root equals Context.stack_commit's; the host verifier accepts device proofs of the full
SyntheticAir at 2^16 rows together with a ChipSet of mixed heights, with v and u equal to a numpy MLE; a device proof over a trace
with one cell changed is refused; runs are deterministic; zkhip_prove gives the same bytes before and after a zero-check."""
import numpy as np
import pytest

import whir_model as wm
import zerocheck_model as zm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_gpu_gkr import _cases, np_mle
from test_zerocheck_cpu import _bus_mix, _fib, _limb, _mixed, _synth, _table
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _upload(zk, traces):
    return [zk.upload(np.asarray(t, dtype=np.uint32).reshape(-1)) for t in traces]


def _against_model(zk, prm, airs, traces, pvs, l, prefix):
    root, proof = zk.zerocheck_prove(_lp(prm), airs, _upload(zk, traces), pvs, l, prefix)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words = zm.prove(ch, prm, airs, traces, pvs, l)
    assert root.tolist() == mroot and len(proof) == len(words) == z.zerocheck_proof_words(_lp(prm), airs, l)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    assert z.zerocheck_verify(_lp(prm), prefix, airs, pvs, l, proof).tolist() == mroot


@pytest.mark.parametrize("m", range(1, 9))
def test_fibonacci_words_equal_model(zk, m):
    """m = 1: round 0 and the last fold both from the base trace; m = 2, 3, 4: the streaming pass 1, 2 and 3 rounds deep"""
    a, tr, pvs = _fib(m)
    _against_model(zk, _params(1, 1, 0), [a], [tr], [pvs], min(m + 1, 5), [m, 9])


@pytest.mark.parametrize("case", ["synth3", "synth5", "limb", "bus_mix", "table"])
def test_single_air_words_equal_model(zk, case):
    a, tr, pvs = {"synth3": lambda: _synth(3, 3), "synth5": lambda: _synth(3, 5), "limb": lambda: _limb(3), "bus_mix": lambda: _bus_mix(2),
                  "table": lambda: _table(2)}[case]()
    _against_model(zk, _params(1, 2, 1), [a], [tr], [pvs], 4, [1, 2, 3])


@pytest.mark.parametrize("b,k,fl", [(1, 1, 0), (2, 2, 1)])
def test_mixed_set_words_equal_model(zk, b, k, fl):
    airs, traces, pvs = _mixed()
    _against_model(zk, _params(b, k, fl, pow_bits=1 + b, nq=2 + k), airs, traces, pvs, 4, [])


@pytest.mark.parametrize("m", [9, 10, 11, 12])
def test_rotation_reduction_tails_equal_model(zk, m):
    """the reduction's single-workgroup tail straight from F_a, F_b and eq (m = 9), after one streamed round (10), and from the
    folded tables after two and three (11, 12)"""
    a, tr, pvs = _fib(m)
    _against_model(zk, _params(1, 4, 2), [a], [tr], [pvs], 9, [m])


def test_root_equals_stack_commit(zk):
    airs, traces, pvs = _mixed()
    prm = _lp(_params(1, 2, 1))
    root, _ = zk.zerocheck_prove(prm, airs, _upload(zk, traces), pvs, 4, [1])
    cols = [zk.upload(np.asarray(c, dtype=np.uint32)) for t in traces for c in t]
    assert zk.stack_commit(prm, cols, 4).root.tolist() == root.tolist()


def _np_mle_base(col, point):
    c4 = np.zeros((col.size, 4), dtype=np.int64)
    c4[:, 0] = col
    return np_mle(c4, [p.tolist() for p in point])


def _replay_points(prm, prefix, airs, pvs, proof):
    """(r, r', offset of v) per AIR with proven constraints, by replaying the transcript with the model's challenger"""
    ch = Challenger()
    ch.observe(prefix)
    ch.observe(proof[:8].tolist())
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    out, q = [], 8
    for a in airs:
        pl = zm.Plan(a)
        if not pl.proven:
            [ch.sample_ext() for _ in range(pl.m)]
            out.append(None)
            continue
        [ch.sample_ext() for _ in range(pl.m + 1)]
        r = []
        for _ in range(pl.m):
            ch.observe(proof[q:q + 4 * pl.D].tolist())
            r.append(ch.sample_ext())
            q += 4 * pl.D
        qv, nv = q, pl.w + len(pl.rot)
        ch.observe(proof[q:q + 4 * nv].tolist())
        q += 4 * nv
        rp = r
        if pl.rot:
            ch.sample_ext()
            rp = []
            for _ in range(pl.m):
                ch.observe(proof[q:q + 8].tolist())
                rp.append(ch.sample_ext())
                q += 8
            ch.observe(proof[q:q + 4 * pl.w].tolist())
            q += 4 * pl.w
        out.append((pl, r, rp, qv))
    return out


def test_host_verifier_accepts_wide_and_mixed_device_proofs(zk):
    """the full SyntheticAir (width 300) at 2^16 rows with a ChipSet of twelve chips of mixed heights in the same proof"""
    sa = air.SyntheticAir()
    tr, pv = sa.gen_trace(16, seed=5)
    airs = [dict(program=sa.program(), log_height=16, width=sa.width, n_pvs=len(pv), trace=tr, pvs=pv)]
    airs += air.ChipSet(n_chips=12, log_max=14, log_min=4, total_width=120, seed=2).gen(seed=2)[:-1]   # without the preprocessed table
    assert len({a["log_height"] for a in airs}) >= 5
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    l, prefix = 19, [4, 2]
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    pvs = [a["pvs"] for a in airs]
    root, proof = zk.zerocheck_prove(prm, vairs, _upload(zk, [a["trace"] for a in airs]), pvs, l, prefix)
    assert z.zerocheck_verify(prm, prefix, vairs, pvs, l, proof).tolist() == root.tolist()
    # v, v' and u against numpy: the SyntheticAir's first, a rotated and its last column, and a chip's
    pts = _replay_points(prm, prefix, vairs, pvs, proof)
    for i in (0, next(i for i in range(1, len(pts)) if pts[i][0].rot)):
        pl, r, rp, qv = pts[i]
        t = np.asarray(airs[i]["trace"], dtype=np.uint32)
        qu = qv + 4 * (pl.w + len(pl.rot)) + 8 * pl.m
        for j in (0, pl.rot[0], pl.w - 1):
            assert proof[qv + 4 * j:qv + 4 * j + 4].tolist() == _np_mle_base(t[j], np.array(r))
            assert proof[qu + 4 * j:qu + 4 * j + 4].tolist() == _np_mle_base(t[j], np.array(rp))
        k = qv + 4 * pl.w
        assert proof[k:k + 4].tolist() == _np_mle_base(np.roll(t[pl.rot[0]], -1), np.array(r))
    bad = proof.copy()
    bad[len(bad) // 5] = (int(bad[len(bad) // 5]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.zerocheck_verify(prm, prefix, vairs, pvs, l, bad)


def test_device_proof_over_a_trace_with_one_cell_changed_is_refused(zk):
    sa = air.SyntheticAir(width=40, n_free=10, n_bool=4, n_boundary=3, seed=3)
    tr, pv = sa.gen_trace(12, seed=1)
    a = dict(program=sa.program(), log_height=12, width=40, n_pvs=len(pv))
    prm = _lp(_params(1, 4, 4, pow_bits=4, nq=8))
    root, proof = zk.zerocheck_prove(prm, [a], _upload(zk, [tr]), [pv], 14, [1])
    z.zerocheck_verify(prm, [1], [a], [pv], 14, proof)
    tr[17, 1234] = (int(tr[17, 1234]) + 1) % P
    assert len(air.check_trace(a["program"], tr, pv)) >= 1
    root, proof = zk.zerocheck_prove(prm, [a], _upload(zk, [tr]), [pv], 14, [1])
    with pytest.raises(z.ZkhipError):
        z.zerocheck_verify(prm, [1], [a], [pv], 14, proof)


def test_two_runs_give_identical_words(zk):
    airs, traces, pvs = _mixed()
    prm = _lp(_params(1, 2, 1))
    d = _upload(zk, traces)
    x = zk.zerocheck_prove(prm, airs, d, pvs, 4, [1])
    y = zk.zerocheck_prove(prm, airs, d, pvs, 4, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_interleaved_zerocheck_leaves_prove_unchanged(zk):
    airs = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    before = pk.prove(d_traces, pvs)
    prm = _lp(_params(2, 2, 2, pow_bits=4, nq=8))
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    root, proof = zk.zerocheck_prove(prm, vairs, d_traces, pvs, 8, [2])
    after = pk.prove(d_traces, pvs)
    assert before == after
    assert z.verify(params, airs, pvs, after) == 0
    z.zerocheck_verify(prm, [2], vairs, pvs, 8, proof)
