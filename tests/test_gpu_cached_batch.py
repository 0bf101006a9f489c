"""GPU: the keyed batched form with cached partitions (docs/cached_main.md) -- the device prover's words equal the independent model's
(tests/cached_batch_model.py), word for word, on the CPU test's sets and on the smallest shapes that reach each device path: a cached
partition at m = 1 beside an AIR at m = 8; a partition of 2^12 rows cut into sixteen stacked columns (log_stack_cached 8) and padded
(14); 2^16 rows beside 2^3 and a twelve-chip ChipSet with one chip's leading columns cached (the model's words for these two are
recorded in tests/golden/cached_batch_words.npz, see tests/cached_batch_sets.py).  The roots against Context.stack_commit; one handle
for two proofs, the first proof's traces freed in between; tampered inputs; determinism; the other provers' words before and after a
cached call; the zb_* launch counts against AirKey.prove_batch's for 1 and 4 partitions."""
import numpy as np
import pytest

import airbatch_model as bm
import airset_model as am
import cached_batch_model as cm
import cached_batch_sets as cs
import keyed_batch_model as kb
import keyed_model as km
import zerocheck_model as zm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_cached_batch_cpu import CASES, _program_pair, cset
from test_gpu_keyed import _kairs, _lp, _params, _upload
from test_keyed_cpu import _fib, _range_pair

pytestmark = pytest.mark.gpu
P = z.P
PRM = _params(1, 2, 1)


def _split(items):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items]


def _commit(key, d, lsc):
    return [key.commit_cached(a, d[a], lsc[a]) if lsc[a] is not None else None for a in range(len(lsc))]


def _close(*things):
    for t in things:
        for c in (t if isinstance(t, list) else [t]):
            if c is not None:
                c.close()


def _same_words(proof, words):
    assert len(proof) == len(words)
    if proof.tolist() != [int(x) for x in words]:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words, dtype=np.uint32))[0][0]), len(words)))


def _against_model(zk, prm, airs, traces, preps, pvs, l, lpr, lsc, wb, prefix):
    key = zk.airkey(_lp(prm), _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    root, proof = key.prove_batch_cached(d, pvs, cached, l, prefix, with_bus=wb)
    mkey = km.Key(prm, airs, preps, lpr)
    mcached = [cm.Cached(prm, airs, a, traces[a], lsc[a]) if lsc[a] is not None else None for a in range(len(airs))]
    ch = Challenger()
    ch.observe(prefix)
    mroot, words, info = cm.prove(ch, prm, airs, [np.asarray(t).tolist() for t in traces], preps, pvs, l, mkey, mcached, wb)
    assert key.root.tolist() == mkey.root and root.tolist() == mroot
    assert [c.root.tolist() for c in cached if c] == [c.root for c in mcached if c]
    assert len(words) == z.airkey_cached_proof_words(_lp(prm), airs, l, lpr, lsc, wb)
    _same_words(proof, words)
    out = z.airkey_cached_verify(_lp(prm), prefix, airs, key.root, lpr, lsc, pvs, l, proof, wb)
    assert out[0].tolist() == mroot and out[-1].tolist() == [c.root for c in mcached if c]
    _close(cached, key)
    return info, proof


@pytest.mark.parametrize("name,with_bus", CASES)
def test_cpu_shapes_words_equal_model(zk, name, with_bus):
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset(name)
    _against_model(zk, PRM, airs, traces, preps, pvs, l, lpr, lsc, with_bus, [7, 1])


def test_a_partition_at_m_1_beside_m_8(zk):
    """the program AIR at m = 1 (its partition padded to 2^2) beside Fibonacci at m = 8, also cached (cut into 2^4 stacked columns),
    and the range table at m = 8"""
    items = _program_pair(1, 2, seed=1) + [_fib(8)] + _range_pair(8, mu=4, seed=3)
    airs, traces, preps, pvs = _split(items)
    airs[2] = dict(airs[2], program=z.air.with_cached_width(airs[2]["program"], 1))
    for wb in (True, False):
        _against_model(zk, PRM, airs, traces, preps, pvs, 8, 8, [2, None, 4, None, None], wb, [1, 8])


@pytest.mark.parametrize("lsc", [8, 14])
def test_a_partition_of_4096_rows_cut_and_padded(zk, lsc):
    """2^12 rows at log_stack_cached 8 (sixteen stacked columns a cached column: the opening's values pass sums over them) and 14
    (both columns on one stacked column, padded)"""
    items = _program_pair(12, 3, seed=lsc) + _range_pair(2, mu=3)
    airs, traces, preps, pvs = _split(items)
    _against_model(zk, _params(1, 4, 2), airs, traces, preps, pvs, 12, 4, [lsc, None, None, None], True, [12, lsc])


@pytest.mark.parametrize("name", ["big", "chipset"])
def test_larger_sets_words_equal_the_recorded_model_words(zk, name):
    """2^16 rows beside 2^3; twelve ChipSet chips with one chip's three leading columns cached.  The expected words are the model's,
    recorded (the model takes minutes on these)."""
    prm, airs, traces, preps, pvs, l, lpr, lsc, prefix = cs.SETS[name]()
    kr, cr, mroot, words = cs.recorded(name)
    key = zk.airkey(_lp(prm), _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    root, proof = key.prove_batch_cached(d, pvs, cached, l, prefix)
    assert key.root.tolist() == kr.tolist() and root.tolist() == mroot.tolist()
    assert [c.root.tolist() for c in cached if c] == cr.tolist()
    _same_words(proof, words)
    _close(cached, key)


def test_roots_against_stack_commit(zk):
    """CachedMain.root is the stacked commitment of the cached columns, the main root that of the common columns only"""
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("five")
    prm = _lp(PRM)
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    cw = [cm.cached_width(a) for a in airs]
    assert cw == [0, 1, 0, 0, 2]
    for a, c in enumerate(cached):
        if c is not None:
            cols = [zk.upload(np.asarray(col, dtype=np.uint32)) for col in traces[a][:cw[a]]]
            assert zk.stack_commit(prm, cols, lsc[a]).root.tolist() == c.root.tolist()
            assert (c.air_index, c.log_height, c.cached_width, c.log_stack_cached) == (a, airs[a]["log_height"], cw[a], lsc[a])
    root, proof = key.prove_batch_cached(d, pvs, cached, l, [5])
    common = [zk.upload(np.asarray(col, dtype=np.uint32)) for a, t in enumerate(traces) for col in t[cw[a]:]]
    assert zk.stack_commit(prm, common, l).root.tolist() == root.tolist() == proof[16:24].tolist()
    assert proof[:16].tolist() == cached[1].root.tolist() + cached[4].root.tolist()
    everything = [zk.upload(np.asarray(col, dtype=np.uint32)) for t in traces for col in t]
    assert zk.stack_commit(prm, everything, l).root.tolist() == key.prove_batch(d, pvs, l, [5])[0].tolist() != root.tolist()
    _close(cached, key)


def test_commit_once_prove_many(zk):
    """one handle, two proofs whose common columns differ (another run of the same program); the device buffers of the first proof,
    the trace the handle was made from among them, are freed before the second"""
    import torch

    prm = _lp(PRM)
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("program")
    second = _program_pair(2, 3, run=11) + _range_pair(2, mu=3, seed=11)
    traces2 = [x[1] for x in second]
    assert [traces2[0][0], traces2[0][1]] == [traces[0][0], traces[0][1]] and traces2[0][2] != traces[0][2]   # the same program, run otherwise
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    proofs = [key.prove_batch_cached(d, pvs, cached, l, [1])]
    del d
    torch.cuda.empty_cache()
    junk = zk.upload(np.full(1 << 12, 12345, dtype=np.uint32))   # something else takes the freed memory
    d2 = _upload(zk, traces2)
    proofs.append(key.prove_batch_cached(d2, pvs, cached, l, [2]))
    mkey = km.Key(PRM, airs, preps, lpr)
    mcached = [cm.Cached(PRM, airs, 0, traces[0], lsc[0]), None, None, None]
    for (root, proof), tr, prefix in zip(proofs, (traces, traces2), ([1], [2])):
        ch = Challenger()
        ch.observe(prefix)
        mroot, words, _ = cm.prove(ch, PRM, airs, tr, preps, pvs, l, mkey, mcached, True)
        _same_words(proof, words)
        out = z.airkey_cached_verify(prm, prefix, airs, key.root, lpr, lsc, pvs, l, proof)
        assert out[0].tolist() == root.tolist() == mroot and out[2].tolist() == [cached[0].root.tolist()] == [proof[:8].tolist()]
    assert proofs[0][0].tolist() != proofs[1][0].tolist()
    del junk
    _close(cached, key)


def _code(fn):
    with pytest.raises(z.ZkhipError) as e:
        fn()
    return e.value.code


def test_tampered_inputs(zk):
    prm = _lp(PRM)
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("five")
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    z.airkey_cached_verify(prm, [1], airs, key.root, lpr, lsc, pvs, l, key.prove_batch_cached(d, pvs, cached, l, [1])[1])
    for a in (1, 4):   # one cell of a cached column of the trace differs from the handle's copy: Fibonacci (reduces), the user (does not)
        bad = [[list(c) for c in t] for t in traces]
        bad[a][0][1] = (bad[a][0][1] + 1) % P
        proof = key.prove_batch_cached(_upload(zk, bad), pvs, cached, l, [1])[1]
        assert _code(lambda: z.airkey_cached_verify(prm, [1], airs, key.root, lpr, lsc, pvs, l, proof)) == -7
        # ... committed as well, the proof is honest about another trace: Fibonacci's constraints fail, the user's lookup too
        c2 = list(cached)
        c2[a] = key.commit_cached(a, _upload(zk, bad)[a], lsc[a])
        proof = key.prove_batch_cached(_upload(zk, bad), pvs, c2, l, [1])[1]
        assert _code(lambda: z.airkey_cached_verify(prm, [1], airs, key.root, lpr, lsc, pvs, l, proof)) == -7
        c2[a].close()
    # handles: made for another AIR index, missing, made at another height (the same program in another key)
    other = key.commit_cached(4, d[4], 3)
    assert _code(lambda: key.prove_batch_cached(d, pvs, [None, other, None, None, cached[4]], l, [1])) == -3
    assert _code(lambda: key.prove_batch_cached(d, pvs, [None, None, None, None, cached[4]], l, [1])) == -3
    assert _code(lambda: key.prove_batch_cached(d, pvs, [None, cached[1], None, None, None], l, [1])) == -3
    assert _code(lambda: key.commit_cached(0, d[0], 3)) == -3   # an AIR without a CACHED section
    assert _code(lambda: key.commit_cached(5, d[0], 3)) == -3
    assert _code(lambda: key.commit_cached(1, d[1], 1)) == -3   # log_stack_cached below fold_log
    airs6 = [dict(a) for a in airs]
    airs6[1]["log_height"] = 6
    fib6 = _fib(6)
    key6 = zk.airkey(prm, _kairs(airs6, preps), lpr)
    tall = key6.commit_cached(1, zk.upload(np.asarray(fib6[1], dtype=np.uint32).reshape(-1)), 3)
    assert _code(lambda: key.prove_batch_cached(d, pvs, [None, tall, None, None, cached[4]], l, [1])) == -3
    z.airkey_cached_verify(prm, [1], airs, key.root, lpr, lsc, pvs, l, key.prove_batch_cached(d, pvs, cached, l, [1])[1])   # still whole
    _close(cached, other, tall, key, key6)


def test_two_runs_give_identical_words(zk):
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("five")
    key = zk.airkey(_lp(PRM), _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    x, y = key.prove_batch_cached(d, pvs, cached, l, [1]), key.prove_batch_cached(d, pvs, cached, l, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all()
    _close(cached, key)


def test_the_other_provers_are_unchanged_around_a_cached_call(zk):
    """on one context, on sets whose programs carry a CACHED section ("five": keyed; its AIRs without PREP: unkeyed): AirKey.prove_batch,
    AirKey.prove, airbatch_prove, airset_prove and zerocheck_prove equal their models, which ignore the section, before and after"""
    kairs, ktraces, kpreps, kpvs, kl, klpr, lsc, _ = cset("five")
    sub = [1, 4]   # Fibonacci and the user, both with a CACHED section; the user's sends are unanswered: with_bus = 0 forms only
    airs, traces, pvs = [kairs[a] for a in sub], [ktraces[a] for a in sub], [kpvs[a] for a in sub]
    from test_airbatch_cpu import bset

    bairs, btraces, bpvs, bl = bset("mixed")
    key = zk.airkey(_lp(PRM), _kairs(kairs, kpreps), klpr)
    kd, d, bd = _upload(zk, ktraces), _upload(zk, traces), _upload(zk, btraces)
    cached = _commit(key, kd, lsc)

    def others():
        return (key.prove_batch(kd, kpvs, kl, [2])[1].tolist(), key.prove(kd, kpvs, kl, [2])[1].tolist(),
                zk.airbatch_prove(_lp(PRM), airs, d, pvs, kl, [2], False)[1].tolist(), zk.zerocheck_prove(_lp(PRM), airs, d, pvs, kl, [2])[1].tolist(),
                zk.airbatch_prove(_lp(PRM), bairs, bd, bpvs, bl, [2])[1].tolist(), zk.airset_prove(_lp(PRM), bairs, bd, bpvs, bl, [2])[1].tolist())

    def model(fn, *args):
        ch = Challenger()
        ch.observe([2])
        return fn(ch, *args)[1]

    mkey = km.Key(PRM, kairs, kpreps, klpr)
    want = (model(kb.prove, PRM, kairs, ktraces, kpreps, kpvs, kl, mkey, True), model(km.prove, PRM, kairs, ktraces, kpreps, kpvs, kl, mkey, True),
            model(bm.prove, PRM, airs, traces, pvs, kl, False), model(zm.prove, PRM, airs, traces, pvs, kl),
            model(bm.prove, PRM, bairs, btraces, bpvs, bl), model(am.prove, PRM, bairs, btraces, bpvs, bl))
    assert others() == want
    key.prove_batch_cached(kd, kpvs, cached, kl, [2])
    key.prove_batch_cached(kd, kpvs, cached, kl, [2], with_bus=False)
    assert others() == want
    _close(cached, key)


def _zb(zk, fn):
    zk.profile_reset()
    zk.profile_enable(True)
    fn()
    stats = zk.profile_read()
    zk.profile_enable(False)
    return {n: v[0] for n, v in stats.items() if n.startswith("zb_")}, {n: v[0] for n, v in stats.items() if n.startswith("stack_")}


@pytest.mark.parametrize("k", [1, 4])
def test_zb_launches_equal_prove_batch(zk, k):
    """k program AIRs (each with a partition, its own bus and its sender) beside the range pair: the zb_* launches of prove_batch_cached
    are those of prove_batch on the same set, whatever k; the stacked openings' launches grow (one opening per partition), and no
    commitment is made inside the call beyond the main one (stack_gather: 1 in both)"""
    items = [x for i in range(k) for x in _program_pair(2 + i % 2, 3, seed=i, bus=9 + i)] + _range_pair(2, mu=3)
    airs, traces, preps, pvs = _split(items)
    lsc = [3 if i % 2 == 0 and i < 2 * k else None for i in range(len(airs))]
    prm = _lp(PRM)
    key = zk.airkey(prm, _kairs(airs, preps), 3)
    d = _upload(zk, traces)
    cached = _commit(key, d, lsc)
    zb_c, st_c = _zb(zk, lambda: key.prove_batch_cached(d, pvs, cached, 5, [1]))
    zb_b, st_b = _zb(zk, lambda: key.prove_batch(d, pvs, 5, [1]))
    assert zb_c == zb_b and sum(zb_b.values()) > 0
    assert st_c["stack_gather"] == st_b["stack_gather"] == 1
    assert st_c["stack_values"] == st_b["stack_values"] + 2 * k and st_c["stack_coef"] == st_b["stack_coef"] + k
    z.airkey_cached_verify(prm, [1], airs, key.root, 3, lsc, pvs, 5, key.prove_batch_cached(d, pvs, cached, 5, [1])[1])
    _close(cached, key)
