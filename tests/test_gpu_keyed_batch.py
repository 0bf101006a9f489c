"""GPU: the keyed batched AIR-set proof (docs/airbatch.md, "The keyed batched form") -- the device prover's words equal the independent
model's (tests/keyed_batch_model.py) on the CPU test's sets and on the smallest shapes that reach each device path of the PREP kernels
(tables that run out in rounds 1 and 2 beside an AIR that streams on, a job boundary inside the job search, the hand-built AIR with
rotations on both traces, a reduction whose M' is set by a table that reduces through rot_p alone, PREP and non-PREP classes of one
degree in one round, D = 1 beside D = 8, 64 jobs, boundary keys, a job whose workgroup range hits the cap); the key's root, v_p, v_p'
and u_p against numpy; a ChipSet proof with its preprocessed table; tampered inputs; determinism; the other provers' words before and
after; the launch count against the document's formula."""
import numpy as np
import pytest

import airbatch_model as bm
import airset_model as am
import keyed_batch_model as kb
import keyed_model as km
import zerocheck_model as zm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_gpu_keyed import _boundary_pair, _chipset, _kairs, _lp, _mle, _params, _upload
from test_keyed_batch_cpu import CASES, kset
from test_keyed_cpu import _air, _fib, _hand, _item, _range_pair, _set
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P
PRM = _params(1, 2, 1)


def _split(items):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items]


def _against_model(zk, prm, airs, traces, preps, pvs, l, lpr, wb, prefix):
    key = zk.airkey(_lp(prm), _kairs(airs, preps), lpr)
    root, proof = key.prove_batch(_upload(zk, traces), pvs, l, prefix, with_bus=wb)
    mkey = km.Key(prm, airs, preps, lpr)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words, info = kb.prove(ch, prm, airs, [np.asarray(t).tolist() for t in traces], preps, pvs, l, mkey, wb)
    assert key.root.tolist() == mkey.root and root.tolist() == mroot
    assert len(proof) == len(words) == z.airkey_batch_proof_words(_lp(prm), airs, l, lpr, wb)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    out = z.airkey_batch_verify(_lp(prm), prefix, airs, key.root, lpr, pvs, l, proof, wb)
    assert (out[0] if wb else out).tolist() == mroot
    key.close()
    return info, proof


def _deg1(m):
    """col0 - col1: D = 2, no rotation, no PREP"""
    b = air.AirBuilder(2, 0)
    b.assert_zero(b.var(0) - b.var(1))
    col = np.random.default_rng(m + 7).integers(0, P, size=1 << m, dtype=np.int64)
    return _item(b, m, np.stack([col, col]))


@pytest.mark.parametrize("name,with_bus", CASES)
def test_cpu_shapes_words_equal_model(zk, name, with_bus):
    airs, traces, preps, pvs, l, lpr, _ = kset(name)
    _against_model(zk, PRM, airs, traces, preps, pvs, l, lpr, with_bus, [7, 1])


def test_tables_running_out_in_rounds_1_and_2(zk):
    """tables at m = 1 (round 0 and the last fold both from the key's base columns) and m = 2 beside a user at m = 4 (the second
    table's own user at m = 3)"""
    airs, traces, preps, pvs = _split(_range_pair(1, mu=4, seed=1) + _range_pair(2, mu=3, seed=2))
    for wb in (True, False):
        _against_model(zk, PRM, airs, traces, preps, pvs, 4, 2, wb, [1, 2])


@pytest.mark.parametrize("order", [(8, 2), (2, 8)])
def test_job_search_at_a_job_boundary(zk, order):
    """PREP tables at m = 8 (128 pairs, two workgroups) and m = 2 (one pair) in one class: the job search meets a boundary after two
    workgroups and after one; each with its user"""
    items = [x for i, m in enumerate(order) for x in _range_pair(m, mu=4, seed=10 + i)]
    airs, traces, preps, pvs = _split(items)
    _against_model(zk, PRM, airs, traces, preps, pvs, 8, 8, True, list(order))


def test_hand_built_air_beside_fibonacci(zk):
    """w = 3, n_rot = 2, w_p = 3, n_rot_p = 1 (the rotated preprocessed column is column 1) beside Fibonacci: both reduce"""
    airs, traces, preps, pvs = _split([_hand(3), _fib(4)])
    info, _ = _against_model(zk, PRM, airs, traces, preps, pvs, 4, 3, False, [3])
    pl = info["plans"][0]
    assert (pl.w, pl.rot, pl.wp, pl.rot_p) == (3, [0, 1], 3, [1])


@pytest.mark.parametrize("m", [9, 10, 12])
def test_range_pair_with_the_table_setting_m_prime(zk, m):
    """the range table at m (it reduces through rot_p alone and sets M' = m), a non-reducing AIR at m + 1 (M = m + 1 != M') between it
    and its user, Fibonacci at m = 5 reducing beside it; v_p, v_p', u and u_p of the table against numpy MLEs at the prefixes of r, r'"""
    rt, ru = _range_pair(m, mu=4, seed=m)
    airs, traces, preps, pvs = _split([rt, _deg1(m + 1), ru, _fib(5)])
    info, proof = _against_model(zk, _params(1, 4, 2), airs, traces, preps, pvs, m + 1, 9, True, [m])
    plans = info["plans"]
    act, M, D, red, M2 = kb.dims(plans)
    assert (M, M2, red) == (m + 1, m, [0, 3]) and (plans[0].w, plans[0].rot, plans[0].wp, plans[0].rot_p) == (1, [], 1, [0])
    col = np.asarray(preps[0][0])
    qv, qu = info["val_at"][0], info["u_at"][0]
    r, rp = info["r"][:m], info["rp"][:m]
    assert proof[qv + 4:qv + 8].tolist() == _mle(col, r)                       # v_p
    assert proof[qv + 8:qv + 12].tolist() == _mle(np.roll(col, -1), r)         # v_p'
    assert proof[qu:qu + 4].tolist() == _mle(traces[0][0], rp)                 # u
    assert proof[qu + 4:qu + 8].tolist() == _mle(col, rp)                      # u_p
    assert proof[info["open2_at"]:info["open2_at"] + 4].tolist() == proof[qu + 4:qu + 8].tolist()   # the key opening's value is u_p


def _zb_launches(zk, key, d, pvs, l, wb=True):
    zk.profile_reset()
    zk.profile_enable(True)
    key.prove_batch(d, pvs, l, [1], with_bus=wb)
    stats = zk.profile_read()
    zk.profile_enable(False)
    return {n: v[0] for n, v in stats.items() if n.startswith("zb_")}


def test_prep_and_non_prep_classes_of_one_degree_in_one_round(zk):
    """the range table (D = 3, bus, PREP) beside its user (D = 3, bus, no PREP) at one height: two classes, two launches a round"""
    airs, traces, preps, pvs = _split(_range_pair(3, mu=3, seed=4))
    info, _ = _against_model(zk, PRM, airs, traces, preps, pvs, 4, 3, True, [6])
    assert [(p.D, bool(p.ints), bool(p.wp)) for p in info["plans"]] == [(3, True, True), (3, True, False)]
    key = zk.airkey(_lp(PRM), _kairs(airs, preps), 3)
    got = _zb_launches(zk, key, _upload(zk, traces), pvs, 4)
    assert got["zb_round0"] == 2 and got["zb_pass"] == 2 * 3
    key.close()


def _prep_prod(k, m, seed):
    """prep(0)^k = var(0): D = k + 1 on a preprocessed column"""
    b = air.AirBuilder(1, 0, prep_width=1)
    e = b.prep(0)
    for _ in range(k - 1):
        e = e * b.prep(0)
    b.max_constraint_degree = 9
    b.assert_zero(e - b.var(0))
    col = np.random.default_rng(seed).integers(0, P, size=1 << m, dtype=np.int64)
    return _item(b, m, np.array([[pow(int(x), k, P) for x in col]]), col.reshape(1, -1))


def _prep_deg0(m, c=0x12345):
    """the only constraint is pub(0) - c (D = 1); a PREP section that nothing reads: its columns are folded, sent and opened all the same"""
    b = air.AirBuilder(1, 1, prep_width=1)
    b.assert_zero(b.pub(0) - b.const(c))
    rng = np.random.default_rng(m)
    return _item(b, m, rng.integers(0, P, size=(1, 1 << m)), rng.integers(0, P, size=(1, 1 << m)), [c])


def test_degree_1_beside_degree_8(zk):
    items = [_prep_deg0(3), _prep_prod(7, 2, 1), _prep_deg0(1), _prep_prod(7, 3, 2)]
    airs, traces, preps, pvs = _split(items)
    info, _ = _against_model(zk, PRM, airs, traces, preps, pvs, 4, 3, False, [18])
    assert [p.D for p in info["plans"]] == [1, 8, 1, 8]


def test_64_airs_of_which_half_have_prep(zk):
    rt, ru = _range_pair(2, mu=2, seed=5)
    items = [rt if i % 2 == 0 else ru for i in range(64)]
    airs, traces, preps, pvs = _split(items)
    _against_model(zk, _params(1, 1, 0), airs, traces, preps, pvs, 6, 5, True, [64])


def test_boundary_keys_with_a_cyclic_rotation_read(zk):
    """preprocessed keys 0, 1, p - 1 and (p - 1) / 2; row 3 reads row 0 at rotation 1"""
    airs, traces, preps, pvs = _split(_boundary_pair())
    assert sorted(preps[0][0])[:2] == [0, 1] and P - 1 in preps[0][0]
    for wb in (True, False):
        _against_model(zk, PRM, airs, traces, preps, pvs, 4, 2, wb, [3])


def test_a_job_whose_workgroup_range_hits_the_cap(zk):
    """the range table at m = 18 (2^17 pairs on the cap of 1024 workgroups of 64: two iterations in round 0) beside m = 3, each with a
    user at m = 4; verified, and a proof under a key whose table differs in a row of the second iteration is refused under the right root"""
    m = 18
    user, mult, prep = air.range_traces(4, m, seed=1)
    small = _range_pair(3, mu=4, seed=2)
    airs = [_air(air.range_table_air(), m), _air(air.range_user_air(), 4), small[0][0], small[1][0]]
    kairs = [dict(airs[0], prep=prep), airs[1], dict(airs[2], prep=np.asarray(small[0][2], dtype=np.uint32)), airs[3]]
    pvs = [[], [], [], []]
    prm, l, lpr, prefix = _lp(_params(1, 4, 4, pow_bits=8, nq=20)), 18, 18, [m]
    key = zk.airkey(prm, kairs, lpr)
    d = _upload(zk, [mult, user, small[0][1], small[1][1]])
    root, proof = key.prove_batch(d, pvs, l, prefix)
    lroot, pq = z.airkey_batch_verify(prm, prefix, airs, key.root, lpr, pvs, l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0]
    bad = prep.copy()
    bad[0, 2 * 1024 * 64 + 10] += 1
    key2 = zk.airkey(prm, [dict(airs[0], prep=bad)] + kairs[1:], lpr)
    assert key2.root.tolist() != key.root.tolist()
    _, proof2 = key2.prove_batch(d, pvs, l, prefix)
    with pytest.raises(z.ZkhipError) as e:
        z.airkey_batch_verify(prm, prefix, airs, key.root, lpr, pvs, l, proof2)
    assert e.value.code == -7
    key.close(), key2.close()


def test_key_root_and_values_against_numpy(zk):
    """"five": AirKey.root against Context.stack_commit; v_p, v_p' and u_p against numpy MLEs at the prefixes of r and r'; the key
    opening's values equal u_p (v_p for the table that does not reduce)"""
    airs, traces, preps, pvs, l, lpr, _ = kset("five")
    prm = _lp(PRM)
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    cols = [zk.upload(np.asarray(c, dtype=np.uint32)) for p in preps if p for c in p]
    assert len(cols) == 3 and zk.stack_commit(prm, cols, lpr).root.tolist() == key.root.tolist()
    root, proof = key.prove_batch(_upload(zk, traces), pvs, l, [5])
    ch = Challenger()
    ch.observe([5])
    _, words, info = kb.prove(ch, PRM, airs, traces, preps, pvs, l, km.Key(PRM, airs, preps, lpr), True)
    assert proof.tolist() == words
    plans, red = info["plans"], kb.dims(info["plans"])[3]
    o2, col = info["open2_at"], 0
    for a, pl in enumerate(plans):
        if not pl.wp:
            continue
        r, rp = info["r"][:pl.m], info["rp"][:pl.m]
        qv = info["val_at"][a] + 4 * (pl.w + len(pl.rot))
        for j in range(pl.wp):
            c = np.asarray(preps[a][j])
            assert proof[qv + 4 * j:qv + 4 * j + 4].tolist() == _mle(c, r)
            want = _mle(c, rp) if a in red else _mle(c, r)
            if a in red:
                qu = info["u_at"][a] + 4 * (pl.w + j)
                assert proof[qu:qu + 4].tolist() == want
            assert proof[o2 + 4 * col:o2 + 4 * col + 4].tolist() == want
            col += 1
        for t, j in enumerate(pl.rot_p):
            at = qv + 4 * (pl.wp + t)
            assert proof[at:at + 4].tolist() == _mle(np.roll(np.asarray(preps[a][j]), -1), r)
    key.close()


def test_host_verifier_accepts_a_chipset_device_proof_with_its_table(zk):
    airs = _chipset()
    assert airs[-1].get("prep") is not None and max(a["log_height"] for a in airs) == 14
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    l, lpr, prefix = 17, 4, [4, 2]
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    pvs = [a["pvs"] for a in airs]
    key = zk.airkey(prm, airs, lpr)
    d = _upload(zk, [a["trace"] for a in airs])
    for wb in (True, False):
        root, proof = key.prove_batch(d, pvs, l, prefix, with_bus=wb)
        out = z.airkey_batch_verify(prm, prefix, vairs, key.root, lpr, pvs, l, proof, wb)
        assert (out[0] if wb else out).tolist() == root.tolist()
        if wb:
            assert out[1].tolist()[:4] == [0, 0, 0, 0] and out[1].tolist()[4:] != [0, 0, 0, 0]
        bad = proof.copy()
        bad[len(bad) // 5] = (int(bad[len(bad) // 5]) + 1) % P
        with pytest.raises(z.ZkhipError):
            z.airkey_batch_verify(prm, prefix, vairs, key.root, lpr, pvs, l, bad, wb)
    key.close()


def _refused(fn):
    with pytest.raises(z.ZkhipError) as e:
        fn()
    assert e.value.code == -7


def test_device_proofs_over_tampered_inputs_are_refused(zk):
    prm = _lp(PRM)
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    z.airkey_batch_verify(prm, [1], airs, key.root, lpr, pvs, l, key.prove_batch(_upload(zk, traces), pvs, l, [1])[1])
    bad = [[list(c) for c in t] for t in traces]
    bad[0][0][2] = (bad[0][0][2] + 1) % P   # one multiplicity: P != 0
    proof = key.prove_batch(_upload(zk, bad), pvs, l, [1])[1]
    assert proof[8:12].tolist() != [0, 0, 0, 0]
    _refused(lambda: z.airkey_batch_verify(prm, [1], airs, key.root, lpr, pvs, l, proof))
    bad = [[list(c) for c in t] for t in traces]
    bad[1][1][3] = (bad[1][1][3] + 1) % P   # the user's constraint fails on one row
    for with_bus in (True, False):
        proof = key.prove_batch(_upload(zk, bad), pvs, l, [1], with_bus=with_bus)[1]
        _refused(lambda: z.airkey_batch_verify(prm, [1], airs, key.root, lpr, pvs, l, proof, with_bus))
    # a key built from a table with one cell changed, checked under the right root
    airs, traces, preps, pvs, l, lpr, wb = _set("var_range")
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    row = traces[0][0].index(0)             # a row nobody looks up: only the key catches the change
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][row] = (bad_preps[0][0][row] + 1) % P
    key2 = zk.airkey(prm, _kairs(airs, bad_preps), lpr)
    proof2 = key2.prove_batch(_upload(zk, traces), pvs, l, [2])[1]
    z.airkey_batch_verify(prm, [2], airs, key2.root, lpr, pvs, l, proof2)
    _refused(lambda: z.airkey_batch_verify(prm, [2], airs, key.root, lpr, pvs, l, proof2))


def test_two_runs_give_identical_words(zk):
    airs, traces, preps, pvs, l, lpr, _ = kset("five")
    key = zk.airkey(_lp(PRM), _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    x, y = key.prove_batch(d, pvs, l, [1]), key.prove_batch(d, pvs, l, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all()


def test_the_other_provers_are_unchanged_around_a_keyed_batched_call(zk):
    """on one context: AirKey.prove, airbatch_prove, airset_prove and zerocheck_prove equal their models before and after"""
    from test_airbatch_cpu import bset

    airs, traces, pvs, l = bset("mixed")
    d = _upload(zk, traces)
    kairs, ktraces, kpreps, kpvs, kl, klpr, _ = kset("five")
    key = zk.airkey(_lp(PRM), _kairs(kairs, kpreps), klpr)
    kd = _upload(zk, ktraces)

    def others():
        return (key.prove(kd, kpvs, kl, [2])[1].tolist(), zk.airbatch_prove(_lp(PRM), airs, d, pvs, l, [2])[1].tolist(),
                zk.airset_prove(_lp(PRM), airs, d, pvs, l, [2])[1].tolist(), zk.zerocheck_prove(_lp(PRM), airs, d, pvs, l, [2])[1].tolist())

    def model(fn, *args):
        ch = Challenger()
        ch.observe([2])
        return fn(ch, *args)[1]

    want = (model(km.prove, PRM, kairs, ktraces, kpreps, kpvs, kl, km.Key(PRM, kairs, kpreps, klpr), True),
            model(bm.prove, PRM, airs, traces, pvs, l), model(am.prove, PRM, airs, traces, pvs, l), model(zm.prove, PRM, airs, traces, pvs, l))
    assert others() == want
    key.prove_batch(kd, kpvs, kl, [2])
    key.prove_batch(kd, kpvs, kl, [2], with_bus=False)
    assert others() == want


def test_launch_count_does_not_grow_with_the_number_of_airs(zk):
    """k copies of the range table at m = 5 with one user at m = 5 (it balances all of them: the copies' multiplicities add up):
    docs/airbatch.md's formula with M = M' = 5, two classes ((3, bus, PREP) and (3, bus, no PREP)) alive in every round, one height:
    1 zb_eq (tau) + 1 zb_pows + 2 (M + 1) passes + M zb_round_tr + 1 zb_emit, and for the reduction 1 zb_pows + 1 zb_eq + 1 zb_combine
    + M' zb_rot_pass + M' zb_round_tr + 1 zb_eq + 1 zb_dot"""
    m = 5
    want = {"zb_eq": 3, "zb_pows": 2, "zb_round0": 2, "zb_pass": 2 * m, "zb_round_tr": 2 * m, "zb_emit": 1, "zb_combine": 1, "zb_rot_pass": m, "zb_dot": 1}
    prm = _lp(_params(1, 1, 0))
    for k in (1, 4, 16):
        user, mult, prep = air.range_traces(m, m, seed=k)
        parts = np.zeros((k, 1 << m), dtype=np.int64)   # split the multiplicities over the k copies
        for i, c in enumerate(mult[0]):
            parts[i % k, i] = c
        airs = [_air(air.range_table_air(), m)] * k + [_air(air.range_user_air(), m)]
        key = zk.airkey(prm, [dict(a, prep=prep) for a in airs[:k]] + airs[k:], 7)
        d = _upload(zk, [parts[i:i + 1] for i in range(k)] + [user])
        pvs = [[]] * (k + 1)
        assert _zb_launches(zk, key, d, pvs, 8) == want, k
        z.airkey_batch_verify(prm, [1], airs, key.root, 7, pvs, 8, key.prove_batch(d, pvs, 8, [1])[1])
        key.close()
