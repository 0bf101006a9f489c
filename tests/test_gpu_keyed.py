"""GPU: the keyed zero-check and AIR-set proof (AIR sets with preprocessed columns; docs/airset.md, docs/zerocheck.md) -- the device
prover's words equal the independent model's (tests/keyed_model.py) on the CPU test's shapes, with the table at the heights where the
rotation reduction's tail changes form, and on boundary values in the preprocessed column; the key's root is Context.stack_commit's;
v_p, v_p' and u_p are numpy MLEs of the preprocessed columns; the host verifier accepts device proofs of a ChipSet with its
preprocessed table kept and of a 2^19-row table, and refuses device proofs over a tampered trace or under a key from a tampered table;
runs and keys are deterministic; the other provers' bytes do not change."""
import numpy as np
import pytest

import boundary_inputs as bi
import keyed_model as km
import whir_model as wm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_gpu_gkr import _cases, np_mle
from test_keyed_cpu import NAMES, _air, _item, _range_pair, _set
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _upload(zk, traces):
    return [zk.upload(np.asarray(t, dtype=np.uint32).reshape(-1)) for t in traces]


def _kairs(airs, preps):
    return [dict(a, prep=np.asarray(p, dtype=np.uint32)) if p else a for a, p in zip(airs, preps)]


def _against_model(zk, prm, airs, traces, preps, pvs, l, lpr, wb, prefix):
    key = zk.airkey(_lp(prm), _kairs(airs, preps), lpr)
    root, proof = key.prove(_upload(zk, traces), pvs, l, prefix, with_bus=wb)
    mkey = km.Key(prm, airs, preps, lpr)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words, info = km.prove(ch, prm, airs, traces, preps, pvs, l, mkey, wb)
    assert key.root.tolist() == mkey.root and root.tolist() == mroot
    assert len(proof) == len(words) == z.airkey_proof_words(_lp(prm), airs, l, lpr, wb)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    z.airkey_verify(_lp(prm), prefix, airs, key.root, lpr, pvs, l, proof, wb)
    return info, proof


@pytest.mark.parametrize("name", NAMES)
def test_cpu_shapes_words_equal_model(zk, name):
    airs, traces, preps, pvs, l, lpr, wb = _set(name)
    _against_model(zk, _params(1, 2, 1), airs, traces, preps, pvs, l, lpr, wb, [7, 1])


def _split(items):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items]


def _mle(col, point):
    c4 = np.zeros((len(col), 4), dtype=np.int64)
    c4[:, 0] = np.asarray(col, dtype=np.int64)
    return np_mle(c4, point)


@pytest.mark.parametrize("m", [9, 10, 12])
def test_range_pair_at_the_reductions_tail_heights(zk, m):
    """the table at m = 9 (the reduction's tail in its LDS form from F_a, F_b, eq), 10 and 12 (after one and three streamed rounds);
    v_p, v_p' and u_p of the table against numpy MLEs of the preprocessed column and of np.roll(col, -1)"""
    airs, traces, preps, pvs = _split(_range_pair(m, mu=4, seed=m))
    info, proof = _against_model(zk, _params(1, 4, 2), airs, traces, preps, pvs, 9, 9, True, [m])
    t, pl = info["airs"][0], info["plans"][0]
    col = np.asarray(preps[0][0])
    qv = t["at"] + 4 * pl.D * m
    assert (pl.w, pl.rot, pl.wp, pl.rot_p) == (1, [], 1, [0])
    assert proof[qv + 4:qv + 8].tolist() == _mle(col, t["r"])                       # v_p
    assert proof[qv + 8:qv + 12].tolist() == _mle(np.roll(col, -1), t["r"])         # v_p'
    qu = qv + 12 + 8 * m
    assert proof[qu:qu + 4].tolist() == _mle(traces[0][0], t["rp"])                 # u
    assert proof[qu + 4:qu + 8].tolist() == _mle(col, t["rp"])                      # u_p
    assert proof[info["open2_at"]:info["open2_at"] + 4].tolist() == proof[qu + 4:qu + 8].tolist()


def _boundary_pair(mu=3):
    """a table whose preprocessed keys are 0, 1, p-1 and (p-1)/2 (boundary_inputs.CONST_WORDS), constraints that multiply the key and
    read it at rotation 1 (cyclic: row 3 reads row 0), and a user that sends the keys"""
    keys = np.array(bi.CONST_WORDS[:4], dtype=np.int64)
    tb = air.AirBuilder(3, 0, prep_width=1)
    tb.assert_zero(tb.var(1) - tb.var(0) * tb.prep(0))
    tb.assert_zero(tb.var(2) - tb.prep(0, 1))
    tb.push_interaction(5, [tb.prep(0)], tb.var(0), "receive")
    rng = np.random.default_rng(8)
    pick = rng.integers(0, 4, size=1 << mu)
    user = rng.integers(0, P, size=(4, 1 << mu)).astype(np.int64)
    user[0] = keys[pick]
    user[1] = user[0] * user[0] % P
    mult = np.bincount(pick, minlength=4).astype(np.int64)
    table = np.stack([mult, mult * keys % P, np.roll(keys, -1)])
    assert air.check_trace(tb.program(), table.astype(np.uint32), [], prep=keys.reshape(1, 4).astype(np.uint32)) == []
    return [_item(tb, 2, table, keys.reshape(1, 4)), _item(air.range_user_air(), mu, user)]


def test_boundary_values_in_the_preprocessed_column(zk):
    airs, traces, preps, pvs = _split(_boundary_pair())
    assert sorted(preps[0][0])[:2] == [0, 1] and P - 1 in preps[0][0]
    _against_model(zk, _params(1, 2, 1), airs, traces, preps, pvs, 4, 2, True, [3])


def test_key_root_is_stack_commits(zk):
    airs, traces, preps, pvs, l, lpr, wb = _set("five")
    prm = _lp(_params(1, 2, 1))
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    cols = [zk.upload(np.asarray(c, dtype=np.uint32)) for p in preps if p for c in p]
    assert len(cols) == 3 and zk.stack_commit(prm, cols, lpr).root.tolist() == key.root.tolist()
    key2 = zk.airkey(prm, _kairs(airs, preps), lpr)
    assert key2.root.tolist() == key.root.tolist()
    d = _upload(zk, traces)
    x, y, w = key.prove(d, pvs, l, [1]), key.prove(d, pvs, l, [1]), key2.prove(d, pvs, l, [1])
    assert (x[0] == y[0]).all() and (x[1] == y[1]).all() and (x[1] == w[1]).all()
    zc = key.prove(d, pvs, l, [1], with_bus=False)     # the same key serves the zero-check
    assert z.airkey_verify(prm, [1], airs, key.root, lpr, pvs, l, zc[1], False).tolist() == x[0].tolist()


def _chipset():
    """twelve ChipSet chips of mixed heights up to 2^14 rows and the set's preprocessed range table, as generated"""
    return air.ChipSet(n_chips=12, log_max=14, log_min=4, total_width=120, seed=2).gen(seed=2)


def test_host_verifier_accepts_a_chipset_device_proof_with_its_table(zk):
    airs = _chipset()
    assert airs[-1].get("prep") is not None and max(a["log_height"] for a in airs) == 14
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    l, lpr, prefix = 17, 4, [4, 2]
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in airs]
    pvs = [a["pvs"] for a in airs]
    key = zk.airkey(prm, airs, lpr)
    root, proof = key.prove(_upload(zk, [a["trace"] for a in airs]), pvs, l, prefix)
    lroot, pq = z.airkey_verify(prm, prefix, vairs, key.root, lpr, pvs, l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0] and pq.tolist()[4:] != [0, 0, 0, 0]
    bad = proof.copy()
    bad[len(bad) // 5] = (int(bad[len(bad) // 5]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.airkey_verify(prm, prefix, vairs, key.root, lpr, pvs, l, bad)


def _refused(fn):
    with pytest.raises(z.ZkhipError) as e:
        fn()
    assert e.value.code == -7


def test_strided_loops_at_2_19_rows(zk):
    """the range table at 2^19 rows (verified only): the second iteration of every grid-stride loop that reads the key's columns; a
    proof under a key whose table differs in a row of a later iteration is refused under the right root"""
    m = 19
    user, mult, prep = air.range_traces(4, m, seed=1)
    airs = [_air(air.range_table_air(), m), _air(air.range_user_air(), 4)]
    prm, l, prefix = _lp(_params(1, 4, 4, pow_bits=8, nq=20)), 19, [m]
    key = zk.airkey(prm, [dict(airs[0], prep=prep), airs[1]], 19)
    d = _upload(zk, [mult, user])
    root, proof = key.prove(d, [[], []], l, prefix)
    lroot, pq = z.airkey_verify(prm, prefix, airs, key.root, 19, [[], []], l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0]
    bad = prep.copy()
    bad[0, (1 << 18) + 5] += 1
    key2 = zk.airkey(prm, [dict(airs[0], prep=bad), airs[1]], 19)
    assert key2.root.tolist() != key.root.tolist()
    _, proof2 = key2.prove(d, [[], []], l, prefix)
    _refused(lambda: z.airkey_verify(prm, prefix, airs, key.root, 19, [[], []], l, proof2))


def test_device_proofs_over_tampered_inputs_are_refused(zk):
    prm = _lp(_params(1, 2, 1))
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    z.airkey_verify(prm, [1], airs, key.root, lpr, pvs, l, key.prove(_upload(zk, traces), pvs, l, [1])[1])
    bad = [[list(c) for c in t] for t in traces]
    bad[0][0][2] = (bad[0][0][2] + 1) % P   # one multiplicity: P != 0
    proof = key.prove(_upload(zk, bad), pvs, l, [1])[1]
    assert proof[8:12].tolist() != [0, 0, 0, 0]
    _refused(lambda: z.airkey_verify(prm, [1], airs, key.root, lpr, pvs, l, proof))
    # a key built from a table with one cell changed, checked under the right root
    airs, traces, preps, pvs, l, lpr, wb = _set("var_range")
    key = zk.airkey(prm, _kairs(airs, preps), lpr)
    row = traces[0][0].index(0)             # a row nobody looks up: only the key catches the change
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][row] = (bad_preps[0][0][row] + 1) % P
    key2 = zk.airkey(prm, _kairs(airs, bad_preps), lpr)
    proof2 = key2.prove(_upload(zk, traces), pvs, l, [2])[1]
    z.airkey_verify(prm, [2], airs, key2.root, lpr, pvs, l, proof2)
    _refused(lambda: z.airkey_verify(prm, [2], airs, key.root, lpr, pvs, l, proof2))


def test_key_generation_refusals(zk):
    prm = _lp(_params(1, 2, 1))
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")

    def invalid(kairs, lp_=lpr):
        with pytest.raises(z.ZkhipError):
            zk.airkey(prm, kairs, lp_)

    invalid(airs)                                            # a PREP AIR whose prep_trace is NULL
    invalid([airs[1]])                                       # no PREP in the set
    invalid(_kairs(airs, preps), 1)                          # log_stack_prep below fold_log
    big = [[list(c) for c in p] if p else p for p in preps]
    big[0][0][3] = P
    invalid(_kairs(airs, big))                               # a word that is not canonical
    zk.airkey(prm, _kairs(airs, preps), lpr).close()


def test_interleaved_keyed_proofs_leave_the_other_provers_unchanged(zk):
    cases = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, cases)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in cases]
    cpvs = [a["pvs"] for a in cases]
    prm = _lp(_params(2, 2, 2, pow_bits=4, nq=8))
    vairs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in cases]

    def others():
        zc = zk.zerocheck_prove(prm, vairs, d_traces, cpvs, 8, [2])
        st = zk.airset_prove(prm, vairs, d_traces, cpvs, 8, [2])
        return pk.prove(d_traces, cpvs), zc[0].tolist(), zc[1].tolist(), st[0].tolist(), st[1].tolist()

    before = others()
    airs, traces, preps, pvs, l, lpr, wb = _set("five")
    kp = _lp(_params(1, 2, 1))
    key = zk.airkey(kp, _kairs(airs, preps), lpr)
    d = _upload(zk, traces)
    _, proof = key.prove(d, pvs, l, [2])
    _, zproof = key.prove(d, pvs, l, [2], with_bus=False)
    assert others() == before
    z.airkey_verify(kp, [2], airs, key.root, lpr, pvs, l, proof)
    z.airkey_verify(kp, [2], airs, key.root, lpr, pvs, l, zproof, False)
    assert z.verify(params, cases, cpvs, before[0]) == 0
