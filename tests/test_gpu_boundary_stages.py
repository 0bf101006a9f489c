"""GPU: the stage kernels on STRUCTURED inputs (tests/boundary_inputs.py) against the CPU oracle, bit for bit: the same comparisons as
test_gpu_kernels.py and test_sumcheck_blocks.py, on the cells that uniform inputs show a kernel about once in 2^31 -- device words 0,
p-1, (p+-1)/2, MONTY_ONE, multiples of 2^27; butterflies whose difference is +-(p-1); extension products of four (p-1)^2; constant
Poseidon2 states.  One size per class the transform planner distinguishes (single tile below 2^12, two passes, three passes above 2^22,
a width that is no multiple of the 16-column tile); the largest sizes take one member of each family."""
import numpy as np
import pytest

import boundary_inputs as bi

pytestmark = pytest.mark.gpu
P = 2013265921


def _bitrev_index(log_n):
    return np.array([int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0 for i in range(1 << log_n)])


@pytest.mark.parametrize("log_n,width,small", [(0, 3, False), (1, 2, False), (3, 5, False), (10, 5, False), (12, 17, False), (13, 3, False), (23, 1, True)])
def test_ntt_forward_bitrev_inverse(zk, ora, log_n, width, small):
    rng = np.random.default_rng(1000 + log_n)
    idx = _bitrev_index(log_n)
    for name, m in bi.families(rng, width, 1 << log_n, small):
        exp = ora.dft_batch(m, log_n)
        t = zk.upload(m.reshape(-1))
        zk.ntt_batch(t, log_n, width)
        assert (zk.download(t).reshape(width, -1) == exp).all(), name
        t2 = zk.upload(m.reshape(-1))
        zk.ntt_batch(t2, log_n, width, bitrev_out=True)
        assert (zk.download(t2).reshape(width, -1) == exp[:, idx]).all(), name
        zk.ntt_batch(t, log_n, width, inverse=True)
        assert (zk.download(t).reshape(width, -1) == m).all(), name
        t3 = zk.upload(m.reshape(-1))
        zk.ntt_batch(t3, log_n, width, inverse=True)
        assert (zk.download(t3).reshape(width, -1) == ora.dft_batch(m, log_n, inverse=True)).all(), name


@pytest.mark.parametrize("log_n,added,width,shift,small", [(0, 1, 2, 31, False), (5, 2, 4, 31, False), (10, 1, 5, 31, False), (12, 1, 17, 31, False),
                                                            (13, 2, 3, 7, False), (22, 1, 1, 31, True), (23, 1, 1, 31, True)])
def test_coset_lde(zk, ora, log_n, added, width, shift, small):
    rng = np.random.default_rng(2000 + log_n)
    for name, m in bi.families(rng, width, 1 << log_n, small):
        exp = ora.coset_lde_batch(m, log_n, added, shift, bitrev_out=True)
        t = zk.upload(m.reshape(-1))
        out = zk.lde_batch(t, log_n, added, width, shift)
        assert (zk.download(out).reshape(width, -1) == exp).all(), name
        assert (zk.download(t).reshape(width, -1) == m).all(), name   # input preserved


def test_coset_lde_fused_form(zk, ora, monkeypatch):
    """ZKHIP_LDE_FUSED=1 at 2^22 points (where lde_fused_applies holds), as test_gpu_config_forms.py sets it: the oracle's words"""
    import os

    log_n = 22
    assert "ZKHIP_NTT_MAX_LOG_R" not in os.environ   # 2^22 splits 11 + 11 only with the default stage limit; else the four-pass form runs
    rng = np.random.default_rng(22)
    monkeypatch.setenv("ZKHIP_LDE_FUSED", "1")
    for name, m in bi.families(rng, 1, 1 << log_n, small=True):
        exp = ora.coset_lde_batch(m, log_n, 1, 31, bitrev_out=True)
        assert (zk.download(zk.lde_batch(zk.upload(m.reshape(-1)), log_n, 1, 1, 31)).reshape(1, -1) == exp).all(), name


def test_poseidon2_permutation(zk, ora):
    rng = np.random.default_rng(5)
    states = np.concatenate([m.T for _, m in bi.families(rng, 16, 64)])   # rows of 16: constant states c^16, alternating, one-hot, boundary, sparse
    t = zk.upload(states.reshape(-1))
    zk.poseidon2_permute_batch(t, len(states))
    got = zk.download(t).reshape(-1, 16)
    for i in range(len(states)):
        assert (got[i] == ora.permute(states[i])).all(), states[i]


@pytest.mark.parametrize("shapes", [[(3, 5)], [(4, 9), (2, 3), (0, 2)], [(5, 20), (5, 1), (3, 17), (1, 8)], [(10, 300)], [(12, 37), (11, 8), (12, 4), (6, 70)]])
def test_merkle_commit_and_open(zk, ora, shapes):
    rng = np.random.default_rng(len(shapes) * 31 + shapes[0][1])
    fams = [bi.families(rng, w, 1 << lh) for lh, w in shapes]
    for k in range(min(len(f) for f in fams)):
        mats = [f[k][1] for f in fams]
        name = fams[0][k][0]
        ot = ora.Tree(mats)
        t = zk.merkle_commit([(zk.upload(m.reshape(-1)), lh, w) for m, (lh, w) in zip(mats, shapes)])
        assert t.root.tolist() == ot.root.tolist(), name
        for l in range(t.log_height + 1):
            assert (t.layer(l) == ot.layer(l)).all(), (name, l)
        n = 1 << t.log_height
        idx = sorted({0, n - 1, n // 2, n // 3, (5 * n) // 7})
        ops = t.open(idx)
        for i, q in enumerate(idx):
            assert (ops[i] == ot.open(q)).all(), name
            assert ot.verify(q, ops[i]), name


@pytest.mark.parametrize("log_n_out", [0, 1, 3, 5, 10, 13])
def test_fri_fold(zk, ora, log_n_out):
    rng = np.random.default_rng(log_n_out)
    betas = bi.challenges(rng)
    for name, tab in bi.ext_families(rng, 2 << log_n_out):
        vals = np.ascontiguousarray(tab.reshape(-1))
        d = zk.upload(vals)
        for beta in betas:
            assert (zk.download(zk.fri_fold(d, log_n_out, beta)) == ora.fri_fold(vals, log_n_out, beta)).all(), (name, beta)


@pytest.mark.parametrize("k,log_n", [(1, 0), (2, 3), (3, 10), (4, 13)])
def test_sumcheck_round_and_fold(zk, ora, k, log_n):
    rng = np.random.default_rng(100 * k + log_n)
    n = 1 << log_n
    fams = [bi.ext_families(rng, 2 * n) for _ in range(k)]
    rs = bi.challenges(rng)
    for j in range(len(fams[0])):
        name = fams[0][j][0]
        tabs = [np.ascontiguousarray(f[j][1].reshape(-1)) for f in fams]
        d_tabs = [zk.upload(t) for t in tabs]
        assert (zk.sumcheck_round(d_tabs, n) == ora.sumcheck_round(tabs)).all(), name
        for r in rs:
            assert (zk.download(zk.mle_fold(d_tabs[0], n, r)) == ora.mle_fold(tabs[0], r)).all(), (name, r)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 255, 2048, 2049, 10007])
def test_running_sum_and_inverse(zk, ora, n):
    rng = np.random.default_rng(n)
    for name, tab in bi.ext_families(rng, n):
        den = np.ascontiguousarray(tab.reshape(-1))
        zero = ~tab.any(axis=1)
        den[::4][zero] = 1   # never the zero element (the rule of test_hip_running_sum_and_inverse_vs_oracle; zeros have a test of their own)
        assert (zk.download(zk.ext_batch_inverse(zk.upload(den), n)) == ora.ext_batch_inverse(den)).all(), name
        for mname, num in (("0 / p-1", np.where(rng.random(n) < 0.5, 0, P - 1).astype(np.uint32)), ("raw 0 / p-1", bi.raw_words(np.where(rng.random(n) < 0.5, 0, P - 1))),
                           ("boundary", bi.boundary_cells(rng, n))):
            out, total = zk.logup_running_sum(zk.upload(den), zk.upload(num), n)
            exp = ora.logup_running_sum(den, num)
            assert (zk.download(out) == exp).all() and (total == exp[-4:]).all(), (name, mname)


def test_boundary_golden(zk):
    """tests/golden/kat_boundary_v1.json (written by the big-int model tests/pymodel.py, held to the oracle by test_oracle_kat.py): the kernels"""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_boundary_v1.json")) as f:
        kat = json.load(f)
    u32 = lambda x: np.asarray(x, dtype=np.uint32)
    for case in kat["dft"]:
        t = zk.upload(u32(case["in"]))
        zk.ntt_batch(t, case["log_n"], 1)
        assert zk.download(t).tolist() == case["fwd"], case["kind"]
        t = zk.upload(u32(case["in"]))
        zk.ntt_batch(t, case["log_n"], 1, inverse=True)
        assert zk.download(t).tolist() == case["inv"], case["kind"]
    for case in kat["coset_lde"]:
        out = zk.lde_batch(zk.upload(u32(case["in"])), case["log_n"], case["added_bits"], 1, case["shift"])
        assert zk.download(out).tolist() == case["bitrev"], case["kind"]
    states = u32([s for s, _ in kat["poseidon2_perm"]])
    t = zk.upload(states.reshape(-1))
    zk.poseidon2_permute_batch(t, len(states))
    assert zk.download(t).reshape(-1, 16).tolist() == [e for _, e in kat["poseidon2_perm"]]
    den = u32([a for a, _ in kat["ext_inv"]]).reshape(-1)
    assert zk.download(zk.ext_batch_inverse(zk.upload(den), len(den) // 4)).reshape(-1, 4).tolist() == [ai for _, ai in kat["ext_inv"]]
    for case in kat["fri_fold"]:
        got = zk.download(zk.fri_fold(zk.upload(u32(case["in"]).reshape(-1)), case["log_n_out"], case["beta"]))
        assert got.reshape(-1, 4).tolist() == case["out"]
    for c in kat["mle_fold"]:
        assert zk.download(zk.mle_fold(zk.upload(u32(c["in"]).reshape(-1)), len(c["in"]) // 2, c["r"])).reshape(-1, 4).tolist() == c["out"]
    for c in kat["sumcheck_round"]:
        tabs = [zk.upload(u32(t).reshape(-1)) for t in c["tables"]]
        assert zk.sumcheck_round(tabs, len(c["tables"][0]) // 2).reshape(-1, 4).tolist() == c["out"]


# ---- constraint evaluation, one whole proof ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_blowup,width", [(1, 1, 6), (6, 1, 12), (10, 2, 30), (12, 1, 9)])
def test_constraint_eval_stage(zk, ora, log_n, log_blowup, width):
    """the comparison of test_gpu_kernels.test_constraint_eval_stage on traces of constant, alternating, one-hot, boundary and sparse
    columns (unsatisfying traces evaluate like any other: the quotient values are compared word for word)"""
    from zkvm_prover_amd import air

    sa = air.SyntheticAir(width=width, n_free=max(4, width // 3), n_bool=2, n_boundary=1, seed=log_n)
    _, pv = sa.gen_trace(log_n, seed=3)
    rng = np.random.default_rng(log_n)
    for alpha in (bi.raw_words(np.full(4, P - 1)), bi.boundary_cells(rng, 4)):
        for name, tr in bi.families(rng, width, 1 << log_n):
            lde = ora.coset_lde_batch(tr, log_n, log_blowup, 31)
            exp = ora.constraint_eval(sa.program(), log_n, log_blowup, width, lde, pv, alpha)
            d_lde = zk.lde_batch(zk.upload(tr.reshape(-1)), log_n, log_blowup, width, 31)
            got = zk.download(zk.constraint_eval(sa.program(), log_n, log_blowup, width, d_lde, pv, alpha)).reshape(4, -1)
            assert (got == exp).all(), name


def _constant_columns_air(log_n):
    """Four columns: device words (p-1)/2 and (p+1)/2 on every row (the largest magnitudes center_signed hands the opening kernel), their
    product, and a column alternating between the two."""
    from zkvm_prover_amd import air

    lo, hi = (int(x) for x in bi.raw_words([(P - 1) // 2, (P + 1) // 2]))
    b = air.AirBuilder(4, 2)
    b.when_first_row(b.var(0) - b.pub(0))
    b.when_first_row(b.var(1) - b.pub(1))
    b.when_transition(b.next(0) - b.var(0))
    b.when_transition(b.next(1) - b.var(1))
    b.assert_zero(b.var(2) - b.var(0) * b.var(1))
    b.assert_zero((b.var(3) - b.var(0)) * (b.var(3) - b.var(1)))
    b.when_transition(b.next(3) + b.var(3) - b.var(0) - b.var(1))
    n = 1 << log_n
    tr = np.empty((4, n), np.uint32)
    tr[0], tr[1], tr[2] = lo, hi, lo * hi % P
    tr[3] = np.where(np.arange(n) % 2 == 0, lo, hi)
    pvs = np.array([lo, hi], np.uint32)
    assert air.check_trace(b.program(), tr, pvs) == []
    return dict(program=b.program(), log_height=log_n, width=4, n_pvs=2, trace=tr, pvs=pvs)


@pytest.mark.parametrize("log_n", [3, 8, 12])
@pytest.mark.parametrize("params", [(1, 0, 10, 4, 5), (2, 0, 3, 0, 8)])
def test_proof_of_constant_columns_equals_oracle(zk, ora, log_n, params):
    """the comparison of test_gpu_stark.test_proof_bytes_equal_oracle: proof words == the oracle's, both verifiers accept"""
    import zkvm_prover_amd as z

    airs = [_constant_columns_air(log_n)]
    exp = ora.stark_prove(params, airs)
    pk = z.ProvingKey(zk, params, airs)
    got = pk.prove([zk.upload(a["trace"].reshape(-1)) for a in airs], [a["pvs"] for a in airs])
    got_words = np.frombuffer(got, dtype=np.uint32)
    assert len(got) == pk.proof_size and len(got_words) == len(exp)
    if not (got_words == exp).all():
        pytest.fail("proof differs from oracle at word %d of %d" % (int(np.nonzero(got_words != exp)[0][0]), len(exp)))
    assert z.verify(params, airs, [a["pvs"] for a in airs], got) == 0
    assert ora.stark_verify(params, airs, got_words) == 0


# ---- GKR, WHIR, stacking against the Python models ----------------------------------------------------------------------------------
def _columns(rng, n):
    """(name, column of n canonical cells): const, boundary, sparse"""
    sp = rng.integers(0, P, size=n, dtype=np.uint64).astype(np.uint32)
    sp[rng.random(n) < 0.9] = 0
    return [("const raw p-1", bi.raw_words(np.full(n, P - 1))), ("const raw (p+1)/2", bi.raw_words(np.full(n, (P + 1) // 2))),
            ("boundary", bi.boundary_cells(rng, n)), ("sparse", sp)]


def _points(rng, dim):
    """opening points with coordinates from B: the two hypercube corners (every coordinate 0, every coordinate 1 in the base field),
    every coefficient raw p-1, and drawn coordinates"""
    one = np.zeros((dim, 4), np.uint32)
    one[:, 0] = 1
    return [np.zeros((dim, 4), np.uint32), one, bi.raw_words(np.full((dim, 4), P - 1)), bi.boundary_cells(rng, (dim, 4))]


@pytest.mark.parametrize("log_n", [6, 12])   # single-workgroup tail only; streaming rounds first (table > 2^10)
@pytest.mark.parametrize("ext_num", [False, True])
def test_gkr_words_equal_model(zk, log_n, ext_num):
    import gkr_model as gm
    from pymodel import Challenger

    rng = np.random.default_rng(3000 + 2 * log_n + ext_num)
    n = 1 << log_n
    prefix = bi.boundary_cells(rng, 5)
    for name, den in bi.ext_families(rng, n):
        den = den.copy()
        den[~den.any(axis=1), 0] = 1   # never the zero element
        nums = bi.ext_families(rng, n) if ext_num else [("0 / p-1", np.where(rng.random(n) < 0.5, 0, P - 1).astype(np.uint32))] + _columns(rng, n)[:3]
        for nname, num in nums[:3]:
            proof, point, claims = zk.gkr_prove(zk.upload(num.reshape(-1)), zk.upload(den.reshape(-1)), log_n, prefix, num_is_ext=ext_num)
            ch = Challenger()
            ch.observe([int(x) for x in prefix])
            words, mpoint, mclaims = gm.prove(ch, [x.tolist() if ext_num else int(x) for x in num], den.tolist())
            assert proof.tolist() == words, (name, nname)
            assert point.tolist() == mpoint and claims.tolist() == [list(c) for c in mclaims], (name, nname)


@pytest.mark.parametrize("m", [7, 12])
def test_whir_words_equal_model(zk, m):
    import whir_model as wm
    import zkvm_prover_amd as z
    from pymodel import Challenger

    prm = wm.Params(1, 4, 2, [2] * wm.MAX_ROUNDS, [6] * wm.MAX_ROUNDS)
    lp = z.WhirParams.make(prm.b, prm.k, prm.final_log, prm.pow_bits, prm.num_queries)
    rng = np.random.default_rng(4000 + m)
    fams = _columns(rng, 1 << m)
    for (name, c0), (_, c1) in zip(fams, fams[1:] + fams[:1]):
        cols = np.stack([c0, c1])
        com = zk.whir_commit(lp, zk.upload(cols.reshape(-1)), m)
        mcom = wm.commit(prm, cols.tolist())
        assert com.root.tolist() == mcom.root, name
        prefix = [int(x) for x in com.root] + [7, 8]
        for point in _points(rng, m):
            vals, proof = zk.whir_open(com, point, prefix=prefix)
            ch = Challenger()
            ch.observe(prefix)
            mvals, words = wm.open_(mcom, ch, point.tolist())
            assert vals.tolist() == mvals and proof.tolist() == words, (name, point[0])
            z.whir_verify(lp, prefix, com.root, m, 2, point, vals, proof)


@pytest.mark.parametrize("heights,l", [([6, 0, 3, 5, 0], 4), ([11, 11, 10, 0], 11)])   # tail only; streaming rounds first
def test_stacking_words_equal_model(zk, heights, l):
    import stacking_model as sm
    import whir_model as wm
    import zkvm_prover_amd as z
    from pymodel import Challenger

    prm = wm.Params(1, 4, 2, [2] * wm.MAX_ROUNDS, [6] * wm.MAX_ROUNDS)
    lp = z.WhirParams.make(prm.b, prm.k, prm.final_log, prm.pow_bits, prm.num_queries)
    rng = np.random.default_rng(5000 + l)
    dims = sorted(set(heights))
    col_point = [dims.index(h) for h in heights]
    for f in range(4):
        cols = [_columns(rng, 1 << h)[(f + j) % 4 if f == 3 else f][1] for j, h in enumerate(heights)]   # one family each, then mixed
        scom = zk.stack_commit(lp, [zk.upload(c) for c in cols], l)
        mcom = sm.Commitment(prm, [c.tolist() for c in cols], heights, l)
        assert scom.root.tolist() == mcom.root and scom.n_stack == mcom.lay.n_stack
        prefix = [int(x) for x in scom.root] + [7, 8]
        for k in range(4):
            points = [_points(rng, d)[k] for d in dims]
            vals, proof = zk.stack_open(scom, points, col_point, prefix=prefix)
            ch = Challenger()
            ch.observe(prefix)
            mvals, words = sm.open_(mcom, ch, [p.tolist() for p in points], col_point)
            assert vals.tolist() == mvals and proof.tolist() == words, (f, k)
            z.stack_verify(lp, prefix, scom.root, heights, l, points, col_point, vals, proof)
