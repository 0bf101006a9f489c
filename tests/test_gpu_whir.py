"""GPU: the WHIR commitment (docs/whir.md) -- the device prover's words equal the independent model's (tests/whir_model.py); the
device root equals one rebuilt from a numpy zeta transform and the oracle's DFT, LDE and Merkle tree; the host verifier accepts
device openings up to m = 22 with values equal to a numpy MLE; runs are deterministic; a committed GKR proof verifies and returns
the (P, Q) of the bare GKR proof; a WHIR opening between two zkhip_prove runs leaves their bytes unchanged."""
import numpy as np
import pytest

import oracle_lib as ora
import whir_model as wm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_gpu_gkr import _cases, np_mle

pytestmark = pytest.mark.gpu
P = z.P

# (log_blowup, fold_log, final_log, n_cols)
SETS = [(1, 1, 0, 1), (2, 2, 1, 3), (1, 4, 2, 2), (3, 1, 3, 2), (1, 2, 4, 5)]


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _inputs(rng, m, n_cols):
    cols = rng.integers(0, P, size=(n_cols, 1 << m), dtype=np.uint32)
    point = rng.integers(0, P, size=(m, 4), dtype=np.uint32)
    return cols, point


def _device_open(zk, prm, cols, m, point, prefix_extra=()):
    com = zk.whir_commit(_lp(prm), zk.upload(cols.reshape(-1)), m)
    prefix = [int(x) for x in com.root] + list(prefix_extra)
    vals, proof = zk.whir_open(com, point, prefix=prefix)
    return com, prefix, vals, proof


@pytest.mark.parametrize("b,k,fl,n_cols", SETS)
def test_gpu_words_equal_model(zk, b, k, fl, n_cols):
    prm = _params(b, k, fl, pow_bits=1 + b, nq=2 + k)
    for m in sorted({k, k + 1, 5, 7, 10, 12, 13} if (b, k) == (1, 4) else {k, k + 1, 5, 7, 12}):
        if m < k:
            continue
        rng = np.random.default_rng(100 * m + 10 * b + k)
        cols, point = _inputs(rng, m, n_cols)
        com, prefix, vals, proof = _device_open(zk, prm, cols, m, point, [7, 8])
        mcom = wm.commit(prm, cols.tolist())
        assert com.root.tolist() == mcom.root
        ch = Challenger()
        ch.observe(prefix)
        mvals, words = wm.open_(mcom, ch, point.tolist())
        assert vals.tolist() == mvals
        if proof.tolist() != words:
            pytest.fail("m=%d: proof differs from the model at word %d of %d" % (m, int(np.nonzero(proof != np.array(words))[0][0]), len(words)))


def _np_zeta(cols):
    c = cols.astype(np.int64).copy()
    n = c.shape[1]
    h = 1
    while h < n:
        v = c.reshape(c.shape[0], -1, 2 * h)
        v[:, :, h:] = (v[:, :, h:] - v[:, :, :h]) % P
        h <<= 1
    return c


@pytest.mark.parametrize("m,b,k", [(6, 1, 4), (12, 2, 2), (16, 1, 4), (18, 3, 1)])
def test_root_equals_an_independent_rebuild(zk, m, b, k):
    rng = np.random.default_rng(m)
    n_cols = 3
    cols, _ = _inputs(rng, m, n_cols)
    prm = _params(b, k, 2)
    com = zk.whir_commit(_lp(prm), zk.upload(cols.reshape(-1)), m)
    coeffs = _np_zeta(cols).astype(np.uint32)
    evals = ora.dft_batch(coeffs, m)                       # F on the order-2^m subgroup, natural order
    cw = ora.coset_lde_batch(evals, m, b, 1, bitrev_out=True)   # F on L_0, bit-reversed
    s = 1 << k
    rows = cw.reshape(n_cols, -1, s)                       # [col][row][t]
    mat = rows.transpose(0, 2, 1).reshape(n_cols * s, -1)  # column c * 2^k + t
    assert com.root.tolist() == ora.Tree([mat]).root.tolist()


@pytest.mark.parametrize("m,b,k,fl", [(11, 1, 4, 2), (14, 2, 4, 4), (16, 1, 2, 6), (20, 1, 4, 4), (22, 2, 4, 6)])
def test_host_verifier_accepts_device_openings_and_values_are_the_mle(zk, m, b, k, fl):
    rng = np.random.default_rng(m + 100 * b)
    n_cols = 2
    cols, point = _inputs(rng, m, n_cols)
    prm = _params(b, k, fl, pow_bits=8, nq=20)
    com, prefix, vals, proof = _device_open(zk, prm, cols, m, point, [3])
    z.whir_verify(_lp(prm), prefix, com.root, m, n_cols, point, vals, proof)
    for c in range(n_cols):
        c4 = np.zeros((1 << m, 4), dtype=np.int64)
        c4[:, 0] = cols[c]
        assert np_mle(c4, point.tolist()) == vals[c].tolist()
    bad = proof.copy()
    bad[len(bad) // 2] = (int(bad[len(bad) // 2]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.whir_verify(_lp(prm), prefix, com.root, m, n_cols, point, vals, bad)


def test_two_runs_give_identical_words(zk):
    rng = np.random.default_rng(9)
    m = 17
    cols, point = _inputs(rng, m, 3)
    prm = _params(1, 4, 4, pow_bits=6, nq=10)
    d = zk.upload(cols.reshape(-1))
    com = zk.whir_commit(_lp(prm), d, m)
    a = zk.whir_open(com, point)
    b = zk.whir_open(com, point)
    com2 = zk.whir_commit(_lp(prm), d, m)
    c = zk.whir_open(com2, point)
    assert (com.root == com2.root).all()
    for x, y, w in zip(a, b, c):
        assert (x == y).all() and (x == w).all()
    assert (zk.download(d).reshape(3, -1) == cols).all()   # the columns are untouched


def test_committed_gkr_2_20(zk):
    rng = np.random.default_rng(20)
    log_n = 20
    num = rng.integers(0, P, size=1 << log_n, dtype=np.uint32)
    den = rng.integers(0, P, size=(1 << log_n, 4), dtype=np.uint32)
    prm = _params(1, 4, 4, pow_bits=10, nq=30)
    d_num, d_den = zk.upload(num), zk.upload(den.reshape(-1))
    proof = zk.gkr_committed_prove(_lp(prm), d_num, d_den, log_n, [5, 6])
    root, pq = z.gkr_committed_verify(_lp(prm), [5, 6], proof, log_n)
    assert root.tolist() == proof[:8].tolist()
    bare, _, _ = zk.gkr_prove(d_num, d_den, log_n, [5, 6])
    assert pq.reshape(-1).tolist() == bare[:8].tolist()
    bad = proof.copy()
    bad[-3] = (int(bad[-3]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.gkr_committed_verify(_lp(prm), [5, 6], bad, log_n)


@pytest.mark.parametrize("log_n,num_ext", [(3, False), (6, True), (9, False), (13, True)])
def test_committed_gkr_words_equal_model(zk, log_n, num_ext):
    rng = np.random.default_rng(30 + log_n)
    num = rng.integers(0, P, size=(1 << log_n, 4) if num_ext else 1 << log_n, dtype=np.uint32)
    den = rng.integers(0, P, size=(1 << log_n, 4), dtype=np.uint32)
    prm = _params(1, 2, 2, pow_bits=3, nq=4)
    proof = zk.gkr_committed_prove(_lp(prm), zk.upload(num.reshape(-1)), zk.upload(den.reshape(-1)), log_n, [1], num_is_ext=num_ext)
    ch = Challenger()
    ch.observe([1])
    words = wm.gkr_committed_prove(ch, prm, num.tolist(), den.tolist(), num_ext)
    assert proof.tolist() == words
    z.gkr_committed_verify(_lp(prm), [1], proof, log_n, num_ext)


def test_interleaved_whir_opening_leaves_prove_unchanged(zk):
    airs = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    before = pk.prove(d_traces, pvs)
    rng = np.random.default_rng(3)
    cols, point = _inputs(rng, 14, 2)
    prm = _params(2, 4, 4, pow_bits=4, nq=8)
    com = zk.whir_commit(_lp(prm), zk.upload(cols.reshape(-1)), 14)
    vals, proof = zk.whir_open(com, point)
    after = pk.prove(d_traces, pvs)
    assert before == after
    assert z.verify(params, airs, pvs, after) == 0
    z.whir_verify(_lp(prm), com.root, com.root, 14, 2, point, vals, proof)
