"""GPU: the stacked WHIR commitment (docs/stacking.md) -- the device prover's words equal the independent model's
(tests/stacking_model.py); the device root equals zk.whir_commit's root on a numpy-stacked matrix; the host verifier accepts device
openings up to 2^25 cells (n_stack = 64) with values equal to a numpy MLE; the main traces of a mixed-height key open with one point
per AIR; runs are deterministic; the commitment owns its copy of the columns; a stacked opening between two zkhip_prove runs leaves
their bytes unchanged."""
import numpy as np
import pytest

import stacking_model as sm
import whir_model as wm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_gpu_gkr import _cases, np_mle

pytestmark = pytest.mark.gpu
P = z.P


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _inputs(rng, heights, col_point=None):
    cols = [rng.integers(0, P, size=1 << m, dtype=np.uint32) for m in heights]
    if col_point is None:
        dims = sorted(set(heights))
        col_point = [dims.index(m) for m in heights]
    else:
        dims = [None] * (max(col_point) + 1)
        for j, p in enumerate(col_point):
            dims[p] = heights[j]
    points = [rng.integers(0, P, size=(d, 4), dtype=np.uint32) for d in dims]
    return cols, points, col_point


def _np_mle_base(col, point):
    c4 = np.zeros((col.size, 4), dtype=np.int64)
    c4[:, 0] = col
    return np_mle(c4, [p.tolist() for p in point]) if len(point) else c4[0].tolist()


# (heights, log_stack, col_point): the CPU test's shapes, and shapes whose sum-check streams 1, 2 and 3 rounds before the
# single-workgroup tail (n_stack 2^l = 1024, 2048, 6144), with columns of >= 2^12 entries in the values pass
SHAPES = [
    ([6, 0, 3, 5, 0], 4, None),
    ([5], 5, None),
    ([6], 4, None),
    ([3, 2, 1, 1], 4, None),
    ([4, 4, 4], 4, None),
    ([1, 5, 0, 3, 5, 2, 3], 4, None),
    ([3, 3, 3, 3, 2, 2], 3, [0, 0, 1, 0, 2, 2]),
    ([9, 7, 7, 3, 0], 9, None),
    ([10, 9, 3], 10, None),
    ([11, 11, 10, 0], 11, None),
    ([13, 12, 4, 4, 0, 8], 12, None),
]
SETS = [(1, 1, 0), (2, 2, 1), (1, 4, 2)]


@pytest.mark.parametrize("b,k,fl", SETS)
def test_gpu_words_equal_model(zk, b, k, fl):
    prm = _params(b, k, fl, pow_bits=1 + b, nq=2 + k)
    for i, (heights, l, cp) in enumerate(SHAPES):
        if l < k or (l > 10 and (b, k) != (1, 4)):
            continue   # the largest shapes once, with the cheapest set
        rng = np.random.default_rng(1000 * b + 100 * k + i)
        cols, points, col_point = _inputs(rng, heights, cp)
        scom = zk.stack_commit(_lp(prm), [zk.upload(c) for c in cols], l)
        prefix = [int(x) for x in scom.root] + [7, 8]
        vals, proof = zk.stack_open(scom, points, col_point, prefix=prefix)
        mcom = sm.Commitment(prm, [c.tolist() for c in cols], heights, l)
        assert scom.root.tolist() == mcom.root and scom.n_stack == mcom.lay.n_stack
        ch = Challenger()
        ch.observe(prefix)
        mvals, words = sm.open_(mcom, ch, [p.tolist() for p in points], col_point)
        assert vals.tolist() == mvals
        if proof.tolist() != words:
            pytest.fail("%s: proof differs from the model at word %d of %d" % (heights, int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
        z.stack_verify(_lp(prm), prefix, scom.root, heights, l, points, col_point, vals, proof)


@pytest.mark.parametrize("heights,l", [([6, 0, 3, 5, 0], 4), ([14, 12, 12, 9, 3, 0, 1], 12), ([16, 16, 15], 14)])
def test_root_equals_whir_commit_of_a_numpy_stack(zk, heights, l):
    rng = np.random.default_rng(len(heights) + l)
    cols, _, _ = _inputs(rng, heights)
    prm = _lp(_params(1, 4, 2))
    scom = zk.stack_commit(prm, [zk.upload(c) for c in cols], l)
    order = sorted(range(len(heights)), key=lambda j: -heights[j])
    long = np.concatenate([cols[j] for j in order])
    n_stack = -(-long.size >> l)
    mat = np.zeros(n_stack << l, dtype=np.uint32)
    mat[:long.size] = long
    com = zk.whir_commit(prm, zk.upload(mat), l)
    assert scom.n_stack == n_stack and scom.root.tolist() == com.root.tolist()


@pytest.mark.parametrize("name,heights,l", [
    ("48col_small", [m for m in (16, 14, 12, 10, 8, 6) for _ in range(8)], 16),
    ("n_stack_64", [21] * 8 + [20] * 8 + [19] * 8 + [18] * 16, 19),        # 2^25 cells
    ("split_and_tiny", [22, 22, 17, 9, 4, 0, 0, 3], 18),
])
def test_host_verifier_accepts_device_openings_and_values_are_the_mle(zk, name, heights, l):
    rng = np.random.default_rng(len(heights))
    cols, points, col_point = _inputs(rng, heights)
    prm = _lp(_params(1, 4, 4, pow_bits=8, nq=20))
    scom = zk.stack_commit(prm, [zk.upload(c) for c in cols], l)
    vals, proof = zk.stack_open(scom, points, col_point, prefix=[3] + scom.root.tolist())
    assert len(proof) == z.stack_proof_words(prm, heights, l)
    z.stack_verify(prm, [3] + scom.root.tolist(), scom.root, heights, l, points, col_point, vals, proof)
    for j, c in enumerate(cols):
        assert _np_mle_base(c, points[col_point[j]]) == vals[j].tolist(), (name, j)
    bad = proof.copy()
    bad[len(bad) // 3] = (int(bad[len(bad) // 3]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.stack_verify(prm, [3] + scom.root.tolist(), scom.root, heights, l, points, col_point, vals, bad)


def test_mixed_height_key_traces_open_with_one_point_per_air(zk):
    airs = _cases()["mix_and_lookup"]
    rng = np.random.default_rng(11)
    cols, heights, col_point = [], [], []
    for i, a in enumerate(airs):
        tr = np.asarray(a["trace"], dtype=np.uint32).reshape(a["width"], 1 << a["log_height"])
        for c in tr:
            cols.append(c)
            heights.append(a["log_height"])
            col_point.append(i)
    points = [rng.integers(0, P, size=(a["log_height"], 4), dtype=np.uint32) for a in airs]
    prm = _lp(_params(1, 2, 2, pow_bits=6, nq=10))
    l = 6
    scom = zk.stack_commit(prm, [zk.upload(c) for c in cols], l)
    vals, proof = zk.stack_open(scom, points, col_point)
    z.stack_verify(prm, scom.root, scom.root, heights, l, points, col_point, vals, proof)
    for j, c in enumerate(cols):
        assert _np_mle_base(c, points[col_point[j]]) == vals[j].tolist()


def test_two_runs_give_identical_words_and_the_columns_may_be_overwritten(zk):
    rng = np.random.default_rng(9)
    heights, l = [15, 13, 13, 7, 2, 0], 13
    cols, points, col_point = _inputs(rng, heights)
    prm = _lp(_params(1, 4, 4, pow_bits=6, nq=10))
    d = [zk.upload(c) for c in cols]
    scom = zk.stack_commit(prm, d, l)
    a = zk.stack_open(scom, points, col_point)
    b = zk.stack_open(scom, points, col_point)
    scom2 = zk.stack_commit(prm, d, l)
    c = zk.stack_open(scom2, points, col_point)
    assert (scom.root == scom2.root).all()
    for x, y, w in zip(a, b, c):
        assert (x == y).all() and (x == w).all()
    for j, t in enumerate(d):
        assert (zk.download(t) == cols[j]).all()   # the columns are untouched
        t.fill_(0)                                   # ... and the commitment does not need them
    del d
    e = zk.stack_open(scom, points, col_point)
    assert (e[0] == a[0]).all() and (e[1] == a[1]).all()
    z.stack_verify(prm, scom.root, scom.root, heights, l, points, col_point, e[0], e[1])


def test_interleaved_stacked_opening_leaves_prove_unchanged(zk):
    airs = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    before = pk.prove(d_traces, pvs)
    rng = np.random.default_rng(3)
    heights, l = [14, 12, 9, 9, 0], 12
    cols, points, col_point = _inputs(rng, heights)
    prm = _lp(_params(2, 4, 4, pow_bits=4, nq=8))
    scom = zk.stack_commit(prm, [zk.upload(c) for c in cols], l)
    vals, proof = zk.stack_open(scom, points, col_point)
    after = pk.prove(d_traces, pvs)
    assert before == after
    assert z.verify(params, airs, pvs, after) == 0
    z.stack_verify(prm, scom.root, scom.root, heights, l, points, col_point, vals, proof)
