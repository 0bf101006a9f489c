"""CPU: the stacked WHIR commitment (docs/stacking.md) -- the independent model (tests/stacking_model.py) against a brute-force
placement, a direct hypercube sum and itself, and against the library's host verifier (zkhip_stack_verify): model proofs over a grid of
shapes and parameter sets are accepted; forged, mis-shaped and non-canonical proofs are refused, and so is a proof whose values and
sum-check ran on a stacked vector one cell off from the committed one."""
import random

import pytest

import gkr_model as gm
import stacking_model as sm
import whir_model as wm
from pymodel import P, Challenger


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lib_params(p):
    import zkvm_prover_amd as z

    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _rext(rng):
    return [rng.randrange(P) for _ in range(4)]


def _instance(heights, l, prm, col_point=None, seed=0):
    """columns, points (one per distinct height unless col_point is given), the commitment and a model opening after a prefix"""
    rng = random.Random(seed)
    cols = [[rng.randrange(P) for _ in range(1 << m)] for m in heights]
    if col_point is None:
        dims = sorted(set(heights))
        col_point = [dims.index(m) for m in heights]
    else:
        dims = [None] * (max(col_point) + 1)
        for j, p in enumerate(col_point):
            dims[p] = heights[j]
    points = [[_rext(rng) for _ in range(d)] for d in dims]
    scom = sm.Commitment(prm, cols, heights, l)
    prefix = list(scom.root) + [rng.randrange(P) for _ in range(rng.randrange(0, 4))]
    ch = Challenger()
    ch.observe(prefix)
    vals, words = sm.open_(scom, ch, points, col_point)
    return cols, points, col_point, scom, prefix, vals, words


def _brute_placement(cols, heights, l):
    """walk the columns in sorted order and write each entry at the next free cell of an n x 2^l matrix"""
    order = sorted(range(len(cols)), key=lambda j: -heights[j])
    T = sum(1 << m for m in heights)
    n = -(-T // (1 << l))
    mat = [[0] * (1 << l) for _ in range(n)]
    c = b = 0
    for j in order:
        for v in cols[j]:
            mat[c][b] = v
            b += 1
            if b == 1 << l:
                c, b = c + 1, 0
    return mat


def test_layout_equals_a_brute_force_placement():
    import zkvm_prover_amd as z

    rng = random.Random(3)
    prm = _params(1, 1, 0)
    for _ in range(40):
        heights = [rng.randrange(0, 8) for _ in range(rng.randrange(1, 12))]
        l = rng.randrange(1, 8)
        cols = [[rng.randrange(P) for _ in range(1 << m)] for m in heights]
        lay = sm.Layout(heights, l)
        S = sm.stack_vector(cols, heights, l)
        mat = _brute_placement(cols, heights, l)
        assert [S[c << l:(c + 1) << l] for c in range(lay.n_stack)] == mat
        for j, m in enumerate(heights):
            assert lay.off[j] % min(1 << m, 1 << l) == 0
            assert sum(cnt for _, _, cnt in lay.pieces(j)) == 1 << m
        want = lay.n_stack if lay.n_stack <= 64 else 0
        assert z.stack_width(_lib_params(prm), heights, l) == want == sm.width(prm, heights, l)
        assert z.stack_proof_words(_lib_params(prm), heights, l) == sm.proof_words(prm, heights, l)


def test_limits():
    import zkvm_prover_amd as z

    lp = _lib_params(_params(1, 2, 0))
    assert z.stack_width(lp, [3], 1) == 0                  # log_stack below fold_log
    assert z.stack_width(lp, [3], 27) == 0                 # above ZKHIP_WHIR_MAX_LOG_N
    assert z.stack_width(lp, [3], 2) == 2
    assert z.stack_width(lp, [8] * 64, 8) == 64 and z.stack_width(lp, [8] * 64 + [0], 8) == 0   # n_stack <= 64
    assert z.stack_width(lp, [0] * 1024, 4) == 64 and z.stack_width(lp, [0] * 1025, 4) == 0     # n_cols <= 1024
    assert z.stack_width(lp, [], 4) == 0
    assert z.stack_proof_words(lp, [8] * 65, 8) == 0


def test_w_tilde_equals_a_direct_hypercube_sum():
    rng = random.Random(4)
    for _ in range(12):
        heights = [rng.randrange(0, 7) for _ in range(rng.randrange(1, 7))]
        l = rng.randrange(1, 5)
        lay = sm.Layout(heights, l)
        points = [[_rext(rng) for _ in range(m)] for m in heights]
        apow = [_rext(rng) for _ in heights]
        r = [_rext(rng) for _ in range(l)]
        W = sm.weight_vector(lay, apow, points, list(range(len(heights))))
        direct = [gm.mle_eval(W[c << l:(c + 1) << l], r) for c in range(lay.n_stack)]
        assert sm.w_tilde(lay, apow, points, list(range(len(heights))), r) == direct


def test_claim_identity():
    """sum_j alpha^j v_j = sum_e S(e) W(e)"""
    rng = random.Random(5)
    for _ in range(12):
        heights = [rng.randrange(0, 7) for _ in range(rng.randrange(1, 7))]
        l = rng.randrange(1, 6)
        cols = [[rng.randrange(P) for _ in range(1 << m)] for m in heights]
        lay = sm.Layout(heights, l)
        dims = sorted(set(heights))
        col_point = [dims.index(m) for m in heights]
        points = [[_rext(rng) for _ in range(d)] for d in dims]
        alpha = _rext(rng)
        apow = sm._powers(alpha, len(cols))
        lhs = wm.ZERO
        for j, c in enumerate(cols):
            lhs = wm.ext_add(lhs, wm.ext_mul(apow[j], gm.mle_eval(c, points[col_point[j]])))
        S = sm.stack_vector(cols, heights, l)
        W = sm.weight_vector(lay, apow, points, col_point)
        rhs = wm.ZERO
        for s, w in zip(S, W):
            rhs = wm.ext_add(rhs, wm.ext_scale(w, s))
        assert lhs == rhs


# (heights in caller order, log_stack, col_point or None = one point per height): m_j = 0, split columns, one column, n_stack = 1,
# non-power-of-two n_stack, unsorted caller order, shared points
SHAPES = [
    ([6, 0, 3, 5, 0], 4, None),              # split columns (m > l) and m = 0; n_stack = 7
    ([5], 5, None),                          # one column, n_stack = 1
    ([6], 4, None),                          # one column split over 4 stacked columns
    ([3, 2, 1, 1], 4, None),                 # n_stack = 1, several columns
    ([4, 4, 4], 4, None),                    # n_stack = 3
    ([1, 5, 0, 3, 5, 2, 3], 4, None),        # unsorted caller order; n_stack = 5
    ([3, 3, 3, 3, 2, 2], 3, [0, 0, 1, 0, 2, 2]),   # several columns sharing one point; two points of one dimension
]
SETS = [(1, 1, 0), (2, 2, 1), (1, 4, 2)]


@pytest.mark.parametrize("b,k,fl", SETS)
def test_library_verifier_accepts_model_proofs(b, k, fl):
    import zkvm_prover_amd as z

    prm = _params(b, k, fl, pow_bits=1 + b, nq=2 + k)
    for i, (heights, l, cp) in enumerate(SHAPES):
        if l < k:
            continue
        cols, points, col_point, scom, prefix, vals, words = _instance(heights, l, prm, cp, seed=100 * b + 10 * k + i)
        assert len(words) == sm.proof_words(prm, heights, l) == z.stack_proof_words(_lib_params(prm), heights, l)
        assert vals == [gm.mle_eval(c, points[col_point[j]]) for j, c in enumerate(cols)]
        ch = Challenger()
        ch.observe(prefix)
        assert sm.verify(ch, prm, scom.root, heights, l, points, col_point, words) == vals
        z.stack_verify(_lib_params(prm), prefix, scom.root, heights, l, points, col_point, vals, words)


def _refused(prm, prefix, root, heights, l, points, col_point, vals, words, model=True):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError):
        z.stack_verify(_lib_params(prm), prefix, root, heights, l, points, col_point, vals, words)
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, IndexError)):
            sm.verify(ch, prm, root, heights, l, points, col_point, words)


def test_library_verifier_refuses_forgeries():
    import zkvm_prover_amd as z

    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    heights, l = [1, 5, 0, 3, 5, 2, 3], 4
    cols, points, col_point, scom, prefix, vals, words = _instance(heights, l, prm, seed=77)
    z.stack_verify(_lib_params(prm), prefix, scom.root, heights, l, points, col_point, vals, words)
    n, n_stack = len(heights), scom.lay.n_stack
    head = 4 * n + 8 * l
    # a flipped word in v, in a round polynomial, in the WHIR values and inside the WHIR opening (the claimed values follow the proof)
    for i in (5, 4 * n + 3, 4 * n + 8 * (l - 1) + 6, head + 2, head + 4 * n_stack - 1, head + 4 * n_stack + 9, (head + len(words)) // 2,
              len(words) - 3):
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        bvals = [[bad[4 * j + q] for q in range(4)] for j in range(n)]
        _refused(prm, prefix, scom.root, heights, l, points, col_point, bvals, bad)
    # values that differ from the proof's
    bad_vals = [list(v) for v in vals]
    bad_vals[2][1] = (bad_vals[2][1] + 1) % P
    _refused(prm, prefix, scom.root, heights, l, points, col_point, bad_vals, words, model=False)
    # a wrong root, point, col_point, height list or log_stack
    root = list(scom.root)
    root[5] = (root[5] + 1) % P
    _refused(prm, prefix, root, heights, l, points, col_point, vals, words)
    bad_pts = [[list(e) for e in p] for p in points]
    bad_pts[-1][2][0] = (bad_pts[-1][2][0] + 1) % P
    _refused(prm, prefix, scom.root, heights, l, bad_pts, col_point, vals, words)
    two = [[_rext(random.Random(j)) for _ in range(3)] for j in range(2)]   # columns 3 and 6 (both of height 3) on different points
    pts2 = points + two
    cp2 = list(col_point)
    cp2[3], cp2[6] = len(points), len(points) + 1
    _refused(prm, prefix, scom.root, heights, l, pts2, cp2, vals, words, model=False)
    cp3 = list(col_point)
    cp3[1], cp3[4] = cp3[4], cp3[1]   # same dimension: still accepted, they share the point
    z.stack_verify(_lib_params(prm), prefix, scom.root, heights, l, points, cp3, vals, words)
    h2 = list(heights)
    h2[3], h2[6] = 2, 2   # a different layout (and points of the wrong dimension)
    _refused(prm, prefix, scom.root, h2, l, points, col_point, vals, words)
    h3 = [heights[j] for j in (1, 0, 2, 3, 4, 5, 6)]   # the same multiset in another caller order
    cp4 = [col_point[j] for j in (1, 0, 2, 3, 4, 5, 6)]
    v4 = [vals[j] for j in (1, 0, 2, 3, 4, 5, 6)]
    w4 = [x for v in v4 for x in v] + list(words[4 * n:])
    _refused(prm, prefix, scom.root, h3, l, points, cp4, v4, w4)
    for l2 in (l - 1, l + 1):
        _refused(prm, prefix, scom.root, heights, l2, points, col_point, vals, words, model=False)
    _refused(prm, prefix + [1], scom.root, heights, l, points, col_point, vals, words)
    # truncated, extended, non-canonical
    for bad in (words[:-1], list(words) + [0]):
        _refused(prm, prefix, scom.root, heights, l, points, col_point, vals, bad)
    for i in (1, 4 * n + 2, head + 4 * n_stack + 20):
        big = list(words)
        big[i] += P
        bvals = [[big[4 * j + q] for q in range(4)] for j in range(n)]
        _refused(prm, prefix, scom.root, heights, l, points, col_point, bvals, big)
    big_pts = [[list(e) for e in p] for p in points]
    big_pts[-1][0][0] += P
    _refused(prm, prefix, scom.root, heights, l, big_pts, col_point, vals, words, model=False)


@pytest.mark.parametrize("cell", [0, 37, 75])
def test_refuses_a_sumcheck_on_a_stacked_vector_one_cell_off(cell):
    """The values and the stacking sum-check of a proof ran on a long vector that differs in one cell from the committed one; the
    sum-check itself is honest, only the final check against the WHIR opening's values catches it."""
    import zkvm_prover_amd as z

    prm = _params(1, 2, 1, pow_bits=2, nq=3)
    heights, l = [1, 5, 0, 3, 5, 2, 3], 4   # T = 79
    cols, points, col_point, scom, prefix, vals, words = _instance(heights, l, prm, seed=9)
    S2 = list(scom.S)
    S2[cell] = (S2[cell] + 1) % P
    ch = Challenger()
    ch.observe(prefix)
    vals2, words2 = sm.open_(scom, ch, points, col_point, S=S2)
    assert vals2 != vals
    _refused(prm, prefix, scom.root, heights, l, points, col_point, vals2, words2)
