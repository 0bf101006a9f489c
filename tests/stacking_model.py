"""Independent Python model of the stacked WHIR commitment (docs/stacking.md): the layout, the weight table and its per-piece
evaluation, the prover and the verifier, built on tests/whir_model.py, tests/gkr_model.py and pymodel.Challenger.  It imports nothing
from the product.

Conventions as in whir_model: extension elements are lists of 4 canonical ints, a table of 2^m entries is indexed by i = sum b_j 2^j
(z_0 the lowest bit), words on the wire are canonical."""
import gkr_model as gm
import whir_model as wm
from pymodel import P

ZERO, ONE = wm.ZERO, wm.ONE
MAX_COLS = 1024          # ZKHIP_STACK_MAX_COLS
MAX_POINTS = 64          # ZKHIP_STACK_MAX_POINTS
WHIR_MAX_COLS = 64       # ZKHIP_WHIR_MAX_COLS
WHIR_MAX_LOG_N = 26      # ZKHIP_WHIR_MAX_LOG_N


class Layout:
    """Columns sorted stably by non-increasing height and laid end to end: off[j] (caller order), T, n_stack = ceil(T / 2^l)."""

    def __init__(self, heights, l):
        self.heights, self.l = list(heights), l
        self.order = sorted(range(len(heights)), key=lambda j: -heights[j])   # stable
        self.off = [0] * len(heights)
        o = 0
        for j in self.order:
            self.off[j] = o
            o += 1 << heights[j]
        self.T = o
        self.n_stack = -(-o >> l)

    def pieces(self, j):
        """(stacked column, low entry of the column within it, count of entries) of column j's parts, one per stacked column"""
        m, l, off = self.heights[j], self.l, self.off[j]
        if m <= l:
            return [(off >> l, off & ((1 << l) - 1), 1 << m)]
        return [((off >> l) + h, 0, 1 << l) for h in range(1 << (m - l))]


def width(params, heights, l):
    """n_stack, or 0 when the shape does not fit the limits"""
    if not 1 <= len(heights) <= MAX_COLS or not params.k <= l <= WHIR_MAX_LOG_N or any(m < 0 or m > 32 for m in heights):
        return 0
    n_stack = Layout(heights, l).n_stack
    try:
        params.rounds(l)
    except ValueError:
        return 0
    return n_stack if n_stack <= WHIR_MAX_COLS else 0


def proof_words(params, heights, l):
    n_stack = width(params, heights, l)
    return 4 * len(heights) + 8 * l + wm.proof_words(params, l, n_stack) if n_stack else 0


def stack_vector(cols, heights, l):
    """the long vector S: n_stack 2^l entries, the columns at their offsets, zero from T on"""
    lay = Layout(heights, l)
    S = [0] * (lay.n_stack << l)
    for j, c in enumerate(cols):
        assert len(c) == 1 << heights[j]
        S[lay.off[j]:lay.off[j] + len(c)] = [int(v) % P for v in c]
    return S


def weight_vector(lay, apow, points, col_point):
    """W(off_j + i) = alpha^j eq(z_p(j), i), zero on the padding"""
    W = [ZERO] * (lay.n_stack << lay.l)
    for j, m in enumerate(lay.heights):
        e = gm.eq_table(points[col_point[j]]) if m else [ONE]
        for i in range(1 << m):
            W[lay.off[j] + i] = wm.ext_mul(apow[j], e[i])
    return W


def w_tilde(lay, apow, points, col_point, r):
    """W_c~(r) for every stacked column c, from the public layout: the sum over the pieces on c of coef eq(z^, r)"""
    l, out = lay.l, [ZERO] * lay.n_stack
    for j, m in enumerate(lay.heights):
        z = points[col_point[j]]
        if m <= l:
            c, low, _ = lay.pieces(j)[0]
            hb = low >> m
            zhat = list(z) + [[(hb >> k) & 1, 0, 0, 0] for k in range(l - m)]
            out[c] = wm.ext_add(out[c], wm.ext_mul(apow[j], gm.eq_eval(zhat, r)))
        else:
            e = gm.eq_eval(z[:l], r)
            for h, (c, _, _) in enumerate(lay.pieces(j)):
                coef = wm.ext_mul(apow[j], gm.eq_eval(z[l:], [[(h >> k) & 1, 0, 0, 0] for k in range(m - l)]))
                out[c] = wm.ext_add(out[c], wm.ext_mul(coef, e))
    return out


def _powers(alpha, n):
    out, a = [], ONE
    for _ in range(n):
        out.append(a)
        a = wm.ext_mul(a, alpha)
    return out


class Commitment:
    def __init__(self, params, cols, heights, l):
        if not width(params, heights, l):
            raise ValueError("stack shape")
        self.params, self.heights, self.l = params, list(heights), l
        self.lay = Layout(heights, l)
        self.S = stack_vector(cols, heights, l)
        self.whir = wm.commit(params, [self.S[c << l:(c + 1) << l] for c in range(self.lay.n_stack)])
        self.root = self.whir.root


def commit(params, cols, l):
    return Commitment(params, cols, [len(c).bit_length() - 1 for c in cols], l)


def open_(scom, ch, points, col_point, S=None):
    """The opening, continuing `ch` (which already holds the root): (values, proof words).  S (tests only): run the values and the
    sum-check on this long vector instead of the committed one; the WHIR opening stays the commitment's."""
    lay, l = scom.lay, scom.l
    S = scom.S if S is None else S
    points = [[gm.as_ext(v) for v in p] for p in points]
    words = []
    values = [gm.mle_eval(S[lay.off[j]:lay.off[j] + (1 << m)], points[col_point[j]]) for j, m in enumerate(lay.heights)]
    wm._observe(ch, [x for v in values for x in v], words)
    apow = _powers(ch.sample_ext(), len(values))
    f = [gm.as_ext(v) for v in S]
    w = weight_vector(lay, apow, points, col_point)
    r = []
    for _ in range(l):
        s0, s2 = wm._sumcheck_round(f, w)
        wm._observe(ch, s0 + s2, words)
        rt = ch.sample_ext()
        r.append(rt)
        f = [gm.fold(f[2 * y], f[2 * y + 1], rt) for y in range(len(f) // 2)]
        w = [gm.fold(w[2 * y], w[2 * y + 1], rt) for y in range(len(w) // 2)]
    _, op = wm.open_(scom.whir, ch, r)
    return values, words + op


def verify(ch, params, root, heights, l, points, col_point, words):
    """Replays an opening on `ch` (after the caller observed whatever precedes it, the root included).  Returns the values; raises
    wm.WhirReject."""
    n_stack = width(params, heights, l)
    if not n_stack or not 1 <= len(points) <= MAX_POINTS or len(col_point) != len(heights):
        raise wm.WhirReject("shape")
    points = [[gm.as_ext(v) for v in p] for p in points]
    if any(not 0 <= p < len(points) or len(points[p]) != m for p, m in zip(col_point, heights)):
        raise wm.WhirReject("points")
    if any(x < 0 or x >= P for p in points for e in p for x in e):
        raise wm.WhirReject("points")
    words = [int(x) for x in words]
    if len(words) != proof_words(params, heights, l) or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    values = [rd.ext() for _ in heights]
    ch.observe([x for v in values for x in v])
    apow = _powers(ch.sample_ext(), len(values))
    claim = ZERO
    for a, v in zip(apow, values):
        claim = wm.ext_add(claim, wm.ext_mul(a, v))
    r = []
    for _ in range(l):
        s0, s2 = rd.ext(), rd.ext()
        ch.observe(s0 + s2)
        rt = ch.sample_ext()
        claim = wm._quad(s0, wm.ext_sub(claim, s0), s2, rt)
        r.append(rt)
    u = wm.verify(ch, params, l, n_stack, root, r, words[rd.pos:])
    W = w_tilde(Layout(heights, l), apow, points, col_point, r)
    total = ZERO
    for uc, wc in zip(u, W):
        total = wm.ext_add(total, wm.ext_mul(uc, wc))
    if total != claim:
        raise wm.WhirReject("stacking claim")
    return values
