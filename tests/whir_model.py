"""Independent Python model of the WHIR multilinear commitment (docs/whir.md; Arnon, Chiesa, Fenzi, Yogev 2024) and of the committed
fractional-sum proof: prover and verifier, built on tests/pymodel.py (challenger, extension arithmetic, Merkle hashing, the binary
fold) and tests/gkr_model.py.  It imports nothing from the product.

Conventions: extension elements are lists of 4 canonical ints; a table of 2^m entries is indexed by i = sum b_j 2^j, z_0 is the
lowest bit; words on the wire are canonical."""
import numpy as np

import gkr_model as gm
from pymodel import P, Challenger, bitrev, compress, ext_add, ext_mul, hash_slice, inv, two_adic_generator

ZERO = [0, 0, 0, 0]
ONE = [1, 0, 0, 0]
MAX_ROUNDS = 32


class WhirReject(Exception):
    pass


def ext_sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def ext_scale(a, c):
    return [x * c % P for x in a]


class Params:
    def __init__(self, log_blowup, fold_log, final_log, pow_bits, num_queries):
        self.b, self.k, self.final_log = log_blowup, fold_log, final_log
        self.pow_bits, self.num_queries = list(pow_bits), list(num_queries)

    def rounds(self, m):
        """(R, m_final): R = max(1, floor((m - final_log) / k)) rounds of k variables each; needs m >= k"""
        if not (1 <= self.b <= 3 and 1 <= self.k <= 4 and self.k <= m):
            raise ValueError("whir parameters")
        R = max(1, (m - self.final_log) // self.k) if m > self.final_log else 1
        if R > MAX_ROUNDS or len(self.pow_bits) < R or len(self.num_queries) < R:
            raise ValueError("whir parameters")
        return R, m - self.k * R


def _layout(params, m, n_cols):
    """[(kind, words)] in proof order"""
    R, mf = params.rounds(m)
    k, out = params.k, [("values", 4 * n_cols)]
    n = m + params.b   # log |L_i|
    for i in range(R):
        width = (n_cols if i == 0 else 4) << k
        out += [("sumcheck", 8 * k)]
        last = i == R - 1
        out += [("final", 4 << mf)] if last else [("root", 8), ("ood", 4)]
        out += [("pow", 1), ("queries", params.num_queries[i] * (width + 8 * (n - k)))]
        n -= 1
    return out


def proof_words(params, m, n_cols):
    return sum(w for _, w in _layout(params, m, n_cols))


# ---- multilinear helpers -------------------------------------------------------------------------------------------------------
def zeta(vals):
    """hypercube evaluations -> monomial coefficients (per variable: c[..1..] -= c[..0..])"""
    c = [int(v) % P for v in vals]
    h = 1
    while h < len(c):
        for i in range(len(c)):
            if i & h:
                c[i] = (c[i] - c[i ^ h]) % P
        h <<= 1
    return c


def eq_eval(p, x):
    return gm.eq_eval(p, x)


def pow_point(x, n):
    """(x, x^2, x^4, ..) -- n coordinates: the multilinear point at which f~ equals the univariate F(x)"""
    out = []
    for _ in range(n):
        out.append(x)
        x = ext_mul(x, x)
    return out


def coeff_eval(coeffs, point):
    """f~(point) from monomial coefficients"""
    acc = ZERO
    for i, c in enumerate(coeffs):
        t = gm.as_ext(c)
        for j, z in enumerate(point):
            if i >> j & 1:
                t = ext_mul(t, z)
        acc = ext_add(acc, t)
    return acc


def fold_coeffs(c, r):
    """bind the lowest variable to r in monomial form: c_even + r c_odd"""
    return [ext_add(gm.as_ext(c[2 * i]), ext_mul(r, gm.as_ext(c[2 * i + 1]))) for i in range(len(c) // 2)]


def fold_pair(e0, e1, beta, index, log_height):
    """pymodel.fri_fold at one pair: position `index` of a bit-reversed layer of 2^(log_height+1) values folded to 2^log_height"""
    x = pow(two_adic_generator(log_height + 1), bitrev(index, log_height), P)
    c = inv((-2 * x) % P)
    d = [((b - a) * c) % P for a, b in zip(e0, e1)]
    t = ext_mul([(beta[0] - x) % P] + list(beta[1:]), d)
    return ext_add(e0, t)


def fold_coset(vals, idx, log_n, rs):
    """2^k values at rows idx 2^k .. of a bit-reversed codeword of 2^log_n rows, folded k times: the value at row idx of the
    2^(log_n - k)-row layer"""
    k = len(rs)
    for j, r in enumerate(rs):
        h = log_n - j - 1
        base = idx << (k - j - 1)
        vals = [fold_pair(vals[2 * s], vals[2 * s + 1], r, base + s, h) for s in range(len(vals) // 2)]
    return vals[0]


# ---- encoding and the Merkle commitment ----------------------------------------------------------------------------------------
def _ntt_bitrev(coeffs, log_n):
    """evaluations of sum c_i X^i at w^bitrev(r), r < 2^log_n, w = two_adic_generator(log_n) (radix-2, numpy; checked against
    pymodel.dft_naive by tests/test_whir_cpu.py)"""
    n = 1 << log_n
    a = np.zeros(n, dtype=object)
    a[:len(coeffs)] = [int(c) % P for c in coeffs]
    a = a.astype(np.uint64)
    # decimation in frequency: natural order in, bit-reversed out
    half = n >> 1
    w = two_adic_generator(log_n)
    while half >= 1:
        tw = np.array([pow(w, j, P) for j in range(half)], dtype=np.uint64)
        a = a.reshape(-1, 2 * half)
        lo, hi = a[:, :half].copy(), a[:, half:].copy()
        a[:, :half] = (lo + hi) % P
        a[:, half:] = ((lo + P - hi) % P) * tw % P
        a = a.reshape(-1)
        w = w * w % P
        half >>= 1
    return [int(x) for x in a]


def encode_rows(coef_cols, log_n, k, ext):
    """the committed matrix: rows of 2^(log_n - k); base: row j = [col 0's coset | col 1's | ..]; ext (4 coordinate columns):
    row j = [e_0 (4 words) | e_1 | ..], the coordinates of each element adjacent"""
    cws = [_ntt_bitrev(c, log_n) for c in coef_cols]
    h, s = 1 << (log_n - k), 1 << k
    if ext:
        return [[cws[c][j * s + t] for t in range(s) for c in range(4)] for j in range(h)]
    return [[cw[j * s + t] for cw in cws for t in range(s)] for j in range(h)]


class Tree:
    def __init__(self, rows):
        self.rows = rows
        self.layers = [[hash_slice(r) for r in rows]]
        while len(self.layers[-1]) > 1:
            lay = self.layers[-1]
            self.layers.append([compress(lay[2 * i], lay[2 * i + 1]) for i in range(len(lay) // 2)])
        self.root = self.layers[-1][0]

    def open(self, idx):
        out = list(self.rows[idx])
        for lay in self.layers[:-1]:
            out += lay[idx ^ 1]
            idx >>= 1
        return out


def mmcs_check(root, idx, log_h, width, words):
    row, sib = words[:width], words[width:]
    h = hash_slice(row)
    for l in range(log_h):
        s = sib[8 * l: 8 * l + 8]
        h = compress(s, h) if idx >> l & 1 else compress(h, s)
    return h == list(root)


class Commitment:
    def __init__(self, params, cols):
        self.params, self.cols = params, [[int(v) % P for v in c] for c in cols]
        n = len(self.cols[0])
        self.m = n.bit_length() - 1
        assert n == 1 << self.m and all(len(c) == n for c in self.cols)
        params.rounds(self.m)
        self.coeffs = [zeta(c) for c in self.cols]
        self.tree = Tree(encode_rows(self.coeffs, self.m + params.b, params.k, False))
        self.root = self.tree.root


def commit(params, cols):
    return Commitment(params, cols)


# ---- opening ------------------------------------------------------------------------------------------------------------------
def _sumcheck_round(f, w):
    s0, s2 = ZERO, ZERO
    for y in range(len(f) // 2):
        a0, a1, b0, b1 = f[2 * y], f[2 * y + 1], w[2 * y], w[2 * y + 1]
        s0 = ext_add(s0, ext_mul(a0, b0))
        s2 = ext_add(s2, ext_mul(ext_sub(ext_add(a1, a1), a0), ext_sub(ext_add(b1, b1), b0)))
    return s0, s2


def _quad(s0, s1, s2, r):
    """the quadratic through (0, s0), (1, s1), (2, s2), at r"""
    i2 = inv(2)
    r1, r2 = ext_sub(r, ONE), ext_sub(r, [2, 0, 0, 0])
    l0 = ext_scale(ext_mul(r1, r2), i2)
    l1 = ext_scale(ext_mul(r, r2), P - 1)
    l2 = ext_scale(ext_mul(r, r1), i2)
    return ext_add(ext_add(ext_mul(l0, s0), ext_mul(l1, s1)), ext_mul(l2, s2))


def _eq_table(p):
    return gm.eq_table(p)


def _observe(ch, words, out):
    out += words
    ch.observe(words)


def _query_points(idx_list, log_n, k):
    g = two_adic_generator(log_n - k)
    return [[pow(g, bitrev(q, log_n - k), P), 0, 0, 0] for q in idx_list]


def open_(com, ch, z):
    """WHIR opening of `com` at z (m extension elements), continuing challenger `ch`.  Returns (values, proof words)."""
    params, m, k = com.params, com.m, com.params.k
    R, mf = params.rounds(m)
    z = [gm.as_ext(v) for v in z]
    words = []
    values = [gm.mle_eval(c, z) for c in com.cols]
    _observe(ch, [x for v in values for x in v], words)
    alpha = ch.sample_ext()
    apow, a = [], ONE
    for _ in com.cols:
        apow.append(a)
        a = ext_mul(a, alpha)
    n = len(com.cols[0])
    f = [ZERO] * n
    c = [ZERO] * n
    for j, col in enumerate(com.cols):
        f = [ext_add(x, ext_scale(apow[j], v)) for x, v in zip(f, col)]
        c = [ext_add(x, ext_scale(apow[j], v)) for x, v in zip(c, com.coeffs[j])]
    w = _eq_table(z)
    tree, log_n = com.tree, m + params.b
    for i in range(R):
        rs = []
        for _ in range(k):
            s0, s2 = _sumcheck_round(f, w)
            _observe(ch, s0 + s2, words)
            r = ch.sample_ext()
            rs.append(r)
            f = [gm.fold(f[2 * y], f[2 * y + 1], r) for y in range(len(f) // 2)]
            w = [gm.fold(w[2 * y], w[2 * y + 1], r) for y in range(len(w) // 2)]
            c = fold_coeffs(c, r)
        m_next = m - k * (i + 1)
        if i < R - 1:
            nxt = Tree(encode_rows([[e[q] for e in c] for q in range(4)], log_n - 1, k, True))
            _observe(ch, list(nxt.root), words)
            zeta_pt = ch.sample_ext()
            _observe(ch, coeff_eval(c, pow_point(zeta_pt, m_next)), words)
        else:
            _observe(ch, [x for e in c for x in e], words)
        words.append(ch.grind(params.pow_bits[i]))
        idx = [ch.sample_bits(log_n - k) for _ in range(params.num_queries[i])]
        for q in idx:
            words += tree.open(q)
        if i < R - 1:
            gamma = ch.sample_ext()
            pts = [zeta_pt] + _query_points(idx, log_n, k)
            g = gamma
            add = [ZERO] * len(w)
            for pt in pts:
                e = _eq_table(pow_point(pt, m_next))
                add = [ext_add(x, ext_mul(g, y)) for x, y in zip(add, e)]
                g = ext_mul(g, gamma)
            w = [ext_add(x, y) for x, y in zip(w, add)]
            tree, log_n = nxt, log_n - 1
    return values, words


class _Reader:
    def __init__(self, words):
        self.w, self.pos = words, 0

    def take(self, n):
        if self.pos + n > len(self.w):
            raise WhirReject("short")
        out = self.w[self.pos:self.pos + n]
        self.pos += n
        return out

    def ext(self):
        return self.take(4)


def verify(ch, params, m, n_cols, root, z, words):
    """Replays an opening on `ch` (after the caller observed whatever precedes it).  Returns the n_cols values; raises
    WhirReject."""
    try:
        R, mf = params.rounds(m)
    except ValueError:
        raise WhirReject("parameters")
    words = [int(x) for x in words]
    if len(words) != proof_words(params, m, n_cols) or any(x < 0 or x >= P for x in words) or len(z) != m:
        raise WhirReject("shape")
    k, rd = params.k, _Reader(words)
    z = [gm.as_ext(v) for v in z]
    vals = [rd.ext() for _ in range(n_cols)]
    ch.observe([x for v in vals for x in v])
    alpha = ch.sample_ext()
    apow, a = [], ONE
    for _ in range(n_cols):
        apow.append(a)
        a = ext_mul(a, alpha)
    sigma = ZERO
    for v, ap in zip(vals, apow):
        sigma = ext_add(sigma, ext_mul(ap, v))
    cons = [(ONE, z)]   # (coefficient, point over the variables left when it was added); bound coordinates are tracked below
    rs_all = []         # challenges, in order
    cons_at = [0]       # index into rs_all of the first variable each constraint spans
    log_n, cur_root = m + params.b, list(root)
    for i in range(R):
        rs = []
        for _ in range(k):
            s0, s2 = rd.ext(), rd.ext()
            ch.observe(s0 + s2)
            r = ch.sample_ext()
            sigma = _quad(s0, ext_sub(sigma, s0), s2, r)
            rs.append(r)
        rs_all += rs
        m_next = m - k * (i + 1)
        last = i == R - 1
        if not last:
            nxt_root = rd.take(8)
            ch.observe(nxt_root)
            zeta_pt = ch.sample_ext()
            ood = rd.ext()
            ch.observe(ood)
        else:
            final = [rd.ext() for _ in range(1 << mf)]
            ch.observe([x for e in final for x in e])
        wit = rd.take(1)[0]
        ch.observe([wit])
        if ch.sample_bits(params.pow_bits[i]) != 0:
            raise WhirReject("pow")
        idx = [ch.sample_bits(log_n - k) for _ in range(params.num_queries[i])]
        width = (n_cols if i == 0 else 4) << k
        folded = []
        for q in idx:
            op = rd.take(width + 8 * (log_n - k))
            if not mmcs_check(cur_root, q, log_n - k, width, op):
                raise WhirReject("merkle")
            row = op[:width]
            s = 1 << k
            if i == 0:
                coset = [ZERO] * s
                for j in range(n_cols):
                    coset = [ext_add(e, ext_scale(apow[j], row[j * s + t])) for t, e in enumerate(coset)]
            else:
                coset = [row[4 * t: 4 * t + 4] for t in range(s)]
            folded.append(fold_coset(coset, q, log_n, rs))
        pts = _query_points(idx, log_n, k)
        if not last:
            gamma = ch.sample_ext()
            g = gamma
            for pt, val in zip([zeta_pt] + pts, [ood] + folded):
                sigma = ext_add(sigma, ext_mul(g, val))
                cons.append((g, pow_point(pt, m_next)))
                cons_at.append(len(rs_all))
                g = ext_mul(g, gamma)
            cur_root, log_n = nxt_root, log_n - 1
        else:
            for pt, val in zip(pts, folded):
                if coeff_eval(final, pow_point(pt, mf)) != val:
                    raise WhirReject("final query")
    # sigma = sum_b f_final(b) w_final(b) = sum_t coef_t eq(p_t bound part, r) f_final~(p_t free part)
    total = ZERO
    for (coef, pt), at in zip(cons, cons_at):
        nb = len(rs_all) - at
        t = ext_mul(coef, eq_eval(pt[:nb], rs_all[at:]))
        total = ext_add(total, ext_mul(t, coeff_eval(final, pt[nb:])))
    if total != sigma:
        raise WhirReject("final sum")
    return vals


# ---- the committed fractional sum ---------------------------------------------------------------------------------------------
def gkr_columns(num, den, num_ext):
    """[num column(s) | 4 den columns]: base-field columns of the leaves"""
    cols = [[gm.as_ext(v)[q] for v in num] for q in range(4)] if num_ext else [[int(v) % P for v in num]]
    return cols + [[gm.as_ext(d)[q] for d in den] for q in range(4)]


def combine_coords(vals):
    """sum_c X^c v_c for 4 extension values v_c (the MLE of the coordinate columns, as one extension element)"""
    acc = ZERO
    for c, v in enumerate(vals):
        xc = [1 if q == c else 0 for q in range(4)]
        acc = ext_add(acc, ext_mul(xc, v))
    return acc


def gkr_committed_proof_words(params, log_n, num_ext):
    return 8 + gm.proof_words(log_n) + proof_words(params, log_n, 8 if num_ext else 5)


def gkr_committed_prove(ch, params, num, den, num_ext, gkr_num=None, gkr_den=None):
    """[root | GKR proof | WHIR opening at the GKR point].  gkr_num / gkr_den (tests only): run the GKR part on other tables than
    the committed ones."""
    com = commit(params, gkr_columns(num, den, num_ext))
    ch.observe(list(com.root))
    words, point, claims = gm.prove(ch, num if gkr_num is None else gkr_num, den if gkr_den is None else gkr_den)
    _, op = open_(com, ch, point)
    return list(com.root) + words + op


def gkr_committed_verify(ch, params, log_n, num_ext, words):
    """Returns (root, (P, Q)); raises WhirReject / gkr_model.GkrReject."""
    words = [int(x) for x in words]
    if len(words) != gkr_committed_proof_words(params, log_n, num_ext):
        raise WhirReject("shape")
    root = words[:8]
    ch.observe(root)
    gw = words[8:8 + gm.proof_words(log_n)]
    point, (cp, cq), (Pr, Qr) = gm.verify(ch, gw, log_n)
    n_cols = 8 if num_ext else 5
    vals = verify(ch, params, log_n, n_cols, root, point, words[8 + len(gw):])
    num_v = combine_coords(vals[:4]) if num_ext else vals[0]
    den_v = combine_coords(vals[-4:])
    if num_v != cp or den_v != cq:
        raise WhirReject("claims")
    return root, (Pr, Qr)
