"""Independent Python model of the LogUp-GKR fractional-sum proof (docs/logup_gkr.md; Papini-Habock 2023): prover and verifier,
built on tests/pymodel.py's challenger and extension arithmetic only.  It imports nothing from the product.

Conventions: extension elements are lists of 4 canonical ints; a table of 2^m entries is indexed by i = sum b_j 2^j, z_0 is the
lowest bit; leaves are (num, den) with num a base element (int) or an extension element."""
from pymodel import P, Challenger, ext_add, ext_inv, ext_mul  # noqa: F401  (ext_inv: for callers that check fractions)

ZERO = [0, 0, 0, 0]
ONE = [1, 0, 0, 0]


class GkrReject(Exception):
    pass


def ext_sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def ext_c(c):
    return [c % P, 0, 0, 0]


def as_ext(v):
    return [int(x) % P for x in v] if hasattr(v, "__len__") else ext_c(int(v))


def fold(a, b, r):
    return ext_add(a, ext_mul(r, ext_sub(b, a)))


def proof_words(log_n):
    return 8 + 16 * log_n + 6 * log_n * (log_n - 1)


def layer_offset(k):
    return 8 + 16 * k + 6 * k * (k - 1)


def build_layers(num, den):
    """layers[k] = (p_k, q_k) for k = 0..L (layers[L] = the leaves, numerators promoted to extension elements)."""
    n = len(den)
    L = n.bit_length() - 1
    assert n == 1 << L
    p, q = [as_ext(v) for v in num], [as_ext(v) for v in den]
    layers = [None] * (L + 1)
    layers[L] = (p, q)
    for k in range(L - 1, -1, -1):
        p1, q1 = layers[k + 1]
        layers[k] = ([ext_add(ext_mul(p1[2 * x], q1[2 * x + 1]), ext_mul(p1[2 * x + 1], q1[2 * x])) for x in range(1 << k)],
                     [ext_mul(q1[2 * x], q1[2 * x + 1]) for x in range(1 << k)])
    return layers


def eq_table(rho):
    e = [ONE]
    for j in range(len(rho) - 1, -1, -1):   # add variable j as the new lowest bit
        hi = [ext_mul(v, rho[j]) for v in e]
        e = [x for v, h in zip(e, hi) for x in (ext_sub(v, h), h)]
    return e


def eq_eval(rho, r):
    acc = ONE
    for a, b in zip(rho, r):
        ab = ext_mul(a, b)
        acc = ext_mul(acc, ext_add(ext_sub(ext_sub(ONE, a), b), ext_add(ab, ab)))
    return acc


def mle_eval(vals, point):
    """Multilinear extension of 2^m values at `point` (m extension elements, z_0 first)."""
    t = [as_ext(v) for v in vals]
    for r in point:
        t = [fold(t[2 * i], t[2 * i + 1], r) for i in range(len(t) // 2)]
    assert len(t) == 1
    return t[0]


def _g(v, lam):
    p0, p1, q0, q1, e = v
    s = ext_add(ext_add(ext_mul(p0, q1), ext_mul(p1, q0)), ext_mul(lam, ext_mul(q0, q1)))
    return ext_mul(e, s)


def prove(ch, num, den):
    """GKR proof of the tree over (num, den), continuing challenger `ch`.  Returns (words, point, (p~, q~))."""
    layers = build_layers(num, den)
    L = len(layers) - 1
    P0, Q0 = layers[0][0][0], layers[0][1][0]
    words = P0 + Q0
    ch.observe(P0 + Q0)
    rho = []
    for k in range(L):
        lam = ch.sample_ext()
        p1, q1 = layers[k + 1]
        tabs = [p1[0::2], p1[1::2], q1[0::2], q1[1::2], eq_table(rho)]
        rs = []
        for _ in range(k):
            half = len(tabs[0]) // 2
            acc = [ZERO, ZERO, ZERO]
            for y in range(half):
                a = [t[2 * y] for t in tabs]
                d = [ext_sub(t[2 * y + 1], t[2 * y]) for t in tabs]
                v2 = [ext_add(t[2 * y + 1], dd) for t, dd in zip(tabs, d)]
                v3 = [ext_add(x, dd) for x, dd in zip(v2, d)]
                acc = [ext_add(acc[0], _g(a, lam)), ext_add(acc[1], _g(v2, lam)), ext_add(acc[2], _g(v3, lam))]
            msg = acc[0] + acc[1] + acc[2]
            words += msg
            ch.observe(msg)
            r = ch.sample_ext()
            rs.append(r)
            tabs = [[fold(t[2 * y], t[2 * y + 1], r) for y in range(half)] for t in tabs]
        v = [tabs[0][0], tabs[1][0], tabs[2][0], tabs[3][0]]
        msg = v[0] + v[1] + v[2] + v[3]
        words += msg
        ch.observe(msg)
        mu = ch.sample_ext()
        rho = [mu] + rs
    claims = (fold(v[0], v[1], mu), fold(v[2], v[3], mu))
    return words, rho, claims


def _interp(s, x):
    """The cubic through (0, s0) .. (3, s3), at x."""
    inv2, inv6 = pow(2, P - 2, P), pow(6, P - 2, P)
    x1, x2, x3 = ext_sub(x, ext_c(1)), ext_sub(x, ext_c(2)), ext_sub(x, ext_c(3))
    l0 = ext_mul(ext_mul(ext_mul(x1, x2), x3), ext_c(-inv6))
    l1 = ext_mul(ext_mul(ext_mul(x, x2), x3), ext_c(inv2))
    l2 = ext_mul(ext_mul(ext_mul(x, x1), x3), ext_c(-inv2))
    l3 = ext_mul(ext_mul(ext_mul(x, x1), x2), ext_c(inv6))
    out = ZERO
    for l, v in zip((l0, l1, l2, l3), s):
        out = ext_add(out, ext_mul(l, v))
    return out


def verify(ch, words, log_n):
    """Replays a proof on `ch`.  Returns (point, (p~, q~), (P, Q)); raises GkrReject."""
    words = [int(w) for w in words]
    if log_n < 1 or len(words) != proof_words(log_n) or any(w < 0 or w >= P for w in words):
        raise GkrReject("shape")
    root_p, root_q = words[0:4], words[4:8]
    ch.observe(words[0:8])
    cp, cq, rho = root_p, root_q, []
    for k in range(log_n):
        lam = ch.sample_ext()
        claim = ext_add(cp, ext_mul(lam, cq))
        off = layer_offset(k)
        rs = []
        for i in range(k):
            w = words[off + 12 * i: off + 12 * i + 12]
            s0, s2, s3 = w[0:4], w[4:8], w[8:12]
            s1 = ext_sub(claim, s0)
            ch.observe(w)
            r = ch.sample_ext()
            claim = _interp([s0, s1, s2, s3], r)
            rs.append(r)
        w = words[off + 12 * k: off + 12 * k + 16]
        p0, p1, q0, q1 = w[0:4], w[4:8], w[8:12], w[12:16]
        if ext_mul(eq_eval(rho, rs), _g([p0, p1, q0, q1, ONE], lam)) != claim:
            raise GkrReject("layer %d" % k)
        ch.observe(w)
        mu = ch.sample_ext()
        rho = [mu] + rs
        cp, cq = fold(p0, p1, mu), fold(q0, q1, mu)
    return rho, (cp, cq), (root_p, root_q)


def bus_challenges(ch):
    gamma = ch.sample_ext()
    beta = ch.sample_ext()
    return gamma, beta


def bus_verify(prefix, words, log_leaves):
    """The bus argument: (gamma, beta) after the prefix, the GKR proof, and the balance P = 0, Q != 0."""
    ch = Challenger()
    ch.observe(list(prefix))
    gamma, beta = bus_challenges(ch)
    point, claims, (root_p, root_q) = verify(ch, words, log_leaves)
    if root_p != ZERO or root_q == ZERO:
        raise GkrReject("unbalanced")
    return (gamma, beta), point, claims
