"""Boundary operand sets of the limb chips (modular, ecc, fp2, the four int256 chips, keccak, sha256): pure Python integers, no GPU.
For each chip and each modulus or curve: named families of ACCEPTED records and a short named list of REFUSED ones.  Everything is
derived from the modulus: Tonelli-Shanks for square roots, pow(g, (p - 1) // 3, p) for a cube root of unity, pow(x, -1, p) for slopes;
every point used is asserted to be on its curve.  tests/test_limb_boundary_cpu.py checks the families against Python's integers, the
AIRs and the lookup tables; tests/test_gpu_limb_boundary.py runs the device generators on them.  docs/boundary_tests.md, third section."""
import functools
import json
import os

import numpy as np

import ecc_util as eu
import fp2_util as fu
import int256_util as iu
import modular_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
P_BB = 2013265921

SECP_P = 2**256 - 2**32 - 977
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
BN_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BN_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P256_P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
BLS_P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
MODULI = dict(secp256k1_p=SECP_P, secp256k1_n=SECP_N, bn254_p=BN_P, bn254_r=BN_R, p256_p=P256_P, bls12_381_p=BLS_P)
FP2_MODULI = dict(bn254_p=BN_P, secp256k1_p=SECP_P, bls12_381_p=BLS_P)


def limbs_of(p):
    return 32 if p < 1 << 256 else 48


def _rng(tag):
    return np.random.default_rng(sum(tag.encode()) + 7919 * len(tag))


def _big(rng, nbytes):
    return int.from_bytes(rng.bytes(nbytes), "little")


# ---- number theory ---------------------------------------------------------------------------------------------------------------
def sqrt_mod(n, p):
    """Tonelli-Shanks: a square root of n mod the odd prime p, or None"""
    n %= p
    if n == 0:
        return 0
    if pow(n, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(n, q, p), pow(n, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    assert r * r % p == n
    return r


def cube_root_of_unity(p):
    assert p % 3 == 1
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    w = pow(g, (p - 1) // 3, p)
    assert w != 1 and pow(w, 3, p) == 1
    return w


# ---- modular chip ----------------------------------------------------------------------------------------------------------------
def modular_families(p):
    """{family: [(op, a, b)]} as modular_util.py_trace takes them (op 0 mul, 1 add, 2 sub, 3 div: a / b, 4 is_eq)"""
    L = limbs_of(p)
    M = 1 << (8 * L)
    rng = _rng("modular%d" % (p & 0xFFFF))
    big = lambda: _big(rng, L) % p  # noqa: E731
    x, y, w = big(), big() | 1, big()
    p0 = p & 255
    fam = {}
    fam["add"] = [(1, 1, p - 1), (1, p - 1, 1), (1, x, p - x), (1, (p - 1) // 2, (p + 1) // 2),     # a + b = p: r = 0, q = 1
                  (1, 0, p - 1), (1, x, p - 1 - x), (1, (p - 1) // 2, (p - 1) // 2),                # a + b = p - 1: r = p - 1, q = 0
                  (1, 0, 0), (1, p - 1, p - 1), (1, M - 1, M - 1), (1, p, 0), (1, p - p0, 0)]
    fam["sub"] = [(2, x, x), (2, 0, 0), (2, p - 1, p - 1), (2, x - 1, x), (2, 0, 1), (2, 0, p - 1), (2, p - 1, 0), (2, M - 1, M - 1), (2, M - 2, M - 1),
                  (2, x, y), (2, y, x), (2, p, 1), (2, 1, p)]
    fam["mul"] = [(0, p - 1, p - 1), (0, 0, x), (0, x, 0), (0, 0, 0), (0, 1, p - 1), (0, p - 1, 1), (0, x, pow(x, -1, p)), (0, 1, p - p0),
                  (0, p, 1), (0, p, 3), (0, 255, p), (0, p, p - 1),                                 # exact multiples of p, both factors non-zero (unreduced)
                  (0, M - 1, p - 1), (0, p - 1, M - 1), (0, M - 1, 1), (0, (M - 1) // 255 * 255, p - 1)]
    fam["div"] = [(3, p - y, y), (3, 0, y), (3, y, y), (3, (p - p0) * y % p, y), (3, x, y), (3, 1, p - 1), (3, p - 1, p - 1), (3, x, 1), (3, (p - 2) * w % p, w)]
    flips = [0, 1, L // 2, L - 2]
    fam["eq"] = [(4, x, x), (4, 0, 0), (4, p - 1, p - 1), (4, 0, p - 1), (4, p - 1, 0), (4, 0, 1), (4, 1, 0)]
    fam["eq"] += [(4, x, x ^ (1 << (8 * i))) for i in flips] + [(4, x ^ (1 << (8 * i)), x) for i in flips]
    fam["eq"] += [(4, 1 << (8 * (L - 1)), 0), (4, 0, 1 << (8 * (L - 1)))]
    ops = [0, 1, 2, 3, 4, 0, 2, 3]
    fam["uniform"] = [(ops[i % 8], big(), big() | 1) for i in range(24)]
    return fam


def modular_record_words(row, p):
    """the device record (op | a | b) of a twin row: a division's record holds the quotient in the a slot"""
    op, a, b = row
    nw = limbs_of(p) // 4
    if op == 3:
        a = a * pow(b, -1, p) % p
    return [op] + eu.words(a, nw) + eu.words(b, nw)


def modular_expected(row, p):
    """(a columns, r columns) as Python integers, by divmod: independent of the twin"""
    op, a, b = row
    if op == 0:
        return a, divmod(a * b, p)[1]
    if op == 1:
        return a, divmod(a + b, p)[1]
    if op in (2, 4):
        return a, divmod(a - b, p)[1]
    q = a * pow(b, -1, p) % p
    assert q * b % p == a % p
    return q, a


def modular_refused(p):
    """{name: raw device record words}; none of these has a trace"""
    L = limbs_of(p)
    nw, M = L // 4, 1 << (8 * L)
    w = lambda v: eu.words(v, nw)  # noqa: E731
    out = {"div_unreduced_quotient": [3] + w(p + 5) + w(3), "div_quotient_is_p": [3] + w(p) + w(1), "opcode_5": [5] + w(1) + w(2), "opcode_big": [0xFFFFFFFF] + w(1) + w(2),
           "sub_far_apart_neg": [2] + w(0) + w(M - 1), "sub_far_apart_pos": [2] + w(M - 1) + w(0), "eq_far_apart": [4] + w(M - 1) + w(0)}
    if (M - 1) * (M - 1) // p >= M:
        out["mul_quotient_overflows"] = [0] + w(M - 1) + w(M - 1)
    return out


@functools.lru_cache(maxsize=None)
def modular_twin(name, family, n=None, log_h=None):
    p = MODULI[name]
    rows = modular_families(p)[family] if family != "mixed" else modular_mixed(p)
    rows = rows[:n] if n is not None else rows
    log_h = log_h if log_h is not None else max(1, (len(rows) - 1).bit_length())
    return rows, log_h, mu.py_trace(rows, p, log_h)


@functools.lru_cache(maxsize=None)
def modular_mixed(p, n=512):
    """division, equality and plain rows interleaved (every wave diverges at `if (is_div) hist_add`), the edge rows first"""
    f = modular_families(p)
    base = [r for i in range(16) for k in ("div", "eq", "mul", "add", "sub", "uniform") for r in f[k][i:i + 1]]
    return tuple((base * (n // len(base) + 1))[:n])


# ---- curves ----------------------------------------------------------------------------------------------------------------------
def _curves():
    with open(os.path.join(HERE, "golden", "ecc_kat.json")) as f:
        kat = json.load(f)["curves"]
    c = {k: tuple(int(v[x], 16) for x in ("p", "a", "b", "gx", "gy")) for k, v in kat.items()}
    from test_vm_cpu import BLS12_381_G1
    c["bls12_381"] = (BLS_P, 0, 4, BLS12_381_G1[0], BLS12_381_G1[1])
    assert c["secp256k1"][0] == SECP_P and c["bn254"][0] == BN_P and c["p256"][0] == P256_P
    return c


CURVES = _curves()


class Curve:
    def __init__(self, name):
        self.name = name
        self.p, self.a, self.b, gx, gy = CURVES[name]
        self.g = (gx, gy)
        assert self.on(self.g)

    def on(self, pt):
        return (pt[1] * pt[1] - pt[0] ** 3 - self.a * pt[0] - self.b) % self.p == 0

    def neg(self, pt):
        return (pt[0], (-pt[1]) % self.p)

    def add(self, p1, p2):
        """affine group law from the textbook formulas (no point at infinity: callers keep away from it); -> (slope, point)"""
        p = self.p
        if p1 == p2:
            lam = (3 * p1[0] * p1[0] + self.a) * pow(2 * p1[1], -1, p) % p
        else:
            assert p1[0] != p2[0]
            lam = (p2[1] - p1[1]) * pow(p2[0] - p1[0], -1, p) % p
        x3 = (lam * lam - p1[0] - p2[0]) % p
        r = (x3, (lam * (p1[0] - x3) - p1[1]) % p)
        assert self.on(r)
        return lam, r

    def multiples(self, n):
        pts = [self.g]
        while len(pts) < n:
            pts.append(self.add(pts[-1], self.g)[1])
        return pts

    def chord_with_slope(self, lam, pts):
        """two curve points whose chord has slope lam: the line of that slope through p1 meets the curve again where
        x^2 + (x1 - lam^2) x + (a - 2 lam c + x1 (x1 - lam^2)) = 0, c = y1 - lam x1"""
        p = self.p
        for p1 in pts:
            c = (p1[1] - lam * p1[0]) % p
            bq, cq = (p1[0] - lam * lam) % p, (self.a - 2 * lam * c + p1[0] * (p1[0] - lam * lam)) % p
            s = sqrt_mod(bq * bq - 4 * cq, p)
            if s is None:
                continue
            x2 = (-bq + s) * pow(2, -1, p) % p
            p2 = (x2, (lam * x2 + c) % p)
            if x2 == p1[0]:
                continue
            assert self.on(p2) and (p2[1] - p1[1] - lam * (x2 - p1[0])) % p == 0
            return p1, p2
        return None

    def point_with_x(self, x):
        y = sqrt_mod(x ** 3 + self.a * x + self.b, self.p)
        return None if y is None else (x % self.p, y)


def _call(cv, p1, p2):
    """a chord (or, for p1 == p2, tangent) call record in the twin's form"""
    lam, _ = cv.add(p1, p2)
    return (1, p1, p2, lam) if p1 == p2 else (0, p1, p2, lam)


@functools.lru_cache(maxsize=None)
def ecc_families(name):
    """{family: [(op, (x1, y1), (x2, y2), slope)]}: every point is on the curve (a doubling's second point is ignored by the chip and is
    given as another curve point)"""
    cv = Curve(name)
    p = cv.p
    L = limbs_of(p)
    M = 1 << (8 * L)
    pts = cv.multiples(40)
    fam = {}
    # doubling beside addition, lane by lane
    fam["mixed"] = [(_call(cv, pts[i], pts[i]) if i % 2 else _call(cv, pts[i], pts[i + 3])) for i in range(16)]
    fam["mixed"] += [(1, pts[5], pts[9], cv.add(pts[5], pts[5])[0])]
    # chords of slope 0, 1 and p - 1
    slopes = []
    if cv.a == 0:   # j = 0: (x, y) and (w x, y)
        w = cube_root_of_unity(p)
        for pt in pts[:3]:
            for ww in (w, w * w % p):
                q = (ww * pt[0] % p, pt[1])
                assert cv.on(q) and q[0] != pt[0]
                slopes.append((0, pt, q, 0))
    for lam in (0, 1, p - 1):
        pair = cv.chord_with_slope(lam, pts)
        if pair is not None:
            slopes.append((0, pair[0], pair[1], lam))
            slopes.append((0, pair[1], pair[0], lam))
    for c in slopes:
        assert c[3] == eu.slope_of(0, p, cv.a, c[1], c[2])
        if c[3] == 0:   # the closed form: identity 1 is 0, x3 = -(x1 + x2)
            assert c[1][1] == c[2][1] and cv.add(c[1], c[2])[1][0] == (-(c[1][0] + c[2][0])) % p
    fam["slopes"] = slopes
    # results close to the modulus: x3 = p - k (differs from p in limb 0 only), x3 = 0 where the curve has such a point, x3 or y3 with the modulus's top limb
    marks = []
    for x in [0] + list(range(p - 1, p - 40, -1)):
        t = cv.point_with_x(x)
        if t is None or t[1] == 0:
            continue
        for a_pt in (pts[6], pts[11]):
            for tt in (t, cv.neg(t)):
                b_pt = cv.add(tt, cv.neg(a_pt))[1]
                c = _call(cv, a_pt, b_pt)
                assert cv.add(a_pt, b_pt)[1] == tt
                marks.append(c)
        if len(marks) >= 20:
            break
    top = (p >> (8 * (L - 1))) & 255
    walk, found = pts[-1], [False, False]
    for _ in range(4000):
        nxt = cv.add(walk, cv.g)[1]
        for o in range(2):
            if not found[o] and (nxt[o] >> (8 * (L - 1))) & 255 == top:
                marks.append((0, walk, cv.g, cv.add(walk, cv.g)[0]))
                found[o] = True
        walk = nxt
        if all(found):
            break
    assert all(found), "no multiple of G with the modulus's top limb"
    fam["marks"] = marks
    # unreduced operands (the chip reads bytes, not residues): the largest quotients the record format allows
    k = (M - 1) // p - 1
    big = []
    for i in (3, 7, 12):
        op, p1, p2, lam = _call(cv, pts[i], pts[i + 5])
        if k >= 1:
            big.append((op, p1, p2, lam + k * p))
            big.append((op, (p1[0] + k * p, p1[1]), (p2[0], p2[1] + k * p), lam + k * p))
        op, p1, p2, lam = _call(cv, pts[i], pts[i])
        if k >= 1:
            big.append((op, (p1[0], p1[1] + k * p), p2, lam + k * p))
            big.append((op, (p1[0] + k * p, p1[1]), p2, lam))
    # reduced points with large slope and ordinate (the doubling's 2 l y1 is the largest reduced sum)
    best = sorted(pts, key=lambda q: -(cv.add(q, q)[0] * q[1] * 2 - 3 * q[0] * q[0]))[:3]
    big += [_call(cv, q, q) for q in best]
    best = sorted(pts, key=lambda q: (cv.add(q, q)[0] * q[1] * 2 - 3 * q[0] * q[0]))[:3]
    big += [_call(cv, q, q) for q in best]
    fam["big"] = big
    rng = _rng("ecc" + name)
    uni = []
    for i in range(24):
        i1, i2 = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        uni.append(_call(cv, pts[i1], pts[i2]))
    fam["uniform"] = uni
    for rows in fam.values():
        for op, p1, p2, lam in rows:
            assert cv.on((p1[0] % p, p1[1] % p)) and cv.on((p2[0] % p, p2[1] % p))
    return fam


def ecc_all(name, n=None):
    f = ecc_families(name)
    rows = f["mixed"] + f["slopes"] + f["marks"] + f["big"] + f["uniform"]
    return (rows * (n // len(rows) + 1))[:n] if n is not None else rows


def ecc_expected(call, cv):
    """(x3, y3) by the affine formulas on the reduced points, independent of the twin"""
    op, p1, p2, lam = call
    p = cv.p
    q1, q2 = (p1[0] % p, p1[1] % p), (p2[0] % p, p2[1] % p)
    return cv.add(q1, q1 if op == 1 else q2)[1]


def ecc_accumulators(call, p, a):
    """the three signed sums csrc/ecc.hip hands to signed_divmod (x3 from the second one enters the third)"""
    op, (x1, y1), (x2, y2), lam = call
    v1 = 2 * lam * y1 - 3 * x1 * x1 - a if op == 1 else lam * x2 - lam * x1 - y2 + y1
    v2 = lam * lam - x1 - (x1 if op == 1 else x2)
    v3 = lam * x1 - lam * (v2 % p) - y1
    return [v1, v2, v3]


def ecc_refused(name):
    """{name: call}: a slope that does not solve the chord / tangent identity, an opcode outside the chip's range"""
    cv = Curve(name)
    pts = cv.multiples(6)
    op, p1, p2, lam = _call(cv, pts[1], pts[4])
    _, d1, d2, dl = _call(cv, pts[2], pts[2])
    return {"chord_slope_plus_1": (0, p1, p2, (lam + 1) % cv.p), "tangent_slope_bit": (1, d1, d2, dl ^ (1 << 64)), "chord_as_tangent": (1, p1, p2, lam),
            "opcode_2": (2, p1, p2, lam), "opcode_big": (0x80000000, p1, p2, lam)}


@functools.lru_cache(maxsize=None)
def ecc_twin(name, family, n=None, log_h=None):
    cv = Curve(name)
    rows = ecc_all(name, n) if family == "all" else ecc_families(name)[family]
    rows = rows[:n] if n is not None else rows
    log_h = log_h if log_h is not None else max(1, (len(rows) - 1).bit_length())
    return rows, log_h, eu.twin_trace(rows, cv.p, cv.a, log_h)


# ---- fp2 -------------------------------------------------------------------------------------------------------------------------
def fp2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def fp2_inv(b, p):
    n = pow(b[0] * b[0] + b[1] * b[1], -1, p)
    return (b[0] * n % p, (-b[1]) * n % p)


@functools.lru_cache(maxsize=None)
def fp2_families(p):
    """{family: [(op, (a0, a1), (b0, b1))]} as the RECORDS hold them (op 0 mul, 1 add, 2 sub, 3 div with the quotient in the a slot)"""
    L = limbs_of(p)
    M = 1 << (8 * L)
    rng = _rng("fp2%d" % (p & 0xFFFF))
    big = lambda: _big(rng, L) % p  # noqa: E731
    x, y, s, t = big(), big(), big() | 1, big() | 1
    p0 = p & 255
    fam = {}
    # the real part a0 b0 - a1 b1 a negative exact multiple of p: reduced operands with a1 b1 = a0 b0 + k p, k > 0
    exact = []
    while len(exact) < 4:
        a0, b0, b1 = big(), big(), big() | 1
        a1 = a0 * b0 * pow(b1, -1, p) % p
        if a1 * b1 > a0 * b0:
            assert (a1 * b1 - a0 * b0) % p == 0
            exact.append((0, (a0, a1), (b0, b1)))
    exact += [(0, (0, p), (x, 3)), (0, (0, 1), (0, p)), (2, (0, x), (p, x)), (2, (p - 1, 0), (2 * p - 1 if 2 * p - 1 < M else p - 1, p))]
    fam["exact"] = exact
    fam["small"] = [(2, (x - 1, x), (x, x)), (2, (0, 0), (1, 1)), (2, (0, 0), (p - 1, p - 1)), (2, (x, y), (y, x)), (0, (0, 1), (0, 1)), (0, (1, 1), (1, 1)),
                    (0, (0, 1), (5, 1)), (0, (1, 2), (1, 3))]                                       # negative sums above -p: quotient 0 -> 1
    fam["zero"] = [(2, (x, y), (x, y)), (0, (0, 0), (x, y)), (0, (x, y), (0, 0)), (1, (0, 0), (0, 0)), (2, (0, 0), (0, 0)), (0, (1, 1), (1, p - 1)), (0, (1, 0), (1, 0)),
                   (0, (x, x), (1, 1))]
    fam["add"] = [(1, (x, p - 1 - y), (p - x, y)), (1, (1, 0), (p - 1, p - 1)), (1, (p - 1, p - 1), (p - 1, p - 1)), (1, (M - 1, M - 1), (M - 1, M - 1)),
                  (1, (p - 1, p - p0), (0, 0)), (1, (p, 0), (0, p))]
    fam["mul_big"] = [(0, (p - 1, p - 1), (p - 1, p - 1)), (0, (M - 1, M - 1), (M - 1, M - 1)), (0, (M - 1, 0), (M - 1, 0)), (0, (0, M - 1), (0, M - 1)),
                      (0, (M - 1, 0), (0, M - 1)), (0, (0, M - 1), (M - 1, 0)), (0, (p - 1, 0), (p - 1, 0)), (0, (0, p - 1), (0, p - 1)), (0, (p - 1, 1), (1, 0)),
                      (0, (p - p0, p - 1), (1, 0))]
    dv = [(p - 1, p - 1), (0, 0), (1, 0), (0, 1), (p - p0, p - p0), (x, y), (p - 1, 0), (0, p - 1)]
    fam["div"] = [(3, q, (s, t)) for q in dv] + [(3, (x, y), (1, 0)), (3, (x, y), (0, 1)), (3, (s, t), (p - 1, p - 1))]
    ops = [0, 1, 2, 3, 0, 2]
    fam["uniform"] = [(ops[i % 6], (big(), big()), (big(), big() | 1)) for i in range(24)]
    return fam


def fp2_all(p, n=None):
    f = fp2_families(p)
    rows = [r for k in ("exact", "small", "zero", "add", "mul_big", "div", "uniform") for r in f[k]]
    return (rows * (n // len(rows) + 1))[:n] if n is not None else rows


def fp2_expected(call, p):
    """(value of the r columns, value of the a columns): complex arithmetic mod p, independent of the twin.  A division row is the product
    quotient * divisor: its r columns hold the dividend, and quotient = dividend / divisor is checked through the inverse."""
    op, a, b = call
    ar, br = (a[0] % p, a[1] % p), (b[0] % p, b[1] % p)
    if op == 1:
        return ((ar[0] + br[0]) % p, (ar[1] + br[1]) % p), a
    if op == 2:
        return ((ar[0] - br[0]) % p, (ar[1] - br[1]) % p), a
    r = fp2_mul(ar, br, p)
    if op == 3 and (br[0] * br[0] + br[1] * br[1]) % p:
        assert fp2_mul(r, fp2_inv(br, p), p) == ar
    return r, a


def fp2_accumulators(call):
    op, a, b = call
    if op in (0, 3):
        return [a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]]
    return [a[0] + b[0], a[1] + b[1]] if op == 1 else [a[0] - b[0], a[1] - b[1]]


def fp2_refused(p):
    return {"div_quotient_above_p": (3, (p + 1, 0), (3, 0)), "div_quotient_is_p": (3, (5, p), (3, 1)), "opcode_4": (4, (1, 2), (3, 4)),
            "opcode_big": (0xFFFFFFFF, (1, 2), (3, 4))}


@functools.lru_cache(maxsize=None)
def fp2_twin(name, family, n=None, log_h=None):
    p = FP2_MODULI[name]
    rows = fp2_all(p, n) if family == "all" else fp2_families(p)[family]
    rows = rows[:n] if n is not None else rows
    log_h = log_h if log_h is not None else max(1, (len(rows) - 1).bit_length())
    return rows, log_h, fu.twin_trace(rows, p, log_h)


def signed_divmod_cases(v, p, L):
    """which branches of Signed<NW>::signed_divmod (csrc/limb_dev.hpp) the accumulator v takes, and the quotient's magnitude"""
    cases = set()
    q = abs(v // p)
    if v < 0 and v % p == 0:
        cases.add("neg_exact")          # neg && rem_zero: no increment, no complement
    if -p < v < 0:
        cases.add("neg_small")          # magnitude quotient 0 -> 1
    if v < 0 and v % p:
        cases.add("neg_complement")
    if v == 0:
        cases.add("zero")               # the q_zero normalisation
    if q >> (8 * L):
        cases.add("q_top")              # the quotient needs its (L + 1)-th limb (quo[NW] != 0)
    return cases, q


# ---- int256 ----------------------------------------------------------------------------------------------------------------------
M256 = 1 << 256
MIN256, MAX256 = 1 << 255, (1 << 255) - 1


def shift_cases():
    """[(op, b, c)]: op 9 sll, 10 srl, 11 sra"""
    rng = _rng("shift")
    u = _big(rng, 32)
    vals = [M256 - 1, MIN256, MAX256, 0, 1, u, u | MIN256, u & MAX256, 0x80 << 248 | 1, 0xFF]
    amounts = [0, 1, 7, 8, 9, 248, 255, 15, 16, 63, 64, 128, 247, 249, 254]
    out = [(op, b, s) for op in (9, 10, 11) for b in vals[:4] for s in amounts[:7]]
    out += [(op, b, s) for op in (9, 10, 11) for b in vals[4:] for s in (0, 1, 9, 248, 255)]
    out += [(op, u | MIN256, s) for op in (9, 10, 11) for s in amounts[7:]]
    # the amount is c mod 256: bits above bit 7, the high half of word 0 (CHI0) and the high words (CW) non-zero
    hi = [0x100, 0x1FF, 0xFF00, 0x10000, 0xFFFF0000, 1 << 32, (M256 - 1) ^ 0xFF, M256 - 1, MIN256 | 0x108, (u << 8) % M256 | 9]
    out += [(op, b, c) for op in (9, 10, 11) for b in (M256 - 1, u | MIN256) for c in hi]
    out += [(9, M256 - 1, 255), (9, 1, 255), (9, 2, 255), (9, MIN256, 1), (9, 0xFF << 248, 8)]      # everything (or all but one bit) shifted out
    return out


def cmp_cases():
    """[(op, b, c)]: op 6 sltu, 7 slt, 8 eq"""
    rng = _rng("cmp")
    u, v = _big(rng, 32), _big(rng, 32)
    neg = u | MIN256
    pairs = [(u, u), (0, 0), (M256 - 1, M256 - 1), (MIN256, MIN256), (MAX256, MAX256),                 # equal
             (u, u ^ 1), (u ^ 1, u), (u, u ^ 0x80), (u, u ^ (1 << 248)), (u ^ (1 << 248), u), (u, u ^ MIN256), (u ^ MIN256, u),   # limb 0, limb 31
             (M256 - 1, 0), (0, M256 - 1), (MIN256, MAX256), (MAX256, MIN256), (0x7F << 248, 0x80 << 248), (0x80 << 248, 0x7F << 248),
             (0x7F << 248 | u >> 8, 0x80 << 248 | u >> 8), (neg, neg ^ 1), (neg ^ 1, neg), (neg, neg ^ 0xFF00), (M256 - 1, M256 - 2), (M256 - 2, M256 - 1),
             (MIN256, MIN256 + 1), (0, 1), (1, 0), (0, MIN256), (MIN256, 0), (u, v), (v, u), (0xFF << 248, 0x01 << 248), (0x80 << 248, 0xFF << 248)]
    return [(op, b, c) for op in (6, 7, 8) for b, c in pairs]


def alu_cases():
    """[(op, b, c)]: op 0 add, 1 sub, 2 xor, 3 or, 4 and"""
    rng = _rng("alu")
    u, v = _big(rng, 32), _big(rng, 32)
    rep = int.from_bytes(b"\xff\x00" * 16, "little")
    pairs = [(M256 - 1, 1), (1, M256 - 1), (0, 1), (0, 0), (M256 - 1, M256 - 1), (0, M256 - 1), (MIN256, MIN256), (MAX256, 1), (u, v), (u, u), (u, M256 - 1 - u), (rep, rep << 8),
             (u, 0), (0, v), ((1 << 128) - 1, 1), (1 << 128, 1)]
    return [(op, b, c) for op in range(5) for b, c in pairs]


def mul_cases():
    """[(b, c)]"""
    rng = _rng("mul")
    u, v = _big(rng, 32), _big(rng, 32)
    return [(M256 - 1, M256 - 1), (u, 0), (0, u), (0, 0), (u, 1), (1, u), (u, MIN256), (MIN256, u), (MIN256, MIN256), (M256 - 1, 1), (M256 - 1, 2), (M256 - 1, MIN256),
            (u, v), (v, u), (u, M256 - 1), ((1 << 128) - 1, (1 << 128) - 1), (1 << 128, 1 << 127), (255, M256 - 1), (int.from_bytes(b"\xff" * 16, "little"), M256 - 1)]


INT256 = {"alu": (alu_cases, [(5, 1, 2), (6, 1, 2), (0xFFFFFFFF, 1, 2)]), "cmp": (cmp_cases, [(2, 1, 2), (5, 1, 2), (9, 1, 2), (12, 1, 2)]),
          "shift": (shift_cases, [(6, 1, 2), (8, 1, 2), (12, 1, 2), (0, 1, 2)])}


def int256_expected(op, b, c):
    """Python's &, |, ^, <<, >> on 256-bit values, two's complement for SLT and SRA; op 5 = mul"""
    sgn = lambda v: v - M256 if v >> 255 else v  # noqa: E731
    s = c % 256
    return {0: (b + c) % M256, 1: (b - c) % M256, 2: b ^ c, 3: b | c, 4: b & c, 5: b * c % M256, 6: int(b < c), 7: int(sgn(b) < sgn(c)), 8: int(b == c),
            9: (b << s) % M256, 10: b >> s, 11: (sgn(b) >> s) % M256}[op]


def cycle(rows, n):
    return (list(rows) * (n // len(rows) + 1))[:n]


# ---- numpy recounts of the lookup tables, from a trace's own cells ----------------------------------------------------------------
def _pairs(bw, tr, col, n_limbs, n):
    """byte pairs of the limbs at col .. col + n_limbs of the first n rows (an odd last limb pairs with 0)"""
    lim = tr[col:col + n_limbs, :n].astype(np.int64)
    if n_limbs & 1:
        lim = np.concatenate([lim, np.zeros((1, n), np.int64)])
    np.add.at(bw, (lim[0::2] * 256 + lim[1::2]).reshape(-1), 1)


def _diffs(bw, diff_row, on):
    np.add.at(bw, (((diff_row.astype(np.int64) - 1) & 255) * 256)[on], 1)


def recount_modular(tr, n, L):
    c = mu.cols(L)
    bw, tup = np.zeros(1 << 16, np.int64), np.zeros(mu.SX * mu.SY, np.int64)
    for k in ("A", "B", "Q", "R"):
        _pairs(bw, tr, c[k], L, n)
    nc = c["N_CARRY"]
    np.add.at(tup, (tr[c["CX"]:c["CX"] + nc, :n].astype(np.int64) * mu.SY + tr[c["CY"]:c["CY"] + nc, :n]).reshape(-1), 1)
    real = tr[c["REAL"], :n] == 1
    _diffs(bw, tr[c["DIFF"], :n], real)
    _diffs(bw, tr[c["DIFF2"], :n], tr[c["IS_DIV"], :n] == 1)
    return bw, tup


def recount_ecc(tr, n, L):
    c = eu.cols(L)
    bw, tup = np.zeros(1 << 16, np.int64), np.zeros(eu.SX * eu.SY, np.int64)
    for o in range(7):
        _pairs(bw, tr, L * o, L, n)
    for e in range(3):
        _pairs(bw, tr, c["Q"] + e * c["Q_LIMBS"], c["Q_LIMBS"], n)
    nc = 3 * c["N_CARRY"]
    np.add.at(tup, (tr[c["CX"]:c["CX"] + nc, :n].astype(np.int64) * eu.SY + tr[c["CY"]:c["CY"] + nc, :n]).reshape(-1), 1)
    real = tr[c["REAL"], :n] == 1
    for o in range(2):
        _diffs(bw, tr[c["DIFF"] + o, :n], real)
    return bw, tup


def recount_fp2(tr, n, L):
    c = fu.cols(L)
    bw, tup = np.zeros(1 << 16, np.int64), np.zeros(fu.SX * fu.SY, np.int64)
    for o in range(6):
        _pairs(bw, tr, L * o, L, n)
    for e in range(2):
        _pairs(bw, tr, c["Q"] + e * c["Q_LIMBS"], c["Q_LIMBS"], n)
    nc = 2 * c["N_CARRY"]
    np.add.at(tup, (tr[c["CX"]:c["CX"] + nc, :n].astype(np.int64) * fu.SY + tr[c["CY"]:c["CY"] + nc, :n]).reshape(-1), 1)
    real, is_div = tr[c["REAL"], :n] == 1, tr[c["REAL"] + 3, :n] == 1
    for e in range(2):
        _diffs(bw, tr[c["DIFF"] + e, :n], real)
        _diffs(bw, tr[c["DIFF2"] + e, :n], is_div)
    return bw, tup


def recount_alu(tr, n):
    xc = np.zeros(1 << 16, np.int64)
    a, b, c = (tr[o:o + 32, :n].astype(np.int64) for o in (0, 32, 64))
    bitwise = (tr[98, :n] + tr[99, :n] + tr[100, :n]) == 1
    np.add.at(xc, np.where(bitwise[None, :], b * 256 + c, a * 256 + a).reshape(-1), 1)
    return xc


def recount_mul(tr, n):
    bw, tup = np.zeros(1 << 16, np.int64), np.zeros(iu.SX * iu.SY, np.int64)
    for o in (0, 32, 64):
        _pairs(bw, tr, o, 32, n)
    np.add.at(tup, (tr[96:128, :n].astype(np.int64) * iu.SY + tr[128:160, :n]).reshape(-1), 1)
    return bw, tup


def recount_cmp(tr, n):
    bw = np.zeros(1 << 16, np.int64)
    _pairs(bw, tr, 0, 32, n)
    _pairs(bw, tr, 32, 32, n)
    signed = tr[101, :n] == 1
    msb = lambda col: np.where(tr[col, :n] > P_BB // 2, tr[col, :n].astype(np.int64) - P_BB, tr[col, :n].astype(np.int64))  # noqa: E731
    shift = np.where(signed, 128, 0)
    np.add.at(bw, (msb(98) + shift) * 256 + (msb(99) + shift), 1)
    _diffs(bw, tr[97, :n], tr[65:97, :n].sum(axis=0) == 1)
    return bw


def recount_shift(tr, n):
    bw, xc = np.zeros(1 << 16, np.int64), np.zeros(1 << 16, np.int64)
    bs = np.argmax(tr[145:153, :n], axis=0)
    mult1 = (1 << bs) - 1
    cy = tr[96:128, :n].astype(np.int64)
    np.add.at(bw, (cy * 256 + (mult1[None, :] - cy)).reshape(-1), 1)
    _pairs(bw, tr, 64, 32, n)
    _pairs(bw, tr, 32, 32, n)
    np.add.at(bw, tr[128, :n].astype(np.int64) * 256 + tr[129, :n], 1)
    sra = tr[188, :n] == 1
    np.add.at(xc, (tr[63, :n].astype(np.int64) * 256 + 128)[sra], 1)
    return bw, xc


# ---- proven carry bounds ---------------------------------------------------------------------------------------------------------
def carry_interval(pos_hi, pos_lo):
    """position sums s_k in [pos_lo[k], pos_hi[k]] and c_k = floor((s_k + c_(k-1)) / 256), c_(-1) = 0 -> (max over k of the upper bound, min of the lower bound).
    floor is monotone, so the bounds follow by induction over k."""
    hi = lo = 0
    best_hi, best_lo = 0, 0
    for h, l in zip(pos_hi, pos_lo):
        hi, lo = (h + hi) // 256, (l + lo) // 256
        best_hi, best_lo = max(best_hi, hi), min(best_lo, lo)
    return best_hi, best_lo


def n_terms(k, n_i, n_j):
    """pairs (i, j) with i + j = k, 0 <= i < n_i, 0 <= j < n_j"""
    return max(0, min(k, n_i - 1) - max(0, k - n_j + 1) + 1)


def modular_carry_bounds(p):
    """{identity: (hi, lo)} of the modular chip: position k of (a b | a + b | a - b) -+ q P - r; limbs in [0, 255], the modulus's limbs as they are"""
    L = limbs_of(p)
    pb = list(p.to_bytes(L, "little"))
    qp = [sum(255 * pb[k - i] for i in range(L) if 0 <= k - i < L) for k in range(2 * L - 1)]       # q's limbs at 255
    out = {}
    for name in ("mul", "add", "sub"):
        hi, lo = [], []
        for k in range(2 * L - 1):
            inner = k < L
            if name == "mul":
                h, l = n_terms(k, L, L) * 255 * 255, -qp[k] - (255 if inner else 0)
            elif name == "add":
                h, l = (510 if inner else 0), -qp[k] - (255 if inner else 0)
            else:   # a - b + q P - r with q in {0, 1}: q's limb 0 at most 1
                h, l = (255 if inner else 0) + (pb[k] if inner else 0), -(510 if inner else 0)
            hi.append(h), lo.append(l)
        out[name] = carry_interval(hi, lo)
    return out


def signed_carry_bounds(p, chip):
    """{identity: (hi, lo)} of the ecc / fp2 chips: the quotient (L + 1 limbs in [0, 255]) enters with either sign"""
    L = limbs_of(p)
    pb = list(p.to_bytes(L, "little"))
    qp = [sum(255 * pb[k - i] for i in range(L + 1) if 0 <= k - i < L) for k in range(2 * L)]
    sq = 255 * 255
    if chip == "ecc":   # (products with +, products with -, plain limbs with +, plain limbs with -) per position
        ids = {"slope_chord": (1, 1, 1, 1), "slope_tangent": (2, 3, 0, 1), "x3": (1, 0, 0, 3), "y3": (1, 1, 0, 2)}
    else:
        ids = {"mul_re": (1, 1, 0, 1), "mul_im": (2, 0, 0, 1), "add": (0, 0, 2, 1), "sub": (0, 0, 1, 2)}
    out = {}
    for name, (pp, pn, wp, wn) in ids.items():
        hi, lo = [], []
        for k in range(2 * L):
            t, inner = n_terms(k, L, L), k < L
            hi.append(pp * t * sq + (wp * 255 if inner else 0) + qp[k])
            lo.append(-pn * t * sq - (wn * 255 if inner else 0) - qp[k])
        out[name] = carry_interval(hi, lo)
    return out


def mul256_carry_bound():
    hi = [n_terms(k, 32, 32) * 255 * 255 for k in range(32)]
    return carry_interval(hi, [0] * 32)


def observed_carries(tr, n, cx, cy, count, offset):
    v = tr[cx:cx + count, :n].astype(np.int64) + 256 * tr[cy:cy + count, :n].astype(np.int64) - offset
    return int(v.max()), int(v.min())


# ---- keccak / sha256 -------------------------------------------------------------------------------------------------------------
def keccak_states():
    """{name: 25 lanes}: all-zero, all-one, single-bit states"""
    one = np.zeros(25, np.uint64)
    one[0] = 1
    top = np.zeros(25, np.uint64)
    top[24] = np.uint64(1 << 63)
    mid = np.zeros(25, np.uint64)
    mid[12] = np.uint64(1 << 31)
    return {"zero": np.zeros(25, np.uint64), "ones": np.full(25, np.uint64((1 << 64) - 1)), "bit0": one, "bit1599": top, "bit_mid": mid}


def sha256_records():
    """{name: (H_in[8] | M[16])}: all-zero, all-one and single-bit blocks and states"""
    from sha256_util import IV
    z8, z16, f8, f16 = [0] * 8, [0] * 16, [0xFFFFFFFF] * 8, [0xFFFFFFFF] * 16
    b0 = [0x80000000] + [0] * 15
    b511 = [0] * 15 + [1]
    rec = {"iv_zero_block": IV + z16, "iv_ones_block": IV + f16, "zero_state_zero_block": z8 + z16, "ones_state_ones_block": f8 + f16, "iv_bit0": IV + b0,
           "iv_bit511": IV + b511, "bit_state_zero_block": [1] + [0] * 7 + z16, "top_bit_state": [0] * 7 + [0x80000000] + z16}
    return {k: np.array(v, dtype=np.uint32) for k, v in rec.items()}
