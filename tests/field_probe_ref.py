"""The reference and the operand sets of the field probe (tests/field_probe.hip), shared by test_field_probe_cpu.py (host forms, g++)
and test_gpu_field_probe.py (device forms, hipcc).

Python integers only.  A raw word r stands for the field element r * 2^-32 mod p (Montgomery form, R = 2^32); the extension is
F_p[x] / (x^4 - 11).  Nothing here comes from tests/pymodel.py; the permutation alone is cross-checked against it by the tests.
For every operation the check is (a) the exact word where the header promises a canonical result, the congruence mod p otherwise,
and (b) the range the header's comment promises for the raw word."""
import itertools
import os
import random
import re
import struct
import subprocess

P = 2013265921
R = 1 << 32
RINV = pow(R, -1, P)
MONTY_ONE = R % P
MONTY_R2 = R * R % P
W = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkvm-prover_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "field_probe.hip")
MAGIC = 0x31425046

OPS = ("red_2p mmul_lazy mmul madd msub mneg smml canon_signed center_signed smred64 canon_signed_wide mred64 lazyacc to_monty "
       "from_monty mpow minv ext_add ext_sub ext_mul ext_mul_base ext_frobenius ext_inv mdouble mhalve mdiv2 mdiv3 mdiv4 mdiv8 mdiv27 "
       "sbox7 sbox7_rcs sbox7_rc p2_external p2_internal p2_permute ext_neg ext_sqr ext_pow two_adic_gen bitrev32 p2_compress "
       "p2_hash_slice monty_roundtrip").split()
OP = {name: i + 1 for i, name in enumerate(OPS)}
PLAIN = "red_2p canon_signed center_signed mhalve mdouble mdiv2 mdiv3 mdiv4 mdiv8 mdiv27 sbox7 identity".split()
OP.update({"plain_" + name: 100 + i for i, name in enumerate(PLAIN)})
OUTW = {"ext_add": 4, "ext_sub": 4, "ext_mul": 4, "ext_mul_base": 4, "ext_frobenius": 4, "ext_inv": 4, "ext_neg": 4, "ext_sqr": 4, "ext_pow": 4,
        "p2_external": 16, "p2_internal": 16, "p2_permute": 16, "p2_compress": 8, "p2_hash_slice": 8}

# ---- the boundary set B of raw words (all in [0, p)) --------------------------------------------------------------------------
_B = [0, 1, 2, 3, P - 1, P - 2, P - 3, (P - 1) // 2 - 1, (P - 1) // 2, (P + 1) // 2, (P + 1) // 2 + 1,
      MONTY_ONE - 1, MONTY_ONE, MONTY_ONE + 1, P - MONTY_ONE - 1, P - MONTY_ONE, P - MONTY_ONE + 1, MONTY_R2,
      (1 << 27) - 1, 1 << 27, (1 << 27) + 1, 15 << 27, 14 << 27, (14 << 27) + 1, 1 << 28, 1 << 29, (1 << 30) - 1, 1 << 30, (1 << 30) + 1,
      0x2AAAAAAA, 0x55555555 % P, 0x77FFFFFF, 0x78000000, W * R % P]
B = sorted(set(_B))
assert all(0 <= b < P for b in B)


def u32(x):
    return x & 0xFFFFFFFF


def s32(w):
    return w - (1 << 32) if w >= 1 << 31 else w


def lohi(t):
    t &= (1 << 64) - 1
    return [t & 0xFFFFFFFF, t >> 32]


def uniform(rng, n, hi=P, lo=0):
    return [rng.randrange(lo, hi) for _ in range(n)]


# ---- the extension, on raw words ------------------------------------------------------------------------------------------------
def val(r):
    return r * RINV % P


def raw(v):
    return v * R % P


def emul_v(a, b):   # on values
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return [(c[k] + W * (c[k + 4] if k < 3 else 0)) % P for k in range(4)]


def epow_v(a, e):
    r = [1, 0, 0, 0]
    while e:
        if e & 1:
            r = emul_v(r, a)
        a = emul_v(a, a)
        e >>= 1
    return r


def on_vals(f, *raws):
    return [raw(x) for x in f(*[[val(w) for w in r] for r in raws])]


# ---- Poseidon2 on raw words -------------------------------------------------------------------------------------------------------
def round_constants_raw():
    text = open(os.path.join(CSRC, "poseidon2_rc.inc")).read()
    rc = [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]{8})u", text)]
    assert len(rc) == 141
    return rc


_M4 = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
_I2 = (P + 1) // 2
_DIAG = [-2, 1, 2, _I2, 3, 4, -_I2, -3, -4, pow(_I2, 8, P), pow(_I2, 2, P), pow(_I2, 3, P), pow(_I2, 27, P), -pow(_I2, 8, P), -pow(_I2, 4, P),
         -pow(_I2, 27, P)]


def external_linear(s):   # linear with integer coefficients: the same map on raw words as on values
    t = []
    for b in range(0, 16, 4):
        t += [sum(_M4[i][j] * s[b + j] for j in range(4)) % P for i in range(4)]
    col = [(t[k] + t[4 + k] + t[8 + k] + t[12 + k]) % P for k in range(4)]
    return [(t[i] + col[i % 4]) % P for i in range(16)]


def internal_linear(s):
    tot = sum(s)
    return [(tot + _DIAG[i] * s[i]) % P for i in range(16)]


def sbox_raw(x):   # Montgomery x^7: seven factors, six reductions
    return pow(x, 7, P) * pow(RINV, 6, P) % P


def permute_raw(s, rc=None):
    rc = rc or round_constants_raw()
    s = external_linear(list(s))
    for r in range(4):
        s = external_linear([sbox_raw(s[i] + rc[16 * r + i]) for i in range(16)])
    for r in range(13):
        s[0] = sbox_raw(s[0] + rc[64 + r])
        s = internal_linear(s)
    for r in range(4):
        s = external_linear([sbox_raw(s[i] + rc[77 + 16 * r + i]) for i in range(16)])
    return s


def hash_slice_raw(xs, rc):
    s = [0] * 16
    for i in range(0, len(xs), 8):
        chunk = xs[i:i + 8]
        s[:len(chunk)] = chunk
        s = permute_raw(s, rc)
    return s[:8]


# ---- jobs: (name, items, check) ------------------------------------------------------------------------------------------------
# check(item, out_words) raises AssertionError with the operands in its message
def _exact(f):
    def check(item, out):
        exp = f(*item)
        exp = exp if isinstance(exp, list) else [exp]
        assert out == exp, (item, out, exp)
    return check


def _mmul_lazy_check(item, out):
    a, b = item
    t = a * b
    assert t + (R - 1) * P < 1 << 64, "operand outside the precondition"
    r = out[0]
    assert r % P == t * RINV % P, (item, r)
    assert r * R - t >= 0 and (r * R - t) % P == 0 and (r * R - t) // P < R, (item, r)   # r = (t + m p) / 2^32 exactly, no wrap
    assert r < t // R + P + 1, (item, r)
    if t <= R * P:   # both operands in [0, p], or one below 2^32 and the other at most p: the [0, 2p) the callers count on
        assert r < 2 * P, (item, r)


def _smml_check(item, out):
    a, b = s32(item[0]), s32(item[1])
    assert -P <= a <= P and -P <= b <= P
    d = s32(out[0])
    assert (d - a * b * RINV) % P == 0, (a, b, d)
    assert abs(d) * 100 < 97 * P, (a, b, d)                      # "operands in [-p, p] give |d| < 0.97 p"
    assert abs(d) * R <= abs(a * b) + R * P // 2 + R, (a, b, d)  # |d| <= |ab| / 2^32 + p/2


def _smred64_check(item, out):
    t = item[0] | item[1] << 32
    t = t - (1 << 64) if t >= 1 << 63 else t
    assert abs(t) * 100 < 121 * P * P
    d = s32(out[0])
    assert (d - t * RINV) % P == 0, (t, d)
    assert abs(d) * R <= abs(t) + R * P // 2 + R, (t, d)       # |d| <= |t| / 2^32 + p/2, which for |t| < 1.21 p^2 is < 2^31
    assert abs(d) < 1 << 31


def _center_check(item, out):
    d = s32(out[0])
    assert (d - item[0]) % P == 0 and -(P - 1) // 2 <= d <= (P - 1) // 2, (item, d)
    assert -P // 2 < d <= P // 2, (item, d)


def _ext_inv_check(item, out):
    a = list(item)
    assert all(0 <= w < P for w in out), (item, out)
    if not any(a):
        assert out == [0, 0, 0, 0], (item, out)
    else:
        assert on_vals(emul_v, a, out) == [MONTY_ONE, 0, 0, 0], (item, out)


def signed_words(mags):
    return sorted({u32(s * m) for m in mags for s in (1, -1)})


def prover_opening_shapes():
    """The second smred64 of the opening kernel (csrc/prover.hip): d1 * MONTY_ONE + four products of centred words, |.| <= 1.13 p^2."""
    h, d1 = (P - 1) // 2, 97 * P // 100
    out = []
    for signs in itertools.product((1, -1), repeat=5):
        for mag in (h, h - 1):
            out.append(signs[0] * d1 * MONTY_ONE + sum(s * mag * h for s in signs[1:]))
    return out


def build_jobs(seed=20240607, n_uniform=4000):
    rng = random.Random(seed)
    rc = round_constants_raw()
    jobs = []

    def add(name, items, check, op=None):
        jobs.append((name, op or name, [tuple(it) for it in items], check))

    pairs = list(itertools.product(B, B)) + list(zip(uniform(rng, n_uniform), uniform(rng, n_uniform)))
    ones = [(b,) for b in B] + [(x,) for x in uniform(rng, n_uniform)]

    # red_2p: [0, 2p) reduces; [2p, 2^32) comes back as x - p (documented: the lazy S-box relies on it)
    low = sorted(set(B + [P + b for b in B] + [P, P + 1, 2 * P - 1, 2 * P - 2] + uniform(rng, n_uniform, 2 * P)))
    high = sorted(set([2 * P, 2 * P + 1, R - 1, R - 2, 1 << 31 | 1 << 27, 0xF0000002, 0xF0000003] + uniform(rng, 500, R, 2 * P)))
    for name in ("red_2p", "plain_red_2p"):
        add(name + "[0,2p)", [(x,) for x in low], _exact(lambda x: x % P), name)
        add(name + "[2p,2^32)", [(x,) for x in high], _exact(lambda x: x - P), name)

    # mmul_lazy: B x B, uniform, and the precondition limit a*b + (2^32 - 1) p < 2^64 for operands above p
    lim = (1 << 64) - 1 - (R - 1) * P
    edge = []
    for a in (2 * P - 1, 2 * P - 2, 2 * P, R - 1, 1 << 31, P, P + 1, 3 * P // 2):
        bmax = min(R - 1, lim // a)
        edge += [(a, bmax), (bmax, a), (a, bmax - 1), (a, bmax - 2)]
    add("mmul_lazy", pairs + edge + [(P, P), (R - 1, P), (P, R - 1)], _mmul_lazy_check)
    add("mmul", pairs, _exact(lambda a, b: a * b * RINV % P))
    add("madd", pairs, _exact(lambda a, b: (a + b) % P))
    add("msub", pairs, _exact(lambda a, b: (a - b) % P))
    add("mneg", ones, _exact(lambda a: -a % P))

    # signed forms: every sign combination of magnitudes in [0, p]
    sw = signed_words(B + [P])
    spairs = list(itertools.product(sw, sw)) + [(u32(rng.randrange(-P, P + 1)), u32(rng.randrange(-P, P + 1))) for _ in range(n_uniform)]
    add("smml", spairs, _smml_check)
    cs = [(w,) for w in signed_words(B)] + [(u32(rng.randrange(-P + 1, P)),) for _ in range(n_uniform)]
    for name in ("canon_signed", "plain_canon_signed"):
        add(name, cs, _exact(lambda w: s32(w) % P), name)
    for name in ("center_signed", "plain_center_signed"):
        add(name, ones, _center_check, name)
    t_lim = 12099 * P * P // 10000
    ts = [0, 1, -1, t_lim, -t_lim, t_lim - 1, 1 - t_lim, P * P, -P * P, (P - 1) ** 2, -(P - 1) ** 2] + prover_opening_shapes()
    ts += [a * b for a, b in itertools.product([s32(w) for w in sw], repeat=2)]
    ts += [rng.randrange(-t_lim, t_lim + 1) for _ in range(n_uniform)]
    add("smred64", [lohi(t) for t in ts], _smred64_check)
    wide = signed_words(B + [P + b for b in B if P + b < 1 << 31] + [(1 << 31) - 1, 2 * P - (1 << 31)]) + [1 << 31]
    wide += [u32(rng.randrange(-(1 << 31), 1 << 31)) for _ in range(n_uniform)]
    add("canon_signed_wide", [(w,) for w in wide], _exact(lambda w: s32(w) % P))

    # mred64: t < 4 p^2
    t4 = [0, 1, P, P * P, 4 * (P - 1) ** 2, 4 * P * P - 1, 4 * P * P - P, P * R - 1, P * R, P * R + 1, (P + 1) * R - 1]   # all < 4 p^2
    assert all(t < 4 * P * P for t in t4)
    t4 += [k * a * b for (a, b) in itertools.product(B, B) for k in (1, 4)]
    t4 += [sum(rng.choice(B) * rng.choice(B) for _ in range(rng.randrange(1, 5))) for _ in range(n_uniform)]
    t4 += uniform(rng, n_uniform, 4 * P * P)
    add("mred64", [lohi(t) for t in t4], _exact(lambda lo, hi: (lo | hi << 32) * RINV % P))
    # LazyAcc: 10^5 and 2^22 maximal groups (a group is a sum of four products of residues: at most 4 (p-1)^2)
    gmax = 4 * (P - 1) ** 2
    acc = [(gmax, gmax, 50000), (gmax, gmax, 1 << 21), (gmax, gmax - 1, 1 << 20), (0, 1, 3), (gmax, 0, 0), (R - 1, R, 77777)]
    acc += [(rng.randrange(4 * P * P), rng.randrange(4 * P * P), rng.randrange(1, 5000)) for _ in range(40)]
    add("lazyacc", [lohi(a) + lohi(b) + [n] for a, b, n in acc],
        _exact(lambda al, ah, bl, bh, n: n * ((al | ah << 32) + (bl | bh << 32)) * RINV % P))

    add("to_monty", ones, _exact(lambda x: x * R % P))
    add("from_monty", ones, _exact(lambda x: x * RINV % P))
    add("monty_roundtrip", ones, _exact(lambda x: x))
    add("plain_identity", ones, _exact(lambda x: x))
    exps = [0, 1, 2, 3, P - 2, P - 1, P, (1 << 64) - 1, 1 << 63, 0x5555555555555555]
    add("mpow", [(a,) + tuple(lohi(e)) for a in B for e in exps], _exact(lambda a, lo, hi: raw(pow(val(a), lo | hi << 32, P))))
    add("minv", ones, _exact(lambda a: raw(pow(val(a), P - 2, P))))

    # the extension: coefficients from B only (all p-1 included), constants c^4, base-field elements
    els = [(c,) * 4 for c in B] + [(c, 0, 0, 0) for c in B] + [tuple(rng.choice(B) for _ in range(4)) for _ in range(300)]
    top = (P - 1,) * 4
    epairs = [(top, top)] + [(rng.choice(els), rng.choice(els)) for _ in range(3000)] + [(e, top) for e in els[:len(B)]]
    epairs += [(tuple(uniform(rng, 4)), tuple(uniform(rng, 4))) for _ in range(500)]
    flat = [a + b for a, b in epairs]
    add("ext_add", flat, _exact(lambda *w: [(x + y) % P for x, y in zip(w[:4], w[4:])]))
    add("ext_sub", flat, _exact(lambda *w: [(x - y) % P for x, y in zip(w[:4], w[4:])]))
    add("ext_mul", flat, _exact(lambda *w: on_vals(emul_v, w[:4], w[4:])))
    add("ext_mul_base", [e + (b,) for e in els[:80] for b in B], _exact(lambda *w: [x * w[4] * RINV % P for x in w[:4]]))
    add("ext_neg", els, _exact(lambda *w: [-x % P for x in w]))
    add("ext_sqr", els, _exact(lambda *w: on_vals(emul_v, w, w)))
    some = els[:len(B)] + els[2 * len(B):2 * len(B) + 40]
    add("ext_frobenius", some, _exact(lambda *w: on_vals(lambda a: epow_v(a, P), w)))
    add("ext_pow", [e + tuple(lohi(x)) for e in some[::3] for x in (0, 1, 2, P, (1 << 64) - 1)],
        _exact(lambda *w: on_vals(lambda a: epow_v(a, w[4] | w[5] << 32), w[:4])))
    # ext_inv: also elements of norm 1, b^(p-1) = frobenius(b) / b
    norm1 = []
    for e in els[2 * len(B):2 * len(B) + 12] + [top]:
        v = [val(x) for x in e]
        if any(v):
            norm1.append(tuple(raw(x) for x in epow_v(v, P - 1)))
    for e in norm1:
        n = epow_v([val(x) for x in e], 1 + P + P * P + P ** 3)
        assert n == [1, 0, 0, 0]
    add("ext_inv", els + norm1 + [tuple(uniform(rng, 4)) for _ in range(200)], _ext_inv_check)

    add("mdouble", ones, _exact(lambda x: 2 * x % P))
    add("plain_mdouble", ones, _exact(lambda x: 2 * x % P))
    for k, name in ((1, "mhalve"), (2, "mdiv2"), (3, "mdiv3"), (4, "mdiv4"), (8, "mdiv8"), (27, "mdiv27")):
        mults = [(x,) for x in (1 << k, (1 << k) - 1, (1 << k) + 1, P - (1 << k), ((P - 1) >> k) << k)]
        for nm in (name, "plain_" + name):
            add(nm, ones + mults, _exact(lambda x, k=k: x * pow(2, -k, P) % P), nm)
    add("sbox7", ones, _exact(sbox_raw))
    add("plain_sbox7", ones, _exact(sbox_raw))
    rcp = list(itertools.product(B, B)) + [(rng.choice(B), c) for c in rc] + list(zip(uniform(rng, n_uniform), uniform(rng, n_uniform)))
    add("sbox7_rc", rcp, _exact(lambda s, c: sbox_raw(s + c)))
    add("sbox7_rcs", [(s, u32(c - P)) for s, c in rcp], _exact(lambda s, cs: sbox_raw(s + s32(cs))))   # the signed word rc - p

    # the permutation and its layers: constant states c^16, states drawn from B, one lane differing, uniform
    states = [(c,) * 16 for c in B] + [tuple(rng.choice(B) for _ in range(16)) for _ in range(300)]
    states += [tuple(P - 1 if i != k else 0 for i in range(16)) for k in range(16)] + [tuple(0 if i != k else P - 1 for i in range(16)) for k in range(16)]
    states += [tuple(rng.choice((0, P - 1)) for _ in range(16)) for _ in range(100)] + [tuple(uniform(rng, 16)) for _ in range(200)]
    add("p2_external", states, _exact(lambda *s: external_linear(s)))
    add("p2_internal", states, _exact(lambda *s: internal_linear(s)))
    add("p2_permute", states, _exact(lambda *s: permute_raw(s, rc)))
    add("p2_compress", states[:len(B) + 60], _exact(lambda *s: permute_raw(s, rc)[:8]))
    sl = [(n,) + tuple(rng.choice(B) if k < n else 0xFFFFFFFF for k in range(24)) for n in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24) for _ in range(3)]
    add("p2_hash_slice", sl, _exact(lambda n, *w: hash_slice_raw(list(w[:n]), rc)))

    def gen(bits):
        g = pow(31, (P - 1) >> bits, P)   # 31 generates F_p^*: any element of exact order 2^bits serves the check below
        return g
    def two_adic_check(item, out):
        bits, g = item[0], val(out[0])
        assert out[0] < P and pow(g, 1 << bits, P) == 1 and (bits == 0 or pow(g, 1 << (bits - 1), P) == P - 1), (item, out)
        assert g == pow(0x1A427A41, 1 << (27 - bits), P), (item, out)
    assert pow(gen(27), 1 << 26, P) == P - 1 and pow(0x1A427A41, 1 << 26, P) == P - 1
    add("two_adic_gen", [(b,) for b in range(28)], two_adic_check)
    br = [(x & ((1 << b) - 1), b) for b in (0, 1, 2, 5, 12, 27, 31, 32) for x in (0, 1, 2, 5, (1 << b) - 1, 0x12345678, 0x80000001)]
    add("bitrev32", br, _exact(lambda x, b: int(format(x, "0%db" % b)[::-1], 2) if b else 0))
    return jobs


# ---- exhaustive passes: (fast, plain, start, count, bias).  index = start + k * stride, operand word = u32(index - bias) --------
def exhaustive_jobs(stride):
    def span(lo, hi):   # indices lo, lo + stride, ... below hi
        return lo, (hi - lo + stride - 1) // stride
    full = [("red_2p", "plain_red_2p", 0, R, 0),
            ("canon_signed", "plain_canon_signed", 0, 2 * P - 1, P - 1)]       # d = index - (p - 1) over (-p, p)
    full += [(name, "plain_" + name, 0, P, 0) for name in ("center_signed", "mhalve", "mdouble", "mdiv2", "mdiv3", "mdiv4", "mdiv8", "mdiv27", "sbox7")]
    full += [("monty_roundtrip", "plain_identity", 0, P, 0)]
    return [(f, pl) + span(lo, hi) + (stride, bias) for f, pl, lo, hi, bias in full]


def write_jobs(path, jobs, exh):
    words = [MAGIC, len(jobs) + len(exh)]
    for _, op, items, _ in jobs:
        words += [0, OP[op], len(items)]
        for it in items:
            words += it
    for f, pl, start, count, stride, bias in exh:
        words += [1, OP[f], OP[pl]] + lohi(start) + lohi(count) + [stride, bias]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<%dI" % len(words), *words))


def check_results(path, jobs, exh):
    data = open(path, "rb").read()
    words = struct.unpack("<%dI" % (len(data) // 4), data)
    assert words[0] == MAGIC and words[1] == len(jobs) + len(exh)
    pos, seen = 2, {}
    for name, op, items, check in jobs:
        w = OUTW.get(op, 1)
        for it in items:
            check(it, list(words[pos:pos + w]))
            pos += w
        seen[name] = len(items)
    for f, pl, start, count, stride, bias in exh:
        bad, first = words[pos] | words[pos + 1] << 32, words[pos + 2] | words[pos + 3] << 32
        assert bad == 0, "%s differs from %s at %d of %d operands, first at operand word 0x%08x" % (f, pl, bad, count, u32(first - bias))
        pos += 4
        seen["exhaustive " + f] = count
    assert pos == len(words)
    return seen


def run_probe(exe, workdir, stride, timeout):
    """Writes the operand file, runs the probe ONCE as a child process, checks every result; returns {job: operands seen}."""
    jobs, exh = build_jobs(), exhaustive_jobs(stride)
    fin, fout = os.path.join(str(workdir), "operands.bin"), os.path.join(str(workdir), "results.bin")
    write_jobs(fin, jobs, exh)
    try:
        out = subprocess.run([str(exe), fin, fout], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:   # the probe names every finished job with its time on stderr: the last line is the step before the slow one
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        raise AssertionError("the probe ran longer than %d s; its last lines:\n%s" % (timeout, err[-1500:]))
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    slow = sorted(((float(l.rsplit(":", 1)[1].split()[0]), l) for l in out.stderr.splitlines() if l.startswith("job ")), reverse=True)
    print("probe: slowest jobs:", [l for _, l in slow[:4]])
    return check_results(fout, jobs, exh)


def cross_check_permutation_with_pymodel():
    """The raw-word permutation above against the independent canonical-form model, at boundary states."""
    import pymodel

    rc = round_constants_raw()
    assert [val(c) for c in rc] == list(pymodel.RC)
    rng = random.Random(1)
    for s in [(P - 1,) * 16, (0,) * 16, (MONTY_ONE,) * 16, tuple(rng.choice(B) for _ in range(16)), tuple(uniform(rng, 16))]:
        assert [val(x) for x in permute_raw(s, rc)] == list(pymodel.permute([val(x) for x in s]))
