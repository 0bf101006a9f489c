"""The reduced-opening chip in Python integers (air.reduced_opening_air, zkhip_reduced_opening_host / _tracegen): the twin the CPU and
GPU tests compare with, and the call sets they share.  ro is the DIRECT power sum  sum_i alpha^i (b_i - a_i); the trace's accumulator
column runs by Horner from the last element, and trace() insists that the two meet on every call's last row -- they agree by algebra,
not by shared code.  A call is (alpha[4], a[L], b[L][4]) of canonical integers.  Test infrastructure."""
import numpy as np

P = 2013265921
W = 11   # X^4 = 11
WIDTH = 18
ALPHA, A, B, ACC, IDX, FIRST, LAST, REAL, CALL = 0, 4, 5, 9, 13, 14, 15, 16, 17
PMAX = (P - 1,) * 4


def ext_mul(x, y):
    x0, x1, x2, x3 = x
    y0, y1, y2, y3 = y
    return ((x0 * y0 + W * (x1 * y3 + x2 * y2 + x3 * y1)) % P, (x0 * y1 + x1 * y0 + W * (x2 * y3 + x3 * y2)) % P,
            (x0 * y2 + x1 * y1 + x2 * y0 + W * x3 * y3) % P, (x0 * y3 + x1 * y2 + x2 * y1 + x3 * y0) % P)


def term(a, b):
    """b - a: the base cell leaves coordinate 0 only"""
    return ((b[0] - a) % P, b[1], b[2], b[3])


def power_sum(alpha, a, b):
    """ro = sum_i alpha^i (b_i - a_i)"""
    ro, pw, alpha = [0, 0, 0, 0], (1, 0, 0, 0), tuple(int(x) for x in alpha)
    for ai, bi in zip(a, b):
        t = ext_mul(pw, term(int(ai), [int(x) for x in bi]))
        ro = [(r + c) % P for r, c in zip(ro, t)]
        pw = ext_mul(pw, alpha)
    return tuple(ro)


def trace(calls, log_height, check=True):
    """[18, 2^log_height] canonical uint32: call c on consecutive rows, row t of it holding element L - 1 - t; check: the accumulator of
    every call's last row is power_sum() of the call"""
    t = np.zeros((WIDTH, 1 << log_height), np.uint32)
    r = 0
    for c, (alpha, a, b) in enumerate(calls):
        L = len(a)
        assert L >= 1 and len(b) == L
        alpha = tuple(int(x) for x in alpha)
        acc = (0, 0, 0, 0)
        for k in range(L):
            ai, bi = int(a[L - 1 - k]), [int(x) for x in b[L - 1 - k]]
            d = term(ai, bi)
            acc = d if k == 0 else tuple((m + v) % P for m, v in zip(ext_mul(acc, alpha), d))
            t[ALPHA:ALPHA + 4, r], t[A, r], t[B:B + 4, r], t[ACC:ACC + 4, r] = alpha, ai, bi, acc
            t[IDX, r], t[FIRST, r], t[LAST, r], t[REAL, r], t[CALL, r] = k, k == 0, k == L - 1, 1, c
            r += 1
        if check:
            assert acc == power_sum(alpha, a, b)
    return t


def _ext_mul_np(x, y):
    """ext_mul on [4][n] uint64 arrays of canonical words (every product reduced before it is summed: p^2 fits 64 bits, 4 p^2 does not)"""
    m = lambda i, j: x[i] * y[j] % P  # noqa: E731
    return np.stack([(m(0, 0) + W * ((m(1, 3) + m(2, 2) + m(3, 1)) % P)) % P, (m(0, 1) + m(1, 0) + W * ((m(2, 3) + m(3, 2)) % P)) % P,
                     (m(0, 2) + m(1, 1) + m(2, 0) + W * m(3, 3)) % P, (m(0, 3) + m(1, 2) + m(2, 1) + m(3, 0)) % P])


def trace_np(alpha, lens, a, b, log_height):
    """trace() from the generator's arrays (records()), in numpy: for call counts that Python integers are too slow for.  Row t of every
    call at once, t = 0, 1, ..: as many steps as the longest call has rows.  tests/test_reduced_opening_cpu.py holds it against trace()."""
    alpha, lens = np.asarray(alpha, np.uint64).reshape(-1, 4), np.asarray(lens, np.int64)
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64).reshape(-1, 4)
    n, off = int(lens.sum()), np.concatenate([[0], np.cumsum(lens)])
    call = np.repeat(np.arange(len(lens)), lens)
    idx = np.arange(n) - off[call]
    elem = off[call + 1] - 1 - idx
    t = np.zeros((WIDTH, 1 << log_height), np.uint64)
    t[ALPHA:ALPHA + 4, :n], t[A, :n], t[B:B + 4, :n] = alpha[call].T, a[elem], b[elem].T
    t[IDX, :n], t[FIRST, :n], t[LAST, :n], t[REAL, :n], t[CALL, :n] = idx, idx == 0, idx == lens[call] - 1, 1, call
    term = t[B:B + 4, :n].copy()
    term[0] = (term[0] + P - t[A, :n]) % P
    acc = term.copy()
    for k in range(1, int(lens.max()) if len(lens) else 0):
        rows = np.nonzero(idx == k)[0]
        acc[:, rows] = (_ext_mul_np(acc[:, rows - 1], t[ALPHA:ALPHA + 4, rows]) + term[:, rows]) % P
    t[ACC:ACC + 4, :n] = acc
    return t.astype(np.uint32)


def records(calls):
    """the generator's arrays: alpha [n_calls][4], len [n_calls], a [n_elems], b [n_elems][4] (uint32)"""
    alpha = np.array([c[0] for c in calls], np.uint32).reshape(-1, 4)
    lens = np.array([len(c[1]) for c in calls], np.uint32)
    a = np.concatenate([np.asarray(c[1], np.uint32) for c in calls]) if calls else np.zeros(0, np.uint32)
    b = np.concatenate([np.asarray(c[2], np.uint32).reshape(-1, 4) for c in calls]) if calls else np.zeros((0, 4), np.uint32)
    return alpha, lens, a, b


def random_call(rng, L, alpha=None):
    al = rng.integers(0, P, 4, dtype=np.int64) if alpha is None else alpha
    return (tuple(int(x) for x in al), rng.integers(0, P, L, dtype=np.int64).tolist(), rng.integers(0, P, (L, 4), dtype=np.int64).tolist())


def random_calls(rng, lengths):
    return [random_call(rng, L) for L in lengths]


def boundary_calls():
    """every boundary alpha (0, 1, all p - 1, and a seeded one) at every length 1, 2, 5, 300, with the boundary cells spread over the
    elements: a = 0, a = p - 1 under b_0 = 0 (the subtraction wraps), b = p - 1 in every coordinate"""
    rng = np.random.default_rng(41)
    calls = []
    for alpha in ((0, 0, 0, 0), (1, 0, 0, 0), PMAX, None):
        for L in (1, 2, 5, 300):
            al, a, b = random_call(rng, L, alpha)
            for i in range(L):
                kind = (i + L) % 4
                if kind == 0:
                    a[i] = 0
                elif kind == 1:
                    a[i], b[i][0] = P - 1, 0
                elif kind == 2:
                    b[i] = list(PMAX)
            calls.append((al, a, b))
    return calls


def call_sets(W_ROWS, which=None):
    """name -> (log_height, calls), seeded.  W_ROWS: the rows a workgroup of the generator covers at a time."""
    rng = np.random.default_rng(7)
    sets = {}
    # 2^6 rows exactly full (1 + 1 + 2 + 60 = 64)
    sets["full_64"] = (6, random_calls(rng, [1, 1, 2, 60]))
    # one call across a wave, then single rows, then padding
    sets["wave_crossing"] = (8, random_calls(rng, [65] + [1] * 100))
    # one call of 2 W + 3 rows across two boundaries (of a pass and of a workgroup's two passes), one that ends exactly on a boundary, one
    # that starts on it and ends on the next workgroup's, one that starts there
    L0 = 10
    sets["block_crossing"] = (11, random_calls(rng, [L0, 2 * W_ROWS + 3, 3 * W_ROWS - (L0 + 2 * W_ROWS + 3), W_ROWS, W_ROWS + 44]))
    if which == "cpu":
        return sets
    sets["one_call_4096"] = (12, random_calls(rng, [1 << 12]))
    sets["4096_calls_of_1"] = (12, random_calls(rng, [1] * (1 << 12)))
    sets["one_row_padded"] = (1, random_calls(rng, [1]))
    sets["one_row"] = (0, random_calls(rng, [1]))
    lens, left = [], (1 << 17) - 777
    while left:
        lens.append(min(int(rng.integers(1, 1501)), left))
        left -= lens[-1]
    sets["seeded_2_17"] = (17, random_calls(rng, lens))
    sets["boundary_operands"] = (11, boundary_calls())
    return sets


def many_short_calls(n_calls, seed=19):
    """the generator's arrays for n_calls seeded calls of 1, 2 or 3 elements (mostly 1): a call count at which the offset kernels loop"""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.array([1, 2, 3], np.uint32), n_calls, p=[0.9, 0.05, 0.05])
    n = int(lens.sum())
    return (rng.integers(0, P, (n_calls, 4)).astype(np.uint32), lens, rng.integers(0, P, n).astype(np.uint32), rng.integers(0, P, (n, 4)).astype(np.uint32))
