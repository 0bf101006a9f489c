"""The FRI final-polynomial chip's twin (air.fri_final_air, zkhip_fri_final_host / zkhip_fri_final_tracegen): a query's last check in
Python integers (value_int: Horner at x = g_lvl^bitrev(k, lvl), the point computed from 0x1A427A41 by powering, independently of the W
tables) and in numpy (trace_np: all calls at once), held against each other by the CPU tests; the call sets the CPU and GPU tests share; and
an honest low-degree FRI instance built from the oracle's own primitives (final_instance: a seeded polynomial evaluated on the bit-reversed
domain, folded with ora.fri_fold, the last layer interpolated in Python integers), on which the twin insists that every query's last eval
from zkhip_fri_query_host is the interpolated polynomial at the query's point.  A call is (k, lvl, poly) against a table coef
[n_polys][L][4] of canonical integers, ascending.  Test infrastructure."""
from collections import OrderedDict

import numpy as np

import fri_query_util as fq

P = fq.P
WIDTH = 19
COEF, ACC, X, XINV, XI2, K, LVL, J, POLY, FIRST, LAST, REAL, CALL = 0, 4, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18
G27 = 0x1A427A41


# ---- Python integers: the definition -----------------------------------------------------------------------------------------------------
def bitrev(k, bits):
    return sum(((k >> i) & 1) << (bits - 1 - i) for i in range(bits))


def point(k, lvl):
    """g_lvl^bitrev(k, lvl), g_lvl the generator of the subgroup of order 2^lvl: the point of index k in the bit-reversed domain"""
    return pow(pow(G27, 1 << (27 - lvl), P), bitrev(k, lvl), P)


def value_int(coef, lvl, k):
    """-> (x, the polynomial with coefficients coef [L][4] (ascending) at x): the verifier's Horner"""
    x = point(k, lvl)
    acc = [int(v) for v in coef[-1]]
    for c in reversed(list(coef[:-1])):
        acc = [(a * x + int(w)) % P for a, w in zip(acc, c)]
    return x, acc


# ---- numpy: all calls at once ----------------------------------------------------------------------------------------------------------------
def trace_np(lfp, k, lvl, poly, coef, log_height):
    """-> (trace [19, 2^log_height], values [n_calls, 4]), canonical uint32"""
    L, N = 1 << lfp, 1 << log_height
    k, lvl, poly = (np.asarray(v, np.int64).reshape(-1) for v in (k, lvl, poly))
    coef = np.asarray(coef, np.uint64).reshape(-1, L, 4)
    n, R = len(k), len(k) * L
    assert R <= N and ((lvl >= 1) & (lvl <= 26)).all() and ((k >> lvl) == 0).all() and (poly < len(coef)).all() and (coef < P).all()
    xinv = fq.x_inv_np(k)                                   # what domain_point_air holds for k
    xi2 = xinv * xinv % P
    x = np.array([pow(int(v), P - 2, P) for v in xi2], np.uint64)
    co = coef[poly][:, ::-1, :] if n else np.zeros((0, L, 4), np.uint64)   # row t holds coefficient L - 1 - t
    acc = np.zeros((n, L, 4), np.uint64)
    for t in range(L):
        acc[:, t] = co[:, t] if t == 0 else (acc[:, t - 1] * x[:, None] + co[:, t]) % P
    tr = np.zeros((WIDTH, N), np.uint32)
    t = np.arange(R) & (L - 1)
    rep = lambda v: np.repeat(v, L)  # noqa: E731
    tr[COEF:COEF + 4, :R], tr[ACC:ACC + 4, :R] = co.reshape(R, 4).T, acc.reshape(R, 4).T
    tr[X, :R], tr[XINV, :R], tr[XI2, :R], tr[K, :R], tr[LVL, :R], tr[POLY, :R] = rep(x), rep(xinv), rep(xi2), rep(k), rep(lvl), rep(poly)
    tr[J, :R], tr[FIRST, :R], tr[LAST, :R], tr[REAL, :R], tr[CALL, :R] = L - 1 - t, t == 0, t == L - 1, 1, rep(np.arange(n))
    return tr, acc[:, L - 1].astype(np.uint32).reshape(n, 4)


def trace(s):
    return trace_np(s["lfp"], s["k"], s["lvl"], s["poly"], s["coef"], s["lh"])


# ---- call sets ---------------------------------------------------------------------------------------------------------------------------------
def call_set(rng, lfp, lh, n_calls, n_polys=1):
    lvl = rng.integers(1, 27, n_calls)
    return dict(lfp=lfp, lh=lh, lvl=lvl, k=rng.integers(0, 1 << 26, n_calls) >> (26 - lvl), poly=rng.integers(0, n_polys, n_calls),
                coef=rng.integers(0, P, (n_polys, 1 << lfp, 4), dtype=np.int64))


def boundary_set(lfp, lh):
    """k = 0 (x = 1), 1 (x = p - 1) and 2^lvl - 1 at lvl 1, 12 and 26, against a polynomial of zeros, one of p - 1 and a seeded one with
    zeros and p - 1 among its words, the calls taking the polynomials in turn (two and more polynomials used by interleaved calls)"""
    rng = np.random.default_rng(31 + lfp)
    L = 1 << lfp
    seeded = rng.integers(0, P, (L, 4), dtype=np.int64)
    seeded.reshape(-1)[::3], seeded.reshape(-1)[1::3] = 0, P - 1
    coef = np.stack([np.zeros((L, 4), np.int64), np.full((L, 4), P - 1), seeded])
    recs = [(k, lvl) for lvl in (1, 12, 26) for k in sorted({0, 1, (1 << lvl) - 1, int(rng.integers(0, 1 << lvl))})]
    recs = [(k, lvl, c % 3) for c, (k, lvl) in enumerate(recs + recs + recs[:1])]      # every (k, lvl) meets at least two polynomials
    return dict(lfp=lfp, lh=lh, k=np.array([r[0] for r in recs]), lvl=np.array([r[1] for r in recs]), poly=np.array([r[2] for r in recs]), coef=coef)


def call_sets(which=None):
    """name -> dict(lfp, lh, k, lvl, poly, coef), seeded: the smallest shapes at which the generator can go wrong.  A workgroup is 256 rows,
    a wave 64; L <= 64 scans inside a wave, L = 128 / 256 carries between waves."""
    rng = np.random.default_rng(29)
    sets = OrderedDict()
    sets["lfp0_one_call"] = call_set(rng, 0, 0, 1)                       # one row, the whole trace
    sets["lfp3_five_calls"] = call_set(rng, 3, 6, 5, 2)                  # several calls inside one wave; padding starts inside the wave
    sets["lfp3_full"] = call_set(rng, 3, 6, 8, 2)                        # exactly full
    sets["lfp1_boundary"] = boundary_set(1, 6)
    if which == "cpu":
        return sets
    sets["lfp0_past_a_workgroup"] = call_set(rng, 0, 9, 300, 3)          # 300 one-row calls: a second workgroup, padding behind
    sets["lfp6_three_calls"] = call_set(rng, 6, 8, 3, 2)                 # a call per wave: the scan's last step must cross nothing
    sets["lfp7_three_calls"] = call_set(rng, 7, 9, 3, 2)                 # a call across two waves: carries through LDS
    sets["lfp8_one_call"] = call_set(rng, 8, 8, 1)                       # a whole workgroup per call, exactly full
    sets["lfp8_three_calls"] = call_set(rng, 8, 10, 3, 2)                # ... with a padding workgroup behind
    sets["lfp0_boundary"] = boundary_set(0, 5)
    sets["lfp3_boundary"] = boundary_set(3, 8)
    sets["lfp8_boundary"] = boundary_set(8, 13)
    return sets


# ---- an honest low-degree FRI instance from the oracle's primitives ----------------------------------------------------------------------------
def final_instance(ora, z, log_max, log_blowup, lfp, seed=11, n_queries=12):
    """What a prover builds for a polynomial of degree < 2^(log_max - log_blowup): its evaluations on the bit-reversed domain of 2^log_max
    points, n_layers = log_max - log_blowup - lfp folds with ora.fri_fold (no joining vectors), every folded-from layer committed as an
    [n / 2][8] matrix with the oracle's Mmcs, and the final polynomial interpolated from the last layer in Python integers.  Asserts,
    independently of the chip: the interpolant has at most 2^lfp non-zero coefficients, and every query's last eval from fri_query_host is
    value_int of it at k = idx >> n_layers -- which pins the point formula, the squaring included, to the fold itself.  The result has
    fri_query_util.fri_instance's attributes (so path_records and bus_tables take it) and coef [2^lfp][4], lvl, lfp."""
    rng = np.random.default_rng(seed)
    n_layers, lvl, deg = log_max - log_blowup - lfp, log_blowup + lfp, 1 << (log_max - log_blowup)
    assert n_layers >= 1 and lvl >= 1
    f = rng.integers(0, P, (deg, 4), dtype=np.int64).tolist()
    top = np.zeros((1 << log_max, 4), np.uint32)
    for i in range(1 << log_max):
        x, acc = point(i, log_max), [0, 0, 0, 0]
        for c in reversed(f):
            acc = [(a * x + w) % P for a, w in zip(acc, c)]
        top[i] = acc
    betas = rng.integers(0, P, (n_layers, 4), dtype=np.int64).astype(np.uint32)
    layers, trees = [top], []
    for l in range(n_layers):
        h = log_max - l - 1
        layers.append(ora.fri_fold(layers[l].reshape(-1), h, betas[l]).reshape(1 << h, 4))
        trees.append(ora.Tree([np.ascontiguousarray(layers[l].reshape(1 << h, 8).T)]))
        assert trees[l].log_height == h
    last, n = layers[n_layers], 1 << lvl
    assert last.shape == (n, 4)
    # the inverse transform over the 2^lvl points: coef_m = (1 / n) sum_k last[k] x_k^-m
    pts_inv, n_inv = [pow(point(k, lvl), P - 2, P) for k in range(n)], pow(n, P - 2, P)
    interp = [[sum(int(last[k][w]) * pow(pts_inv[k], m, P) for k in range(n)) * n_inv % P for w in range(4)] for m in range(n)]
    assert all(c == [0, 0, 0, 0] for c in interp[1 << lfp:]), "the last layer is no polynomial of degree < 2^lfp"
    coef = np.array(interp[:1 << lfp], np.uint32)
    first = int(rng.integers(0, 1 << log_max))
    indices = [first, first ^ 1, first ^ 2] + [int(x) for x in rng.integers(0, 1 << log_max, n_queries - 3)]
    calls, openings = [], []
    zeros = np.zeros((n_layers, 4), np.uint32)
    for idx in indices:
        sib, root = [], []
        for t in range(n_layers):
            h, k = log_max - t - 1, idx >> (t + 1)
            sib.append(layers[t][(idx >> t) ^ 1]), root.append(trees[t].root)
            op = trees[t].open(k)
            assert z.mmcs_verify(trees[t].root, [h], [8], k, op) == 0
            openings.append((t, h, k, op))
        call = (idx, log_max, betas, np.array(root), np.array(sib), np.zeros(n_layers, np.uint32), zeros, layers[0][idx])
        _, _, ev = z.fri_query_host(idx, log_max, call[2], call[4], call[5], call[6], call[7])
        assert ev[-1].tolist() == value_int(coef, lvl, idx >> n_layers)[1], "query %d does not end on the final polynomial" % idx
        assert ev[-1].tolist() == last[idx >> n_layers].tolist()
        calls.append(call)
    inst = fq.FriInstance()
    inst.log_max, inst.n_layers, inst.betas, inst.layers, inst.trees, inst.joins = log_max, n_layers, betas, layers, trees, {}
    inst.indices, inst.calls, inst.openings = indices, calls, openings
    inst.coef, inst.lvl, inst.lfp = coef, lvl, lfp
    return inst


def final_records(inst, poly=0):
    """the final chip's records for the instance's queries: (k [n], lvl [n], poly [n]) -- call c is query c of the query chip"""
    n = len(inst.indices)
    return np.array([idx >> inst.n_layers for idx in inst.indices], np.uint32), np.full(n, inst.lvl, np.uint32), np.full(n, poly, np.uint32)


def coeff_table(inst, poly=0):
    """a plain table for the coefficient bus: (poly, j, coef[4] | mult), one row per coefficient, received once by every query"""
    L, n = 1 << inst.lfp, len(inst.indices)
    lh = max(1, inst.lfp)
    t = np.zeros((7, 1 << lh), np.uint32)
    t[0, :L], t[1, :L], t[2:6, :L], t[6, :L] = poly, np.arange(L), inst.coef.T, n
    return t
