"""The FRI query chip's twin (air.fri_query_air, zkhip_fri_query_host / zkhip_fri_query_tracegen): one query's fold loop in Python integers
(chain_int: the definition, a dozen lines) and in numpy for large counts (trace_np: all calls at once, layer by layer), held against each
other by the CPU tests; the call sets the CPU and GPU tests share; and an honest FRI instance built from the oracle's own primitives as a
prover would build it (fri_instance: ora.fri_fold from layer to layer, every layer committed with the oracle's Mmcs), on which the twin
insists that every chain's eval is the next layer's stored value and every opened pair verifies.  A call is (index, log_max, beta[n][4],
root[n][8], sibling[n][4], has_ro[n], ro[n][4], ro_top[4]) of canonical integers.  Test infrastructure."""
import ctypes as C
from collections import OrderedDict

import numpy as np

P = 2013265921
WIDTH = 61
E0, E1, BETA, BSQ, XINV, FOLDED, RO, EVAL, ST_OUT, ROOT, BIT, HAS_RO, K, LVL, FIRST, LAST, REAL, CALL = 0, 4, 8, 12, 16, 17, 21, 25, 29, 45, 53, 54, 55, 56, 57, 58, 59, 60
G27 = 0x1A427A41
WINV = [pow(pow(G27, 1 << (27 - (j + 2)), P), P - 2, P) for j in range(26)]   # air.domain_point_inverse_roots
INV2 = (P + 1) // 2


# ---- Python integers: the definition -----------------------------------------------------------------------------------------------------
def emul(x, y):
    out = [0, 0, 0, 0]
    for i in range(4):
        for j in range(4):
            out[(i + j) % 4] += x[i] * y[j] * (11 if i + j >= 4 else 1)
    return [v % P for v in out]


def x_inv(k):
    """1 / g^bitrev(k) from the set bits of k: the same constants for a layer of any size"""
    acc = 1
    for j in range(26):
        if (k >> j) & 1:
            acc = acc * WINV[j] % P
    return acc


def fold(e0, e1, beta, xinv):
    pr = emul(beta, [(a - b) % P for a, b in zip(e0, e1)])
    return [((a + b) + xinv * c) * INV2 % P for a, b, c in zip(e0, e1, pr)]


def chain_int(index, log_max, beta, sibling, has_ro, ro, ro_top):
    """-> per layer (e0, e1, eval): the verifier's loop"""
    ev, out = [int(v) for v in ro_top], []
    for t in range(len(has_ro)):
        sib, b = [int(v) for v in sibling[t]], [int(v) for v in beta[t]]
        e0, e1 = (sib, ev) if (index >> t) & 1 else (ev, sib)
        f = fold(e0, e1, b, x_inv(index >> (t + 1)))
        ev = [(a + c) % P for a, c in zip(f, emul(emul(b, b), [int(v) for v in ro[t]]))] if has_ro[t] else f
        out.append((e0, e1, ev))
    return out


# ---- numpy: all calls at once ----------------------------------------------------------------------------------------------------------------
def emul_np(x, y):
    x, y = x.astype(np.uint64), y.astype(np.uint64)
    out = np.zeros(x.shape, np.uint64)
    for i in range(4):
        for j in range(4):
            t = x[..., i] * y[..., j] % P
            out[..., (i + j) % 4] = (out[..., (i + j) % 4] + (t * 11 % P if i + j >= 4 else t)) % P
    return out


def x_inv_np(k):
    acc = np.ones(k.shape, np.uint64)
    for j in range(26):
        acc = acc * np.where((k >> j) & 1, np.uint64(WINV[j]), np.uint64(1)) % P
    return acc


def records(calls):
    """the generator's arrays: n_layers, log_max, index [n], ro_top [n][4]; beta [R][4], root [R][8], sibling [R][4], has_ro [R], ro [R][4]"""
    n = len(calls)
    cat = lambda k, w: (np.concatenate([np.asarray(c[k], np.uint32).reshape(-1, w) for c in calls]) if n else np.zeros((0, w), np.uint32))  # noqa: E731
    return (np.array([len(c[5]) for c in calls], np.uint32), np.array([c[1] for c in calls], np.uint32), np.array([c[0] for c in calls], np.uint32),
            np.array([c[7] for c in calls], np.uint32).reshape(n, 4), cat(2, 4), cat(3, 8), cat(4, 4), cat(5, 1).reshape(-1), cat(6, 4))


def trace_np(ora, n_layers, log_max, index, ro_top, beta, root, sibling, has_ro, ro, log_height):
    """-> (trace [61, 2^log_height], hash_inputs [2^log_height, 16], leaf digests [n_rows, 8], final [n_calls, 4]), canonical uint32"""
    nl, lm, index = np.asarray(n_layers, np.int64), np.asarray(log_max, np.int64), np.asarray(index, np.int64)
    n, N, R = len(nl), 1 << log_height, int(nl.sum())
    assert R <= N and (nl >= 1).all() and (nl + 1 <= lm).all() and (lm <= 27).all() and ((index >> lm) == 0).all()
    beta, sibling, ro = (np.asarray(v, np.uint64).reshape(R, 4) for v in (beta, sibling, ro))
    has = np.asarray(has_ro, np.int64).reshape(R)
    assert (has <= 1).all() and (ro[has == 0] == 0).all()
    roff = np.concatenate([[0], np.cumsum(nl)])
    call = np.repeat(np.arange(n), nl)
    t = np.arange(R) - roff[call]
    idx = index[call]
    bit, k, lvl = (idx >> t) & 1, idx >> (t + 1), lm[call] - 1 - t
    xinv, bsq = x_inv_np(k), emul_np(beta, beta)
    join = emul_np(bsq, ro)
    e0, e1, folded, ev = (np.zeros((R, 4), np.uint64) for _ in range(4))
    cur = np.asarray(ro_top, np.uint64).reshape(n, 4).copy()
    for tt in range(int(nl.max()) if n else 0):
        rs = np.nonzero(t == tt)[0]
        cs, b = call[rs], bit[rs, None].astype(bool)
        e0[rs], e1[rs] = np.where(b, sibling[rs], cur[cs]), np.where(b, cur[cs], sibling[rs])
        pr = emul_np(beta[rs], (e0[rs] + P - e1[rs]) % P)
        folded[rs] = ((e0[rs] + e1[rs]) % P + xinv[rs, None] * pr % P) % P * INV2 % P
        ev[rs] = (folded[rs] + join[rs]) % P
        cur[cs] = ev[rs]
    hin = np.zeros((N, 16), np.uint32)
    hin[:R, :4], hin[:R, 4:8] = e0, e1
    sout = hin[:max(R, 1)].copy()
    lib, base, u32p = ora.lib(), sout.ctypes.data, C.POINTER(C.c_uint32)
    for r in range(R):
        lib.ora_poseidon2_permute(C.cast(base + 64 * r, u32p))
    tr = np.zeros((WIDTH, N), np.uint32)
    for col, v in ((E0, e0), (E1, e1), (BETA, beta), (BSQ, bsq), (FOLDED, folded), (RO, ro), (EVAL, ev)):
        tr[col:col + 4, :R] = v.T
    tr[XINV, :R], tr[ST_OUT:ST_OUT + 16, :R], tr[ROOT:ROOT + 8, :R] = xinv, sout[:R].T, np.asarray(root, np.uint32).reshape(R, 8).T
    tr[BIT, :R], tr[HAS_RO, :R], tr[K, :R], tr[LVL, :R] = bit, has, k, lvl
    tr[FIRST, :R], tr[LAST, :R], tr[REAL, :R], tr[CALL, :R] = t == 0, t == nl[call] - 1, 1, call
    return tr, hin, sout[:R, :8].copy(), cur.astype(np.uint32)


def trace(ora, calls, log_height):
    return trace_np(ora, *records(calls), log_height)


def n_rows(calls):
    return sum(len(c[5]) for c in calls)


# ---- call sets ---------------------------------------------------------------------------------------------------------------------------------
def random_call(rng, n, log_max=None, index=None, has=None):
    log_max = int(rng.integers(n + 1, 28)) if log_max is None else log_max
    index = int(rng.integers(0, 1 << log_max)) if index is None else index
    f = lambda w: rng.integers(0, P, (n, w), dtype=np.int64)  # noqa: E731
    has_ro = rng.integers(0, 2, n) if has is None else np.full(n, has)
    return (index, log_max, f(4), f(8), f(4), has_ro, f(4) * has_ro[:, None], rng.integers(0, P, 4, dtype=np.int64))


def boundary_calls():
    """betas, siblings, ro and ro_top of 0 and p - 1, index 0 and 2^log_max - 1, has_ro all 0 and all 1"""
    rng = np.random.default_rng(43)
    calls = []
    for n, lm, index in ((1, 2, 0), (1, 2, 3), (2, 3, 7), (26, 27, (1 << 27) - 1), (26, 27, 0), (5, 9, 0x155)):
        for kind in range(3):
            c = [index, lm] + [np.array(v) for v in random_call(rng, n, lm, index, has=1 if kind else 0)[2:]]
            for arr in (c[2], c[4], c[6], c[7]):
                flat = arr.reshape(-1)
                flat[(np.arange(flat.size) + kind) % 3 == 0] = 0
                flat[(np.arange(flat.size) + kind) % 3 == 1] = P - 1
            c[6] = c[6] * c[5][:, None]
            if kind == 2:
                c[3][:] = P - 1
            calls.append(tuple(c))
    z4, m4 = np.zeros((3, 4), np.int64), np.full((3, 4), P - 1)
    calls.append((0, 4, z4, np.zeros((3, 8), np.int64), z4, np.zeros(3, np.int64), z4, np.zeros(4, np.int64)))
    calls.append((15, 4, m4, np.full((3, 8), P - 1), m4, np.ones(3, np.int64), m4, np.full(4, P - 1)))
    return calls


def call_sets(which=None):
    """name -> (log_height, calls), seeded.  The generator stages nothing (one lane per row), so there is no staging boundary to straddle;
    the sets around 16 rows stay as shapes where a workgroup's lanes split between calls."""
    rng = np.random.default_rng(19)
    rc = lambda lengths: [random_call(rng, n) for n in lengths]  # noqa: E731
    sets = OrderedDict()
    sets["one_row"] = (0, rc([1]))
    sets["rows_26"] = (5, [random_call(rng, 26, 27)])                     # the 26-bit pair index
    sets["full_16"] = (4, rc([1, 2, 5, 3, 4, 1]))                          # 16 rows: the trace exactly full
    sets["short_padded"] = (6, rc([3, 1, 2]))
    for n in (3, 4, 5):
        sets["calls_%d" % n] = (6, rc([int(x) for x in rng.integers(1, 12, n)]))
    sets["boundary_operands"] = (8, boundary_calls())
    if which == "cpu":
        return sets
    sets["calls_65"] = (10, rc([int(x) for x in rng.integers(1, 16, 65)]))
    sets["rows_15_16_17"] = (6, rc([15, 16, 17]))
    sets["seventeen_one_row"] = (5, rc([1] * 17))
    sets["past_a_workgroup"] = (9, rc([26] * 11 + [1] * 3))               # 289 rows: the row kernel's second workgroup is part padding
    return sets


def many_one_row_calls(n_calls, seed=23):
    """the generator's arrays for n_calls seeded calls of one row: a call count at which the shared offset kernels loop"""
    rng = np.random.default_rng(seed)
    u = lambda hi, shape: rng.integers(0, hi, shape).astype(np.uint32)  # noqa: E731
    lm = u(26, n_calls) + 2
    has = u(2, n_calls)
    return (np.ones(n_calls, np.uint32), lm, (rng.integers(0, 1 << 27, n_calls) >> (27 - lm.astype(np.int64))).astype(np.uint32), u(P, (n_calls, 4)), u(P, (n_calls, 4)),
            u(P, (n_calls, 8)), u(P, (n_calls, 4)), has, u(P, (n_calls, 4)) * has[:, None])


# ---- an honest FRI instance from the oracle's primitives -------------------------------------------------------------------------------------
class FriInstance:
    pass


def fri_instance(ora, z, log_max=5, seed=7, n_queries=12):
    """What a prover builds: layer 0 = the reduced openings at log_max; layer l + 1 = ora.fri_fold(layer l, beta_l), plus beta_l^2 ro_h
    where a vector of reduced openings joins at that height; every folded-from layer committed as an [n / 2][8] matrix with the oracle's
    Mmcs.  Then n_queries indices opened (at least two share their high bits).  Asserts, independently of the chip: every chain's eval
    equals the next layer's stored value at k, and every opening passes zkhip_mmcs_verify."""
    rng = np.random.default_rng(seed)
    n_layers = log_max - 1
    ext = lambda h: rng.integers(0, P, (1 << h, 4), dtype=np.int64).astype(np.uint32)  # noqa: E731
    joins = {log_max - 2: ext(log_max - 2), 2: ext(2)}                  # two lower heights
    betas = rng.integers(0, P, (n_layers, 4), dtype=np.int64).astype(np.uint32)
    layers, trees = [ext(log_max)], []
    for l in range(n_layers):
        h = log_max - l - 1
        nxt = ora.fri_fold(layers[l].reshape(-1), h, betas[l]).reshape(1 << h, 4)
        if h in joins:
            b2 = emul_np(betas[l][None, :], betas[l][None, :])
            nxt = ((nxt.astype(np.uint64) + emul_np(np.broadcast_to(b2, (1 << h, 4)), joins[h])) % P).astype(np.uint32)
        layers.append(nxt)
        trees.append(ora.Tree([np.ascontiguousarray(layers[l].reshape(1 << h, 8).T)]))
        assert trees[l].log_height == h
    first = int(rng.integers(0, 1 << log_max))
    indices = [first, first ^ 1, first ^ 2] + [int(x) for x in rng.integers(0, 1 << log_max, n_queries - 3)]
    calls, openings = [], []
    for idx in indices:
        sib, has, ro, root = [], [], [], []
        for t in range(n_layers):
            h, k = log_max - t - 1, idx >> (t + 1)
            sib.append(layers[t][(idx >> t) ^ 1]), root.append(trees[t].root)
            has.append(1 if h in joins else 0), ro.append(joins[h][k] if h in joins else np.zeros(4, np.uint32))
            op = trees[t].open(k)
            assert z.mmcs_verify(trees[t].root, [h], [8], k, op) == 0
            openings.append((t, h, k, op))
        call = (idx, log_max, betas, np.array(root), np.array(sib), np.array(has), np.array(ro), layers[0][idx])
        for t, (e0, e1, ev) in enumerate(chain_int(idx, log_max, call[2], call[4], call[5], call[6], call[7])):
            assert ev == layers[t + 1][idx >> (t + 1)].tolist(), "the chain leaves layer %d at query %d" % (t + 1, idx)
            assert e0 + e1 == openings[len(openings) - n_layers + t][3][:8].tolist()
        calls.append(call)
    inst = FriInstance()
    inst.log_max, inst.n_layers, inst.betas, inst.layers, inst.trees, inst.joins = log_max, n_layers, betas, layers, trees, joins
    inst.indices, inst.calls, inst.openings = indices, calls, openings
    return inst


def path_records(inst):
    """the MMCS path generator's records for every opening of the instance, in row order of the query chip: (index [n], starts [n + 1],
    kinds [steps] all sibling, digests [steps][8]); the leaves are the query chip's leaf digests"""
    idx = np.array([k for (_, _, k, _) in inst.openings], np.uint32)
    starts = np.concatenate([[0], np.cumsum([h for (_, h, _, _) in inst.openings])]).astype(np.uint32)
    digs = np.concatenate([op[8:].reshape(-1, 8) for (_, _, _, op) in inst.openings])
    return idx, starts, np.zeros(int(starts[-1]), np.uint32), digs


def bus_tables(inst):
    """plain tables for the three buses nothing here serves, from the instance (not from the chip's trace, except the final evals which
    are the instance's last layer): ro (call, lvl, ro[4] | mult) sent, layer (call, lvl, beta[4], root[8] | mult) received, final (call,
    lvl, k, eval[4] | mult) received"""
    ro_rows, layer_rows, final_rows = [], [], []
    for c, call in enumerate(inst.calls):
        idx = call[0]
        ro_rows.append([c, inst.log_max] + inst.layers[0][idx].tolist() + [1])
        for t in range(inst.n_layers):
            h = inst.log_max - t - 1
            if call[5][t]:
                ro_rows.append([c, h] + inst.joins[h][idx >> (t + 1)].tolist() + [1])
            layer_rows.append([c, h] + inst.betas[t].tolist() + inst.trees[t].root.tolist() + [1])
        kf = idx >> inst.n_layers
        final_rows.append([c, inst.log_max - inst.n_layers, kf] + inst.layers[inst.n_layers][kf].tolist() + [1])

    def table(rows):
        lh = max(1, int(np.ceil(np.log2(len(rows)))))
        t = np.zeros((len(rows[0]), 1 << lh), np.uint32)
        t[:, :len(rows)] = np.array(rows, np.uint32).T
        return t
    return table(ro_rows), table(layer_rows), table(final_rows)
