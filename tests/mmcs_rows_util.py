"""The row-digest chip in numpy over the oracle's permutation (air.mmcs_rows_air, zkhip_hash_slice_host / zkhip_mmcs_rows_tracegen): the
twin the CPU and GPU tests compare with, the call sets they share, the values-bus receiver table and the calls of the reference's stored
openings.  The twin walks a call ROW BY ROW (overwrite the rate lanes, ora_poseidon2_permute, carry) and insists on every call that lanes
0..7 of its last output equal ora_hash_slice of the whole call -- the direct definition; the two share the permutation and nothing else.
A call is (words[L], root[8], lvl, idx, mult) of canonical integers.  Test infrastructure."""
import ctypes as C
from collections import OrderedDict

import numpy as np

P = 2013265921
WIDTH = 56
ST_IN, ST_OUT, F, FIRST, LAST, REAL, ROOT, LVL, IDX, MULT, CALL, BLK = 0, 16, 32, 40, 41, 42, 43, 51, 52, 53, 54, 55
STAGE_ROWS = 16   # rows a 16-lane group of the generator stages in LDS before it stores them (csrc/mmcs_rows.hip MR_SLOTS)


def hash_slice(ora, words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(8, np.uint32)
    ora.lib().ora_hash_slice(ora.p32(w), len(w), ora.p32(out))
    return out


def records(calls):
    """the generator's arrays: len [n], root [n][8], lvl [n], idx [n], mult [n], values [n_words] (uint32)"""
    n = len(calls)
    lens = np.array([len(c[0]) for c in calls], np.uint32)
    root = np.array([c[1] for c in calls], np.uint32).reshape(n, 8)
    lvl, idx, mult = (np.array([c[k] for c in calls], np.uint32) for k in (2, 3, 4))
    values = np.concatenate([np.asarray(c[0], np.uint32) for c in calls]) if n else np.zeros(0, np.uint32)
    return lens, root, lvl, idx, mult, values


def trace_np(ora, lens, root, lvl, idx, mult, values, log_height, check=True):
    """-> (trace [56, 2^log_height], hash_inputs [2^log_height, 16], digests [n_calls, 8]), canonical uint32.  Call c on consecutive rows,
    row t of it absorbing words 8 t .. of the call; check: every call's digest is ora_hash_slice of its words."""
    lens = np.asarray(lens, np.int64)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    n, N = len(lens), 1 << log_height
    assert (lens >= 1).all() and int(lens.sum()) == len(values)
    nb = (lens + 7) // 8
    roff, woff = np.concatenate([[0], np.cumsum(nb)]), np.concatenate([[0], np.cumsum(lens)])
    rows = int(roff[-1])
    assert rows <= N
    call = np.repeat(np.arange(n), nb)
    blk = np.arange(rows) - roff[call]
    k = np.minimum(8, lens[call] - 8 * blk)
    w0 = woff[call] + 8 * blk
    sin, sout = np.zeros((max(rows, 1), 16), np.uint32), np.zeros((max(rows, 1), 16), np.uint32)
    lib, base, u32p = ora.lib(), sout.ctypes.data, C.POINTER(C.c_uint32)
    lane = np.arange(8)
    for blk_t in range(int(nb.max()) if n else 0):          # block t of every call that has one: assembled at once, permuted row by row
        rs = np.nonzero(blk == blk_t)[0]
        if blk_t:
            sin[rs] = sout[rs - 1]
        over = lane[None, :] < k[rs, None]
        words = values[np.minimum(w0[rs, None] + lane[None, :], max(len(values) - 1, 0))]
        sin[rs, :8] = np.where(over, words, sin[rs, :8])
        sout[rs] = sin[rs]
        for r in rs.tolist():
            lib.ora_poseidon2_permute(C.cast(base + 64 * r, u32p))
    t = np.zeros((WIDTH, N), np.uint32)
    hin = np.zeros((N, 16), np.uint32)
    hin[:rows] = sin[:rows]
    last = blk == nb[call] - 1
    t[ST_IN:ST_IN + 16, :rows], t[ST_OUT:ST_OUT + 16, :rows] = sin[:rows].T, sout[:rows].T
    t[F:F + 8, :rows] = np.arange(8)[:, None] < k[None, :]
    t[FIRST, :rows], t[LAST, :rows], t[REAL, :rows] = blk == 0, last, 1
    if n:
        t[ROOT:ROOT + 8, :rows] = np.asarray(root, np.uint32).reshape(n, 8)[call].T
        t[LVL, :rows], t[IDX, :rows] = np.asarray(lvl, np.uint32)[call], np.asarray(idx, np.uint32)[call]
        t[MULT, :rows] = np.where(last, np.asarray(mult, np.uint32)[call], 0)
    t[CALL, :rows], t[BLK, :rows] = call, blk
    digests = sout[roff[1:] - 1, :8].copy() if n else np.zeros((0, 8), np.uint32)
    if check:
        direct = np.zeros((max(n, 1), 8), np.uint32)
        vbase, dbase = values.ctypes.data, direct.ctypes.data
        for c, (o, ln) in enumerate(zip(woff[:-1].tolist(), lens.tolist())):
            lib.ora_hash_slice(C.cast(vbase + 4 * o, u32p), ln, C.cast(dbase + 32 * c, u32p))
        differ = np.nonzero((digests != direct[:n]).any(axis=1))[0]
        assert len(differ) == 0, "row-wise walk != ora_hash_slice on call %d" % int(differ[0])
    return t, hin, digests


def trace(ora, calls, log_height, check=True):
    return trace_np(ora, *records(calls), log_height, check=check)


def claims_of(calls, digests):
    """what the chip receives on the claims bus: [(root tuple, lvl, idx, digest tuple)] x mult"""
    out = []
    for c, d in zip(calls, digests):
        out += [(tuple(int(x) for x in c[1]), int(c[2]), int(c[3]), tuple(int(x) for x in d))] * int(c[4])
    return out


def values_table(calls, log_height):
    """the receiver of the values bus: columns call | pos | value | mult, one row per word of every call"""
    n = sum(len(c[0]) for c in calls)
    assert n <= 1 << log_height
    t = np.zeros((4, 1 << log_height), np.uint32)
    r = 0
    for c, call in enumerate(calls):
        for pos, w in enumerate(call[0]):
            t[:, r] = (c, pos, int(w), 1)
            r += 1
    return t


def random_call(rng, L, mult=1):
    return (rng.integers(0, P, L, dtype=np.int64).tolist(), rng.integers(0, P, 8, dtype=np.int64).tolist(), int(rng.integers(0, 28)),
            int(rng.integers(0, 1 << 27)), mult)


def random_calls(rng, lengths):
    return [random_call(rng, L, int(rng.integers(0, 4))) for L in lengths]


def boundary_calls():
    """words 0 and p - 1 in every lane position of full and partial blocks, and record fields at p - 1"""
    rng = np.random.default_rng(43)
    calls = []
    for L in (1, 7, 8, 9, 16, 17, 40):
        for kind in range(3):
            words, root, lvl, idx, mult = random_call(rng, L)
            for i in range(L):
                if (i + kind) % 3 == 0:
                    words[i] = 0
                elif (i + kind) % 3 == 1:
                    words[i] = P - 1
            calls.append((words, [P - 1] * 8 if kind == 0 else root, P - 1 if kind == 1 else lvl, P - 1 if kind == 2 else idx, P - 1 if kind == 0 else mult))
    calls.append(([0] * 8, [0] * 8, 0, 0, 0))
    calls.append(([P - 1] * 17, root, 3, 5, 2))
    return calls


def call_sets(which=None):
    """name -> (log_height, calls), seeded"""
    rng = np.random.default_rng(17)
    S = STAGE_ROWS
    sets = OrderedDict()
    sets["one_word"] = (0, random_calls(rng, [1]))
    sets["L8"] = (1, random_calls(rng, [8]))                  # one full row that is also last
    sets["L9"] = (1, random_calls(rng, [9]))                  # the second row has one lane
    sets["L16"] = (1, random_calls(rng, [16]))
    sets["L17"] = (2, random_calls(rng, [17]))
    sets["full_16"] = (4, random_calls(rng, [1, 8, 9, 17, 16, 40, 3]))      # 1 + 1 + 2 + 3 + 2 + 5 + 1 = 15 ... + 1 below
    sets["full_16"][1].append(random_call(rng, 5))            # 16 rows: the trace exactly full
    sets["short_padded"] = (6, random_calls(rng, [3, 20, 1]))  # 5 rows of 64
    for n in (3, 4, 5):
        sets["calls_%d" % n] = (5, random_calls(rng, [int(x) for x in rng.integers(1, 30, n)]))
    sets["boundary_words"] = (8, boundary_calls())
    if which == "cpu":
        return sets
    sets["calls_65"] = (9, random_calls(rng, [int(x) for x in rng.integers(1, 50, 65)]))
    sets["imbalance"] = (11, random_calls(rng, [1] * 100 + [8 << 10] + [1] * 100))   # one call of 2^10 rows beside 200 one-row calls
    # calls that end and start on the staging boundary: S rows exactly, S + 1, S - 1 then 1, 2 S + 3 across two of them, then single rows
    sets["stage_boundaries"] = (8, random_calls(rng, [8 * S, 8 * (S + 1), 8 * (S - 1), 1, 8 * (2 * S + 3) - 5] + [1] * (S + 1) + [8 * S - 7]))
    return sets


def many_one_word_calls(n_calls, seed=23):
    """the generator's arrays for n_calls seeded calls of one word: a call count at which the shared offset kernels loop"""
    rng = np.random.default_rng(seed)
    u = lambda hi, shape: rng.integers(0, hi, shape).astype(np.uint32)  # noqa: E731
    return (np.ones(n_calls, np.uint32), u(P, (n_calls, 8)), u(28, n_calls), u(1 << 27, n_calls), u(3, n_calls), u(P, n_calls))


def calls_of_fixture(ora, vec, limit=None, merge=True):
    """The calls of the reference's stored openings (tests/golden/ref_v1_vectors.json): for every query and every batch with a path, one
    call per height class -- the opened words of the batch's matrices of that height, in matrix order (the grouping of
    mmcs_path_util.records_of_fixture) -- under the batch's root at (lvl, idx) = (height, query index shifted to that height).  merge:
    calls with the same (root, lvl, idx) -- queries whose indices share high bits open the same row of a short matrix -- become one call
    whose mult counts them."""
    calls, seen = [], {}
    for q in vec["openings"][:limit]:
        H = q["log_max_height"]
        for b in q["batches"]:
            lhs, ws, opening = b["log_heights"], b["widths"], b["opening"]
            hb = max(lhs)
            if hb == 0:
                continue   # a single-row batch has no path
            index = q["index"] >> (H - hb)
            offs = np.concatenate([[0], np.cumsum(ws)])
            for level in sorted(set(lhs), reverse=True):
                words = [int(x) for m in range(len(ws)) if lhs[m] == level for x in opening[offs[m]:offs[m + 1]]]
                key = (tuple(int(x) for x in b["root"]), level, index >> (hb - level))
                if merge and key in seen:
                    assert seen[key][0] == words
                    seen[key][4] += 1
                else:
                    seen[key] = [words, list(key[0]), key[1], key[2], 1]
                    calls.append(seen[key])
    return [tuple(c) for c in calls]


def path_digest_sources(vec, calls, limit=None):
    """Where mmcs_path_util.records_of_fixture's digests come from among `calls` (calls_of_fixture, merged), in its order of paths and
    steps: (the call whose digest is each path's leaf, the positions of the injected steps, the call of each) -- so that the path
    generator can be fed from the row-digest generator's d_digest."""
    at = {(tuple(c[1]), c[2], c[3]): i for i, c in enumerate(calls)}
    leaf_call, inj_pos, inj_call, step = [], [], [], 0
    for q in vec["openings"][:limit]:
        H = q["log_max_height"]
        for b in q["batches"]:
            lhs = b["log_heights"]
            hb = max(lhs)
            if hb == 0:
                continue
            index, root = q["index"] >> (H - hb), tuple(int(x) for x in b["root"])
            leaf_call.append(at[(root, hb, index)])
            for l in range(hb):
                step += 1                                  # the sibling
                if hb - l - 1 in lhs:
                    inj_pos.append(step), inj_call.append(at[(root, hb - l - 1, index >> (l + 1))])
                    step += 1
    return np.array(leaf_call, np.int64), np.array(inj_pos, np.int64), np.array(inj_call, np.int64)
