"""The row-digest generator's time on one MI355X (docs/mmcs_rows.md "Measured"): the `mmcs_rows_tracegen` scope, median of 15 calls after 3
warm-up calls, with min and max, on the stored chunk proof's shape (for each of its 44 query indices one call per height class of each
batch of shapes["chunk-proof-feynman.json"]) and on 2^20 rows of seeded lengths; and, at the same number of permutation rows, the two ways
this code base walked permutation chains before: zkhip_mmcs_path_tracegen (one lane per chain; one path per call, as many steps as the
call has rows) and zkhip_duplex_tracegen (one lane in all; at most 2^14 rows of it are timed, it is linear in the rows).  Prints one JSON
line per measurement, time per permutation row in ns.  Per kernel:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/mmcs_rows_bench.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkvm_prover_amd as z  # noqa: E402

P = 2013265921


def timed(zk, scope, call, reps=15):
    for _ in range(3):
        call()
    zk.sync()
    zk.profile_enable(True)
    times = []
    for _ in range(reps):
        zk.profile_reset()
        call()
        zk.sync()
        times.append(zk.profile_read()[scope][1])
    zk.profile_enable(False)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(zk, name, lens, lh):
    rng = np.random.default_rng(1)
    lens = np.asarray(lens, np.uint32)
    n, rows_of = len(lens), (lens.astype(np.int64) + 7) // 8
    rows = int(rows_of.sum())
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)  # noqa: E731
    d = [dev(lens), dev(rng.integers(0, P, (n, 8))), dev(rng.integers(0, 28, n)), dev(rng.integers(0, 1 << 27, n)), dev(np.ones(n)),
         dev(rng.integers(0, P, int(lens.sum())))]
    out = []

    def report(kind, scope, call, r):
        med, lo, hi = timed(zk, scope, call)
        out.append(dict(shape=name, generator=kind, calls=n, rows=r, log_height=lh, median_ms=med, min_ms=lo, max_ms=hi, ns_per_row=med * 1e6 / r))
        print(json.dumps(out[-1]), flush=True)

    report("mmcs_rows (16 lanes per call)", "mmcs_rows_tracegen", lambda: zk.mmcs_rows_tracegen(*d, lh), rows)
    # one lane per chain: a path of rows_of[c] sibling steps per call
    starts = np.concatenate([[0], np.cumsum(rows_of)])
    p = [dev(rng.integers(0, P, (n, 8))), dev(rng.integers(0, 1 << 20, n)), dev(starts), dev(np.zeros(rows)), dev(rng.integers(0, P, (rows, 8)))]
    report("mmcs_path (one lane per chain)", "mmcs_path_tracegen", lambda: zk.mmcs_path_tracegen(*p, lh), rows)
    # one lane in all
    r1 = min(rows, 1 << 14)
    lh1 = int(np.ceil(np.log2(max(r1, 2))))
    q = [dev(np.full(r1, 8)), dev(rng.integers(0, P, (r1, 8))), dev(np.zeros(r1))]
    report("duplex (one lane)", "duplex_tracegen", lambda: zk.duplex_tracegen(*q, lh1), r1)
    return out


def main():
    zk = z.Context(0)
    with open(os.path.join(ROOT, "tests", "golden", "ref_v1_vectors.json")) as f:
        shape = json.load(f)["shapes"]["chunk-proof-feynman.json"]
    per_query = []
    for b in shape["batches"]:   # one call per height class: the widths of the batch's matrices of one height, added up
        lhs = b["log_height"] if isinstance(b["log_height"], list) else [b["log_height"]] * len(b["widths"])
        per_query += [sum(w for w, h in zip(b["widths"], lhs) if h == level) for level in sorted(set(lhs), reverse=True)]
    lens = per_query * shape["n_queries"]
    rows = sum((x + 7) // 8 for x in lens)
    run(zk, "chunk-proof-feynman", lens, int(np.ceil(np.log2(rows))))
    rng = np.random.default_rng(2)
    big, left = [], (1 << 20) - 100
    while left:   # 1 to 55 rows a call, like the reference's stored openings
        big.append(min(int(rng.integers(1, 441)), 8 * left))
        left -= (big[-1] + 7) // 8
    run(zk, "seeded 2^20 rows", big, 20)
    zk.close()


if __name__ == "__main__":
    main()
