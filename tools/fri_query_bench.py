"""The FRI query generator's time on one MI355X (docs/fri_query.md "Measured"): the `fri_query_tracegen` scope, median of 15 calls after 3
warm-up calls, with min and max, on the stored chunk proof's shape (44 queries x n_fri_layers of shapes["chunk-proof-feynman.json"]) and on
2^20 rows of seeded chain lengths; and, at the same number of rows, what this code base could do before for the same cells without the
chain: zkhip_fri_fold_chip_tracegen (the fold line of every row) plus zkhip_mmcs_rows_tracegen on one-block calls (the leaf of every row).
Prints one JSON line per measurement, time per row in ns.  Per kernel:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/fri_query_bench.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkvm_prover_amd as z  # noqa: E402

P = 2013265921


def timed(zk, scopes, call, reps=15):
    for _ in range(3):
        call()
    zk.sync()
    zk.profile_enable(True)
    times = []
    for _ in range(reps):
        zk.profile_reset()
        call()
        zk.sync()
        stats = zk.profile_read()
        times.append(sum(stats[s][1] for s in scopes))
    zk.profile_enable(False)
    return float(np.median(times)), float(min(times)), float(max(times))


def run(zk, name, n_layers, log_max, lh):
    rng = np.random.default_rng(1)
    nl, lm = np.asarray(n_layers, np.int64), np.asarray(log_max, np.int64)
    n, rows = len(nl), int(nl.sum())
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)  # noqa: E731
    has = rng.integers(0, 2, rows)
    index = rng.integers(0, 1 << 27, n) >> (27 - lm)
    d = [dev(nl), dev(lm), dev(index), dev(rng.integers(0, P, (n, 4))), dev(rng.integers(0, P, (rows, 4))), dev(rng.integers(0, P, (rows, 8))),
         dev(rng.integers(0, P, (rows, 4))), dev(has), dev(rng.integers(0, P, (rows, 4)) * has[:, None])]

    def report(kind, scopes, call):
        med, lo, hi = timed(zk, scopes, call)
        out = dict(shape=name, generator=kind, calls=n, rows=rows, log_height=lh, median_ms=med, min_ms=lo, max_ms=hi, ns_per_row=med * 1e6 / rows)
        print(json.dumps(out), flush=True)

    report("fri_query (chain per call, then one lane per row)", ["fri_query_tracegen"], lambda: zk.fri_query_tracegen(*d, lh))
    # before: the rows' fold lines and leaves as independent records -- no chain, nothing ties a row to the next
    call = np.repeat(np.arange(n), nl)
    t = np.arange(rows) - np.repeat(np.concatenate([[0], np.cumsum(nl)])[:-1], nl)
    f = [dev(rng.integers(0, P, (rows, 4))), dev(rng.integers(0, P, (rows, 4))), dev(rng.integers(0, P, (rows, 4))), dev(index[call] >> (t + 1)), dev(lm[call] - 1 - t)]
    m = [dev(np.full(rows, 8)), dev(rng.integers(0, P, (rows, 8))), dev(lm[call] - 1 - t), dev(index[call] >> (t + 1)), dev(np.ones(rows)), dev(rng.integers(0, P, 8 * rows))]

    def before():
        zk.fri_fold_chip_tracegen(*f, lh)
        zk.mmcs_rows_tracegen(*m, lh)
    report("fri_fold_chip + mmcs_rows on one-block calls", ["fri_fold_chip_tracegen", "mmcs_rows_tracegen"], before)


def main():
    zk = z.Context(0)
    with open(os.path.join(ROOT, "tests", "golden", "ref_v1_vectors.json")) as f:
        shape = json.load(f)["shapes"]["chunk-proof-feynman.json"]
    q, layers = shape["n_queries"], shape["n_fri_layers"]
    log_max = shape["log_max_height"] + shape["log_blowup"]   # the tallest LDE
    run(zk, "chunk-proof-feynman", [layers] * q, [log_max] * q, int(np.ceil(np.log2(q * layers))))
    rng = np.random.default_rng(2)
    big, left = [], (1 << 20) - 100
    while left:   # 1 to 26 layers a query
        big.append(min(int(rng.integers(1, 27)), left))
        left -= big[-1]
    run(zk, "seeded 2^20 rows", big, [int(x) for x in np.maximum(np.array(big) + 1, rng.integers(2, 28, len(big)))], 20)
    zk.close()


if __name__ == "__main__":
    main()
