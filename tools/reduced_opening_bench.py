"""The reduced-opening generator's time on one MI355X (docs/reduced_opening.md "Measured"): the `reduced_opening_tracegen` scope, median of
15 calls after 3 warm-up calls, on the stored chunk proof's shape (for each of its 44 query indices one call per matrix of each batch of
shapes["chunk-proof-feynman.json"], length = width) and on 2^24 rows of seeded lengths in [1, 1500] to read the rate against HBM.
Prints one JSON line per workload.  Per kernel:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/reduced_opening_bench.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkvm_prover_amd as z  # noqa: E402

P = 2013265921


def run(zk, name, lens, lh, reps=15):
    rng = np.random.default_rng(1)
    lens = np.asarray(lens, np.uint32)
    n = int(lens.sum())
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)  # noqa: E731
    d = [dev(rng.integers(0, P, (len(lens), 4))), dev(lens), dev(rng.integers(0, P, n)), dev(rng.integers(0, P, (n, 4)))]
    for _ in range(3):
        zk.reduced_opening_tracegen(*d, lh)
    zk.sync()
    zk.profile_enable(True)
    times = []
    for _ in range(reps):
        zk.profile_reset()
        zk.reduced_opening_tracegen(*d, lh)
        zk.sync()
        times.append(zk.profile_read()["reduced_opening_tracegen"][1])
    zk.profile_enable(False)
    N = 1 << lh
    must = 20 * n + 72 * N + 20 * len(lens)   # 20 B per element read, 72 B per row written (padding rows included), alpha and length per call
    med = float(np.median(times))
    out = dict(shape=name, calls=len(lens), elems=n, log_height=lh, median_ms=med, min_ms=float(min(times)), max_ms=float(max(times)), bytes=must,
               gb_per_s=must / med / 1e6)
    print(json.dumps(out), flush=True)
    return out


def main():
    zk = z.Context(0)
    with open(os.path.join(ROOT, "tests", "golden", "ref_v1_vectors.json")) as f:
        shape = json.load(f)["shapes"]["chunk-proof-feynman.json"]
    per_query = [w for b in shape["batches"] for w in b["widths"]]
    lens = per_query * shape["n_queries"]
    lh = int(np.ceil(np.log2(sum(lens))))
    run(zk, "chunk-proof-feynman", lens, lh)
    rng = np.random.default_rng(2)
    big, left = [], (1 << 24) - 1000
    while left:
        big.append(min(int(rng.integers(1, 1501)), left))
        left -= big[-1]
    run(zk, "seeded 2^24", big, 24)
    zk.close()


if __name__ == "__main__":
    main()
