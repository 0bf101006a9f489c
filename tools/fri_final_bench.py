"""The FRI final-polynomial generator's time on one MI355X (docs/fri_final.md "Measured"): the `fri_final_tracegen` scope (device events around
the launch), median of 15 calls after 3 warm-up calls, with min and max, on the stored chunk proof's shape (its n_queries calls at
log_final_poly_len 0, lvl = log_blowup: shapes["chunk-proof-feynman.json"]) and on 2^20 rows at log_final_poly_len 8 (4096 calls of 256 rows
against 16 polynomials).  Prints one JSON line per measurement, time per row in ns.
Per kernel:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/fri_final_bench.py"""
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


def run(zk, name, lfp, n_calls, lvl, n_polys, lh):
    rng = np.random.default_rng(1)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32).reshape(-1)).to(zk.device)  # noqa: E731
    lvl = np.asarray(lvl, np.int64)
    d = [dev(rng.integers(0, 1 << 26, n_calls) >> (26 - lvl)), dev(lvl), dev(rng.integers(0, n_polys, n_calls)), dev(rng.integers(0, P, (n_polys, 1 << lfp, 4)))]
    med, lo, hi = timed(zk, ["fri_final_tracegen"], lambda: zk.fri_final_tracegen(*d, lfp, lh))
    rows = n_calls << lfp
    print(json.dumps(dict(shape=name, generator="fri_final (one lane per row, scan in the wave, carries through LDS)", log_final_poly_len=lfp, calls=n_calls, rows=rows,
                          log_height=lh, median_ms=med, min_ms=lo, max_ms=hi, ns_per_row=med * 1e6 / rows)), flush=True)


def main():
    zk = z.Context(0)
    with open(os.path.join(ROOT, "tests", "golden", "ref_v1_vectors.json")) as f:
        shape = json.load(f)["shapes"]["chunk-proof-feynman.json"]
    q = shape["n_queries"]
    run(zk, "chunk-proof-feynman", 0, q, [shape["log_blowup"]] * q, 1, int(np.ceil(np.log2(q))))
    rng = np.random.default_rng(2)
    run(zk, "2^20 rows at log_final_poly_len 8", 8, 1 << 12, rng.integers(1, 27, 1 << 12), 16, 20)
    zk.close()


if __name__ == "__main__":
    main()
