"""WHIR on the device (docs/whir.md): launches, kernel time (the library's kernel stats, zkhip_profile_*) and wall time of
zkhip_whir_commit + zkhip_whir_open, of zkhip_gkr_committed_prove, and -- for comparison on a column of the same size -- of the v1
path: the coset LDE, the Merkle commit and the FRI fold loop (a fold and a commit per layer).  Every figure is the median of --reps
runs after one warm-up.  Prints one JSON object.

  python tools/whir_bench.py [--reps 5] [--logs 16,20,22,24] [--gkr-logs 20,24]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zkvm_prover_amd as z  # noqa: E402

P = z.P
# the bench's parameter set: 2^k-cosets, final_log 6, 16 bits of grinding and the query counts of docs/whir.md
QUERIES = {1: 80, 2: 40, 3: 27}


def _params(b, k):
    return z.WhirParams.make(b, k, 6, 16, QUERIES[b])


def _sync():
    import torch

    torch.cuda.synchronize()


def _profiled(zk, fn, reps):
    fn()
    runs = []
    for _ in range(reps):
        _sync()
        zk.profile_reset()
        zk.profile_enable(True)
        t0 = time.perf_counter()
        fn()
        _sync()
        wall = (time.perf_counter() - t0) * 1e3
        stats = zk.profile_read()
        zk.profile_enable(False)
        runs.append((stats, wall))
    names = sorted(set().union(*[s for s, _ in runs]))
    per = {n: {"launches": runs[0][0].get(n, (0, 0))[0], "ms": round(statistics.median(s.get(n, (0, 0.0))[1] for s, _ in runs), 4)}
           for n in names}
    return {"launches": sum(v["launches"] for v in per.values()), "kernel_ms": round(sum(v["ms"] for v in per.values()), 3),
            "wall_ms": round(statistics.median(w for _, w in runs), 3), "by_name": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", default="16,20,22,24")
    ap.add_argument("--gkr-logs", default="20,24")
    a = ap.parse_args()
    zk = z.Context(0)
    rng = np.random.default_rng(0)
    out = {"whir": [], "v1": [], "gkr_committed": []}
    for m in [int(x) for x in a.logs.split(",") if x]:
        col = zk.upload(rng.integers(0, P, size=1 << m, dtype=np.uint32))
        point = rng.integers(0, P, size=(m, 4), dtype=np.uint32)
        for b, k in ((1, 4), (2, 4), (1, 2)):
            prm = _params(b, k)

            def run():
                com = zk.whir_commit(prm, col, m)
                zk.whir_open(com, point)
                com.close()

            r = _profiled(zk, run, a.reps)
            r.update(m=m, log_blowup=b, fold_log=k, proof_words=z.whir_proof_words(prm, m, 1))
            out["whir"].append(r)
            print(json.dumps({k2: v for k2, v in r.items() if k2 != "by_name"}), file=sys.stderr)
        for b in (1, 2):
            ext = zk.upload(rng.integers(0, P, size=4 << (m + b), dtype=np.uint32))

            def v1():
                lde = zk.lde_batch(col, m, b, 1, 31)
                zk.merkle_commit([(lde, m + b, 1)], want_root=False)
                t, ln = ext, m + b
                while ln > 6:
                    t = zk.fri_fold(t, ln - 1, [1, 2, 3, 4])
                    ln -= 1
                    zk.merkle_commit([(t, ln - 1, 8)], want_root=False)

            r = _profiled(zk, v1, a.reps)
            r.update(m=m, log_blowup=b)
            out["v1"].append(r)
            print(json.dumps({k2: v for k2, v in r.items() if k2 != "by_name"}), file=sys.stderr)
        del col
    for L in [int(x) for x in a.gkr_logs.split(",") if x]:
        num = zk.upload(rng.integers(0, P, size=1 << L, dtype=np.uint32))
        den = zk.upload(rng.integers(0, P, size=4 << L, dtype=np.uint32))
        prm = _params(1, 4)
        r = _profiled(zk, lambda: zk.gkr_committed_prove(prm, num, den, L, [1]), a.reps)
        r.update(log_n=L, log_blowup=1, fold_log=4)
        out["gkr_committed"].append(r)
        print(json.dumps({k2: v for k2, v in r.items() if k2 != "by_name"}), file=sys.stderr)
        del num, den
    print(json.dumps(out))


if __name__ == "__main__":
    main()
