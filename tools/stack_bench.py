"""The stacked WHIR commitment on the device (docs/stacking.md): launches, kernel time (the library's kernel stats, zkhip_profile_*),
wall time and proof words of zkhip_stack_commit + zkhip_stack_open, against one zkhip_whir_commit + zkhip_whir_open per height class
of the same columns.  Parameters (b, k, final_log) = (1, 4, 6), 80 queries and 16 bits of grinding in every round.  Every figure is the
median of --reps runs after one warm-up.  Prints one JSON object.

  python tools/stack_bench.py [--reps 3] [--shapes 48col,wide64,bus_keys]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zkvm_prover_amd as z  # noqa: E402
from whir_bench import _profiled  # noqa: E402

P = z.P


def _bus_key_heights():
    """the main traces of the GKR bus keys (tests/test_gpu_gkr.py, mix_and_lookup): one column per trace column"""
    from test_gpu_gkr import _cases

    return [a["log_height"] for a in _cases()["mix_and_lookup"] for _ in range(a["width"])]


SHAPES = {
    # (heights, log_stack)
    "48col": (lambda: [m for m in (20, 18, 16, 14, 12, 10) for _ in range(8)], 20),
    "wide64": (lambda: [22] * 8 + [21] * 8 + [20] * 8 + [19] * 16, 20),
    "bus_keys": (_bus_key_heights, 9),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    zk = z.Context(0)
    prm = z.WhirParams.make(1, 4, 6, 16, 80)
    rng = np.random.default_rng(0)
    out = {"stacked": [], "separate": []}
    for name in [s for s in a.shapes.split(",") if s]:
        heights_fn, l = SHAPES[name]
        heights = heights_fn()
        classes = sorted(set(heights), reverse=True)
        cols = {m: zk.upload(rng.integers(0, P, size=(heights.count(m), 1 << m), dtype=np.uint32).reshape(-1)) for m in classes}
        points = [rng.integers(0, P, size=(m, 4), dtype=np.uint32) for m in classes]
        # the stacked form: every column a view of its class's tensor; column j on its class's point
        views, cnt = [], {m: 0 for m in classes}
        for m in heights:
            views.append(cols[m][cnt[m] << m:(cnt[m] + 1) << m])
            cnt[m] += 1
        col_point = [classes.index(m) for m in heights]

        def stacked():
            scom = zk.stack_commit(prm, views, l)
            zk.stack_open(scom, points, col_point)
            scom.close()

        def separate():
            for m, pt in zip(classes, points):
                com = zk.whir_commit(prm, cols[m], m)
                zk.whir_open(com, pt)
                com.close()

        common = dict(shape=name, n_cols=len(heights), log_stack=l, total_cells=sum(1 << m for m in heights))
        r = _profiled(zk, stacked, a.reps)
        r.update(common, n_stack=z.stack_width(prm, heights, l), proof_words=z.stack_proof_words(prm, heights, l))
        out["stacked"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
        r = _profiled(zk, separate, a.reps)
        r.update(common, openings=len(classes), proof_words=sum(z.whir_proof_words(prm, m, heights.count(m)) for m in classes))
        out["separate"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
        del cols, views
    print(json.dumps(out))


if __name__ == "__main__":
    main()
