"""LogUp-GKR on the device (docs/logup_gkr.md): launches and kernel time of zkhip_bus_gkr_prove next to the v1 LogUp phase of
zkhip_prove for the same key, and of zkhip_gkr_fraction_prove alone.  Kernel figures come from the library's kernel stats
(zkhip_profile_*); every figure is the median of --reps runs after one warm-up.  Prints one JSON object.

  python tools/gkr_bench.py [--reps 5] [--fraction-logs 16,20,24]

v1 LogUp phase = its own kernels (logup_chal / logup_denoms / ext_batch_inverse / logup_rows / logup_scan / logup_sums) from a
profiled zkhip_prove, plus the coset LDE and the Merkle commit of matrices of the permutation trace's shape (4 (groups + 1) columns
per chip with interactions, at the key's blow-up), timed on their own because they share kernel names with the main trace's."""
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
from zkvm_prover_amd import air  # noqa: E402

P = z.P
NOPV = np.zeros(0, np.uint32)
V1_LOGUP = ("logup_chal", "logup_denoms", "ext_batch_inverse", "logup_rows", "logup_scan", "logup_sums")


def _sync():
    import torch

    torch.cuda.synchronize()


def _profiled(zk, fn, reps):
    """median over reps of (launches, kernel ms by name, wall ms) of fn()"""
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
    out = {}
    for n in names:
        out[n] = {"launches": runs[0][0].get(n, (0, 0))[0], "ms": round(statistics.median(s.get(n, (0, 0.0))[1] for s, _ in runs), 4)}
    return out, round(statistics.median(w for _, w in runs), 3)


def _sum(stats, pred):
    sel = {n: v for n, v in stats.items() if pred(n)}
    return {"launches": sum(v["launches"] for v in sel.values()), "kernel_ms": round(sum(v["ms"] for v in sel.values()), 4),
            "by_kernel": sel}


def _lookup_key(log_s, log_t, sender_width, extra=()):
    s, t = air.lookup_traces(log_s, log_t, seed=9, sender_width=sender_width)
    return [dict(program=air.lookup_sender_air(sender_width).program(), log_height=log_s, width=sender_width, n_pvs=0, trace=s, pvs=NOPV),
            *extra,
            dict(program=air.lookup_table_air().program(), log_height=log_t, width=3, n_pvs=0, trace=t, pvs=NOPV)]


def _perm_shapes(airs):
    """(log_height, columns) of each chip's permutation trace: 4 (interaction groups + 1) extension coordinates"""
    out = []
    for a in airs:
        w = [int(x) for x in a["program"]]
        if 0x554C4B5A not in w[4:]:
            continue
        # the interaction section: [magic, n_int, then per interaction bus, sign, count, nf, fields.., group]
        q = len(w) - 1 - w[::-1].index(0x554C4B5A)
        n_int, q = w[q + 1], q + 2
        group = 0
        for _ in range(n_int):
            nf = w[q + 3]
            q += 4 + nf
            group = w[q]
            q += 1
        out.append((a["log_height"], 4 * (group + 2)))
    return out


def bench_key(zk, label, airs, params, reps):
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    prefix = [1, 2, 3, 4, 5, 6, 7, 8]
    gkr_stats, gkr_wall = _profiled(zk, lambda: pk.bus_gkr_prove(d_traces, pvs, prefix), reps)
    proof = pk.bus_gkr_prove(d_traces, pvs, prefix)
    z.bus_gkr_verify(prefix, proof, pk.bus_gkr_log_leaves())
    v1_stats, v1_wall = _profiled(zk, lambda: pk.prove(d_traces, pvs), reps)
    # the permutation trace's LDE + commit, at its shapes
    mats = [(zk.upload(np.random.default_rng(lh).integers(0, P, size=cols << lh, dtype=np.uint32)), lh, cols) for lh, cols in _perm_shapes(airs)]
    lb = params[0]

    def lde_commit():
        ldes = [(zk.lde_batch(t, lh, lb, cols, 31), lh + lb, cols) for t, lh, cols in mats]
        z.MerkleTree(zk, ldes, want_root=False).close()

    perm_stats, perm_wall = _profiled(zk, lde_commit, reps)
    v1 = _sum(v1_stats, lambda n: n in V1_LOGUP)
    perm = _sum(perm_stats, lambda n: True)
    return {
        "key": label,
        "leaves_log2": pk.bus_gkr_log_leaves(),
        "bus_gkr_prove": dict(_sum(gkr_stats, lambda n: True), wall_ms=gkr_wall),
        "v1_logup_phase": {"launches": v1["launches"] + perm["launches"], "kernel_ms": round(v1["kernel_ms"] + perm["kernel_ms"], 4),
                           "logup_kernels": v1, "perm_lde_commit": perm},
        "zkhip_prove_wall_ms": v1_wall,
    }


def bench_fraction(zk, log_n, reps):
    rng = np.random.default_rng(log_n)
    d_num = zk.upload(rng.integers(0, P, size=1 << log_n, dtype=np.uint32))
    d_den = zk.upload(rng.integers(0, P, size=4 << log_n, dtype=np.uint32))
    stats, wall = _profiled(zk, lambda: zk.gkr_prove(d_num, d_den, log_n, [1, 2, 3]), reps)
    proof, _, _ = zk.gkr_prove(d_num, d_den, log_n, [1, 2, 3])
    z.gkr_verify([1, 2, 3], proof, log_n)
    return dict(_sum(stats, lambda n: True), log_n=log_n, wall_ms=wall, proof_words=int(len(proof)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fraction-logs", default="16,20,24")
    ap.add_argument("--skip-keys", action="store_true")
    args = ap.parse_args()
    zk = z.Context(0)
    params = z.DEFAULT_PARAMS
    out = {"cmd": " ".join(["python"] + sys.argv), "keys": [], "fraction": []}
    if not args.skip_keys:
        out["keys"].append(bench_key(zk, "lookup 2^20 sender x 2^16 table", _lookup_key(20, 16, 3), params, args.reps))
        mix_tr, mix_pv = air.bus_mix_trace(16, 5)
        mix = dict(program=air.bus_mix_air().program(), log_height=16, width=6, n_pvs=1, trace=mix_tr, pvs=mix_pv)
        out["keys"].append(bench_key(zk, "lookup 2^18 x 16 fields + bus_mix 2^16 + table 2^12", _lookup_key(18, 12, 16, (mix,)), params,
                                     args.reps))
    for lg in [int(x) for x in args.fraction_logs.split(",") if x]:
        out["fraction"].append(bench_fraction(zk, lg, args.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
