"""The AIR zero-check on the device (docs/zerocheck.md): launches, kernel time per kernel name (the library's kernel stats,
zkhip_profile_*), wall time and proof words of zkhip_zerocheck_prove, split into commit (a zkhip_stack_commit of the same columns,
measured on its own), zero-check (the zc_* kernels) and opening (the stack_* and whir_* kernels less the commit), beside zkhip_prove
of the same key on the same library build, whose quotient evaluation and quotient commit are what the zero-check replaces.
`chipset42_keyed` is ChipSet().gen() as generated, with its preprocessed range table, proven through the key (Context.airkey,
with_bus = False, log_stack_prep = 4); key generation is timed on its own.
Parameters (b, k, final_log) = (1, 4, 6), 80 queries and 16 bits of grinding in every round; v1 parameters (1, 0, 100, 16, 16).  Every
figure is the median of --reps runs after one warm-up.  Prints one JSON object.

  python tools/zerocheck_bench.py [--reps 3] [--shapes synth18,synth20,synth22,chipset42,chipset42_keyed] [--no-v1]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import zkvm_prover_amd as z  # noqa: E402
from whir_bench import _profiled  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402


def _synth(log_n):
    sa = air.SyntheticAir()
    tr, pv = sa.gen_trace(log_n, seed=1)
    return [dict(program=sa.program(), log_height=log_n, width=sa.width, n_pvs=len(pv), trace=tr, pvs=pv)]


def _chipset():
    return air.ChipSet().gen()[:-1]   # the 42 chips; the range table has preprocessed keys (out of scope)


SHAPES = {
    # (AIRs, log_stack)
    "synth18": (lambda: _synth(18), 21),
    "synth20": (lambda: _synth(20), 23),
    "synth22": (lambda: _synth(22), 25),
    "chipset42": (_chipset, 20),
    "chipset42_keyed": (lambda: air.ChipSet().gen(), 20),
}
KEYED = {"chipset42_keyed": 4}   # shape -> log_stack_prep


def _group(by_name):
    g = {"zerocheck": {"launches": 0, "ms": 0.0}, "commit_and_opening": {"launches": 0, "ms": 0.0}}
    for n, v in by_name.items():
        k = "zerocheck" if n.startswith("zc_") else "commit_and_opening"
        g[k]["launches"] += v["launches"]
        g[k]["ms"] = round(g[k]["ms"] + v["ms"], 3)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-v1", action="store_true")
    a = ap.parse_args()
    zk = z.Context(0)
    prm = z.WhirParams.make(1, 4, 6, 16, 80)
    out = {"zerocheck": [], "commit": [], "v1": [], "keygen": []}
    for name in [s for s in a.shapes.split(",") if s]:
        airs_fn, l = SHAPES[name]
        airs = airs_fn()
        vairs = [{k: x[k] for k in ("program", "log_height", "width", "n_pvs")} for x in airs]
        pvs = [x["pvs"] for x in airs]
        d = [zk.upload(np.asarray(x["trace"], dtype=np.uint32).reshape(-1)) for x in airs]
        cols = [t[c << x["log_height"]:(c + 1) << x["log_height"]] for t, x in zip(d, airs) for c in range(x["width"])]
        lpr = KEYED.get(name)
        words = z.airkey_proof_words(prm, vairs, l, lpr, False) if lpr is not None else z.zerocheck_proof_words(prm, vairs, l)
        common = dict(shape=name, n_airs=len(airs), n_cols=len(cols), log_stack=l, total_cells=sum(x["width"] << x["log_height"] for x in airs))
        if not words:
            out["zerocheck"].append(dict(common, refused=True))
            continue
        proof, key = {}, None
        if lpr is not None:
            r = _profiled(zk, lambda: zk.airkey(prm, airs, lpr).close(), a.reps)
            r.update(common, log_stack_prep=lpr)
            out["keygen"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
            key = zk.airkey(prm, airs, lpr)

        def zerocheck():
            if key is not None:
                proof["p"] = key.prove(d, pvs, l, [1], with_bus=False)[1]
            else:
                proof["p"] = zk.zerocheck_prove(prm, vairs, d, pvs, l, [1])[1]

        r = _profiled(zk, zerocheck, a.reps)
        if key is not None:
            z.airkey_verify(prm, [1], vairs, key.root, lpr, pvs, l, proof["p"], False)
            key.close()
        else:
            z.zerocheck_verify(prm, [1], vairs, pvs, l, proof["p"])
        r.update(common, proof_words=words, split=_group(r["by_name"]))
        out["zerocheck"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
        r = _profiled(zk, lambda: zk.stack_commit(prm, cols, l).close(), a.reps)
        r.update(common)
        out["commit"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
        if not a.no_v1:
            pk = z.ProvingKey(zk, z.DEFAULT_PARAMS, airs)
            r = _profiled(zk, lambda: pk.prove(d, pvs), a.reps)
            r.update(common, proof_words=pk.proof_size // 4)
            out["v1"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)
            pk.close()
        del d, cols
    print(json.dumps(out))


if __name__ == "__main__":
    main()
