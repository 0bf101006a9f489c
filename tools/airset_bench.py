"""The AIR-set proof on the device (docs/airset.md) and its batched form (docs/airbatch.md, an `airbatch` row per shape): launches, kernel time per kernel name (the library's kernel stats,
zkhip_profile_*), wall time and proof words of zkhip_airset_prove, split into the bus part (as_* and gkr_*), the sum-checks (zc_*) and
commit plus opening (stack_*, whir_*), and beside it the fair comparison on the same key and the same library build: the two separate
calls zkhip_zerocheck_prove plus zkhip_bus_gkr_prove (which prove less: their bus proof is not tied to the committed traces), and
zkhip_prove.  Shapes: the lookup key of tools/gkr_bench.py (a sender of 2^20 rows, a table of 2^16) and the 42-chip ChipSet with a
main-column range table in place of its preprocessed one, and `chipset42_keyed`: ChipSet().gen() as generated, with its preprocessed
range table, proven through the key (Context.airkey; key generation is timed on its own, log_stack_prep = 4): a `keyed` row
(AirKey.prove) and, from the same key in the same run, a `keyed_batch` row (AirKey.prove_batch); `chipset42_cached`: the same set with
the four leading columns of chip 30 (one of its tallest, 2^16 rows, 8 columns) declared a cached main partition (docs/cached_main.md,
log_stack_cached = 16): a `keyed_batch` row (AirKey.prove_batch, which ignores the section), a `cached_batch` row
(AirKey.prove_batch_cached) and a `commit_cached` row (AirKey.commit_cached, once per program) from the same key in the same run.  Parameters (b, k, final_log) = (1, 4, 6), 80 queries and 16 bits of
grinding in every round; v1 parameters z.DEFAULT_PARAMS.  Every figure is the median of --reps runs after one warm-up.  Prints one
JSON object.

  python tools/airset_bench.py [--reps 3] [--shapes lookup20x16,chipset42,chipset42_keyed,chipset42_cached] [--no-v1]"""
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

NOPV = np.zeros(0, np.uint32)


def _lookup(ls, lt):
    snd, tab = air.lookup_traces(ls, lt, seed=1)
    return [dict(program=air.lookup_sender_air().program(), log_height=ls, width=3, n_pvs=0, trace=snd, pvs=NOPV),
            dict(program=air.lookup_table_air().program(), log_height=lt, width=3, n_pvs=0, trace=tab, pvs=NOPV)]


def _chipset():
    """the 42 chips; the set's range table has preprocessed keys (out of scope): a two-row table with its keys in a main column"""
    chips = air.ChipSet().gen()[:-1]
    counts = sum(np.bincount(c["trace"][1].astype(np.int64), minlength=2)[:2] for c in chips)
    tb = air.AirBuilder(2, 0)
    tb.push_interaction(air.ChipSet.RANGE_BUS, [tb.var(0)], tb.var(1), "receive")
    return chips + [dict(program=tb.program(), log_height=1, width=2, n_pvs=0, trace=np.array([[0, 1], counts % z.P], dtype=np.uint32), pvs=NOPV)]


CACHED_CHIP, CACHED_WIDTH, CACHED_LOG_STACK = 30, 4, 16


def _chipset_cached():
    airs = air.ChipSet().gen()
    airs[CACHED_CHIP] = dict(airs[CACHED_CHIP], program=air.with_cached_width(airs[CACHED_CHIP]["program"], CACHED_WIDTH))
    return airs


SHAPES = {
    # (AIRs, log_stack)
    "lookup20x16": (lambda: _lookup(20, 16), 20),
    "chipset42": (_chipset, 20),
    "chipset42_keyed": (lambda: air.ChipSet().gen(), 20),
    "chipset42_cached": (_chipset_cached, 20),
}
KEYED = {"chipset42_keyed": 4, "chipset42_cached": 4}   # shape -> log_stack_prep
CACHED = {"chipset42_cached": {CACHED_CHIP: CACHED_LOG_STACK}}   # shape -> AIR -> log_stack_cached


def _group(by_name):
    g = {k: {"launches": 0, "ms": 0.0} for k in ("bus", "sumchecks", "commit_and_opening")}
    for n, v in by_name.items():
        k = "bus" if n.startswith(("as_", "gkr_")) else "sumchecks" if n.startswith(("zc_", "zb_")) else "commit_and_opening"
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
    out = {"airbatch": [], "airset": [], "zerocheck": [], "bus_gkr": [], "v1": [], "keyed": [], "keyed_batch": [], "keygen": [],
           "cached_batch": [], "commit_cached": []}

    def note(r):
        print(json.dumps({k: v for k, v in r.items() if k != "by_name"}), file=sys.stderr)

    for name in [s for s in a.shapes.split(",") if s]:
        airs_fn, l = SHAPES[name]
        airs = airs_fn()
        vairs = [{k: x[k] for k in ("program", "log_height", "width", "n_pvs")} for x in airs]
        pvs = [x["pvs"] for x in airs]
        d = [zk.upload(np.asarray(x["trace"], dtype=np.uint32).reshape(-1)) for x in airs]
        words = z.airset_proof_words(prm, vairs, l)
        common = dict(shape=name, n_airs=len(airs), log_stack=l, total_cells=sum(x["width"] << x["log_height"] for x in airs))
        if name in KEYED:   # the set as generated, through the key; beside it zkhip_prove of the same set
            lpr, proof = KEYED[name], {}
            r = _profiled(zk, lambda: zk.airkey(prm, airs, lpr).close(), a.reps)
            r.update(common, log_stack_prep=lpr)
            out["keygen"].append(r)
            note(r)
            key = zk.airkey(prm, airs, lpr)

            def keyed():
                proof["p"] = key.prove(d, pvs, l, [1])[1]

            r = _profiled(zk, keyed, a.reps)
            z.airkey_verify(prm, [1], vairs, key.root, lpr, pvs, l, proof["p"])
            r.update(common, log_stack_prep=lpr, proof_words=z.airkey_proof_words(prm, vairs, l, lpr), split=_group(r["by_name"]))
            out["keyed"].append(r)
            note(r)

            def keyed_batch():   # the batched form of the same statement under the same key (docs/airbatch.md), same build, same run
                proof["b"] = key.prove_batch(d, pvs, l, [1])[1]

            r = _profiled(zk, keyed_batch, a.reps)
            z.airkey_batch_verify(prm, [1], vairs, key.root, lpr, pvs, l, proof["b"])
            r.update(common, log_stack_prep=lpr, proof_words=z.airkey_batch_proof_words(prm, vairs, l, lpr), split=_group(r["by_name"]),
                     zb_launches={n: v["launches"] for n, v in r["by_name"].items() if n.startswith("zb_")})
            out["keyed_batch"].append(r)
            note(r)
            if name in CACHED:   # the same set with the partition committed once, outside the proof (docs/cached_main.md)
                lsc = [CACHED[name].get(i) for i in range(len(airs))]
                r = _profiled(zk, lambda: [key.commit_cached(i, d[i], x).close() for i, x in enumerate(lsc) if x is not None], a.reps)
                r.update(common, log_stack_cached=CACHED[name])
                out["commit_cached"].append(r)
                note(r)
                cached = [key.commit_cached(i, d[i], x) if x is not None else None for i, x in enumerate(lsc)]

                def cached_batch():
                    proof["c"] = key.prove_batch_cached(d, pvs, cached, l, [1])[1]

                r = _profiled(zk, cached_batch, a.reps)
                roots = z.airkey_cached_verify(prm, [1], vairs, key.root, lpr, lsc, pvs, l, proof["c"])[2]
                assert roots.tolist() == [c.root.tolist() for c in cached if c is not None]
                r.update(common, log_stack_prep=lpr, proof_words=z.airkey_cached_proof_words(prm, vairs, l, lpr, lsc), split=_group(r["by_name"]),
                         zb_launches={n: v["launches"] for n, v in r["by_name"].items() if n.startswith("zb_")})
                out["cached_batch"].append(r)
                note(r)
                for c in cached:
                    if c is not None:
                        c.close()
            key.close()
            if not a.no_v1:
                pk = z.ProvingKey(zk, z.DEFAULT_PARAMS, airs)
                r = _profiled(zk, lambda: pk.prove(d, pvs), a.reps)
                r.update(common, proof_words=pk.proof_size // 4)
                out["v1"].append(r)
                note(r)
                pk.close()
            del d
            continue
        if not words:
            out["airset"].append(dict(common, refused=True))
            continue
        proof = {}

        def airbatch():   # the batched form of the same statement (docs/airbatch.md), same build, same run
            proof["b"] = zk.airbatch_prove(prm, vairs, d, pvs, l, [1])[1]

        r = _profiled(zk, airbatch, a.reps)
        z.airbatch_verify(prm, [1], vairs, pvs, l, proof["b"])
        r.update(common, proof_words=z.airbatch_proof_words(prm, vairs, l), split=_group(r["by_name"]),
                 zb_launches={n: v["launches"] for n, v in r["by_name"].items() if n.startswith("zb_")})
        out["airbatch"].append(r)
        note(r)

        def airset():
            proof["p"] = zk.airset_prove(prm, vairs, d, pvs, l, [1])[1]

        r = _profiled(zk, airset, a.reps)
        z.airset_verify(prm, [1], vairs, pvs, l, proof["p"])
        r.update(common, proof_words=words, split=_group(r["by_name"]))
        out["airset"].append(r)
        note(r)
        r = _profiled(zk, lambda: zk.zerocheck_prove(prm, vairs, d, pvs, l, [1]), a.reps)
        r.update(common, proof_words=z.zerocheck_proof_words(prm, vairs, l))
        out["zerocheck"].append(r)
        note(r)
        pk = z.ProvingKey(zk, z.DEFAULT_PARAMS, airs)
        r = _profiled(zk, lambda: pk.bus_gkr_prove(d, pvs, [1]), a.reps)
        r.update(common, proof_words=int(pk.bus_gkr_prove(d, pvs, [1]).size))
        out["bus_gkr"].append(r)
        note(r)
        if not a.no_v1:
            r = _profiled(zk, lambda: pk.prove(d, pvs), a.reps)
            r.update(common, proof_words=pk.proof_size // 4)
            out["v1"].append(r)
            note(r)
        pk.close()
        del d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
