"""The two larger AIR sets of the cached-partition tests (docs/cached_main.md) whose model proofs take minutes in Python: the model's
words are recorded once in tests/golden/cached_batch_words.npz (written by `python tests/cached_batch_sets.py [names]`, which runs the
model alone) and the device prover's words are compared with them word for word (tests/test_gpu_cached_batch.py); the host verifier replays
them without a GPU (tests/test_cached_batch_cpu.py)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cached_batch_words.npz")


def _wm_params(b, k, fl, pow_bits, nq):
    import whir_model as wm

    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def big_set():
    """a program-like AIR of 2^16 rows (cached width 2, log_stack_cached 12: sixteen stacked columns a cached column) beside its
    sender at 2^3 and the range pair: (params, airs, traces, preps, pvs, log_stack, log_stack_prep, log_stack_cached, prefix)"""
    from test_cached_batch_cpu import _program_pair, _range_pair

    items = _program_pair(16, 3, seed=16) + _range_pair(2, mu=3, seed=16)
    airs, traces, preps, pvs = ([x[i] for x in items] for i in range(4))
    return _wm_params(1, 4, 4, 2, 3), airs, traces, preps, pvs, 16, 4, [12, None, None, None], [16]


def chipset_set():
    """twelve ChipSet chips of mixed heights up to 2^9 rows with the set's preprocessed range table, as generated; the leading three
    columns of the first tallest chip are declared cached (log_stack_cached 8)"""
    from zkvm_prover_amd import air

    gen = air.ChipSet(n_chips=12, log_max=9, log_min=3, total_width=84, seed=2).gen(seed=2)
    tall = max(range(len(gen)), key=lambda i: gen[i]["log_height"])
    assert gen[tall]["width"] > 3 and gen[-1].get("prep") is not None
    airs = [{k: a[k] for k in ("program", "log_height", "width", "n_pvs")} for a in gen]
    airs[tall]["program"] = air.with_cached_width(airs[tall]["program"], 3)
    traces = [np.asarray(a["trace"]).tolist() for a in gen]
    preps = [np.asarray(a["prep"]).tolist() if a.get("prep") is not None else None for a in gen]
    pvs = [[int(x) for x in a["pvs"]] for a in gen]
    lsc = [8 if i == tall else None for i in range(len(gen))]
    return _wm_params(1, 4, 2, 2, 3), airs, traces, preps, pvs, 12, 4, lsc, [12, 3]


SETS = {"big": big_set, "chipset": chipset_set}


def model_words(name):
    """(key root, cached roots, main root, words) of the model's proof of a set, with_bus = 1"""
    import cached_batch_model as cm
    import keyed_model as km
    from pymodel import Challenger

    prm, airs, traces, preps, pvs, l, lpr, lsc, prefix = SETS[name]()
    key = km.Key(prm, airs, preps, lpr)
    cached = [cm.Cached(prm, airs, a, traces[a], lsc[a]) if lsc[a] is not None else None for a in range(len(airs))]
    ch = Challenger()
    ch.observe(prefix)
    root, words, _ = cm.prove(ch, prm, airs, traces, preps, pvs, l, key, cached, True)
    return key.root, [c.root for c in cached if c], root, words


def recorded(name):
    with np.load(GOLDEN) as f:
        return f[name + "_key_root"], f[name + "_cached_roots"], f[name + "_root"], f[name + "_words"]


if __name__ == "__main__":
    import sys
    import time

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    out = {}
    if os.path.exists(GOLDEN):
        with np.load(GOLDEN) as f:
            out = {k: f[k] for k in f.files}
    for name in sys.argv[1:] or SETS:
        t = time.time()
        kr, cr, root, words = model_words(name)
        out.update({name + "_key_root": np.array(kr, dtype=np.uint32), name + "_cached_roots": np.array(cr, dtype=np.uint32),
                    name + "_root": np.array(root, dtype=np.uint32), name + "_words": np.array(words, dtype=np.uint32)})
        print(name, len(words), "words, %.0f s" % (time.time() - t), flush=True)
    np.savez_compressed(GOLDEN, **out)
