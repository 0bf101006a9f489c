"""Operand-family sets of the batched AIR-set forms (docs/boundary_tests.md, "The batched AIR-set forms: operand families"), shared by
tests/test_zb_families_cpu.py and tests/test_gpu_zb_boundary.py.  Every set mixes heights and degree classes, so that the arithmetic the
batched kernels own (the extension of s_a from 0..D_a to 0..D, the weights mu^j 2^(M - m_a), the used-up AIRs' halved constants, the
reduction's 2^(M' - m_a)) carries non-trivial values while the traces are the families of tests/boundary_inputs.py:

  mixed_nobus   airbatch_prove without the bus part: Fibonacci m = 1, deg0 m = 2, SyntheticAir degree 3 m = 2, all_rot(3) m = 5,
                SyntheticAir degree 5 m = 3
  mixed_bus     airbatch_prove with it: bus_mix at m = 1, 3, 5 and a lookup pair (sender m = 2, table m = 4); the three count-column
                variants are applied to every count column at once
  keyed         AirKey.prove_batch, both with_bus values: the range table (PREP, m = 1) and its user (no PREP, m = 4) of one degree,
                Fibonacci m = 5, the hand-built AIR with rotations on both traces (PREP, D = 4, m = 3), the variable range table (PREP,
                D = 2, m = 4) and its user (m = 2); a second pass puts two families into the preprocessed columns (a key per family)
  cached        AirKey.prove_batch_cached: the keyed set with Fibonacci's first column a cached partition at m = 5, and a program AIR
                with a cached partition at m = 1 beside its sender; the families go into the cached columns too

A family is (name, traces, preps, pvs); family 0 is the builders' own satisfying traces ("honest"), the others hold one member of
boundary_inputs.families in every trace (named after the tallest AIR's list: a shorter AIR has fewer periods and positions and takes
its nearest member), public values rotating through PV_POOL.  `model(set, with_bus, i)` is the independent model's proof of family i
(cached: the GPU tests of one set share it), None if a denominator of the bus part is zero."""
import functools

import numpy as np

import airbatch_model as bm
import boundary_inputs as bi
import cached_batch_model as cm
import gkr_model as gm
import keyed_batch_model as kb
import keyed_model as km
import whir_model as wm
import zc_edge_shapes as es
from pymodel import P, Challenger
from test_airset_cpu import PARAM_SETS, _bus_mix, _lookup
from test_cached_batch_cpu import _cached, _program_pair
from test_keyed_cpu import _fib as _kfib
from test_keyed_cpu import _hand, _range_pair, _var_range_pair
from test_zerocheck_cpu import _fib, _synth
from zkvm_prover_amd import air

SEED, PV_POOL = es.SEED, es.PV_POOL
SETS = ["mixed_nobus", "mixed_bus", "keyed", "cached"]
GROUP = 4            # families of one GPU case
PREP_FAMILIES = ("boundary", "const raw 0x%08x" % (P - 1))
VALUE_FAMILIES = ("boundary", "alternate raw p-1/0 period 2", "delta at 0")
ALL_ROT_M = 5


def _kind(name):
    for k in ("const", "alternate raw", "alternate canonical", "delta"):
        if name.startswith(k):
            return k
    return name


def family_traces(shapes, seed):
    """[(name, [one [width, 2^m] trace per (width, m) of `shapes`])]: member i of a kind for the tallest shape is member i of the same
    kind for every other one (its last member for the last, and where it has fewer)"""
    per = [bi.families(np.random.default_rng(seed + a), w, 1 << m) for a, (w, m) in enumerate(shapes)]
    groups = []
    for fams in per:
        g = {}
        for name, t in fams:
            g.setdefault(_kind(name), []).append(t)
        groups.append(g)
    tall = max(range(len(shapes)), key=lambda a: shapes[a][1])
    out, seen = [], {}
    for name, _ in per[tall]:
        k = _kind(name)
        i, n = seen.get(k, 0), len(groups[tall][k])
        seen[k] = i + 1
        out.append((name, [g[k][len(g[k]) - 1 if i == n - 1 else min(i, len(g[k]) - 1)] for g in groups]))
    return out


def _pvs(airs, i):
    return [[PV_POOL[(i + a + j) % 4] for j in range(x["n_pvs"])] for a, x in enumerate(airs)]


def _arr(traces):
    return [np.ascontiguousarray(np.asarray(t, dtype=np.int64) % P, dtype=np.uint32) for t in traces]


@functools.lru_cache(maxsize=None)
def fset(name):
    """dict(form, airs, l, lpr, lsc, with_bus: the values the set runs under, count_cols, fams)"""
    lpr, lsc, count_cols = None, None, {}
    if name == "mixed_nobus":
        items = [_fib(1), es.deg0(2), _synth(2, 3), es.all_rot(3, ALL_ROT_M), _synth(3, 5)]
        form, l, wbs = "airbatch", 4, (False,)
    elif name == "mixed_bus":
        items = [_bus_mix(1), _lookup(2, 4)[0], _bus_mix(5), _lookup(2, 4)[1], _bus_mix(3)]
        form, l, wbs, count_cols = "airbatch", 4, (True,), {0: 3, 2: 3, 3: 2, 4: 3}
    else:
        rt, ru = _range_pair(1, mu=4, seed=1)
        vt, vu = _var_range_pair(3, mu=2)
        items = [rt, _kfib(5), _hand(3), ru, vt, vu]
        form, l, lpr, wbs = "keyed", 4, 3, (True, False)
        if name == "cached":
            items = [rt, _cached(_kfib(5), 1), _hand(3), ru, vt, vu] + _program_pair(1, 2, seed=1)
            form, lsc = "cached", [None, 3, None, None, None, None, 2, None]
    airs = [x[0] for x in items]
    honest = _arr([x[1] for x in items])
    preps = [(_arr([x[2]])[0] if x[2] is not None else None) for x in items] if form != "airbatch" else [None] * len(items)
    hpvs = [[int(v) for v in x[-1]] for x in items]
    fams = [("honest", honest, preps, hpvs)]
    shapes = [(a["width"], a["log_height"]) for a in airs]
    for name_f, traces in family_traces(shapes, SEED + 1000 * SETS.index(name)):
        fams.append((name_f, traces, preps, _pvs(airs, len(fams))))
    for vname, v in (("raw p-1", PV_POOL[3]), ("canonical p-1", P - 1), ("zero", 0)):
        if count_cols:
            traces = [t.copy() for t in honest]
            for a, col in count_cols.items():
                traces[a][col] = v
            fams.append(("count " + vname, traces, preps, _pvs(airs, len(fams))))
    if form != "airbatch":   # the second pass: the families in the preprocessed columns, the main traces honest
        with_prep = [a for a, p in enumerate(preps) if p is not None]
        by_name = dict(family_traces([preps[a].shape[0:1] + (airs[a]["log_height"],) for a in with_prep], SEED + 7 + 1000 * SETS.index(name)))
        for name_f in PREP_FAMILIES:
            pr = list(preps)
            for a, t in zip(with_prep, by_name[name_f]):
                pr[a] = t
            fams.append(("prep " + name_f, honest, pr, _pvs(airs, len(fams))))
    return dict(form=form, airs=airs, l=l, lpr=lpr, lsc=lsc, with_bus=wbs, fams=fams)


def groups(name):
    return list(range((len(fset(name)["fams"]) + GROUP - 1) // GROUP))


CASES = [(name, wb, g) for name in SETS for wb in fset(name)["with_bus"] for g in groups(name)]


def case_families(name, g):
    return list(range(GROUP * g, min(GROUP * (g + 1), len(fset(name)["fams"]))))


def prm_index(name, wb, i):
    """the two parameter sets alternate over the cases"""
    return CASES.index((name, wb, i // GROUP)) % 2


def prefix_of(name, wb, i):
    return [SETS.index(name), int(wb), i]


def satisfied(name, i):
    """every trace of family i passes air.check_trace"""
    S = fset(name)
    _, traces, preps, pvs = S["fams"][i]
    return all(air.check_trace(a["program"], t, pv, **({"prep": p} if p is not None else {})) == []
               for a, t, p, pv in zip(S["airs"], traces, preps, pvs))


def _lists(traces):
    return [t.tolist() if t is not None else None for t in traces]


@functools.lru_cache(maxsize=None)
def model(name, wb, i):
    """the model's proof of family i, continuing a challenger that observed prefix_of: dict(root, words, info, accepted: the model's
    verifier took it, balanced: the GKR's P is zero (True without the bus part), key_root, cached_roots), or None for a zero denominator"""
    S = fset(name)
    prm = PARAM_SETS[prm_index(name, wb, i)]
    airs, l, lpr, lsc, form = S["airs"], S["l"], S["lpr"], S["lsc"], S["form"]
    _, traces, preps, pvs = S["fams"][i]
    traces, preps = _lists(traces), _lists(preps)
    ch = Challenger()
    ch.observe(prefix_of(name, wb, i))
    out = dict(key_root=None, cached_roots=[])
    try:
        if form == "airbatch":
            root, words, info = bm.prove(ch, prm, airs, traces, pvs, l, wb, leaf_hook=es.no_zero_den)
            gkr_at = 8
        else:
            key = km.Key(prm, airs, preps, lpr)
            out["key_root"] = list(key.root)
            if form == "keyed":
                root, words, info = kb.prove(ch, prm, airs, traces, preps, pvs, l, key, wb, leaf_hook=es.no_zero_den)
                gkr_at = 8
            else:
                cached = [cm.Cached(prm, airs, a, traces[a], lsc[a]) if lsc[a] is not None else None for a in range(len(airs))]
                out["cached_roots"] = [list(c.root) for c in cached if c]
                root, words, info = cm.prove(ch, prm, airs, traces, preps, pvs, l, key, cached, wb, leaf_hook=es.no_zero_den)
                gkr_at = 8 + info["pre"]
    except es.ZeroDenominator:
        return None
    ch = Challenger()
    ch.observe(prefix_of(name, wb, i))
    try:
        if form == "airbatch":
            bm.verify(ch, prm, airs, pvs, l, words, wb)
        elif form == "keyed":
            kb.verify(ch, prm, airs, out["key_root"], lpr, pvs, l, words, wb)
        else:
            cm.verify(ch, prm, airs, out["key_root"], lpr, lsc, pvs, l, words, wb)
        accepted = True
    except (wm.WhirReject, gm.GkrReject):
        accepted = False
    out.update(root=root, words=words, info=info, accepted=accepted, balanced=not wb or words[gkr_at:gkr_at + 4] == bm.ZERO)
    return out


def plans_of(name, wb):
    """(plans, active AIRs, M, D, reducing AIRs, M') of a set under either PARAM_SETS member (the plans do not depend on it)"""
    S = fset(name)
    if S["form"] == "airbatch":
        plans = bm.shape(PARAM_SETS[0], S["airs"], S["l"], wb)[0]
        return (plans,) + tuple(bm.dims(plans))
    plans = [km.Plan(a, wb) for a in S["airs"]]
    return (plans,) + tuple(kb.dims(plans))
