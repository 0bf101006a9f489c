"""CPU: the verifier circuits of the aggregation layer, PINNED (zkvm-prover_amd/csrc/recursion.hip).  The other circuit tests check that a
circuit accepts and rejects; a gate that moves changes the node key's commitment without changing either.  Here one circuit per build
form is hashed -- wire / gate / permutation counts, the three chips' programs, heights and preprocessed traces, the same again after
`pad` -- and its witness is run on fixed oracle proofs: the wire values, the node's public values, the return code and the error text
(which names the first failing gate) of an accepted run with every child, one with fewer children and one with a tampered child.
Everything is compared with tests/golden/recursion_fingerprints.json (written by tests/golden/gen_recursion_fingerprints.py).

The forms: leaf (mode 0) without / with an app id, internal (1), wrapper (1, uniform), uniform node over two leaf shapes (2), deferral
node over roots / over joins (3), join over a deferral node / over a fold of deferral nodes (4), and a leaf whose child key has cached
partitions, a preprocessed trace and a final polynomial.  The shapes are those of tests/test_recursion_cpu.py and
tests/test_deferral_cpu.py with the arities cut to two.  Every circuit is built a second time with `parallel_queries` off: the witness
of the accepted run must not depend on how the queries are scheduled."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import zkvm_prover_amd as z

import recursion_util as ru

PARAMS = (1, 0, 4, 3, 3)
CACHED_PARAMS = (2, 2, 3, 2, 2)
NOPV = ru.NOPV
REGION_BASE = 0x00402000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recursion_fingerprints.json")
FORMS = ["leaf", "leaf_app_id", "internal", "wrapper", "uniform_two_shapes", "deferral", "deferral_over_joins", "join_deferral_node",
         "join_fold", "leaf_cached_prep_final_poly"]


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _air_words(rc):
    for a in rc.airs():
        yield a["program"].astype(np.uint32)
        yield np.array([a["log_height"], a["width"], a["n_pvs"]], np.uint64)
        yield a["prep"].astype(np.uint32)


def _stats(rc):
    out = (C.c_size_t * 4)()
    assert rc.lib.zkhip_recursion_stats(rc.h, out) == 0
    return [int(x) for x in out]


def _set_parallel_queries(on):
    cfg = z.Config.default()
    if not on:
        cfg.parallel_queries = 0
    assert z.load_library().zkhip_set_process_config(C.byref(cfg)) == 0


def _tamper(proof, word=300):
    bad = bytearray(proof)
    bad[4 * word] ^= 1
    return bytes(bad)


def _run(rc, args):
    st, npv = rc.witness(*args[0], **args[1])
    return dict(status=int(st), wires=_sha([rc.wires()]), public_values=_sha([npv]), error=rc.last_error())


def fingerprint(form):
    """form: dict(circuit, build, full, partial, tampered) -- `circuit` as the tests built it, `build()` the same circuit once more."""
    rc = form["circuit"]
    out = dict(stats=_stats(rc))
    runs = {k: _run(rc, form[k]) for k in ("full", "partial", "tampered") if form.get(k)}
    _set_parallel_queries(False)
    try:
        twin = form["build"]()
    finally:
        _set_parallel_queries(True)
    serial = _run(twin, form["full"])
    lh = twin.log_heights()
    words = list(_air_words(rc))
    assert _sha(words) == _sha(_air_words(twin))   # (the schedule is no part of the circuit)
    twin.pad(lh[0] + 1, lh[1] + 1)
    out["circuit"] = _sha([np.array(out["stats"], np.uint64)] + words + list(_air_words(twin)))
    out["witness"] = runs
    twin.close()
    return out, serial


def _node(ora, params, rc, npv):
    """(proof bytes, verifying AIRs) of the node whose witness was just run on `rc`."""
    node = ru.node_instance(rc, npv)
    return ora.stark_prove(params, node).tobytes(), ru.verifying(params, node)


def _plain(proofs, pvs):
    return ((proofs, pvs), {})


def _nodes(children):
    return ([c[0] for c in children], [[NOPV, NOPV, c[1]] for c in children])


def build_forms(ora):
    F = {}
    # ---- the app: counter segments (tests/test_recursion_cpu.py); the narrow shape carries no Fibonacci chip ----
    segs = [ru.counter_segment(s, seed=i) for i, s in enumerate([5, 12, 19, 26])]
    narrow_seg = [segs[2][0], segs[2][1], segs[2][3]]
    proofs = [ora.stark_prove(PARAMS, k).tobytes() for k in segs]
    pvs = [[a["pvs"] for a in k] for k in segs]
    vk, vk_narrow = ru.verifying(PARAMS, segs[0]), ru.verifying(PARAMS, narrow_seg)

    def mk_leaf():
        return z.RecursionCircuit(PARAMS, vk, 4, stmt=ru.COUNTER_STMT)

    leaf = mk_leaf()
    F["leaf"] = dict(circuit=leaf, build=mk_leaf, full=_plain(proofs, pvs), partial=_plain(proofs[:2], pvs[:2]),
                     tampered=_plain([proofs[0], _tamper(proofs[1])], pvs[:2]))
    app_id = z.vk_digest(PARAMS, vk_narrow)

    def mk_leaf_app():
        return z.RecursionCircuit(PARAMS, vk, 2, stmt=ru.COUNTER_STMT, uniform=True, app_id=app_id)

    leaf_app = mk_leaf_app()
    F["leaf_app_id"] = dict(circuit=leaf_app, build=mk_leaf_app, full=_plain(proofs[:2], pvs[:2]), partial=_plain(proofs[:1], pvs[:1]),
                            tampered=_plain([_tamper(proofs[0]), proofs[1]], pvs[:2]))

    # ---- internal circuit over proofs of the leaf circuit ----
    kids, nvk = [], None
    for g in ([0, 1], [2, 3]):
        st, npv = leaf.witness([proofs[i] for i in g], [pvs[i] for i in g])
        assert st == 0, leaf.last_error()
        pr, nvk = _node(ora, PARAMS, leaf, npv)
        kids.append((pr, npv))

    def mk_internal():
        return z.RecursionCircuit(PARAMS, nvk, 2, stmt="node")

    F["internal"] = dict(circuit=mk_internal(), build=mk_internal, full=(_nodes(kids), {}), partial=(_nodes(kids[:1]), {}),
                         tampered=(_nodes([kids[0], (_tamper(kids[1][0]), kids[1][1])]), {}))

    # ---- wrapper: one fixed node key with the one-key layout, restated ----
    wkids, wvk = [], None
    for i in (0, 1):
        st, npv = leaf_app.witness([proofs[i]], [pvs[i]])
        assert st == 0, leaf_app.last_error()
        pr, wvk = _node(ora, PARAMS, leaf_app, npv)
        wkids.append((pr, npv))

    def mk_wrapper():
        return z.RecursionCircuit(PARAMS, wvk, 2, stmt="node", uniform=True)

    F["wrapper"] = dict(circuit=mk_wrapper(), build=mk_wrapper, full=(_nodes(wkids), {}), partial=(_nodes(wkids[:1]), {}),
                        tampered=(_nodes([(_tamper(wkids[0][0]), wkids[0][1]), wkids[1]]), {}))

    # ---- uniform node over two leaf shapes (shape 0 = narrow, shape 1 = the full set) ----
    nproof = ora.stark_prove(PARAMS, narrow_seg).tobytes()
    npvs = [a["pvs"] for a in narrow_seg]
    leafs, internal, _ = ru.one_key_circuits_shapes(PARAMS, [vk_narrow, vk], ru.COUNTER_STMT, arity_leaf=2, arity_internal=2)
    keys = [ru.node_key_commits(PARAMS, l.airs()) for l in leafs]
    int_pcs, IC = ru.node_key_commits(PARAMS, internal.airs())
    st, a = leafs[1].witness(proofs[:2], pvs[:2])
    assert st == 0, leafs[1].last_error()
    st, b = leafs[0].witness([nproof], [npvs])
    assert st == 0, leafs[0].last_error()
    ukids = [(_node(ora, PARAMS, leafs[1], a)[0], a), (_node(ora, PARAMS, leafs[0], b)[0], b)]
    H = internal.log_heights()[:2]
    child = [{k: x[k] for k in ("program", "log_height", "width", "n_pvs")} for x in leafs[0].airs()]

    def mk_uniform():
        return z.RecursionCircuit(PARAMS, child, 2, stmt="uniform", min_log_height=H, n_leaf_shapes=2)

    def uni(children, kinds):
        return (_nodes(children), dict(prep_commits=[keys[k - 1][0] if k else int_pcs for k in kinds], is_leaf=kinds,
                                       leaf_commit=np.concatenate([keys[0][1], keys[1][1]]), internal_commit=IC))

    F["uniform_two_shapes"] = dict(circuit=internal, build=mk_uniform, full=uni(ukids, [2, 1]), partial=uni(ukids[:1], [2]),
                                   tampered=uni([ukids[0], (_tamper(ukids[1][0]), ukids[1][1])], [2, 1]))

    # ---- the deferral circuits over toy guest flows (tests/test_deferral_cpu.py) ----
    rng = np.random.default_rng(5)

    def dig():
        return rng.integers(0, ora.P, 8, dtype=np.uint64).astype(np.uint32)

    image, mid = dig(), dig()
    seg0 = ru.state_segment([0x200000] + list(image), [0x200040] + list(mid))
    sleaf, sint = ru.one_key_circuits(PARAMS, ru.verifying(PARAMS, seg0), ru.STATE_STMT, arity_leaf=2, arity_internal=2)
    leaf_pcs, LC = ru.node_key_commits(PARAMS, sleaf.airs())
    sint_pcs, SIC = ru.node_key_commits(PARAMS, sint.airs())
    ivk = ru.verifying(PARAMS, [dict(x, prep_commit=c) for x, c in zip(sint.airs(), sint_pcs)])

    def child_flow(pv_bytes, region=None):
        extra = {}
        if region is None:
            root1, cells, sibs = ru.memory_root_with_public_values(pv_bytes, rng)
        else:
            root1, cells, sibs, rsibs, ridx = ru.memory_root_with_public_values_and_region(pv_bytes, region, REGION_BASE, rng)
            extra = dict(region=np.asarray(region, np.uint32), region_sibs=rsibs, region_index=ridx)
        ss = [ru.state_segment([0x200000] + list(image), [0x200040] + list(mid)), ru.state_segment([0x200040] + list(mid), [0] + list(root1))]
        sp = [ora.stark_prove(PARAMS, s).tobytes() for s in ss]
        st, npv = sleaf.witness(sp, [[x["pvs"] for x in s] for s in ss])
        assert st == 0, sleaf.last_error()
        lp = _node(ora, PARAMS, sleaf, npv)[0]
        st, rpv = sint.witness([lp], [[NOPV, NOPV, npv]], prep_commits=[leaf_pcs], is_leaf=[1], leaf_commit=LC, internal_commit=SIC)
        assert st == 0, sint.last_error()
        rp = _node(ora, PARAMS, sint, rpv)[0]
        return dict(proof=rp, pvs=rpv, aux=np.concatenate([cells, sibs.reshape(-1)]), cells=cells, **extra)

    flows = [child_flow(bytes([i + 1] * 32)) for i in range(2)]

    def dfr(ks, **kw):
        return (([k["proof"] for k in ks], [[NOPV, NOPV, k["pvs"]] for k in ks]), dict(aux=[k["aux"] for k in ks], **kw))

    def mk_deferral():
        return z.RecursionCircuit(PARAMS, ivk, 2, stmt="deferral")

    D = mk_deferral()
    F["deferral"] = dict(circuit=D, build=mk_deferral, full=dfr(flows), partial=dfr(flows[:1]),
                         tampered=dfr([flows[0], dict(flows[1], proof=_tamper(flows[1]["proof"]))]))

    def d_node(ks, **kw):
        args = dfr(ks, **kw)
        st, dpv = D.witness(*args[0], **args[1])
        assert st == 0, D.last_error()
        pr, dvk = _node(ora, PARAMS, D, dpv)
        return pr, dpv, dvk

    claims = [ru.deferral_claim(k["pvs"], k["cells"]) for k in flows]
    dproof, dpv, dvk = d_node(flows)

    def mk_join():
        return z.RecursionCircuit.join(PARAMS, ivk, PARAMS, dvk)

    J = mk_join()
    g = child_flow(bytes([0x42] * 32), region=ru.deferral_region_cells(claims))   # a guest that deferred: its memory holds the claims
    root = (g["proof"], g["pvs"])
    F["join_deferral_node"] = dict(circuit=J, build=mk_join, full=(_nodes([root, (dproof, dpv)]), {}),
                                   tampered=(_nodes([root, (_tamper(dproof), dpv)]), {}))
    st, jpv = J.witness(*F["join_deferral_node"]["full"][0])
    assert st == 0, J.last_error()
    jproof, jvk = _node(ora, PARAMS, J, jpv)
    batch = dict(g, proof=jproof, pvs=jpv)
    batch["aux"] = np.concatenate([g["aux"], g["region"], g["region_sibs"].reshape(-1), np.array([1 if k < len(claims) else 0 for k in range(63)], np.uint32)])

    def mk_deferral_joins():
        return z.RecursionCircuit(PARAMS, jvk, 2, stmt="deferral", region_index=g["region_index"])

    # (the children of a deferral node do not chain: the one batch proof stands in both slots)
    F["deferral_over_joins"] = dict(circuit=mk_deferral_joins(), build=mk_deferral_joins, full=dfr([batch, batch]), partial=dfr([batch]),
                                    tampered=dfr([batch, dict(batch, proof=_tamper(batch["proof"]))]))

    # ---- a fold of two deferral nodes in slot 1 of the join (32 public values) ----
    zero = np.zeros(8, np.uint32)
    p0, d0, _ = d_node(flows[:1])
    p1, d1, _ = d_node(flows[1:], acc_start=ru.deferral_chain(zero, claims[:1]))
    fold = z.RecursionCircuit(PARAMS, dvk, 2, stmt=dict(start=[(2, k) for k in range(8)], end=[(2, 8 + k) for k in range(8)]))
    st, fpv = fold.witness(*_nodes([(p0, d0), (p1, d1)]))
    assert st == 0, fold.last_error()
    fproof, fvk = _node(ora, PARAMS, fold, fpv)

    def mk_join_fold():
        return z.RecursionCircuit.join(PARAMS, ivk, PARAMS, fvk)

    F["join_fold"] = dict(circuit=mk_join_fold(), build=mk_join_fold, full=(_nodes([root, (fproof, fpv)]), {}),
                          tampered=(_nodes([(_tamper(root[0]), root[1]), (fproof, fpv)]), {}))

    # ---- cached partitions, a preprocessed trace, blow-up 4, a final polynomial of four coefficients ----
    from test_cached_main_cpu import cached_case

    cairs = cached_case()
    cproof = ora.stark_prove(CACHED_PARAMS, cairs).tobytes()
    cpvs = [x["pvs"] for x in cairs]
    cvk = ru.verifying(CACHED_PARAMS, cairs)

    def mk_cached():
        return z.RecursionCircuit(CACHED_PARAMS, cvk, 2)

    # (no chained state: the one proof stands in both slots)
    F["leaf_cached_prep_final_poly"] = dict(circuit=mk_cached(), build=mk_cached, full=_plain([cproof, cproof], [cpvs, cpvs]),
                                            partial=_plain([cproof], [cpvs]), tampered=_plain([cproof, _tamper(cproof)], [cpvs, cpvs]))
    assert sorted(F) == sorted(FORMS)
    return F


@pytest.fixture(scope="module")
def forms(ora):
    return build_forms(ora)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", FORMS)
def test_circuit_and_witness_are_the_recorded_ones(forms, golden, name):
    got, serial = fingerprint(forms[name])
    want = golden[name]
    assert got["stats"] == want["stats"]
    assert got["circuit"] == want["circuit"]
    runs = got["witness"]
    assert sorted(runs) == sorted(want["witness"])
    for k in runs:
        assert runs[k] == want["witness"][k], k
    assert runs["full"]["status"] == 0 and runs["full"]["error"] == ""
    assert "partial" not in runs or runs["partial"]["status"] == 0
    assert runs["tampered"]["status"] == -7 and "gate" in runs["tampered"]["error"]   # ZKHIP_ERR_VERIFY
    assert serial == runs["full"]   # queries side by side or one after the other: the same wires
