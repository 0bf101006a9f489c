"""GPU: the batched AIR-set provers (airbatch_prove, AirKey.prove_batch, AirKey.prove_batch_cached) on the operand-family sets of
tests/zb_family_sets.py (docs/boundary_tests.md, "The batched AIR-set forms: operand families").

1. Words against the model: for every set and family the device prover's root and words equal the independent model's, word for word,
   and the host verifier accepts exactly when the model's does.  A case is (set, with_bus, a group of zb_family_sets.GROUP families);
   the two parameter sets of the per-AIR boundary file alternate over the cases.  At most one family of a case may be skipped for a
   zero denominator (none is under the committed seed: tests/test_zb_families_cpu.py asserts that without a device).
2. Values against numpy: for mixed_nobus and keyed, on the boundary, alternating raw p-1 / 0 and one-hot families, v, v' (v_p, v_p') and
   u (u_p) of every AIR are the multilinear extensions of its columns, and of the columns rolled by one row, at the prefixes of the
   replayed r and r'.  This does not go through the model: it is the reference of k_zb_emit and k_zb_dot."""
import numpy as np
import pytest

import zb_family_sets as zf
import zkvm_prover_amd as z
from test_gpu_airbatch import _replay
from test_gpu_keyed import _lp, _upload
from test_gpu_zc_boundary import PARAM_SETS
from test_gpu_zerocheck import _np_mle_base

pytestmark = pytest.mark.gpu
ERR_VERIFY = -7


def _prm(name, wb, i):
    return PARAM_SETS[zf.prm_index(name, wb, i)]


def _device_prove(zk, name, wb, i, keys):
    """(root, proof, key root, cached roots) of family i on the device.  keys: the case's AirKeys by preprocessed columns (a family of
    the second pass brings its own columns and so its own key)"""
    S = zf.fset(name)
    prm = _lp(_prm(name, wb, i))
    _, traces, preps, pvs = S["fams"][i]
    d, prefix = _upload(zk, traces), zf.prefix_of(name, wb, i)
    if S["form"] == "airbatch":
        return zk.airbatch_prove(prm, S["airs"], d, pvs, S["l"], prefix, wb) + (None, [])
    kid = (zf.prm_index(name, wb, i), i if S["fams"][i][0].startswith("prep ") else -1)
    if kid not in keys:
        keys[kid] = zk.airkey(prm, [dict(a, prep=p) if p is not None else a for a, p in zip(S["airs"], preps)], S["lpr"])
    key = keys[kid]
    if S["form"] == "keyed":
        return key.prove_batch(d, pvs, S["l"], prefix, with_bus=wb) + (key.root.tolist(), [])
    cached = [key.commit_cached(a, d[a], c) if c is not None else None for a, c in enumerate(S["lsc"])]
    try:
        return key.prove_batch_cached(d, pvs, cached, S["l"], prefix, with_bus=wb) + (key.root.tolist(), [c.root.tolist() for c in cached if c])
    finally:
        for c in cached:
            if c is not None:
                c.close()


def _host_accepts(name, wb, i, proof, key_root):
    S = zf.fset(name)
    prm, pvs, prefix = _lp(_prm(name, wb, i)), S["fams"][i][3], zf.prefix_of(name, wb, i)
    try:
        if S["form"] == "airbatch":
            out = z.airbatch_verify(prm, prefix, S["airs"], pvs, S["l"], proof, wb)
            return (out[0] if wb else out).tolist()
        if S["form"] == "keyed":
            out = z.airkey_batch_verify(prm, prefix, S["airs"], key_root, S["lpr"], pvs, S["l"], proof, wb)
            return (out[0] if wb else out).tolist()
        return z.airkey_cached_verify(prm, prefix, S["airs"], key_root, S["lpr"], S["lsc"], pvs, S["l"], proof, wb)[0].tolist()
    except z.ZkhipError as e:
        assert e.code == ERR_VERIFY, e
        return None


# ---- 1. words against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,wb,group", zf.CASES)
def test_words_equal_model(zk, name, wb, group):
    S = zf.fset(name)
    keys, done = {}, 0
    fams = zf.case_families(name, group)
    try:
        for i in fams:
            fam = "%s with_bus=%d %s" % (name, wb, S["fams"][i][0])
            res = zf.model(name, wb, i)
            if res is None:   # a zero denominator: the model's GKR cannot invert it
                continue
            done += 1
            root, proof, key_root, croots = _device_prove(zk, name, wb, i, keys)
            assert key_root == res["key_root"] and croots == res["cached_roots"], fam
            assert root.tolist() == res["root"], fam
            assert len(proof) == len(res["words"]), fam
            if proof.tolist() != res["words"]:
                pytest.fail("%s: proof differs from the model at word %d of %d"
                            % (fam, int(np.nonzero(proof != np.array(res["words"], dtype=np.uint32))[0][0]), len(proof)))
            got = _host_accepts(name, wb, i, proof, key_root)
            assert (got is not None) == res["accepted"], fam
            assert got is None or got == res["root"], fam
    finally:
        for k in keys.values():
            k.close()
    assert done >= len(fams) - 1


# ---- 2. values against numpy ----------------------------------------------------------------------------------------------------------
def _check_values(name, wb, i, proof, key_root):
    S = zf.fset(name)
    fam, traces, preps, pvs = S["fams"][i]
    keyed = (key_root, S["lpr"]) if S["form"] == "keyed" else None
    plans, act, red, r, rp, qv, qu = _replay(_prm(name, wb, i), zf.prefix_of(name, wb, i), S["airs"], pvs, S["l"], proof, wb, keyed)
    assert len(act) >= 5 and len(red) >= 3
    r, rp = np.array(r), np.array(rp)

    def same(at, col, point, what):
        assert proof[at:at + 4].tolist() == _np_mle_base(np.asarray(col, dtype=np.uint32), point), (fam, what)

    for a in act:
        pl, t, p = plans[a], traces[a], preps[a]
        wp, rot_p = (pl.wp, pl.rot_p) if keyed else (0, [])
        for j in range(pl.w):
            same(qv + 4 * j, t[j], r[:pl.m], "v of AIR %d column %d" % (a, j))
        for k, j in enumerate(pl.rot):
            same(qv + 4 * (pl.w + k), np.roll(t[j], -1), r[:pl.m], "v' of AIR %d column %d" % (a, j))
        o = qv + 4 * (pl.w + len(pl.rot))
        for j in range(wp):
            same(o + 4 * j, p[j], r[:pl.m], "v_p of AIR %d column %d" % (a, j))
        for k, j in enumerate(rot_p):
            same(o + 4 * (wp + k), np.roll(p[j], -1), r[:pl.m], "v_p' of AIR %d column %d" % (a, j))
        qv = o + 4 * (wp + len(rot_p))
        if a in red:
            for j in range(pl.w):
                same(qu + 4 * j, t[j], rp[:pl.m], "u of AIR %d column %d" % (a, j))
            for j in range(wp):
                same(qu + 4 * (pl.w + j), p[j], rp[:pl.m], "u_p of AIR %d column %d" % (a, j))
            qu += 4 * (pl.w + wp)


@pytest.mark.parametrize("fam", zf.VALUE_FAMILIES)
@pytest.mark.parametrize("name,wb", [("mixed_nobus", False), ("keyed", True), ("keyed", False)])
def test_values_against_numpy(zk, name, wb, fam):
    i = [f[0] for f in zf.fset(name)["fams"]].index(fam)
    keys = {}
    try:
        root, proof, key_root, _ = _device_prove(zk, name, wb, i, keys)
    finally:
        for k in keys.values():
            k.close()
    _check_values(name, wb, i, proof, key_root)
