"""CPU: the WHIR commitment (docs/whir.md) -- the independent model (tests/whir_model.py) against itself, against a direct MLE and
against the library's host verifiers (zkhip_whir_verify, zkhip_gkr_committed_verify); forged, truncated and mis-sized proofs are
refused, and so is a committed GKR proof whose GKR part ran on other leaves than the committed ones."""
import ctypes as C
import os
import random
import re

import pytest

import gkr_model as gm
import whir_model as wm
from pymodel import P, Challenger, bitrev, dft_naive, fri_fold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (log_blowup, fold_log, final_log, n_cols)
SETS = [(1, 1, 0, 1), (2, 2, 1, 3), (1, 4, 2, 2), (3, 1, 3, 2), (1, 2, 4, 5)]


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lib_params(p):
    import zkvm_prover_amd as z

    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _model_opening(prm, m, n_cols, seed):
    rng = random.Random(seed)
    cols = [[rng.randrange(P) for _ in range(1 << m)] for _ in range(n_cols)]
    z = [[rng.randrange(P) for _ in range(4)] for _ in range(m)]
    com = wm.commit(prm, cols)
    prefix = list(com.root) + [rng.randrange(P) for _ in range(rng.randrange(0, 5))]
    ch = Challenger()
    ch.observe(prefix)
    vals, words = wm.open_(com, ch, z)
    return cols, z, com, prefix, vals, words


def test_model_building_blocks():
    rng = random.Random(1)
    for ln in range(0, 6):
        c = [rng.randrange(P) for _ in range(1 << ln)]
        ev = dft_naive(c)
        assert wm._ntt_bitrev(c, ln) == [ev[bitrev(r, ln)] for r in range(1 << ln)]
    c = [rng.randrange(P) for _ in range(16)]
    pt = [[rng.randrange(P) for _ in range(4)] for _ in range(4)]
    assert wm.coeff_eval(wm.zeta(c), pt) == gm.mle_eval(c, pt)
    x = [rng.randrange(P) for _ in range(4)]
    # F(x) = f~(x, x^2, x^4, ..)
    F = [0, 0, 0, 0]
    xp = [1, 0, 0, 0]
    for ci in c:
        F = wm.ext_add(F, [ci * v % P for v in xp])
        xp = wm.ext_mul(xp, x)
    assert wm.coeff_eval(c, wm.pow_point(x, 4)) == F
    # the pointwise fold is pymodel.fri_fold, and folding a codeword is the codeword of the folded coefficients
    vals = [[rng.randrange(P) for _ in range(4)] for _ in range(16)]
    beta = [rng.randrange(P) for _ in range(4)]
    full = fri_fold(vals, beta)
    assert [wm.fold_pair(vals[2 * i], vals[2 * i + 1], beta, i, 3) for i in range(8)] == full
    coeffs = [rng.randrange(P) for _ in range(8)]
    cw = wm._ntt_bitrev(coeffs, 4)
    folded = fri_fold([gm.as_ext(v) for v in cw], beta)
    fc = wm.fold_coeffs(coeffs, beta)
    assert folded == [[wm._ntt_bitrev([e[q] for e in fc], 3)[i] for q in range(4)] for i in range(8)]


@pytest.mark.parametrize("b,k,fl,n_cols", SETS)
def test_model_opening_verifies_and_values_are_the_mle(b, k, fl, n_cols):
    prm = _params(b, k, fl)
    for m in (k, k + 3, 8):
        cols, z, com, prefix, vals, words = _model_opening(prm, m, n_cols, 10 * m + b)
        assert len(words) == wm.proof_words(prm, m, n_cols)
        assert vals == [gm.mle_eval(c, z) for c in cols]
        ch = Challenger()
        ch.observe(prefix)
        assert wm.verify(ch, prm, m, n_cols, com.root, z, words) == vals


def test_proof_length_formula():
    import zkvm_prover_amd as z

    for (b, k, fl, n_cols) in SETS:
        prm = _params(b, k, fl)
        for m in range(1, 27):
            want = wm.proof_words(prm, m, n_cols) if m >= k else 0
            assert z.whir_proof_words(_lib_params(prm), m, n_cols) == want
    prm = _params(1, 4, 2)
    assert z.whir_proof_words(_lib_params(prm), 27, 1) == 0 and z.whir_proof_words(_lib_params(prm), 8, 0) == 0
    assert z.whir_proof_words(_lib_params(_params(4, 1, 0)), 8, 1) == 0
    assert z.whir_proof_words(_lib_params(_params(1, 1, 0, nq=0)), 8, 1) == 0


def test_params_struct_mirrors_header():
    """zkhip_whir_params: the C header, the ctypes struct and the Rust FFI struct list the same fields in the same order."""
    import zkvm_prover_amd as z

    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} zkhip_whir_params;", hdr).group(1)
    c_fields = re.findall(r"uint32_t\s+(\w+)", body)
    assert c_fields == [f for f, _ in z.WhirParams._fields_]
    assert "pow_bits[ZKHIP_WHIR_MAX_ROUNDS]" in body and "num_queries[ZKHIP_WHIR_MAX_ROUNDS]" in body
    rs = open(os.path.join(ROOT, "integration", "hip-backend", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct zkhip_whir_params \{([^}]*)\}", rs).group(1)
    assert re.findall(r"pub (\w+):", rbody) == c_fields
    assert rbody.count("[u32; ZKHIP_WHIR_MAX_ROUNDS]") == 2
    assert re.search(r"ZKHIP_WHIR_MAX_ROUNDS: usize = (\d+)", rs).group(1) == re.search(r"#define ZKHIP_WHIR_MAX_ROUNDS (\d+)", hdr).group(1)
    assert C.sizeof(z.WhirParams) == 4 * (3 + 2 * z._binding.WHIR_MAX_ROUNDS)


@pytest.mark.parametrize("b,k,fl,n_cols", SETS)
def test_library_verifier_accepts_model_proofs(b, k, fl, n_cols):
    import zkvm_prover_amd as z

    prm = _params(b, k, fl, pow_bits=1 + b, nq=2 + k)
    for m in range(max(1, k), 13):
        if m > 9 and (b, k) != (1, 4):
            continue   # keeps the model's share of the run short; m 10..12 are covered with the cheapest set
        cols, zpt, com, prefix, vals, words = _model_opening(prm, m, n_cols, 1000 * b + 100 * k + m)
        z.whir_verify(_lib_params(prm), prefix, com.root, m, n_cols, zpt, vals, words)


def _parts(prm, m, n_cols):
    """offset of one word in each part of an opening"""
    lay, off, out = wm._layout(prm, m, n_cols), 0, {}
    R, mf = prm.rounds(m)
    for kind, w in lay:
        if kind == "queries" and "leaf" not in out:
            out["leaf"] = off + 1
            width = n_cols << prm.k
            out["sibling"] = off + width + 3
        elif kind != "queries":
            out.setdefault(kind, off + w // 2)
        off += w
    return out


def test_library_verifier_refuses_forgeries():
    import zkvm_prover_amd as z

    prm = _params(1, 2, 1, pow_bits=4, nq=3)
    m, n_cols = 7, 3
    lp = _lib_params(prm)
    cols, zpt, com, prefix, vals, words = _model_opening(prm, m, n_cols, 77)
    z.whir_verify(lp, prefix, com.root, m, n_cols, zpt, vals, words)
    parts = _parts(prm, m, n_cols)
    assert set(parts) == {"values", "sumcheck", "root", "ood", "pow", "leaf", "sibling", "final"}
    for name, i in parts.items():
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        bvals = vals if name != "values" else [[bad[4 * c + q] for q in range(4)] for c in range(n_cols)]
        with pytest.raises(z.ZkhipError):
            z.whir_verify(lp, prefix, com.root, m, n_cols, zpt, bvals, bad)
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises(wm.WhirReject):
            wm.verify(ch, prm, m, n_cols, com.root, zpt, bad)
    # the root, the point, a value, the prefix
    root = list(com.root)
    root[3] = (root[3] + 1) % P
    bad_pt = [list(p) for p in zpt]
    bad_pt[2][1] = (bad_pt[2][1] + 1) % P
    bad_vals = [list(v) for v in vals]
    bad_vals[1][0] = (bad_vals[1][0] + 1) % P
    for args in [(prefix, root, zpt, vals), (prefix, com.root, bad_pt, vals), (prefix, com.root, zpt, bad_vals),
                 (prefix + [1], com.root, zpt, vals)]:
        with pytest.raises(z.ZkhipError):
            z.whir_verify(lp, args[0], args[1], m, n_cols, args[2], args[3], words)
    # truncated, extended, a wrong m or n_cols, non-canonical words
    for bad in (words[:-1], list(words) + [0]):
        with pytest.raises(z.ZkhipError):
            z.whir_verify(lp, prefix, com.root, m, n_cols, zpt, vals, bad)
    with pytest.raises(z.ZkhipError):
        z.whir_verify(lp, prefix, com.root, m, n_cols - 1, zpt, vals[:-1], words)
    for i in (0, parts["sumcheck"], parts["leaf"]):
        big = list(words)
        big[i] += P
        with pytest.raises(z.ZkhipError):
            z.whir_verify(lp, prefix, com.root, m, n_cols, zpt, vals if i else [[big[q] for q in range(4)]] + vals[1:], big)


def _gkr_leaves(rng, log_n, num_ext):
    n = 1 << log_n
    num = [[rng.randrange(P) for _ in range(4)] if num_ext else rng.randrange(P) for _ in range(n)]
    den = [[rng.randrange(P) for _ in range(4)] for _ in range(n)]
    return num, den


@pytest.mark.parametrize("num_ext", [False, True])
def test_committed_gkr_verifier_accepts_model_proofs(num_ext):
    import zkvm_prover_amd as z

    prm = _params(1, 2, 2, pow_bits=2, nq=3)
    for log_n in (2, 5, 7):
        rng = random.Random(log_n + 10 * num_ext)
        num, den = _gkr_leaves(rng, log_n, num_ext)
        prefix = [rng.randrange(P) for _ in range(3)]
        ch = Challenger()
        ch.observe(prefix)
        words = wm.gkr_committed_prove(ch, prm, num, den, num_ext)
        assert len(words) == z._binding.load_library().zkhip_gkr_committed_proof_words(C.byref(_lib_params(prm)), log_n, int(num_ext))
        ch = Challenger()
        ch.observe(prefix)
        root, (Pr, Qr) = wm.gkr_committed_verify(ch, prm, log_n, num_ext, words)
        lroot, pq = z.gkr_committed_verify(_lib_params(prm), prefix, words, log_n, num_ext)
        assert lroot.tolist() == root and pq.tolist() == [Pr, Qr]
        s = gm.ZERO
        for a, d in zip(num, den):
            s = gm.ext_add(s, gm.ext_mul(gm.as_ext(a), gm.ext_inv(d)))
        assert gm.ext_mul(Pr, gm.ext_inv(Qr)) == s
        bad = list(words)
        bad[-5] = (bad[-5] + 1) % P
        with pytest.raises(z.ZkhipError):
            z.gkr_committed_verify(_lib_params(prm), prefix, bad, log_n, num_ext)


@pytest.mark.parametrize("which", ["num", "den"])
def test_committed_gkr_refuses_a_substituted_leaf(which):
    """The soundness gap this closes: a GKR proof of tables that differ in one leaf from the committed ones.  The bare fraction
    verifier accepts the GKR part; the committed verifier refuses the whole."""
    import zkvm_prover_amd as z

    prm = _params(1, 2, 2, pow_bits=2, nq=3)
    log_n = 6
    rng = random.Random(5)
    num, den = _gkr_leaves(rng, log_n, False)
    gnum, gden = list(num), [list(d) for d in den]
    if which == "num":
        gnum[17] = (gnum[17] + 1) % P
    else:
        gden[17][2] = (gden[17][2] + 1) % P
    prefix = [9, 8, 7]
    ch = Challenger()
    ch.observe(prefix)
    words = wm.gkr_committed_prove(ch, prm, num, den, False, gkr_num=gnum, gkr_den=gden)
    gw = words[8:8 + gm.proof_words(log_n)]
    # the GKR part alone is a valid proof (after the root the committed form observes)
    z.gkr_verify(prefix + words[:8], gw, log_n)
    with pytest.raises(z.ZkhipError):
        z.gkr_committed_verify(_lib_params(prm), prefix, words, log_n, False)
    ch = Challenger()
    ch.observe(prefix)
    with pytest.raises(wm.WhirReject):
        wm.gkr_committed_verify(ch, prm, log_n, False, words)
