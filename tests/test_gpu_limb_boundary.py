"""GPU: the limb-chip trace generators (csrc/modular.hip, ecc.hip, fp2.hip with limb_dev.hpp, int256.hip, keccak.hip, sha256.hip) on
the boundary operand sets of tests/limb_boundary_inputs.py: every family cell for cell against the twin, count for count against the twin
and against a numpy recount from the trace's own cells, the result columns against Python's integers; row counts across wave and workgroup
boundaries with the padding rows zero; the histogram's two extremes; timestamps at 0, P - 1, P, 2^32 - 1; refused records between accepted
launches; one proof per chip on a boundary family.  docs/boundary_tests.md, third section."""
import hashlib

import numpy as np
import pytest
import torch

import zkvm_prover_amd as z

import ecc_util as eu
import fp2_util as fu
import int256_util as iu
import limb_boundary_inputs as lb
import modular_util as mu
from test_limb_boundary_cpu import ECC_FAMILIES, FP2_FAMILIES, MOD_FAMILIES, value

pytestmark = pytest.mark.gpu
PARAMS = (1, 0, 4, 3, 3)
P = lb.P_BB
TS = [0, P - 1, P, 2**32 - 1]


def dev(zk, words):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(words, dtype=np.uint32).reshape(-1)).view(np.int32)).to(zk.device)


def tables(zk, sy):
    return torch.zeros(2 << 16, dtype=torch.int32, device=zk.device), torch.zeros(256 * sy, dtype=torch.int32, device=zk.device)


def same(got, want, what):
    """cell for cell (or count for count); on failure the first differing (column, row)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.astype(np.int64) != want.astype(np.int64))
    assert not len(bad), "%s: first difference at %s: device %d, expected %d (%d cells differ)" % (what, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def restricted(tr, n, log_h):
    """the twin's trace restricted to its first n rows, at height 2^log_h"""
    out = np.zeros((tr.shape[0], 1 << log_h), np.uint32)
    out[:, :n] = tr[:, :n]
    return out


# ---- launches ---------------------------------------------------------------------------------------------------------------------
def run_modular(zk, p, rows, log_h, recs=None):
    recs = recs if recs is not None else [lb.modular_record_words(r, p) for r in rows]
    d_bw, d_tup = tables(zk, mu.SY)
    d_tr = zk.modular_tracegen(p, dev(zk, recs) if len(recs) else None, len(recs), log_h, d_bw, d_tup, mu.SX, mu.SY)
    bw = zk.download(d_bw)
    assert not bw[1 << 16:].any()
    return zk.download(d_tr).reshape(mu.cols(lb.limbs_of(p))["WIDTH"], -1), bw[:1 << 16], zk.download(d_tup), (d_tr, d_bw, d_tup)


def run_ecc(zk, cv, rows, log_h, ts=None):
    nw = lb.limbs_of(cv.p) // 4
    recs = [eu.record(*c, n=nw) for c in rows]
    d_bw, d_tup = tables(zk, eu.SY)
    d_tr = zk.ec_tracegen(cv.p, cv.a, dev(zk, recs) if len(recs) else None, len(recs), log_h, d_bw, d_tup, eu.SX, eu.SY, t_ts=ts)
    bw = zk.download(d_bw)
    assert not bw[1 << 16:].any()
    return zk.download(d_tr).reshape(-1, 1 << log_h), bw[:1 << 16], zk.download(d_tup), (d_tr, d_bw, d_tup)


def run_fp2(zk, p, rows, log_h, ts=None):
    nw = lb.limbs_of(p) // 4
    recs = [fu.record(*c, n=nw) for c in rows]
    d_bw, d_tup = tables(zk, fu.SY)
    d_tr = zk.fp2_tracegen(p, dev(zk, recs) if len(recs) else None, len(recs), log_h, d_bw, d_tup, fu.SX, fu.SY, t_ts=ts)
    bw = zk.download(d_bw)
    assert not bw[1 << 16:].any()
    return zk.download(d_tr).reshape(-1, 1 << log_h), bw[:1 << 16], zk.download(d_tup), (d_tr, d_bw, d_tup)


def run_int256(zk, chip, cases, log_h, ts=None):
    """-> (trace, range counts, xor counts, tuple counts or None, device tensors)"""
    d_bw = torch.zeros(2 << 16, dtype=torch.int32, device=zk.device)
    d_tup = None
    if chip == "mul":
        recs = [iu.words(b) + iu.words(c) for b, c in cases]
        d_tup = torch.zeros(iu.SX * iu.SY, dtype=torch.int32, device=zk.device)
        d_tr = zk.int256_mul_tracegen(dev(zk, recs) if len(recs) else None, len(recs), log_h, d_bw, d_tup, iu.SX, iu.SY)
    else:
        recs = iu.records(cases) if len(cases) else []
        d_recs = dev(zk, recs) if len(recs) else None
        if chip == "alu":
            d_tr = zk.int256_alu_tracegen(d_recs, len(recs), log_h, d_bw)
        elif chip == "cmp":
            d_tr = zk.int256_cmp_tracegen(d_recs, len(recs), log_h, d_bw, t_ts=ts)
        else:
            d_tr = zk.int256_shift_tracegen(d_recs, len(recs), log_h, d_bw, t_ts=ts)
    bw = zk.download(d_bw)
    return zk.download(d_tr).reshape(-1, 1 << log_h), bw[:1 << 16], bw[1 << 16:], None if d_tup is None else zk.download(d_tup), [d_tr, d_bw] + ([d_tup] if d_tup is not None else [])


_int256_twins = {}


def int256_twin(ora, chip, n=None):
    """(cases, trace at the smallest height, range counts, xor counts, tuple counts): computed once"""
    key = (chip, n)
    if key not in _int256_twins:
        cases = {"alu": lb.alu_cases, "cmp": lb.cmp_cases, "shift": lb.shift_cases, "mul": lb.mul_cases}[chip]()
        cases = lb.cycle(cases, n) if n is not None else cases
        log_h = max(1, (len(cases) - 1).bit_length())
        zero = np.zeros(1 << 16, np.uint32)
        if chip == "alu":
            tr, xc, bad = iu.ora_trace(ora, cases, log_h)
            assert bad == 0
            out = (cases, tr, zero, xc, None)
        elif chip == "mul":
            tr, bw, tup, bad = iu.ora_mul_trace(ora, cases, log_h)
            assert bad == 0
            out = (cases, tr, bw, zero, tup)
        elif chip == "cmp":
            tr, bw = iu.cmp_twin_trace(cases, log_h)
            out = (cases, tr, bw, zero, None)
        else:
            tr, bw, xc = iu.shift_twin_trace(cases, log_h)
            out = (cases, tr, bw, xc, None)
        _int256_twins[key] = out
    return _int256_twins[key]


def int256_recount(chip, tr, n):
    """(range counts, xor counts, tuple counts) from the trace's own cells"""
    zero = np.zeros(1 << 16, np.int64)
    if chip == "alu":
        return zero, lb.recount_alu(tr, n), None
    if chip == "mul":
        bw, tup = lb.recount_mul(tr, n)
        return bw, zero, tup
    if chip == "cmp":
        return lb.recount_cmp(tr, n), zero, None
    bw, xc = lb.recount_shift(tr, n)
    return bw, xc, None


def check_int256(chip, got, want_tr, n, what):
    tr, bw, xc, tup = got
    same(tr, want_tr, what)
    rbw, rxc, rtup = int256_recount(chip, want_tr, n)
    same(bw, rbw, what + " range counts"), same(xc, rxc, what + " xor counts")
    if rtup is not None:
        same(tup, rtup, what + " tuple counts")


# ---- operand families -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", MOD_FAMILIES)
@pytest.mark.parametrize("name", list(lb.MODULI))
def test_modular_family(zk, name, family):
    p = lb.MODULI[name]
    L = lb.limbs_of(p)
    rows, log_h, (tr, bw, tup) = lb.modular_twin(name, family)
    got, gbw, gtup, _ = run_modular(zk, p, rows, log_h)
    what = "modular %s/%s" % (name, family)
    same(got, tr, what), same(gbw, bw, what + " bitwise"), same(gtup, tup, what + " tuple")
    rbw, rtup = lb.recount_modular(got, len(rows), L)
    same(gbw, rbw, what + " bitwise recount"), same(gtup, rtup, what + " tuple recount")
    c = mu.cols(L)
    for row, r in enumerate(rows):
        assert (value(got, c["A"], L, row), value(got, c["R"], L, row)) == lb.modular_expected(r, p), (what, row)


@pytest.mark.parametrize("family", ECC_FAMILIES)
@pytest.mark.parametrize("name", list(lb.CURVES))
def test_ecc_family(zk, name, family):
    cv = lb.Curve(name)
    L = lb.limbs_of(cv.p)
    rows, log_h, (tr, bw, tup) = lb.ecc_twin(name, family)
    got, gbw, gtup, _ = run_ecc(zk, cv, rows, log_h)
    what = "ecc %s/%s" % (name, family)
    same(got, tr, what), same(gbw, bw, what + " bitwise"), same(gtup, tup, what + " tuple")
    rbw, rtup = lb.recount_ecc(got, len(rows), L)
    same(gbw, rbw, what + " bitwise recount"), same(gtup, rtup, what + " tuple recount")
    for row, call in enumerate(rows):
        assert (value(got, 5 * L, L, row), value(got, 6 * L, L, row)) == lb.ecc_expected(call, cv), (what, row)


@pytest.mark.parametrize("family", FP2_FAMILIES)
@pytest.mark.parametrize("name", list(lb.FP2_MODULI))
def test_fp2_family(zk, name, family):
    p = lb.FP2_MODULI[name]
    L = lb.limbs_of(p)
    rows, log_h, (tr, bw, tup) = lb.fp2_twin(name, family)
    got, gbw, gtup, _ = run_fp2(zk, p, rows, log_h)
    what = "fp2 %s/%s" % (name, family)
    same(got, tr, what), same(gbw, bw, what + " bitwise"), same(gtup, tup, what + " tuple")
    rbw, rtup = lb.recount_fp2(got, len(rows), L)
    same(gbw, rbw, what + " bitwise recount"), same(gtup, rtup, what + " tuple recount")
    for row, call in enumerate(rows):
        r, a = lb.fp2_expected(call, p)
        assert (value(got, 4 * L, L, row), value(got, 5 * L, L, row)) == r and (value(got, 0, L, row), value(got, L, L, row)) == a, (what, row)


@pytest.mark.parametrize("chip", ["alu", "mul", "cmp", "shift"])
def test_int256_family(zk, ora, chip):
    cases, tr, bw, xc, tup = int256_twin(ora, chip)
    log_h = max(1, (len(cases) - 1).bit_length())
    got = run_int256(zk, chip, cases, log_h)
    check_int256(chip, got[:4], tr, len(cases), "int256 " + chip)
    same(got[1], bw, chip + " range counts (twin)"), same(got[2], xc, chip + " xor counts (twin)")
    if tup is not None:
        same(got[3], tup, chip + " tuple counts (twin)")
    for row, case in enumerate(cases):
        if chip == "mul":
            assert value(got[0], 0, 32, row) == lb.int256_expected(5, *case)
        elif chip == "cmp":
            out = int(got[0][64, row]) if case[0] != 8 else 1 - int(got[0][65:97, row].sum())
            assert out == lb.int256_expected(*case), (chip, row)
        else:
            assert value(got[0], 0, 32, row) == lb.int256_expected(*case), (chip, row)


# ---- row-count edges --------------------------------------------------------------------------------------------------------------
EDGES_64 = [(1, 7), (63, 6), (64, 6), (65, 7), (128, 7), (0, 1)]
EDGES_256 = [(1, 9), (255, 8), (256, 8), (257, 9), (512, 9), (0, 1)]


@pytest.mark.parametrize("name", ["secp256k1", "bls12_381"])
def test_ecc_row_count_edges(zk, name):
    cv = lb.Curve(name)
    L = lb.limbs_of(cv.p)
    rows, _, (tr, bw, tup) = lb.ecc_twin(name, "all", 128, 7)
    for n, log_h in EDGES_64:
        got, gbw, gtup, _ = run_ecc(zk, cv, rows[:n], log_h)
        what = "ecc %s n = %d of 2^%d" % (name, n, log_h)
        want = restricted(tr, n, log_h)
        same(got, want, what)
        assert not got[:, n:].any()
        rbw, rtup = lb.recount_ecc(want, n, L)
        same(gbw, rbw, what + " bitwise"), same(gtup, rtup, what + " tuple")
        if n == 128:
            same(gbw, bw, what + " bitwise (twin)"), same(gtup, tup, what + " tuple (twin)")


@pytest.mark.parametrize("name", ["bn254_p", "bls12_381_p"])
def test_fp2_row_count_edges(zk, name):
    p = lb.FP2_MODULI[name]
    L = lb.limbs_of(p)
    rows, _, (tr, bw, tup) = lb.fp2_twin(name, "all", 128, 7)
    for n, log_h in EDGES_64:
        got, gbw, gtup, _ = run_fp2(zk, p, rows[:n], log_h)
        what = "fp2 %s n = %d of 2^%d" % (name, n, log_h)
        want = restricted(tr, n, log_h)
        same(got, want, what)
        assert not got[:, n:].any()
        rbw, rtup = lb.recount_fp2(want, n, L)
        same(gbw, rbw, what + " bitwise"), same(gtup, rtup, what + " tuple")
        if n == 128:
            same(gbw, bw, what + " bitwise (twin)"), same(gtup, tup, what + " tuple (twin)")


@pytest.mark.parametrize("name", ["secp256k1_p", "bls12_381_p"])
def test_modular_row_count_edges(zk, name):
    """the mixed family interleaves division, equality and plain rows: every wave diverges at `if (is_div) hist_add`"""
    p = lb.MODULI[name]
    L = lb.limbs_of(p)
    rows, _, (tr, bw, tup) = lb.modular_twin(name, "mixed", 512, 9)
    for n, log_h in EDGES_256:
        got, gbw, gtup, _ = run_modular(zk, p, rows[:n], log_h)
        what = "modular %s n = %d of 2^%d" % (name, n, log_h)
        want = restricted(tr, n, log_h)
        same(got, want, what)
        assert not got[:, n:].any()
        rbw, rtup = lb.recount_modular(want, n, L)
        same(gbw, rbw, what + " bitwise"), same(gtup, rtup, what + " tuple")
        if n == 512:
            same(gbw, bw, what + " bitwise (twin)"), same(gtup, tup, what + " tuple (twin)")


@pytest.mark.parametrize("chip", ["alu", "mul", "cmp", "shift"])
def test_int256_row_count_edges(zk, ora, chip):
    """the case lists alternate opcodes lane by lane (SRA beside SLL, equal beside unequal operands)"""
    cases, tr, bw, xc, tup = int256_twin(ora, chip, 512)
    for n, log_h in EDGES_256:
        got = run_int256(zk, chip, cases[:n], log_h)
        assert not got[0][:, n:].any()
        check_int256(chip, got[:4], restricted(tr, n, log_h), n, "int256 %s n = %d of 2^%d" % (chip, n, log_h))
        if n == 512:
            same(got[1], bw, chip + " range counts (twin)"), same(got[2], xc, chip + " xor counts (twin)")


# ---- the histogram's extremes -----------------------------------------------------------------------------------------------------
def test_histogram_one_record_256_times(zk, ora):
    """every wave asks for each entry with all 64 lanes: one atomic of 64 per request"""
    p = lb.SECP_P
    row = (3, 5, 7)
    tr1, bw1, tup1 = mu.py_trace([row], p, 0)
    got, gbw, gtup, _ = run_modular(zk, p, [row] * 256, 8)
    same(got, np.repeat(tr1, 256, axis=1), "modular x256"), same(gbw, 256 * bw1.astype(np.int64), "modular x256 bitwise"), same(gtup, 256 * tup1.astype(np.int64), "modular x256 tuple")
    rbw, rtup = lb.recount_modular(got, 256, 32)
    same(gbw, rbw, "modular x256 bitwise recount"), same(gtup, rtup, "modular x256 tuple recount")
    cv = lb.Curve("bn254")
    call = lb.ecc_families("bn254")["slopes"][0]
    tr1, bw1, tup1 = eu.twin_trace([call], cv.p, cv.a, 0)
    got, gbw, gtup, _ = run_ecc(zk, cv, [call] * 256, 8)
    same(got, np.repeat(tr1, 256, axis=1), "ecc x256"), same(gbw, 256 * bw1.astype(np.int64), "ecc x256 bitwise"), same(gtup, 256 * tup1.astype(np.int64), "ecc x256 tuple")
    call = lb.fp2_families(lb.BN_P)["exact"][0]
    tr1, bw1, tup1 = fu.twin_trace([call], lb.BN_P, 0)
    got, gbw, gtup, _ = run_fp2(zk, lb.BN_P, [call] * 256, 8)
    same(got, np.repeat(tr1, 256, axis=1), "fp2 x256"), same(gbw, 256 * bw1.astype(np.int64), "fp2 x256 bitwise"), same(gtup, 256 * tup1.astype(np.int64), "fp2 x256 tuple")
    for chip, case in (("alu", (0, lb.M256 - 1, 1)), ("mul", (lb.M256 - 1, lb.M256 - 1)), ("cmp", (7, lb.MIN256, lb.MAX256)), ("shift", (11, lb.M256 - 1, 255))):
        g = run_int256(zk, chip, [case] * 256, 8)
        assert (g[0] == g[0][:, :1]).all()
        check_int256(chip, g[:4], g[0], 256, "int256 %s x256" % chip)


def test_histogram_all_lanes_differ(zk, ora):
    """the low byte pair of one operand runs through 256 values: 64 loop trips in hist_add for that request, in every wave"""
    p = lb.SECP_P
    x, y = lb.modular_families(p)["uniform"][0][1:]
    rows = [(1, (x & ~0xFF) | i, y) for i in range(256)]
    tr, bw, tup = mu.py_trace(rows, p, 8)
    got, gbw, gtup, _ = run_modular(zk, p, rows, 8)
    same(got, tr, "modular a0 = 0..255"), same(gbw, bw, "modular a0 = 0..255 bitwise"), same(gtup, tup, "modular a0 = 0..255 tuple")
    rbw, rtup = lb.recount_modular(got, 256, 32)
    same(gbw, rbw, "modular a0 = 0..255 bitwise recount"), same(gtup, rtup, "modular a0 = 0..255 tuple recount")
    frows = [(1, ((x & ~0xFF) | i, y), (y, (x & ~0xFFFF) | (i << 8))) for i in range(256)]
    tr, bw, tup = fu.twin_trace(frows, lb.SECP_P, 8)
    got, gbw, gtup, _ = run_fp2(zk, lb.SECP_P, frows, 8)
    same(got, tr, "fp2 a0 = 0..255"), same(gbw, bw, "fp2 a0 = 0..255 bitwise"), same(gtup, tup, "fp2 a0 = 0..255 tuple")
    b = x % lb.M256
    for chip, cases in (("alu", [(2 + i % 3, (b & ~0xFF) | i, (y & ~0xFF) | (255 - i)) for i in range(256)]), ("cmp", [(6 + i % 3, (b & ~0xFF) | i, b) for i in range(256)]),
                        ("shift", [(9 + i % 3, b | lb.MIN256, i) for i in range(256)]), ("mul", [((b & ~0xFF) | i, y) for i in range(256)])):
        g = run_int256(zk, chip, cases, 8)
        if chip == "alu":
            want = iu.ora_trace(ora, cases, 8)[0]
        elif chip == "mul":
            want = iu.ora_mul_trace(ora, cases, 8)[0]
        else:
            want = iu.cmp_twin_trace(cases, 8)[0] if chip == "cmp" else iu.shift_twin_trace(cases, 8)[0]
        check_int256(chip, g[:4], want, 256, "int256 %s, 256 different requests" % chip)


# ---- timestamps -------------------------------------------------------------------------------------------------------------------
def test_timestamps(zk, ora):
    """the bindings that take a timestamp array (ecc, fp2, comparison, shift): the column is ts % P"""
    ts = dev(zk, TS)
    want_ts = np.array([t % P for t in TS], np.uint32)
    cv = lb.Curve("secp256k1")
    rows = lb.ecc_families("secp256k1")["slopes"][:4]
    got, gbw, gtup, _ = run_ecc(zk, cv, rows, 2, ts=ts)
    tr, bw, tup = eu.twin_trace(rows, cv.p, cv.a, 2)
    same(got[:-1], tr, "ecc with timestamps"), same(got[-1], want_ts, "ecc timestamps"), same(gbw, bw, "ecc bitwise"), same(gtup, tup, "ecc tuple")
    rows = lb.fp2_families(lb.BN_P)["exact"][:4]
    got, gbw, gtup, _ = run_fp2(zk, lb.BN_P, rows, 2, ts=ts)
    tr, bw, tup = fu.twin_trace(rows, lb.BN_P, 2)
    same(got[:-1], tr, "fp2 with timestamps"), same(got[-1], want_ts, "fp2 timestamps"), same(gbw, bw, "fp2 bitwise"), same(gtup, tup, "fp2 tuple")
    cases = [(6, 1, 2), (7, lb.MIN256, 0), (8, 5, 5), (7, lb.M256 - 1, lb.M256 - 1)]
    g = run_int256(zk, "cmp", cases, 2, ts=ts)
    tr, bw = iu.cmp_twin_trace(cases, 2)
    same(g[0][:103], tr, "cmp with timestamps"), same(g[0][103], want_ts, "cmp timestamps"), same(g[1], bw, "cmp bitwise")
    assert not g[0][104:107].any() and g[0][107].tolist() == [c[0] for c in cases]      # no branch rows; the opcode the adapter announces
    cases = [(9, 1, 255), (10, lb.M256 - 1, 0x1FF), (11, lb.MIN256, 248), (11, lb.MAX256, 0)]
    g = run_int256(zk, "shift", cases, 2, ts=ts)
    tr, bw, xc = iu.shift_twin_trace(cases, 2)
    same(g[0][:189], tr, "shift with timestamps"), same(g[0][189], want_ts, "shift timestamps"), same(g[1], bw, "shift bitwise"), same(g[2], xc, "shift xor")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_records_between_accepted_launches(zk, ora):
    """each refused record in a launch of its own raises; the accepted launch after it still matches the twin (the flag is cleared)"""
    for name in ("bn254_p", "bls12_381_p"):
        p = lb.MODULI[name]
        rows, log_h, (tr, bw, tup) = lb.modular_twin(name, "sub")
        same(run_modular(zk, p, rows, log_h)[0], tr, "modular before")
        for what, rec in lb.modular_refused(p).items():
            with pytest.raises(Exception):
                run_modular(zk, p, None, 1, recs=[rec])
            got, gbw, gtup, _ = run_modular(zk, p, rows, log_h)
            same(got, tr, "modular after " + what), same(gbw, bw, "modular bitwise after " + what), same(gtup, tup, "modular tuple after " + what)
    for name in ("bn254", "bls12_381"):
        cv = lb.Curve(name)
        rows, log_h, (tr, bw, tup) = lb.ecc_twin(name, "slopes")
        same(run_ecc(zk, cv, rows, log_h)[0], tr, "ecc before")
        for what, call in lb.ecc_refused(name).items():
            with pytest.raises(Exception):
                run_ecc(zk, cv, [call], 1)
            got, gbw, gtup, _ = run_ecc(zk, cv, rows, log_h)
            same(got, tr, "ecc after " + what), same(gbw, bw, "ecc bitwise after " + what), same(gtup, tup, "ecc tuple after " + what)
    for name in ("bn254_p", "bls12_381_p"):
        p = lb.FP2_MODULI[name]
        rows, log_h, (tr, bw, tup) = lb.fp2_twin(name, "exact")
        same(run_fp2(zk, p, rows, log_h)[0], tr, "fp2 before")
        for what, call in lb.fp2_refused(p).items():
            with pytest.raises(Exception):
                run_fp2(zk, p, [call], 1)
            got, gbw, gtup, _ = run_fp2(zk, p, rows, log_h)
            same(got, tr, "fp2 after " + what), same(gbw, bw, "fp2 bitwise after " + what), same(gtup, tup, "fp2 tuple after " + what)
    for chip in ("alu", "cmp", "shift"):
        cases, tr, bw, xc, _ = int256_twin(ora, chip)
        log_h = max(1, (len(cases) - 1).bit_length())
        for rec in lb.INT256[chip][1]:
            with pytest.raises(Exception):
                run_int256(zk, chip, [rec], 1)
            check_int256(chip, run_int256(zk, chip, cases, log_h)[:4], tr, len(cases), "int256 %s after opcode %d" % (chip, rec[0]))
    # more records than rows is refused before any launch
    with pytest.raises(Exception):
        run_modular(zk, lb.SECP_P, [(0, 1, 2)] * 3, 1)


# ---- one proof per chip -----------------------------------------------------------------------------------------------------------
def prove_and_compare(zk, ora, inst, traces):
    pk = z.ProvingKey(zk, PARAMS, inst)
    pvs = [mu.NOPV] * len(inst)
    proof = pk.prove(traces, pvs)
    assert z.verify(PARAMS, pk.verifying_airs(), pvs, proof) == 0
    assert proof == ora.stark_prove(PARAMS, inst).tobytes()
    pk.close()


def test_modular_proof_on_the_wrap_around_subtraction(zk, ora):
    rows, log_h, (tr, bw, tup) = lb.modular_twin("secp256k1_p", "sub")
    got, gbw, gtup, d = run_modular(zk, lb.SECP_P, rows, log_h)
    same(got, tr, "modular sub")
    prove_and_compare(zk, ora, mu.instance(lb.SECP_P, got, gbw, gtup, log_h), list(d))


def test_ecc_proof_on_the_slope_0_chord(zk, ora):
    cv = lb.Curve("secp256k1")
    rows, log_h, (tr, bw, tup) = lb.ecc_twin("secp256k1", "slopes")
    assert any(c[3] == 0 for c in rows)
    got, gbw, gtup, d = run_ecc(zk, cv, rows, log_h)
    same(got, tr, "ecc slopes")
    prove_and_compare(zk, ora, eu.instance(cv.p, cv.a, got, gbw, gtup, log_h), list(d))


def test_fp2_proof_on_the_exact_multiple(zk, ora):
    rows, log_h, (tr, bw, tup) = lb.fp2_twin("bn254_p", "exact")
    got, gbw, gtup, d = run_fp2(zk, lb.BN_P, rows, log_h)
    same(got, tr, "fp2 exact")
    prove_and_compare(zk, ora, fu.instance(lb.BN_P, got, gbw, gtup, log_h), list(d))


@pytest.mark.parametrize("chip", ["alu", "mul", "cmp", "shift"])
def test_int256_proof(zk, ora, chip):
    cases = int256_twin(ora, chip)[0][:32]
    tr, bw, xc, tup, d = run_int256(zk, chip, cases, 5)
    inst = {"alu": lambda: iu.instance(tr, xc, 5), "mul": lambda: iu.mul_instance(tr, bw, tup, 5), "cmp": lambda: iu.cmp_instance(tr, bw, 5),
            "shift": lambda: iu.shift_instance(tr, bw, xc, 5)}[chip]()
    prove_and_compare(zk, ora, inst, d)


# ---- keccak and sha256 ------------------------------------------------------------------------------------------------------------
def test_keccak_boundary_states_and_counts(zk, ora):
    """all-zero, all-one and single-bit states; one permutation; the largest count a height holds (24 rows each: 5 of 128, 8 rows of
    padding) and one less (a whole padding permutation)"""
    from test_keccak_cpu import one_block_state, ora_trace

    states = list(lb.keccak_states().values())
    for n, log_h in ((1, 5), (5, 7), (4, 7), (len(states), 7)):
        st = np.stack((states * 2)[:n])
        got = zk.download(zk.keccak_f_tracegen(dev(zk, st.view(np.uint32)), n, log_h)).reshape(2633, -1)
        same(got, ora_trace(ora, st, log_h), "keccak n = %d of 2^%d" % (n, log_h))
    msgs = [b"", b"\x00", b"\xff" * 135, b"\x80"]
    st = np.stack([one_block_state(m) for m in msgs])
    got = zk.download(zk.keccak_f_tracegen(dev(zk, st.view(np.uint32)), len(msgs), 7)).reshape(2633, -1)
    same(got, ora_trace(ora, st, 7), "keccak messages")
    for k, m in enumerate(msgs):
        row = 24 * k + 23
        lanes = [[int(got[2629 + j, row]) for j in range(4)]] + [[int(got[2465 + 4 * x + j, row]) for j in range(4)] for x in (1, 2, 3)]
        assert b"".join(sum(v << (16 * i) for i, v in enumerate(l)).to_bytes(8, "little") for l in lanes).hex() == hashlib.sha3_256(m).hexdigest()
    zero = np.zeros(25, np.uint64)
    assert (z.keccak_f1600_host(zero) != 0).any()


def test_sha256_boundary_blocks_and_counts(zk, ora):
    """all-zero, all-one and single-bit blocks and states; one block; the largest count a height holds (65 rows each: 7 of 512) and one
    less (a whole padding block)"""
    from sha256_util import ROWS, WIDTH, chained_records, digest_of_row, ora_trace

    recs = list(lb.sha256_records().values())
    for n, log_h in ((1, 7), (7, 9), (6, 9), (len(recs), 10)):
        r = np.stack((recs * 2)[:n])
        assert n <= (1 << log_h) // ROWS
        got = zk.download(zk.sha256_tracegen(dev(zk, r), n, log_h)).reshape(WIDTH, -1)
        same(got, ora_trace(ora, r, log_h), "sha256 n = %d of 2^%d" % (n, log_h))
    msgs = [b"", b"\x00" * 55, b"\xff" * 56, b"\x00" * 64, b"\xff" * 119]
    r, last = chained_records(msgs, z.sha256_compress_host)
    got = zk.download(zk.sha256_tracegen(dev(zk, r), len(r), 10)).reshape(WIDTH, -1)
    same(got, ora_trace(ora, r, 10), "sha256 messages")
    for m, b in zip(msgs, last):
        assert digest_of_row(got, ROWS * b + 64).hex() == hashlib.sha256(m).hexdigest()
