"""GPU: the limb-chip trace generators (csrc/modular.hip, fp2.hip, ecc.hip, int256.hip) under zkhip_tables_canonical, the mode of the vm
flow in which no generator converts the shared count tables around its increments.  The same accepted records (tests/limb_boundary_inputs.py)
run twice into zeroed bitwise and tuple tables: in the default mode, and in canonical mode followed by one zkhip_to_monty.  Trace and both
tables must agree word for word, and in canonical mode the raw bitwise counts are the counts of the trace's own cells."""
import ctypes as C

import numpy as np
import pytest
import torch

import ecc_util as eu
import fp2_util as fu
import int256_util as iu
import limb_boundary_inputs as lb
from test_gpu_limb_boundary import dev, same

pytestmark = pytest.mark.gpu
SX, SY = 256, 2048   # one tuple table wide enough for every chip (the modular chip asks for y < 128, int256 mul for y < 32)
SHAPES = [(5, 3), (65, 7)]   # padding rows; past the 64-lane workgroup of k_fp2_trace / k_ec_trace


def modular(name):
    p = lb.MODULI[name]

    def run(zk, n, log_h, d_bw, d_tup):
        recs = [lb.modular_record_words(r, p) for r in lb.cycle(lb.modular_mixed(p), n)]
        return zk.modular_tracegen(p, dev(zk, recs), n, log_h, d_bw, d_tup, SX, SY)

    return run, lambda tr, n: (lb.recount_modular(tr, n, lb.limbs_of(p))[0], None)


def fp2(name):
    p = lb.MODULI[name]

    def run(zk, n, log_h, d_bw, d_tup):
        recs = [fu.record(*c, n=lb.limbs_of(p) // 4) for c in lb.fp2_all(p, n)]
        return zk.fp2_tracegen(p, dev(zk, recs), n, log_h, d_bw, d_tup, SX, SY)

    return run, lambda tr, n: (lb.recount_fp2(tr, n, lb.limbs_of(p))[0], None)


def ecc(name):
    cv = lb.Curve(name)

    def run(zk, n, log_h, d_bw, d_tup):
        recs = [eu.record(*c, n=lb.limbs_of(cv.p) // 4) for c in lb.ecc_all(name, n)]
        return zk.ec_tracegen(cv.p, cv.a, dev(zk, recs), n, log_h, d_bw, d_tup, SX, SY)

    return run, lambda tr, n: (lb.recount_ecc(tr, n, lb.limbs_of(cv.p))[0], None)


def int256(chip):
    def run(zk, n, log_h, d_bw, d_tup):
        if chip == "mul":
            recs = [iu.words(b) + iu.words(c) for b, c in lb.cycle(lb.mul_cases(), n)]
            return zk.int256_mul_tracegen(dev(zk, recs), n, log_h, d_bw, d_tup, SX, SY)
        cases = lb.cycle(lb.cmp_cases() if chip == "cmp" else lb.shift_cases(), n)
        gen = zk.int256_cmp_tracegen if chip == "cmp" else zk.int256_shift_tracegen
        return gen(dev(zk, iu.records(cases)), n, log_h, d_bw)

    def recount(tr, n):   # (range counts, XOR counts or None where the chip leaves that column alone)
        if chip == "mul":
            return lb.recount_mul(tr, n)[0], None
        return (lb.recount_cmp(tr, n), None) if chip == "cmp" else lb.recount_shift(tr, n)

    return run, recount


CHIPS = {"modular8": modular("secp256k1_p"), "modular12": modular("bls12_381_p"), "fp2": fp2("bn254_p"), "ecc": ecc("secp256k1"),
         "int256_mul": int256("mul"), "int256_cmp": int256("cmp"), "int256_shift": int256("shift")}


@pytest.mark.parametrize("n,log_h", SHAPES)
@pytest.mark.parametrize("chip", list(CHIPS))
def test_canonical_tables_give_the_default_mode_words(zk, chip, n, log_h):
    run, recount = CHIPS[chip]
    fresh = lambda: (torch.zeros(2 << 16, dtype=torch.int32, device=zk.device), torch.zeros(SX * SY, dtype=torch.int32, device=zk.device))  # noqa: E731
    bw, tup = fresh()
    tr = run(zk, n, log_h, bw, tup)
    bw2, tup2 = fresh()
    assert zk.lib.zkhip_tables_canonical(zk.h, 1) == 0
    try:
        tr2 = run(zk, n, log_h, bw2, tup2)
        zk.sync()
        raw = bw2.cpu().numpy().view(np.uint32).reshape(2, -1)   # canonical counts as they are
    finally:
        assert zk.lib.zkhip_tables_canonical(zk.h, 0) == 0
    for t in (bw2, tup2):
        zk._check(zk.lib.zkhip_to_monty(zk.h, C.c_void_p(t.data_ptr()), t.numel()))
    assert torch.equal(tr, tr2), chip + ": trace"
    assert torch.equal(bw, bw2), chip + ": bitwise table"
    assert torch.equal(tup, tup2), chip + ": tuple table"
    want_range, want_xor = recount(zk.download(tr2).reshape(-1, 1 << log_h), n)
    same(raw[0], want_range, chip + " canonical range counts")
    same(raw[1], want_xor if want_xor is not None else np.zeros(1 << 16, np.int64), chip + " canonical xor counts")
    assert raw[0].any() and (chip == "int256_cmp" or chip == "int256_shift" or zk.download(tup).any())
