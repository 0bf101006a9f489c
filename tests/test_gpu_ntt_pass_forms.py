"""GPU: the three bodies of the transform passes give the same device words (zkhip_config.ntt_pass_form, include/zkhip.h).

* form 0 (the default): k_ntt_pass4_ct_sq -- shape and mode as compile-time constants, every HBM read of a tile issued before the first
  wait -- for the passes of the two-pass 2^22-point transform (plain, input twiddle
  and bit-reversed scaled source: every pass of the flagship's LDEs); for every other pass k_ntt_pass4_ct, one instantiation per tile
  shape, or the run-time-shaped k_ntt_pass4 where no instantiation fits (both passes of 2^12 points, the second pass of 2^13 points,
  and its first pass at 1024 lanes);
* form 1: k_ntt_pass4_ct for the passes of the 2^22-point transform too, the body of rounds 1 - 6;
* form 2: the radix-2 passes k_ntt_dif_pass and the bit-reversal scaling, at every size.

Every pass shape the dispatcher can choose is run: transforms of 2^12 .. 2^24 points (two and three passes, tiles of 2^7 .. 2^11 rows) under
ntt_log_lanes = 8, 9, 10, forward, inverse and bit-reversed output (plain and input-twiddle passes), and coset LDEs of blow-up 2 and 4 with two
shifts (the bit-reversed scaled source and its coset scaling).  Inputs: seeded random columns and the structured operands of
tests/boundary_inputs.py (raw device words 0, 1, p-1, (p+-1)/2, columns of all p-1, deltas, sparse columns).  The comparison is of the raw
device words (Montgomery form, each < p), with no tolerance: these are exact field elements, and a word that is right modulo p but not
reduced is a difference too.  The column-table form of the passes (lde_batch_cols: the prover's LDEs) is compared through whole proofs."""
import numpy as np
import pytest

import boundary_inputs as bi


def _has_gpu():
    try:
        import torch

        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _has_gpu(), reason="needs a GPU (never skipped on a GPU machine)")]

P = bi.P
FORMS = (0, 1, 2)


def words(t):
    """the tensor's device words as they are (no conversion)"""
    return t.cpu().numpy().view(np.uint32)


def run_forms(zk, fn, what, forms=FORMS):
    """fn() under every form: all words < p and equal to form 1's (the retained body) -- so forms 0 and 2 equal each other too"""
    got = {}
    for f in forms:
        zk.set_config(ntt_pass_form=f)
        got[f] = fn()
        assert (got[f] < P).all(), "%s: form %d leaves an unreduced word" % (what, f)
    for f in forms:
        if f != 1:
            bad = np.flatnonzero(got[f] != got[1])
            assert bad.size == 0, "%s: form %d differs from form 1 in %d words, first at %d" % (what, f, bad.size, bad[0])
    return got[1]


def transforms(zk, m, log_n, what, lde=((1, 31),)):
    """forward, inverse, bit-reversed output and coset LDEs of the [width, 2^log_n] canonical matrix m under every form"""
    width = m.shape[0]

    def ntt(**kw):
        def fn():
            t = zk.upload(m.reshape(-1))
            zk.ntt_batch(t, log_n, width, **kw)
            return words(t)
        return fn

    run_forms(zk, ntt(), what + " forward")
    run_forms(zk, ntt(inverse=True), what + " inverse")
    run_forms(zk, ntt(bitrev_out=True), what + " forward, bit-reversed out")
    for added_bits, shift in lde:
        d = zk.upload(m.reshape(-1))
        run_forms(zk, lambda: words(zk.lde_batch(d, log_n, added_bits, width, shift)), what + " LDE blow-up %d shift %d" % (1 << added_bits, shift))


SIZES = [(12, 5), (13, 3), (14, 4), (15, 3), (16, 3), (17, 2), (18, 3), (19, 2), (20, 3), (21, 2), (22, 3)]
# (ntt_log_lanes reaches the passes of at most 2^10 rows: the two passes of 2^22 points have 2^11 and run once)
CASES = [(lanes, log_n, width) for lanes in (10, 9, 8) for log_n, width in SIZES if log_n < 22 or lanes == 10]


@pytest.mark.parametrize("log_lanes,log_n,width", CASES)
def test_every_pass_shape_on_random_columns(zk, log_lanes, log_n, width):
    zk.set_config(ntt_log_lanes=log_lanes)
    rng = np.random.default_rng(700 + 100 * log_lanes + log_n)
    m = rng.integers(0, P, size=(width, 1 << log_n), dtype=np.uint64).astype(np.uint32)
    transforms(zk, m, log_n, "2^%d x %d, random, %d lanes" % (log_n, width, 1 << log_lanes), lde=((1, 31), (2, 7)))


@pytest.mark.parametrize("log_lanes,log_n,width", CASES)
def test_every_pass_shape_on_boundary_operands(zk, log_lanes, log_n, width):
    zk.set_config(ntt_log_lanes=log_lanes)
    rng = np.random.default_rng(900 + 100 * log_lanes + log_n)
    # every family at the specialised shape and at the smallest size; one member of each family in between
    small = log_n not in (12, 22) or log_lanes != 10
    for name, m in bi.families(rng, width, 1 << log_n, small=small):
        transforms(zk, m, log_n, "2^%d x %d, %s, %d lanes" % (log_n, width, name, 1 << log_lanes), lde=((1, 31),))


@pytest.mark.parametrize("log_n", [23, 24])
def test_three_pass_shapes(zk, log_n):
    rng = np.random.default_rng(log_n)
    m = rng.integers(0, P, size=(1, 1 << log_n), dtype=np.uint64).astype(np.uint32)
    transforms(zk, m, log_n, "2^%d, random" % log_n)
    m = bi.boundary_cells(rng, (1, 1 << log_n))
    transforms(zk, m, log_n, "2^%d, boundary" % log_n)


def test_wide_batches_and_column_strides_at_the_specialised_shape(zk):
    """2^22 points: a batch wider than the tile grid's row of workgroups needs (33 columns), with column strides larger than the height, and
    four cosets with another shift"""
    log_n, width = 22, 33
    n = 1 << log_n
    rng = np.random.default_rng(2233)
    m = rng.integers(0, P, size=(width, n), dtype=np.uint64).astype(np.uint32)
    m[5] = bi.raw_words(np.full(n, P - 1))
    m[6] = bi.boundary_cells(rng, n)
    d = zk.upload(m.reshape(-1))
    run_forms(zk, lambda: words(zk.lde_batch(d, log_n, 1, width, 31)), "33 columns LDE")
    in_stride, out_stride = n + 4096, 4 * n + 8192
    padded = np.zeros((4, in_stride), np.uint32)
    padded[:, :n] = m[3:7]
    dp = zk.upload(padded.reshape(-1))
    run_forms(zk, lambda: words(zk.lde_batch(dp, log_n, 2, 4, 7, in_stride=in_stride, out_stride=out_stride)).reshape(4, out_stride)[:, :4 * n].copy(),
              "strided LDE, four cosets")

    def strided_ntt():
        t = zk.upload(padded.reshape(-1))
        zk.ntt_batch(t, log_n, 4, stride=in_stride, bitrev_out=True)
        return words(t)
    run_forms(zk, strided_ntt, "strided forward")


def test_whole_proofs_are_the_same_bytes(zk):
    """the prover's LDEs go through the column-table form of the passes (per-column source and destination pointers): a proof over 2^22 rows
    under forms 0 and 1"""
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    sa = air.SyntheticAir(width=24, n_free=8, n_bool=2, n_boundary=2, seed=34)
    tr, pv = sa.gen_trace(22, seed=4)
    airs = [dict(program=sa.program(), log_height=22, width=24, n_pvs=len(pv))]
    dt = zk.upload(tr.reshape(-1))
    proofs = []
    for f in (1, 0):
        zk.set_config(ntt_pass_form=f)
        proofs.append(z.ProvingKey(zk, z.DEFAULT_PARAMS, airs).prove([dt], [pv]))
    assert proofs[0] == proofs[1]
    assert z.verify(z.DEFAULT_PARAMS, airs, [pv], proofs[0]) == 0
