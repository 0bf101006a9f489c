"""GPU: the AIR zero-check and the AIR-set proof at edge shapes, on boundary operands and through the second iteration of their
grid-stride loops (docs/boundary_tests.md).

1. Every shape of tests/zc_edge_shapes.py: the device words equal the model's and the host verifier accepts (the helpers of
   test_gpu_zerocheck.py / test_gpu_airset.py); the largest program the prover takes (ZC_MAX_SLOTS live intermediates: the extension
   pass's 64 KiB of dynamic LDS) is found by scanning, proven, and one more intermediate is ZKHIP_ERR_INVALID.
2. / 3. The families of tests/boundary_inputs.py as traces (raw p-1, (p+-1)/2, MONTY_ONE, zero columns, p-1 / 0 alternations, one-hot
   rows, cells from the boundary set): the words equal the model's; the host verifier accepts exactly when the constraints hold
   (air.check_trace) / when the model's verifier accepts, and refuses whenever the buses do not balance.
4. 2^19 rows: every grid-stride loop of the per-AIR kernels runs its second iteration.  The model is out of
   reach there; the references are the host verifier (a wrong partial sum fails a round check except with probability about
   m D / 2^124), numpy MLEs of v, v' and u, and the refusal of proofs over a trace with one cell changed in a row that only a later
   iteration reads."""
import numpy as np
import pytest

import airset_model as am
import boundary_inputs as bi
import test_gpu_airset as ga
import test_gpu_zerocheck as gz
import zc_edge_shapes as es
import zerocheck_model as zm
import zkvm_prover_amd as z
from pymodel import Challenger
from test_zerocheck_cpu import ERR_INVALID, ERR_VERIFY, _air, _fib, _synth
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P
PRM = gz._params(1, 2, 1)
PARAM_SETS = [gz._params(1, 1, 0), gz._params(2, 2, 1, pow_bits=3, nq=4)]
SEED = 20240611
# public values: canonical 0, 1, p-1 and the value whose Montgomery word is p-1
PV_POOL = [0, 1, P - 1, int(bi.raw_words([P - 1])[0])]


# ---- 1. edge shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(es.ZC_SHAPES))
def test_zerocheck_edge_shape(zk, name):
    a, tr, pvs = es.ZC_SHAPES[name]()
    gz._against_model(zk, PRM, [a], [tr], [pvs], 4, [3, 1])


def test_zerocheck_64_airs(zk):
    airs, traces, pvs = es.many(64)
    gz._against_model(zk, PRM, airs, traces, pvs, 4, [64])


@pytest.mark.parametrize("name", sorted(es.AS_SHAPES))
def test_airset_edge_shape(zk, name):
    airs, traces, pvs, l, L = es.as_shape(name)
    assert ga._against_model(zk, PRM, airs, traces, pvs, l, [5, 2])["L"] == L


def _refused(call, code=ERR_INVALID):
    with pytest.raises(z.ZkhipError) as e:
        call()
    assert e.value.code == code


def _verify_refused(call):
    _refused(call, ERR_VERIFY)


def test_degree_and_field_limits_are_error_returns(zk):
    """D = 9 and a message of 33 fields: ZKHIP_ERR_INVALID from the provers before anything is launched"""
    a = _air(es.prod_builder(8), 2)
    _refused(lambda: zk.zerocheck_prove(gz._lp(PRM), [a], gz._upload(zk, [np.zeros((8, 4))]), [[]], 4, []))
    a = es.fields33_air()
    _refused(lambda: zk.airset_prove(gz._lp(PRM), [a], gz._upload(zk, [np.zeros((34, 2))]), [[]], 4, []))


def _largest_accepted(prove_k, lo=48, hi=80):
    """the largest k in [lo, hi) that prove_k takes, scanning upward; k + 1 must be ZKHIP_ERR_INVALID (an error return, no launch
    failure: any other error code fails here)"""
    k = lo
    prove_k(k)
    while k + 1 < hi:
        try:
            prove_k(k + 1)
        except z.ZkhipError as e:
            assert e.code == ERR_INVALID, e
            return k
        k += 1
    pytest.fail("no program up to k = %d was refused" % hi)


def test_zerocheck_program_at_the_slot_limit(zk):
    """the largest `slots(k)` the prover takes asks k_zc_pass for all of its dynamic LDS (64 slots x 64 lanes x 16 B = 64 KiB)"""
    def prove_k(k):
        a, tr, pvs = es.slots(k, 1)
        return zk.zerocheck_prove(gz._lp(PRM), [a], gz._upload(zk, [tr]), [pvs], 4, [k])

    k = _largest_accepted(prove_k)
    assert 56 <= k <= 64    # k live x_i and a few sums: the limit is 64 slots
    for m in (1, 3):
        a, tr, pvs = es.slots(k, m)
        gz._against_model(zk, PRM, [a], [tr], [pvs], 4, [k, m])


def test_airset_interaction_program_at_the_slot_limit(zk):
    """the same for an interaction's operand program (k_as_leaves: 64 slots x 256 lanes x 4 B = 64 KiB) and the joint pass"""
    def prove_k(k):
        a, tr, pvs = es.slots_bus(k, 1)
        return zk.airset_prove(gz._lp(PRM), [a], gz._upload(zk, [tr]), [pvs], 4, [k])

    k = _largest_accepted(prove_k)
    assert 56 <= k <= 64
    for m in (1, 3):
        a, tr, pvs = es.slots_bus(k, m)
        ga._against_model(zk, PRM, [a], [tr], [pvs], 4, [k, m])


# ---- 2. operand families, the zero-check --------------------------------------------------------------------------------------------------
def _zc_air(kind, m):
    if kind == "fib":
        return _fib(m)[0]
    if kind == "synth":
        return _synth(m, 3)[0]
    return _air(es.all_rot_builder(3), m)


def _zc_words_equal(zk, prm, a, tr, pvs, l, prefix, name):
    root, proof = zk.zerocheck_prove(gz._lp(prm), [a], gz._upload(zk, [tr]), [pvs], l, prefix)
    ch = Challenger()
    ch.observe(prefix)
    mroot, words = zm.prove(ch, prm, [a], [tr.tolist()], [pvs], l)
    assert root.tolist() == mroot, name
    if proof.tolist() != words:
        pytest.fail("%s: proof differs from the model at word %d of %d" % (name, int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    if air.check_trace(a["program"], tr, pvs) == []:
        assert z.zerocheck_verify(gz._lp(prm), prefix, [a], [pvs], l, proof).tolist() == mroot, name
    else:
        _verify_refused(lambda: z.zerocheck_verify(gz._lp(prm), prefix, [a], [pvs], l, proof))


M10_CONSTS = ["const raw 0x%08x" % c for c in (0, (P + 1) // 2, bi.MONTY_ONE)]
ZC_FAMILY_CASES = [(k, m) for k in ("fib", "synth", "all_rot") for m in (1, 2, 5)] + [("fib", 10)]


@pytest.mark.parametrize("kind,m", ZC_FAMILY_CASES)
def test_zerocheck_operand_families(zk, kind, m):
    """every family as the trace (it does not satisfy the constraints, bar the all-zero one: the verifier must then refuse); public
    values from {0, 1, p-1, raw p-1}; the two parameter sets alternate over the cases.  m = 10: the rotation reduction streams one
    round before its LDS tail (there the model takes 0.7 s per proof: one member of each family plus the constants raw 0,
    (p+1)/2 and MONTY_ONE)"""
    a = _zc_air(kind, m)
    case = ZC_FAMILY_CASES.index((kind, m))
    prm, l = (gz._params(1, 4, 2), 9) if m == 10 else (PARAM_SETS[case % 2], 4)
    rng = np.random.default_rng(SEED + case)
    refused = 0
    fams = bi.families(rng, a["width"], 1 << m, small=m == 10)
    if m == 10:
        fams += [f for f in bi.families(rng, a["width"], 1 << m) if f[0] in M10_CONSTS]
        assert len(fams) == 4 + len(M10_CONSTS)
    for i, (name, tr) in enumerate(fams):
        pvs = [PV_POOL[(i + j) % 4] for j in range(a["n_pvs"])]
        refused += air.check_trace(a["program"], tr, pvs) != []
        _zc_words_equal(zk, prm, a, tr, pvs, l, [case, i], "%s m=%d %s" % (kind, m, name))
    assert refused >= len(fams) - 1


# ---- 3. operand families, the AIR-set ------------------------------------------------------------------------------------------------------
def _as_words_equal(zk, prm, airs, traces, pvs, l, prefix, name):
    """False: a denominator is zero, the family is skipped (the model's GKR cannot invert it)"""
    ch = Challenger()
    ch.observe(prefix)
    try:
        mroot, words, info = am.prove(ch, prm, airs, [t.tolist() for t in traces], pvs, l, leaf_hook=es.no_zero_den)
    except es.ZeroDenominator:
        return False
    root, proof = zk.airset_prove(gz._lp(prm), airs, gz._upload(zk, traces), pvs, l, prefix)
    assert root.tolist() == mroot, name
    if proof.tolist() != words:
        pytest.fail("%s: proof differs from the model at word %d of %d" % (name, int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    ch = Challenger()
    ch.observe(prefix)
    try:
        am.verify(ch, prm, airs, pvs, l, words)
        accepted = True
    except (ga.wm.WhirReject, ga.gm.GkrReject):
        accepted = False
    assert not (accepted and words[8:12] != am.ZERO), name    # unbalanced buses are never accepted
    if accepted:
        assert z.airset_verify(gz._lp(prm), prefix, airs, pvs, l, proof)[0].tolist() == mroot, name
    else:
        _verify_refused(lambda: z.airset_verify(gz._lp(prm), prefix, airs, pvs, l, proof))
    return True


@pytest.mark.parametrize("kind,m", es.AS_FAMILY_CASES)
def test_airset_operand_families(zk, kind, m):
    """every family as the trace(s) of bus_mix_air / of a sender and table pair, plus count columns at raw p-1 (multiplicity -1 on
    every row), canonical p-1 and zero; at most one family per case may be skipped for a zero denominator (none is under the
    committed seed: test_zc_edges_cpu.py checks that without a device)"""
    airs, prm, fams = es.as_family_case(kind, m)
    done = 0
    for name, traces, pvs, prefix in fams:
        done += _as_words_equal(zk, PARAM_SETS[prm], airs, traces, pvs, 4, prefix, "%s m=%d %s" % (kind, m, name))
    assert done >= len(fams) - 1


# ---- 4. the second iteration of the grid-stride loops ------------------------------------------------------------------------------------
def _fib_trace(m, a0=3, b0=5):
    a, b, ca, cb = a0, b0, [], []
    for _ in range(1 << m):
        ca.append(a), cb.append(b)
        a, b = b, (a + b) % P
    return np.array([ca, cb], dtype=np.uint32), [a0, b0, cb[-1]]


def _check_values(prm, prefix, airs, pvs, proof, traces, i):
    """v, v' and u of AIR i's first and last column against numpy MLEs of the column and of the column rolled by one row"""
    pl, r, rp, qv = gz._replay_points(prm, prefix, airs, pvs, proof)[i]
    t = np.asarray(traces[i], dtype=np.uint32)
    qu = qv + 4 * (pl.w + len(pl.rot)) + 8 * pl.m
    for j in (0, pl.w - 1):
        assert proof[qv + 4 * j:qv + 4 * j + 4].tolist() == gz._np_mle_base(t[j], np.array(r))
        assert proof[qu + 4 * j:qu + 4 * j + 4].tolist() == gz._np_mle_base(t[j], np.array(rp))
        k = qv + 4 * (pl.w + pl.rot.index(j))
        assert proof[k:k + 4].tolist() == gz._np_mle_base(np.roll(t[j], -1), np.array(r))


def test_zerocheck_strided_loops(zk):
    """Fibonacci at 2^19 rows beside one of 2^10 and col2 = col0 col1 at 2^19 rows: k_zc_round0 runs four iterations per lane, k_zc_pass<from the base trace>,
    k_zc_combine, k_sc_pass and the loops sized by grid_of two.  Fibonacci's constraints are a selector times a linear form, so an
    honest pair adds zero to every round-0 sum at every point and its acceptance says nothing about k_zc_round0's later
    iterations: the product AIR is there for them (its honest pairs do add to the sums at t = 2).  One Fibonacci cell is changed in row 2^17 + 5 (its second iteration), in row 2^18 + 5 (its third, and the second of the
    others) and in the last row, and each of the three proofs must be refused."""
    m = 19
    big, pv = _fib_trace(m)
    small = _fib(10)
    mb = air.AirBuilder(3, 0)
    mb.assert_zero(mb.var(0) * mb.var(1) - mb.var(2))
    mt = np.random.default_rng(SEED).integers(0, P, size=(3, 1 << m), dtype=np.int64)
    mt[2] = mt[0] * mt[1] % P
    airs = [dict(small[0], log_height=m), small[0], _air(mb, m)]
    traces, pvs = [big, np.array(small[1], dtype=np.uint32), mt.astype(np.uint32)], [pv, small[2], []]
    prm, l, prefix = gz._lp(gz._params(1, 4, 4, pow_bits=8, nq=20)), 19, [19]
    root, proof = zk.zerocheck_prove(prm, airs, gz._upload(zk, traces), pvs, l, prefix)
    assert z.zerocheck_verify(prm, prefix, airs, pvs, l, proof).tolist() == root.tolist()
    _check_values(prm, prefix, airs, pvs, proof, traces, 0)
    for row in ((1 << 17) + 5, (1 << 18) + 5, (1 << m) - 1):
        bad = big.copy()
        bad[0, row] = (int(bad[0, row]) + 1) % P
        _, proof = zk.zerocheck_prove(prm, airs, gz._upload(zk, [bad] + traces[1:]), pvs, l, prefix)
        _verify_refused(lambda: z.zerocheck_verify(prm, prefix, airs, pvs, l, proof))


AS_STRIDE_M = 19


def test_airset_strided_loops(zk):
    """bus_mix_air at 2^19 rows (6 blocks of 2^19 leaves, L = 22): k_zc_round0<BUS> runs four iterations per lane, k_zc_pass<BUS> from
    the base trace two, k_as_claims 192 per AIR (the AIR reads no next row, so there is no rotation reduction here).  Constraint 0 has
    degree 2, so honest pairs do add to the round sums and acceptance checks every iteration; one cell is then changed in a row of
    the second, of the third and of the last iteration of k_zc_round0.  The leaves in numpy (every B_a) are left out: am.leaves
    is pure Python and 3 M leaves are out of its reach; the host verifier's check of sum B_a against the GKR's claims stands in, and a
    proof over a trace whose last leaf of bus 9 was changed (the buses no longer balance) is refused."""
    m = AS_STRIDE_M
    tr, pv = air.bus_mix_trace(m, seed=3)
    a = _air(air.bus_mix_air(), m)
    prm, l, prefix = gz._lp(gz._params(1, 4, 4, pow_bits=8, nq=20)), 19, [m]
    root, proof = zk.airset_prove(prm, [a], gz._upload(zk, [tr]), [pv], l, prefix)
    lroot, pq = z.airset_verify(prm, prefix, [a], [pv], l, proof)
    assert lroot.tolist() == root.tolist() and pq.tolist()[:4] == [0, 0, 0, 0]
    for row in ((1 << (m - 2)) + 5, (1 << (m - 1)) + 5, (1 << m) - 1):
        bad = tr.copy()
        bad[2, row] = (int(bad[2, row]) + 1) % P    # constraint 0 fails on that row; column 2 is sent and received alike on bus 11
        _, proof = zk.airset_prove(prm, [a], gz._upload(zk, [bad]), [pv], l, prefix)
        assert proof[8:12].tolist() == [0, 0, 0, 0]
        _verify_refused(lambda: z.airset_verify(prm, prefix, [a], [pv], l, proof))
    bad = tr.copy()
    bad[4, -1] = (int(bad[4, -1]) + 1) % P    # the last leaf of bus 9's receiving block: the buses no longer balance, P != 0
    _, proof = zk.airset_prove(prm, [a], gz._upload(zk, [bad]), [pv], l, prefix)
    assert proof[8:12].tolist() != [0, 0, 0, 0]
    _verify_refused(lambda: z.airset_verify(prm, prefix, [a], [pv], l, proof))
