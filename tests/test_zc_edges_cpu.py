"""CPU: the edge shapes of tests/zc_edge_shapes.py through the independent models and the library's host verifiers -- for every shape
the model's proof is accepted by the model verifier and by zkhip_zerocheck_verify / zkhip_airset_verify, its length is what
*_proof_words says, and one flipped word in the AIR's part is refused.  This pins zc_plan, zc_eval_host, zc_rot_eval and the AIR-set
host verifier at D = 1, 2, 7, 8, n_rot = w, a column read only at rotation 1, width 1, each selector alone at m = 1, 64 AIRs, L = 1,
no padding block, mixed block sizes and 32 fields before a device is involved, and it checks the builders themselves."""
import pytest

import airset_model as am
import gkr_model as gm
import whir_model as wm
import zc_edge_shapes as es
import zerocheck_model as zm
from pymodel import P, Challenger
from test_zerocheck_cpu import ERR_INVALID, ERR_VERIFY, _lp, _params

PRM = _params(1, 2, 1)


def _flip(words, i):
    bad = list(words)
    bad[i] = (bad[i] + 1) % P
    return bad


def _zc(airs, traces, pvs, l, prefix):
    import zkvm_prover_amd as z

    ch = Challenger()
    ch.observe(prefix)
    root, words = zm.prove(ch, PRM, airs, traces, pvs, l)
    assert len(words) == zm.proof_words(PRM, airs, l) == z.zerocheck_proof_words(_lp(PRM), airs, l)
    ch = Challenger()
    ch.observe(prefix)
    assert zm.verify(ch, PRM, airs, pvs, l, words) == root
    assert z.zerocheck_verify(_lp(PRM), prefix, airs, pvs, l, words).tolist() == root
    head = 8 + sum(zm.Plan(a).words() for a in airs)
    for i in sorted({8, 8 + (head - 8) // 2, head - 1}):   # a round polynomial, the middle, the last value
        with pytest.raises(z.ZkhipError) as e:
            z.zerocheck_verify(_lp(PRM), prefix, airs, pvs, l, _flip(words, i))
        assert e.value.code == ERR_VERIFY
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises(wm.WhirReject):
            zm.verify(ch, PRM, airs, pvs, l, _flip(words, i))
    return words


@pytest.mark.parametrize("name", sorted(es.ZC_SHAPES))
def test_zerocheck_edge_shape(name):
    a, tr, pvs = es.ZC_SHAPES[name]()
    _zc([a], [tr], [pvs], 4, [3, 1])


def test_zerocheck_many_airs():
    """64 AIRs (ZKHIP_STACK_MAX_POINTS) of m = 1, 2, 3: Fibonacci, D = 1, no proven constraint and width 1 in turn"""
    airs, traces, pvs = es.many(64)
    _zc(airs, traces, pvs, 4, [64])


def test_degree_limit():
    """D = 9 is refused by the model and by zerocheck_proof_words and zerocheck_verify (ZKHIP_ERR_INVALID); D = 8 is taken above"""
    import zkvm_prover_amd as z

    a = es._air(es.prod_builder(8), 2)
    assert zm.proof_words(PRM, [a], 4) == 0 == z.zerocheck_proof_words(_lp(PRM), [a], 4)
    with pytest.raises(z.ZkhipError) as e:
        z.zerocheck_verify(_lp(PRM), [], [a], [[]], 4, [0] * 64)
    assert e.value.code == ERR_INVALID
    with pytest.raises(zm.Refused):
        zm.Plan(a)


@pytest.mark.parametrize("name", sorted(es.AS_SHAPES))
def test_airset_edge_shape(name):
    import zkvm_prover_amd as z

    airs, traces, pvs, l, L = es.as_shape(name)
    prefix = [5, 2]
    ch = Challenger()
    ch.observe(prefix)
    root, words, info = am.prove(ch, PRM, airs, traces, pvs, l)
    assert info["L"] == L
    assert len(words) == am.proof_words(PRM, airs, l) == z.airset_proof_words(_lp(PRM), airs, l)
    ch = Challenger()
    ch.observe(prefix)
    mroot, mpq = am.verify(ch, PRM, airs, pvs, l, words)
    lroot, lpq = z.airset_verify(_lp(PRM), prefix, airs, pvs, l, words)
    assert mroot == root == lroot.tolist() and lpq.tolist() == mpq[0] + mpq[1] and mpq[0] == am.ZERO
    g = 8 + gm.proof_words(L)
    head = g + 4 * sum(1 for a in airs if am.Plan(a).ints) + sum(am.Plan(a).words() for a in airs)
    for i in sorted({8, g - 1, g, g + (head - g) // 2, head - 1}):   # the GKR words, a B_a, a round polynomial, the last value
        with pytest.raises(z.ZkhipError) as e:
            z.airset_verify(_lp(PRM), prefix, airs, pvs, l, _flip(words, i))
        assert e.value.code == ERR_VERIFY
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject)):
            am.verify(ch, PRM, airs, pvs, l, _flip(words, i))


def test_field_limit():
    """a message of 33 fields (above LOGUP_MAX_FIELDS) is refused with ZKHIP_ERR_INVALID; 32 are taken above"""
    import zkvm_prover_amd as z

    a = es.fields33_air()
    assert z.airset_proof_words(_lp(PRM), [a], 4) == 0
    with pytest.raises(z.ZkhipError) as e:
        z.airset_verify(_lp(PRM), [], [a], [[]], 4, [0] * 64)
    assert e.value.code == ERR_INVALID


class _LeavesSeen(Exception):
    pass


@pytest.mark.parametrize("kind,m", es.AS_FAMILY_CASES)
def test_operand_families_have_no_zero_denominator(kind, m):
    """the AIR-set operand families of test_gpu_zc_boundary.py under the committed seed, up to the leaves (am.leaves inside am.prove,
    with the challenges the device will draw): a family with a zero denominator is skipped there, and at most one per case may be"""
    airs, pi, fams = es.as_family_case(kind, m)
    prm = [_params(1, 1, 0), _params(2, 2, 1, pow_bits=3, nq=4)][pi]

    def hook(num, den):
        es.no_zero_den(num, den)
        raise _LeavesSeen()

    skipped = 0
    for name, traces, pvs, prefix in fams:
        ch = Challenger()
        ch.observe(prefix)
        try:
            am.prove(ch, prm, airs, [t.tolist() for t in traces], pvs, 4, leaf_hook=hook)
        except es.ZeroDenominator:
            skipped += 1
        except _LeavesSeen:
            pass
    assert len(fams) >= 19 and skipped <= 1
