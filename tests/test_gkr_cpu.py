"""CPU: the LogUp-GKR protocol (docs/logup_gkr.md) -- the independent model (tests/gkr_model.py) against itself and against the
library's host verifiers (zkhip_gkr_fraction_verify, zkhip_bus_gkr_verify); forged, truncated and mis-sized proofs are refused."""
import random

import pytest

import gkr_model as gm
from pymodel import P, Challenger


def _leaves(rng, log_n, ext_num):
    n = 1 << log_n
    num = [[rng.randrange(P) for _ in range(4)] if ext_num else rng.randrange(P) for _ in range(n)]
    den = [[rng.randrange(P) for _ in range(4)] for _ in range(n)]
    return num, den


def _model_proof(log_n, ext_num, seed):
    rng = random.Random(seed)
    prefix = [rng.randrange(P) for _ in range(rng.randrange(0, 12))]
    num, den = _leaves(rng, log_n, ext_num)
    ch = Challenger()
    ch.observe(prefix)
    words, point, claims = gm.prove(ch, num, den)
    return prefix, num, den, words, point, claims


@pytest.mark.parametrize("log_n", [1, 2, 3, 5])
@pytest.mark.parametrize("ext_num", [False, True])
def test_model_proof_verifies_and_claims_are_the_leaves_mle(log_n, ext_num):
    prefix, num, den, words, point, claims = _model_proof(log_n, ext_num, 100 + log_n)
    assert len(words) == gm.proof_words(log_n)
    ch = Challenger()
    ch.observe(prefix)
    vpoint, vclaims, (root_p, root_q) = gm.verify(ch, words, log_n)
    assert vpoint == point and list(vclaims) == list(claims)
    assert claims[0] == gm.mle_eval(num, point) and claims[1] == gm.mle_eval(den, point)
    # the root is the sum of the fractions
    s = gm.ZERO
    for a, b in zip(num, den):
        s = gm.ext_add(s, gm.ext_mul(gm.as_ext(a), gm.ext_inv(b)))
    assert gm.ext_mul(root_p, gm.ext_inv(root_q)) == s


def test_proof_length_formula():
    import zkvm_prover_amd as z

    lib = z.load_library()
    assert gm.proof_words(24) == 3704
    for L in range(1, 29):
        assert lib.zkhip_gkr_proof_words(L) == gm.proof_words(L)
    assert lib.zkhip_gkr_proof_words(0) == 0 and lib.zkhip_gkr_proof_words(29) == 0


@pytest.mark.parametrize("log_n", range(1, 11))
@pytest.mark.parametrize("ext_num", [False, True])
def test_host_verifier_accepts_model_proofs(log_n, ext_num):
    import zkvm_prover_amd as z

    if log_n > 8 and ext_num:
        log_n -= 2   # keeps the model's share of the file short; 9 and 10 are covered with base numerators
    prefix, num, den, words, point, claims = _model_proof(log_n, ext_num, 7 * log_n + ext_num)
    vpoint, vclaims = z.gkr_verify(prefix, words, log_n)
    assert vpoint.tolist() == point
    assert vclaims.tolist() == [list(c) for c in claims]


def _classes(log_n):
    """one word of each class: root, round polynomial, layer values"""
    k = log_n - 1
    return {"root": 5, "round": gm.layer_offset(k) + 6, "layer": gm.layer_offset(k) + 12 * k + 9}


@pytest.mark.parametrize("cls", ["root", "round", "layer"])
def test_single_word_flip_is_refused_by_both_verifiers(cls):
    import zkvm_prover_amd as z

    log_n = 4
    prefix, num, den, words, point, claims = _model_proof(log_n, False, 42)
    bad = list(words)
    i = _classes(log_n)[cls]
    bad[i] = (bad[i] + 1) % P
    ch = Challenger()
    ch.observe(prefix)
    with pytest.raises(gm.GkrReject):
        gm.verify(ch, bad, log_n)
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, bad, log_n)
    # a different prefix is a different transcript
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(list(prefix) + [1], words, log_n)
    # a word that is not canonical
    big = list(words)
    big[i] += P
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, big, log_n)


def test_wrong_log_n_and_truncation_are_refused():
    import zkvm_prover_amd as z

    log_n = 5
    prefix, num, den, words, point, claims = _model_proof(log_n, True, 9)
    z.gkr_verify(prefix, words, log_n)
    for L in (log_n - 1, log_n + 1):
        with pytest.raises(z.ZkhipError):
            z.gkr_verify(prefix, words, L)
        with pytest.raises(gm.GkrReject):
            gm.verify(Challenger(), words, L)
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, words[:-1], log_n)
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, list(words) + [0], log_n)
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, [], 0)


def _bus_model_proof(balanced, seed, log_n=4):
    """leaves of a tiny bus: pairs (+1, d_i), (-1, d_i) cancel; the unbalanced form drops one sign"""
    rng = random.Random(seed)
    prefix = [rng.randrange(P) for _ in range(5)]
    ch = Challenger()
    ch.observe(prefix)
    gamma, beta = gm.bus_challenges(ch)
    n = 1 << log_n
    num, den = [], []
    for i in range(n // 2):
        d = gm.ext_add(gamma, gm.ext_c(1 + rng.randrange(1000)))
        num += [1, P - 1 if (balanced or i) else 1]
        den += [d, d]
    words, point, claims = gm.prove(ch, num, den)
    return prefix, (gamma, beta), num, den, words, point, claims


def test_bus_verifier_checks_the_balance():
    import zkvm_prover_amd as z

    prefix, (gamma, beta), num, den, words, point, claims = _bus_model_proof(True, 3)
    chal, vpoint, vclaims = z.bus_gkr_verify(prefix, words, 4)
    assert chal.tolist() == [gamma, beta]
    assert vpoint.tolist() == point and vclaims.tolist() == [list(c) for c in claims]
    assert gm.bus_verify(prefix, words, 4)[1] == point
    prefix, _, num, den, words, point, claims = _bus_model_proof(False, 3)
    with pytest.raises(z.ZkhipError):
        z.bus_gkr_verify(prefix, words, 4)
    with pytest.raises(gm.GkrReject):
        gm.bus_verify(prefix, words, 4)


def test_bus_verifier_refuses_a_vanishing_denominator():
    import zkvm_prover_amd as z

    rng = random.Random(11)
    prefix = [1, 2, 3]
    ch = Challenger()
    ch.observe(prefix)
    gm.bus_challenges(ch)
    d = [rng.randrange(P) for _ in range(4)]
    num, den = [0, 0, 5, P - 5], [gm.ZERO, gm.ZERO, d, d]   # P = 0 and Q = 0
    words, point, claims = gm.prove(ch, num, den)
    assert words[0:8] == [0] * 8
    with pytest.raises(z.ZkhipError):
        z.bus_gkr_verify(prefix, words, 2)
    with pytest.raises(gm.GkrReject):
        gm.bus_verify(prefix, words, 2)
