"""CPU: the AIR-set proof (docs/airset.md) -- the independent model (tests/airset_model.py) against brute force (the block layout,
the per-block split of the GKR's claims, the joint sum) and against the library's host verifier (zkhip_airset_verify): model proofs
over a grid of AIR sets and parameter sets are accepted; forged, mis-shaped and non-canonical proofs are refused, and so are honest
proofs over unbalanced or constraint-breaking traces and a proof whose GKR part ran on leaves that are not the committed traces'."""
import random

import numpy as np
import pytest

import airset_model as am
import gkr_model as gm
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, Challenger, ext_add, ext_mul

ERR_INVALID, ERR_VERIFY = -3, -7


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


PARAM_SETS = [_params(1, 1, 0), _params(2, 2, 1, pow_bits=3, nq=4)]


def _lp(p):
    import zkvm_prover_amd as z

    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _rext(rng):
    return [rng.randrange(P) for _ in range(4)]


def _air(builder, m):
    return {"program": builder.program(), "log_height": m, "width": builder.width, "n_pvs": builder.n_pvs}


def _lookup(ms, mt, seed=4):
    from zkvm_prover_amd import air

    snd, tab = air.lookup_traces(ms, mt, seed=seed)
    return [(_air(air.lookup_sender_air(), ms), snd.tolist(), []), (_air(air.lookup_table_air(), mt), tab.tolist(), [])]


def _fib(m):
    from zkvm_prover_amd import air

    tr, pvs = air.fibonacci_trace(m, 3, 5)
    return _air(air.fibonacci_air(), m), tr.tolist(), pvs.tolist()


def _limb(m):
    from zkvm_prover_amd import air

    return _air(air.limb_air(), m), air.limb_trace(m, seed=2).tolist(), []


def _bus_mix(m):
    from zkvm_prover_amd import air

    tr, pvs = air.bus_mix_trace(m, seed=3)
    return _air(air.bus_mix_air(), m), tr.tolist(), pvs.tolist()


def _set(name):
    """(airs, traces, pvs, log_stack)"""
    sets = {
        "lookup": lambda: (_lookup(3, 2), 4),
        "limb": lambda: ([_limb(3)], 4),
        "bus_mix": lambda: ([_bus_mix(2)], 4),
        "fib+lookup": lambda: ([_fib(3)] + _lookup(2, 2), 4),
        # a short AIR first (the caller's order is not the block order), T = 2 * 2 + 6 * 2 + 2 * 8 + 32 + 2 = 66 (no power of two),
        # Fibonacci and the sender above log_stack = 4
        "mixed": lambda: ([_limb(1), _bus_mix(1), _fib(5), _limb(3)] + _lookup(5, 1), 4),
    }
    items, l = sets[name]()
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], l


def _prove(prm, airs, traces, pvs, l, prefix, leaf_hook=None):
    ch = Challenger()
    ch.observe(prefix)
    return am.prove(ch, prm, airs, traces, pvs, l, leaf_hook)


def _accept(prm, airs, pvs, l, prefix, root, words):
    import zkvm_prover_amd as z

    assert len(words) == am.proof_words(prm, airs, l) == z.airset_proof_words(_lp(prm), airs, l)
    ch = Challenger()
    ch.observe(prefix)
    mroot, mpq = am.verify(ch, prm, airs, pvs, l, words)
    lroot, lpq = z.airset_verify(_lp(prm), prefix, airs, pvs, l, words)
    assert mroot == root == lroot.tolist()
    assert lpq.tolist() == mpq[0] + mpq[1] and mpq[0] == am.ZERO


def _refused(prm, airs, pvs, l, prefix, words, model=True, code=ERR_VERIFY):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.airset_verify(_lp(prm), prefix, airs, pvs, l, words)
    assert e.value.code == code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject, am.Refused, IndexError)):
            am.verify(ch, prm, airs, pvs, l, words)


# ---- the model's building blocks -------------------------------------------------------------------------------------------------
def test_block_layout_against_brute_force_placement():
    airs, _, _, _ = _set("mixed")
    plans = [am.Plan(a) for a in airs]
    blocks, T, L = am.layout(plans)
    # brute force: take the tallest remaining block (ties: AIR order, then program order) and put it at the first free leaf
    left = [(a, j) for a, p in enumerate(plans) for j in range(len(p.ints))]
    at, want = 0, []
    while left:
        top = max(plans[a].m for a, _ in left)
        a, j = next(b for b in left if plans[b[0]].m == top)
        left.remove((a, j))
        want.append((a, j, top, at))
        at += 1 << top
    assert blocks == want and T == at == 66 and L == 7
    assert all(off % (1 << m) == 0 for _, _, m, off in blocks)           # every block is aligned to its size
    assert [b[0] for b in blocks][:2] != sorted(b[0] for b in blocks)[:2]   # the block order is not the caller's AIR order
    # (the sender's filler constraint var0 (var0 - 1) 0 + .. counts 2 by the degree rule; the table has the bus part only: D = 1 + 1)
    assert [p.D for p in plans] == [3, 3, 3, 3, 3, 2] and [p.d_bus for p in plans] == [2, 1, 0, 2, 1, 1]
    one = am.layout([am.Plan(_lookup(1, 1)[1][0])])
    assert one[1:] == (2, 1)


@pytest.mark.parametrize("name", ["lookup", "mixed"])
def test_claims_split_per_block_with_the_padding_term(name):
    airs, traces, pvs, _ = _set(name)
    rng = random.Random(5)
    plans = [am.Plan(a) for a in airs]
    blocks, T, L = am.layout(plans)
    gamma, beta, kappa = _rext(rng), _rext(rng), _rext(rng)
    num, den = am.leaves(plans, blocks, L, traces, pvs, gamma, beta)
    assert all(n == 0 and d == am.ONE for n, d in zip(num[T:], den[T:]))
    rho = [_rext(rng) for _ in range(L)]
    eb = am.block_eq(blocks, rho)
    p, q = gm.mle_eval(num, rho), gm.mle_eval(den, rho)
    ps, qs, pad = am.ZERO, am.ZERO, am.ONE
    for (a, j, m, off), e in zip(blocks, eb):
        ps = ext_add(ps, ext_mul(e, gm.mle_eval(num[off:off + (1 << m)], rho[:m])))
        qs = ext_add(qs, ext_mul(e, gm.mle_eval(den[off:off + (1 << m)], rho[:m])))
        pad = wm.ext_sub(pad, e)
    assert ps == p and ext_add(qs, pad) == q
    B = am.leaf_claims(plans, blocks, eb, rho, num, den, kappa)
    tot = ext_mul(kappa, pad)
    for b in B:
        tot = ext_add(tot, b)
    assert tot == ext_add(p, ext_mul(kappa, q))


def test_the_joint_sum_equals_the_claim_on_satisfying_traces():
    airs, traces, pvs, _ = _set("mixed")
    rng = random.Random(6)
    plans = [am.Plan(a) for a in airs]
    blocks, T, L = am.layout(plans)
    gamma, beta, kappa = _rext(rng), _rext(rng), _rext(rng)
    num, den = am.leaves(plans, blocks, L, traces, pvs, gamma, beta)
    rho = [_rext(rng) for _ in range(L)]
    eb = am.block_eq(blocks, rho)
    B = am.leaf_claims(plans, blocks, eb, rho, num, den, kappa)
    coef = am.bus_coefs(plans, blocks, eb, beta, kappa)
    with_ints = [a for a, p in enumerate(plans) if p.ints]
    for a, pl in enumerate(plans):
        n = 1 << pl.m
        tau, apow = [_rext(rng) for _ in range(pl.m)], sm._powers(_rext(rng), len(pl.proven))
        et, er = gm.eq_table(tau), gm.eq_table(rho[:pl.m])
        acc = am.ZERO
        for x in range(n):
            cols = [gm.ext_c(c[x]) for c in traces[a]]
            if pl.proven:
                nexts = [gm.ext_c(traces[a][j][(x + 1) % n]) for j in pl.rot]
                c = pl.combine(cols, nexts, gm.ext_c(int(x == 0)), gm.ext_c(int(x == n - 1)), pvs[a], apow)
                acc = ext_add(acc, ext_mul(et[x], c))
            if pl.ints:
                acc = ext_add(acc, ext_mul(er[x], pl.bus_combine(cols, pvs[a], coef[a])))
        want = wm.ext_sub(B[with_ints.index(a)], am.const_of(pl, a, blocks, eb, gamma, kappa)) if pl.ints else am.ZERO
        assert acc == want


# ---- the library's verifier on model proofs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("name", ["lookup", "limb", "bus_mix", "fib+lookup", "mixed"])
def test_accepts_model_proofs(name, pi):
    prm = PARAM_SETS[pi]
    airs, traces, pvs, l = _set(name)
    prefix = [7, pi]
    root, words, _ = _prove(prm, airs, traces, pvs, l, prefix)
    _accept(prm, airs, pvs, l, prefix, root, words)


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, pvs, l = _set("mixed")
    prefix = [11, 12]
    root, words, info = _prove(prm, airs, traces, pvs, l, prefix)
    _accept(prm, airs, pvs, l, prefix, root, words)
    plans = [am.Plan(a) for a in airs]
    g = gm.proof_words(info["L"])
    a0 = 8 + g + 4 * 5              # AIR 0 (limb, m = 1, D = 3, w = 4, no rotation): rounds [a0, a0 + 12), v [a0 + 12, a0 + 28)
    a2 = a0 + plans[0].words() + plans[1].words()   # AIR 2 (Fibonacci, m = 5): rounds 60, v 8, v' 8, reduction 40, u 8
    assert plans[0].words() == 28 and plans[2].words() == 124
    head = 8 + g + 20 + sum(p.words() for p in plans)
    n_cols = sum(p.w for p in plans)
    spots = (3, 8, 8 + 5, 8 + g // 2, 8 + g - 1,            # root, GKR words
             8 + g + 1, 8 + g + 18,                          # a B_a
             a0 + 5, a0 + 14, a2 + 37, a2 + 62, a2 + 71,     # round polynomials, v, v'
             a2 + 76 + 13, a2 + 118,                         # a reduction round, u
             head - 1, head + 2, head + 4 * n_cols + 9, (head + len(words)) // 2, len(words) - 3)   # the opening
    for i in spots:
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, pvs, l, prefix, bad)
    # wrong public values, prefix, log_stack, height, program
    for a, i in ((2, 2), (1, 0)):
        bad_pvs = [list(p) for p in pvs]
        bad_pvs[a][i] = (bad_pvs[a][i] + 1) % P
        _refused(prm, airs, bad_pvs, l, prefix, words)
    _refused(prm, airs, pvs, l, prefix + [1], words)
    _refused(prm, airs, pvs, l, prefix[:1], words)
    for l2 in (l - 1, l + 1):
        _refused(prm, airs, pvs, l2, prefix, words)
    for i, m2 in ((2, 4), (3, 2)):
        a2_ = [dict(a) for a in airs]
        a2_[i]["log_height"] = m2
        _refused(prm, a2_, pvs, l, prefix, words)
    from zkvm_prover_amd import air

    a2_ = [dict(a) for a in airs]
    a2_[0]["program"] = air.limb_air(bus=14).program()   # the same shape, another bus
    _refused(prm, a2_, pvs, l, prefix, words)
    for bad in (words[:-1], list(words) + [0]):
        _refused(prm, airs, pvs, l, prefix, bad)
    for i in (2, 20, 8 + g + 3, a0 + 2, a2 + 64, head + 1, head + 4 * n_cols + 20):
        big = list(words)
        big[i] += P
        _refused(prm, airs, pvs, l, prefix, big)


def test_refuses_an_honest_proof_over_an_unbalanced_table():
    prm = PARAM_SETS[0]
    airs, traces, pvs, l = _set("lookup")
    traces[1][2][1] = (traces[1][2][1] + 1) % P   # one multiplicity
    root, words, _ = _prove(prm, airs, traces, pvs, l, [1])
    assert words[8:12] != am.ZERO                 # P != 0
    _refused(prm, airs, pvs, l, [1], words)


def test_refuses_balanced_buses_with_a_failing_constraint():
    from zkvm_prover_amd import air

    prm = PARAM_SETS[0]
    airs, traces, pvs, l = _set("bus_mix")
    traces[0][5][2] = (traces[0][5][2] + 1) % P   # column 5 is in the messages of bus 11 only, sent and received alike
    bad = air.check_trace(airs[0]["program"], np.array(traces[0], dtype=np.uint32), pvs[0])
    assert bad == []                                # ... and in no constraint: the honest proof still stands
    root, words, _ = _prove(prm, airs, traces, pvs, l, [2])
    _accept(prm, airs, pvs, l, [2], root, words)
    traces[0][2][1] = (traces[0][2][1] + 1) % P   # column 2 = column 0 * column 1 is constraint 0; bus 11 still balances
    assert {k for k, _ in air.check_trace(airs[0]["program"], np.array(traces[0], dtype=np.uint32), pvs[0])} == {0}
    root, words, _ = _prove(prm, airs, traces, pvs, l, [2])
    assert words[8:12] == am.ZERO                 # P = 0: the buses balance
    _refused(prm, airs, pvs, l, [2], words)


def test_refuses_a_bus_proof_over_leaves_that_are_not_the_committed_traces():
    """The test this proof exists for: the GKR part runs on leaves that balance but differ in ONE leaf from those of the committed
    traces (a table row nobody looked up has numerator 0: its denominator is free).  The GKR words alone verify; the set does not."""
    prm = PARAM_SETS[0]
    items = _lookup(2, 3)   # four look-ups into eight rows: some row has multiplicity 0
    airs, traces, pvs, l = [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], 4
    plans = [am.Plan(a) for a in airs]
    blocks, _, L = am.layout(plans)
    row = traces[1][2].index(0)
    at = [off for a, j, m, off in blocks if a == 1][0] + row
    seen = {}

    def hook(num, den):
        assert num[at] == 0
        seen["den"] = list(den[at])
        den[at] = ext_add(den[at], am.ONE)

    prefix = [3]
    root, words, info = _prove(prm, airs, traces, pvs, l, prefix, leaf_hook=hook)
    honest = _prove(prm, airs, traces, pvs, l, prefix)[2]
    assert sum(1 for x, y in zip(zip(info["num"], info["den"]), zip(honest["num"], honest["den"])) if x != y) == 1
    # the GKR words alone: accepted, balanced
    ch = Challenger()
    ch.observe(prefix)
    ch.observe(words[:8])
    gm.bus_challenges(ch)
    _, _, (p0, q0) = gm.verify(ch, words[8:8 + gm.proof_words(L)], L)
    assert p0 == am.ZERO and q0 != am.ZERO
    _refused(prm, airs, pvs, l, prefix, words)
    root, words, _ = _prove(prm, airs, traces, pvs, l, prefix)
    _accept(prm, airs, pvs, l, prefix, root, words)


def test_refused_shapes():
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    lp = _lp(prm)

    def invalid(airs, pvs, l=4):
        assert z.airset_proof_words(lp, airs, l) == 0 == am.proof_words(prm, airs, l)
        with pytest.raises(z.ZkhipError) as e:
            z.airset_verify(lp, [], airs, pvs, l, [0] * 64)
        assert e.value.code == ERR_INVALID

    look = _lookup(2, 2)
    airs, pvs = [x[0] for x in look], [x[2] for x in look]
    assert z.airset_proof_words(lp, airs, 4) > 0
    fib = _fib(3)
    invalid([fib[0]], [fib[2]])                                              # no interaction: zerocheck_prove's case
    assert z.zerocheck_proof_words(lp, [fib[0]], 4) > 0
    invalid(airs + [_air(air.range_table_air(), 3)], pvs + [[]])             # a PREP section
    b = air.AirBuilder(2, 0)
    e = b.var(0)
    for _ in range(7):
        e = e * b.var(0)
    b.push_interaction(4, [e], b.var(1), "send")                              # d_bus = 8, D = 9
    b.push_interaction(4, [e], b.var(1), "receive")
    invalid([_air(b, 3)], [[]])
    b7 = air.AirBuilder(2, 0)
    e = b7.var(0)
    for _ in range(6):
        e = e * b7.var(0)
    b7.max_constraint_degree = 9
    b7.push_interaction(4, [e], b7.var(1), "send")                            # d_bus = 7, D = 8: the cap itself is taken
    b7.push_interaction(4, [e], b7.var(1), "receive")
    assert z.airset_proof_words(lp, [_air(b7, 3)], 4) == am.proof_words(prm, [_air(b7, 3)], 4) > 0
    invalid([airs[0]] * 65, [[]] * 65)                                       # more than ZKHIP_STACK_MAX_POINTS AIRs
    invalid([dict(airs[0], log_height=0), airs[1]], pvs)
    invalid([dict(airs[0], log_height=27), airs[1]], pvs, l=20)
    # L above ZKHIP_GKR_MAX_LOG_N: 27 blocks of 2^24 leaves (L = 29; 2^23: L = 28, taken).  (The per-bus row bound cannot fail below it: every interaction row
    # is a leaf, so p rows on one bus are more than 2^28 leaves.)
    many = air.AirBuilder(1, 0)
    for i in range(9):
        many.push_interaction(20 + i, [many.var(0)], 1, "send")
    assert z.airset_proof_words(lp, [_air(many, 23)] * 3, 20) == am.proof_words(prm, [_air(many, 23)] * 3, 20) > 0
    invalid([_air(many, 24)] * 3, [[]] * 3, l=20)
