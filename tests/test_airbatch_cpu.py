"""CPU: the batched AIR-set proof (docs/airbatch.md) -- the independent model (tests/airbatch_model.py) against brute force over the
M-cube (the batched sum, a used-up AIR's constant in a round, the final claim) and against the library's host verifier
(zkhip_airbatch_verify): model proofs over a grid of AIR sets, parameter sets and both with_bus values are accepted; forged,
mis-shaped and non-canonical proofs are refused, and so are honest proofs over broken traces, a proof batched without the
2^(M - m_a) weights and a proof in the per-AIR format."""
import numpy as np
import pytest

import airbatch_model as bm
import airset_model as am
import gkr_model as gm
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, Challenger, ext_add, ext_mul
from test_airset_cpu import PARAM_SETS, _air, _bus_mix, _fib, _limb, _lookup, _lp, _params, _set
from test_zerocheck_cpu import _synth

ERR_INVALID, ERR_VERIFY = -3, -7


def _items(items, l):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], l


def _inactive(m):
    """an AIR with neither a proven constraint nor an interaction"""
    from zkvm_prover_amd import air

    b = air.AirBuilder(2, 0)
    tr = np.random.default_rng(m).integers(0, P, size=(2, 1 << m), dtype=np.int64)
    return _air(b, m), tr.tolist(), []


def _deg1(m):
    """col0 - col1: D = 2, no rotation"""
    from zkvm_prover_amd import air

    b = air.AirBuilder(2, 0)
    b.assert_zero(b.var(0) - b.var(1))
    col = np.random.default_rng(m + 7).integers(0, P, size=1 << m, dtype=np.int64).tolist()
    return _air(b, m), [col, col], []


def bset(name):
    """(airs, traces, pvs, log_stack) of the sets that are the batched proof's own"""
    sets = {
        # heights 1, 3, 4 in a caller order that is not the height order
        "heights": lambda: _items([_limb(3), _bus_mix(1), _fib(4)] + _lookup(3, 1), 4),
        # Fibonacci (D = 3) beside SyntheticAir at degree 5 (D = 6): two degree classes in one round
        "two_degrees": lambda: _items([_fib(3), _synth(2, 5)] + _lookup(2, 2), 4),
        # interactions only beside constraints only
        "bus_only+cons_only": lambda: _items([_lookup(3, 2)[1], _fib(3), _lookup(3, 2)[0]], 4),
        # an inactive AIR taller than every active one
        "inactive_tall": lambda: _items([_fib(2), _inactive(4)] + _lookup(2, 1), 4),
        # no AIR reduces
        "no_reduction": lambda: _items([_deg1(3), _bus_mix(2), _limb(1)], 4),
    }
    return sets[name]() if name in sets else _set(name)


ALL_SETS = ["lookup", "limb", "bus_mix", "fib+lookup", "mixed", "heights", "two_degrees", "bus_only+cons_only", "inactive_tall", "no_reduction"]


def _prove(prm, airs, traces, pvs, l, prefix, with_bus=True, **kw):
    ch = Challenger()
    ch.observe(prefix)
    return bm.prove(ch, prm, airs, traces, pvs, l, with_bus, **kw)


def _accept(prm, airs, pvs, l, prefix, root, words, with_bus=True):
    import zkvm_prover_amd as z

    assert len(words) == bm.proof_words(prm, airs, l, with_bus) == z.airbatch_proof_words(_lp(prm), airs, l, with_bus)
    ch = Challenger()
    ch.observe(prefix)
    mroot, mpq = bm.verify(ch, prm, airs, pvs, l, words, with_bus)
    out = z.airbatch_verify(_lp(prm), prefix, airs, pvs, l, words, with_bus)
    if with_bus:
        assert mroot == root == out[0].tolist() and out[1].tolist() == mpq[0] + mpq[1] and mpq[0] == bm.ZERO
    else:
        assert mroot == root == out.tolist() and mpq is None


def _refused(prm, airs, pvs, l, prefix, words, with_bus=True, model=True, code=ERR_VERIFY):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.airbatch_verify(_lp(prm), prefix, airs, pvs, l, words, with_bus)
    assert e.value.code == code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject, bm.Refused, IndexError)):
            bm.verify(ch, prm, airs, pvs, l, words, with_bus)


# ---- the identities, by brute force over the cube ---------------------------------------------------------------------------------
def _mle(table, point):
    return gm.mle_eval(table, point)


def _g_at(plan, tabs, pvs, apow, coef, point):
    """g_a at an arbitrary point of its own m variables: the summand on the tables' multilinear extensions"""
    return bm.summand(plan, [_mle(tb, point) for tb in tabs], pvs, apow, coef)


@pytest.mark.parametrize("with_bus", [True, False])
@pytest.mark.parametrize("name", ["heights", "two_degrees"])
def test_identities_by_brute_force(name, with_bus):
    """M <= 4.  (1) sum over the M-cube of sum_j mu^j g_a(x[0..m_a)) = sum_j mu^j 2^(M - m_a) c_a = the prover's first claim;
    (2) every round polynomial the model sent is the brute-force one, and in it a used-up AIR's part is mu^j 2^(M - 1 - i) g_a(r_a);
    (3) the final claim is sum_j mu^j g_a(r_a): step 7's right-hand side."""
    prm = PARAM_SETS[0]
    airs, traces, pvs, l = bset(name)
    root, words, info = _prove(prm, airs, traces, pvs, l, [1], with_bus)
    plans = bm.shape(prm, airs, l, with_bus)[0]
    act, M, D, red, M2 = bm.dims(plans)
    assert 2 <= M <= 4 and len({plans[a].m for a in act}) > 1
    mup = sm._powers(info["mu"], len(act))
    rho = info.get("rho", [])
    coef = [None] * len(airs)
    if with_bus:
        blocks = info["blocks"]
        ch = Challenger()
        ch.observe([1])
        ch.observe(words[:8])
        for pv in pvs:
            ch.observe([int(x) for x in pv])
        gamma, beta = gm.bus_challenges(ch)
        gm.verify(ch, words[8:8 + gm.proof_words(info["L"])], info["L"])
        kappa = ch.sample_ext()
        coef = am.bus_coefs(plans, blocks, am.block_eq(blocks, rho), beta, kappa)
    tabs = {a: bm.tables(plans[a], traces[a], info["tau"], rho) for a in act}
    apow = {a: sm._powers(info["alpha"], max(len(plans[a].proven), 1)) for a in act}

    def g(j, a, point):   # mu^j g_a at the first m_a coordinates of a point of the M-cube
        return ext_mul(mup[j], _g_at(plans[a], tabs[a], pvs[a], apow[a], coef[a], point[:plans[a].m]))

    bits = lambda k, n: [gm.ext_c((k >> t) & 1) for t in range(n)]
    # (1)
    total, want = bm.ZERO, bm.ZERO
    for j, a in enumerate(act):
        for x in range(1 << M):
            total = ext_add(total, g(j, a, bits(x, M)))
        want = ext_add(want, ext_mul(ext_mul(mup[j], bm.pow2(M - plans[a].m)), info["c"].get(a, bm.ZERO)))
    assert total == want == info["claim0"]
    assert with_bus or want == bm.ZERO
    # (2)
    r = info["r"]
    for i in range(M):
        for t in (0, 1, D):
            s = bm.ZERO
            for j, a in enumerate(act):
                part = bm.ZERO
                for x in range(1 << (M - 1 - i)):
                    part = ext_add(part, g(j, a, r[:i] + [gm.ext_c(t)] + bits(x, M - 1 - i)))
                if plans[a].m <= i:   # used up: the stated constant
                    assert part == ext_mul(ext_mul(mup[j], bm.pow2(M - 1 - i)), info["g_end"][a])
                s = ext_add(s, part)
            assert s == info["rounds"][i][t]
        if i:
            assert ext_add(info["rounds"][i][0], info["rounds"][i][1]) == zm.interp(info["rounds"][i - 1], r[i - 1])
    # (3)
    last = bm.ZERO
    for j, a in enumerate(act):
        last = ext_add(last, g(j, a, r))
    assert last == zm.interp(info["rounds"][M - 1], r[M - 1])


# ---- the library's verifier on model proofs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bus", [True, False])
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("name", ALL_SETS)
def test_accepts_model_proofs(name, pi, with_bus):
    prm = PARAM_SETS[pi]
    airs, traces, pvs, l = bset(name)
    prefix = [7, pi]
    root, words, _ = _prove(prm, airs, traces, pvs, l, prefix, with_bus)
    _accept(prm, airs, pvs, l, prefix, root, words, with_bus)


def _layout(prm, airs, l, with_bus, info):
    plans = bm.shape(prm, airs, l, with_bus)[0]
    act, M, D, red, M2 = bm.dims(plans)
    g = gm.proof_words(info["L"]) if with_bus else 0
    o_b = 8 + g
    o_rounds = o_b + (4 * sum(1 for p in plans if bm._ints(p)) if with_bus else 0)
    o_vals = o_rounds + 4 * D * M
    o_red = o_vals + sum(4 * (plans[a].w + len(plans[a].rot)) for a in act)
    o_u = o_red + (8 * M2 if red else 0)
    head = o_u + sum(4 * plans[a].w for a in red)
    return plans, g, o_b, o_rounds, o_vals, o_red, o_u, head


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, pvs, l = bset("mixed")
    prefix = [11, 12]
    root, words, info = _prove(prm, airs, traces, pvs, l, prefix)
    _accept(prm, airs, pvs, l, prefix, root, words)
    plans, g, o_b, o_rounds, o_vals, o_red, o_u, head = _layout(prm, airs, l, True, info)
    assert o_rounds == o_b + 20 and o_vals == o_rounds + 4 * 3 * 5 and o_u == o_red + 40 and head == o_u + 8   # M = M' = 5, D = 3
    n_cols = sum(p.w for p in plans)
    w0 = plans[0].w
    spots = (3, 8, 8 + g // 2, 8 + g - 1,                        # the root, the GKR words
             o_b + 1, o_b + 18,                                  # a B_a
             o_rounds, o_rounds + 29, o_vals - 1,                # the batched rounds
             o_vals + 2, o_vals + 4 * w0 + 4 * plans[1].w + 1,   # v of AIR 0, v of AIR 2 (Fibonacci)
             o_vals + 4 * w0 + 4 * plans[1].w + 9,               # v' of Fibonacci
             o_red + 3, o_u - 2,                                 # a reduction round
             o_u + 5,                                            # u
             head + 2, head + 4 * n_cols + 9, (head + len(words)) // 2, len(words) - 3)   # the opening
    for i in spots:
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, pvs, l, prefix, bad)
    for a, i in ((2, 2), (1, 0)):   # wrong public values, prefix, log_stack, with_bus, height, program
        bad_pvs = [list(p) for p in pvs]
        bad_pvs[a][i] = (bad_pvs[a][i] + 1) % P
        _refused(prm, airs, bad_pvs, l, prefix, words)
    _refused(prm, airs, pvs, l, prefix + [1], words)
    _refused(prm, airs, pvs, l, prefix[:1], words)
    for l2 in (l - 1, l + 1):
        _refused(prm, airs, pvs, l2, prefix, words)
    _refused(prm, airs, pvs, l, prefix, words, with_bus=False)
    for i, m2 in ((2, 4), (3, 2)):
        a2 = [dict(a) for a in airs]
        a2[i]["log_height"] = m2
        _refused(prm, a2, pvs, l, prefix, words)
    from zkvm_prover_amd import air

    a2 = [dict(a) for a in airs]
    a2[0]["program"] = air.limb_air(bus=14).program()
    _refused(prm, a2, pvs, l, prefix, words)
    for bad in (words[:-1], list(words) + [0]):   # truncated, extended, non-canonical
        _refused(prm, airs, pvs, l, prefix, bad)
    for i in (2, 20, o_b + 3, o_rounds + 2, o_vals + 1, o_red + 4, o_u + 1, head + 1, head + 4 * n_cols + 20):
        big = list(words)
        big[i] += P
        _refused(prm, airs, pvs, l, prefix, big)
    # the zero-check form of the same set: a with_bus = 0 proof is refused under with_bus = 1 and the other way round
    root0, words0, _ = _prove(prm, airs, traces, pvs, l, prefix, with_bus=False)
    _accept(prm, airs, pvs, l, prefix, root0, words0, with_bus=False)
    _refused(prm, airs, pvs, l, prefix, words0, with_bus=True)
    bad = list(words0)
    bad[8 + 5] = (bad[8 + 5] + 1) % P
    _refused(prm, airs, pvs, l, prefix, bad, with_bus=False)


@pytest.mark.parametrize("with_bus", [True, False])
def test_refuses_a_changed_cell_in_the_shortest_air(with_bus):
    """'mixed': AIR 0 (limb, m = 1) is the shortest; its term carries 2^(M - 1) = 16.  Column 0 = column 1 + 256 column 2 there."""
    from zkvm_prover_amd import air

    prm = PARAM_SETS[0]
    airs, traces, pvs, l = bset("mixed")
    assert min(a["log_height"] for a in airs) == airs[0]["log_height"] == 1
    traces[0][0][1] = (traces[0][0][1] + 1) % P
    assert air.check_trace(airs[0]["program"], np.array(traces[0], dtype=np.uint32), pvs[0]) != []
    root, words, _ = _prove(prm, airs, traces, pvs, l, [2], with_bus)
    _refused(prm, airs, pvs, l, [2], words, with_bus)


def test_refuses_an_honest_proof_over_an_unbalanced_table():
    prm = PARAM_SETS[0]
    airs, traces, pvs, l = bset("lookup")
    traces[1][2][1] = (traces[1][2][1] + 1) % P
    root, words, _ = _prove(prm, airs, traces, pvs, l, [1])
    assert words[8:12] != bm.ZERO
    _refused(prm, airs, pvs, l, [1], words)


@pytest.mark.parametrize("name", ["heights", "mixed"])
def test_refuses_a_prover_without_the_power_of_two_weights(name):
    prm = PARAM_SETS[0]
    airs, traces, pvs, l = bset(name)
    root, words, _ = _prove(prm, airs, traces, pvs, l, [3], weighted=False)
    assert len(words) == bm.proof_words(prm, airs, l)
    _refused(prm, airs, pvs, l, [3], words)


@pytest.mark.parametrize("name", ["fib+lookup", "mixed"])
def test_refuses_a_proof_in_the_per_air_format(name):
    import zkvm_prover_amd as z

    prm = PARAM_SETS[0]
    airs, traces, pvs, l = bset(name)
    ch = Challenger()
    ch.observe([4])
    root, words, _ = am.prove(ch, prm, airs, traces, pvs, l)
    z.airset_verify(_lp(prm), [4], airs, pvs, l, words)
    assert len(words) != bm.proof_words(prm, airs, l)
    _refused(prm, airs, pvs, l, [4], words)
    n = bm.proof_words(prm, airs, l)
    _refused(prm, airs, pvs, l, [4], (list(words) + [0] * n)[:n])   # ... and cut or padded to the batched length
    root, words, _ = _prove(prm, airs, traces, pvs, l, [4])
    with pytest.raises(z.ZkhipError):
        z.airset_verify(_lp(prm), [4], airs, pvs, l, words)


def test_refused_shapes():
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    lp = _lp(prm)

    def invalid(airs, pvs, l=4, with_bus=(True, False)):
        for wb in with_bus:
            assert z.airbatch_proof_words(lp, airs, l, wb) == 0 == bm.proof_words(prm, airs, l, wb)
            with pytest.raises(z.ZkhipError) as e:
                z.airbatch_verify(lp, [], airs, pvs, l, [0] * 64, wb)
            assert e.value.code == ERR_INVALID

    look = _lookup(2, 2)
    airs, pvs = [x[0] for x in look], [x[2] for x in look]
    assert z.airbatch_proof_words(lp, airs, 4, True) > 0 and z.airbatch_proof_words(lp, airs, 4, False) > 0
    invalid(airs + [_air(air.range_table_air(), 3)], pvs + [[]])   # a PREP program
    b = air.AirBuilder(2, 0)
    e = b.var(0)
    for _ in range(7):
        e = e * b.var(0)
    b.push_interaction(4, [e], b.var(1), "send")                    # d_bus = 8: D = 9 with the bus part
    b.push_interaction(4, [e], b.var(1), "receive")
    invalid([_air(b, 3)], [[]], with_bus=(True,))
    b8 = air.AirBuilder(1, 0)
    e = b8.var(0)
    for _ in range(7):
        e = e * b8.var(0)
    b8.max_constraint_degree = 9
    b8.assert_zero(e)                                                # d_cons = 8: D = 9 in the constraint part
    invalid([_air(b8, 3)] + airs, [[]] + pvs)
    invalid([airs[0]] * 65, [[]] * 65)                              # 65 AIRs
    fib = _fib(3)
    invalid([fib[0]], [fib[2]], with_bus=(True,))                   # no interaction: with_bus = 0's case
    assert z.airbatch_proof_words(lp, [fib[0]], 4, False) > 0
    invalid([dict(airs[0], log_height=0), airs[1]], pvs)
