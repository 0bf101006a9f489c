"""CPU: the AIR zero-check over the stacked WHIR commitment (docs/zerocheck.md) -- the independent model (tests/zerocheck_model.py)
against brute force (the rotation MLE, first / last, the degree rule, the zero sum on a satisfying trace) and against the library's
host verifier (zkhip_zerocheck_verify): model proofs over a grid of AIRs, heights and parameter sets are accepted; forged, mis-shaped
and non-canonical proofs are refused, and so are honest proofs over a trace with one cell changed and proofs whose next-row values
came from a non-cyclic shift."""
import random

import numpy as np
import pytest

import gkr_model as gm
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, Challenger, ext_add, ext_mul

ERR_INVALID, ERR_VERIFY = -3, -7


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


def _lp(p):
    import zkvm_prover_amd as z

    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _rext(rng):
    return [rng.randrange(P) for _ in range(4)]


def _air(builder, m):
    return {"program": builder.program(), "log_height": m, "width": builder.width, "n_pvs": builder.n_pvs}


def _fib(m):
    from zkvm_prover_amd import air

    tr, pvs = air.fibonacci_trace(m, 3, 5)
    return _air(air.fibonacci_air(), m), tr.tolist(), pvs.tolist()


def _synth(m, degree, seed=1):
    from zkvm_prover_amd import air

    s = air.SyntheticAir(width=12, n_free=6, n_bool=2, n_boundary=2, seed=seed, degree=degree)
    tr, pvs = s.gen_trace(m, seed=seed)
    assert air.check_trace(s.program(), tr, pvs) == []
    return _air(s.builder, m), tr.tolist(), pvs.tolist()


def _limb(m):
    from zkvm_prover_amd import air

    return _air(air.limb_air(), m), air.limb_trace(m, seed=2).tolist(), []


def _bus_mix(m):
    from zkvm_prover_amd import air

    tr, pvs = air.bus_mix_trace(m, seed=3)
    return _air(air.bus_mix_air(), m), tr.tolist(), pvs.tolist()


def _table(m):
    from zkvm_prover_amd import air

    _, tab = air.lookup_traces(m + 1, m, seed=4)
    return _air(air.lookup_table_air(), m), tab.tolist(), []


def _mixed():
    """five AIRs of mixed heights: one above log_stack = 4, m = 1 twice, one with interactions, one without proven constraints"""
    return [list(x) for x in zip(_fib(5), _synth(3, 3), _limb(2), _table(1), _bus_mix(1))]


def _prove(prm, airs, traces, pvs, l, prefix, cyclic=True):
    ch = Challenger()
    ch.observe(prefix)
    return zm.prove(ch, prm, airs, traces, pvs, l, cyclic)


def _accept(prm, airs, pvs, l, prefix, root, words):
    import zkvm_prover_amd as z

    assert len(words) == zm.proof_words(prm, airs, l) == z.zerocheck_proof_words(_lp(prm), airs, l)
    ch = Challenger()
    ch.observe(prefix)
    assert zm.verify(ch, prm, airs, pvs, l, words) == root
    assert z.zerocheck_verify(_lp(prm), prefix, airs, pvs, l, words).tolist() == root


def _refused(prm, airs, pvs, l, prefix, words, model=True, code=ERR_VERIFY):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.zerocheck_verify(_lp(prm), prefix, airs, pvs, l, words)
    assert e.value.code == code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, zm.Refused, IndexError)):
            zm.verify(ch, prm, airs, pvs, l, words)


# ---- the model's building blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_rot_is_the_successor_relation(m):
    n = 1 << m
    bits = lambda x: [[(x >> j) & 1, 0, 0, 0] for j in range(m)]
    for a in range(n):
        for b in range(n):
            assert zm.rot_eval(bits(a), bits(b)) == ([1, 0, 0, 0] if b == (a + 1) % n else [0, 0, 0, 0])
    rng = random.Random(m)
    for _ in range(3):
        a, b = [_rext(rng) for _ in range(m)], [_rext(rng) for _ in range(m)]
        ea, eb = gm.eq_table(a), gm.eq_table(b)
        direct = zm.ZERO
        for x in range(n):
            direct = ext_add(direct, ext_mul(ea[x], eb[(x + 1) % n]))
        assert zm.rot_eval(a, b) == direct
        # as a table: rot(r, .)[x] = eq(r, .)[(x - 1) mod n]
        assert gm.mle_eval([ea[(x - 1) % n] for x in range(n)], b) == direct


def test_first_last_and_the_degree_rule():
    rng = random.Random(7)
    for m in (1, 2, 5):
        r = [_rext(rng) for _ in range(m)]
        n = 1 << m
        assert zm.first_eval(r) == gm.mle_eval([1] + [0] * (n - 1), r)
        assert zm.last_eval(r) == gm.mle_eval([0] * (n - 1) + [1], r)
    # along a line through two random values of every table a combination of the proven constraints has degree exactly d
    for (a, _, pvs), d in ((_fib(3), 2), (_synth(3, 3), 3), (_synth(3, 5), 5), (_limb(2), 2), (_bus_mix(2), 2)):
        pl = zm.Plan(a)
        assert pl.d == d and pl.D == d + 1
        nr = len(pl.rot)
        lo, hi = [[_rext(rng) for _ in range(pl.w + nr + 2)] for _ in range(2)]
        apow = sm._powers(_rext(rng), len(pl.proven))

        def g(t):
            v = [zm._at(x, y, t) for x, y in zip(lo, hi)]
            return pl.combine(v[:pl.w], v[pl.w:pl.w + nr], v[-2], v[-1], pvs, apow)

        ys = [g(t) for t in range(d + 3)]
        assert zm.interp(ys[:d + 1], gm.ext_c(d + 1)) == ys[d + 1] and zm.interp(ys[:d + 1], gm.ext_c(d + 2)) == ys[d + 2]
        assert zm.interp(ys[:d], gm.ext_c(d)) != ys[d]
    assert zm.Plan(_table(2)[0]).proven == [] and zm.Plan(_table(2)[0]).words() == 0
    assert zm.Plan(_fib(3)[0]).rot == [0, 1] and zm.Plan(_limb(2)[0]).rot == []


def test_the_sum_is_zero_on_a_satisfying_trace_and_not_after_one_cell_changed():
    rng = random.Random(8)
    for a, tr, pvs in (_fib(3), _synth(3, 3), _bus_mix(2)):
        pl = zm.Plan(a)
        n = 1 << pl.m
        tau, apow = [_rext(rng) for _ in range(pl.m)], sm._powers(_rext(rng), len(pl.proven))
        e = gm.eq_table(tau)

        def total(tr):
            acc = zm.ZERO
            for x in range(n):
                cols = [gm.ext_c(c[x]) for c in tr]
                nexts = [gm.ext_c(tr[j][(x + 1) % n]) for j in pl.rot]
                c = pl.combine(cols, nexts, gm.ext_c(int(x == 0)), gm.ext_c(int(x == n - 1)), pvs, apow)
                acc = ext_add(acc, ext_mul(e[x], c))
            return acc

        assert total(tr) == zm.ZERO
        bad = [list(c) for c in tr]
        bad[2 % pl.w][3] = (bad[2 % pl.w][3] + 1) % P
        assert total(bad) != zm.ZERO


# ---- the library's verifier on model proofs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 9))
def test_accepts_fibonacci(m):
    prm = _params(1, 1, 0)
    a, tr, pvs = _fib(m)
    l = min(m + 1, 5)   # from m = 5 on the columns are split over stacked columns
    prefix = [m, 9]
    root, words = _prove(prm, [a], [tr], [pvs], l, prefix)
    _accept(prm, [a], [pvs], l, prefix, root, words)


@pytest.mark.parametrize("case", ["synth3", "synth5", "limb", "bus_mix", "table"])
def test_accepts_single_airs(case):
    prm = _params(1, 2, 1)
    a, tr, pvs = {"synth3": lambda: _synth(3, 3), "synth5": lambda: _synth(3, 5), "limb": lambda: _limb(3), "bus_mix": lambda: _bus_mix(2),
                  "table": lambda: _table(2)}[case]()
    root, words = _prove(prm, [a], [tr], [pvs], 4, [1, 2, 3])
    _accept(prm, [a], [pvs], 4, [1, 2, 3], root, words)


@pytest.mark.parametrize("b,k,fl", [(1, 1, 0), (2, 2, 1)])
def test_accepts_a_mixed_set_in_two_parameter_sets(b, k, fl):
    prm = _params(b, k, fl, pow_bits=1 + b, nq=2 + k)
    airs, traces, pvs = _mixed()
    root, words = _prove(prm, airs, traces, pvs, 4, [])
    _accept(prm, airs, pvs, 4, [], root, words)


def _fib_variant():
    from zkvm_prover_amd import air

    b = air.AirBuilder(2, 3)
    a0, b0 = b.var(0), b.var(1)
    b.when_first_row(a0 - b.pub(0))
    b.when_first_row(b0 - b.pub(1))
    b.when_transition(b.next(0) - b0)
    b.when_transition(b.next(1) - (a0 + b0 + b0))   # the one changed constraint
    b.when_last_row(b0 - b.pub(2))
    return b


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, pvs = _mixed()
    l, prefix = 4, [11, 12]
    root, words = _prove(prm, airs, traces, pvs, l, prefix)
    _accept(prm, airs, pvs, l, prefix, root, words)
    plans = [zm.Plan(a) for a in airs]
    head = 8 + sum(p.words() for p in plans)
    # AIR 0 (Fibonacci, m = 5, D = 3, w = n_rot = 2): rounds [8, 68), v [68, 76), v' [76, 84), reduction [84, 124), u [124, 132); then AIR 1
    assert plans[0].words() == 124
    n_cols = sum(p.w for p in plans)
    for i in (3, 8, 8 + 37, 70, 79, 84 + 13, 126, 132 + 5, head - 1, head + 2, head + 4 * n_cols + 9, (head + len(words)) // 2, len(words) - 3):
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, pvs, l, prefix, bad)
    # wrong public values, prefix, log_stack, height, program
    bad_pvs = [list(p) for p in pvs]
    bad_pvs[0][2] = (bad_pvs[0][2] + 1) % P
    _refused(prm, airs, bad_pvs, l, prefix, words)
    bad_pvs = [list(p) for p in pvs]
    bad_pvs[4][0] = (bad_pvs[4][0] + 1) % P   # read by no proven constraint, but bound by the transcript
    _refused(prm, airs, bad_pvs, l, prefix, words)
    _refused(prm, airs, pvs, l, prefix + [1], words)
    _refused(prm, airs, pvs, l, prefix[:1], words)
    for l2 in (l - 1, l + 1):
        _refused(prm, airs, pvs, l2, prefix, words)
    for i, m2 in ((0, 4), (2, 3)):
        a2 = [dict(a) for a in airs]
        a2[i]["log_height"] = m2
        _refused(prm, a2, pvs, l, prefix, words)
    a2 = [dict(a) for a in airs]
    a2[0]["program"] = _fib_variant().program()
    _refused(prm, a2, pvs, l, prefix, words)
    # truncated, extended, non-canonical
    for bad in (words[:-1], list(words) + [0]):
        _refused(prm, airs, pvs, l, prefix, bad)
    for i in (2, 20, 72, 128, head + 1, head + 4 * n_cols + 20):
        big = list(words)
        big[i] += P
        _refused(prm, airs, pvs, l, prefix, big)


@pytest.mark.parametrize("col,row", [(1, 5), (0, 15), (1, 0)])
def test_refuses_an_honest_proof_over_a_trace_with_one_cell_changed(col, row):
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    a, tr, pvs = _fib(4)
    tr[col][row] = (tr[col][row] + 1) % P
    assert len(air.check_trace(a["program"], np.array(tr, dtype=np.uint32), pvs)) >= 1
    root, words = _prove(prm, [a], [tr], [pvs], 4, [5])
    _refused(prm, [a], [pvs], 4, [5], words)


def test_one_failing_constraint_on_one_row_is_enough():
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    a, tr, pvs = _synth(3, 3)
    j = zm.Plan(a).w - 1   # the last derived column: read by its own definition only, unless it is a boundary column
    tr[j][4] = (tr[j][4] + 1) % P
    bad = air.check_trace(a["program"], np.array(tr, dtype=np.uint32), pvs)
    assert len(bad) == 1 or len({k for k, _ in bad}) == len(bad)
    root, words = _prove(prm, [a], [tr], [pvs], 4, [])
    _refused(prm, [a], [pvs], 4, [], words)


def test_refuses_next_row_values_from_a_non_cyclic_shift():
    prm = _params(1, 2, 1)
    a, tr, pvs = _fib(3)
    root, words = _prove(prm, [a], [tr], [pvs], 4, [6], cyclic=False)
    good = _prove(prm, [a], [tr], [pvs], 4, [6])[1]
    assert words[:8] == good[:8] and words[8:8 + 36 + 16] != good[8:8 + 36 + 16]   # the same commitment, another zero-check
    _refused(prm, [a], [pvs], 4, [6], words)


def test_refused_shapes():
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    lp = _lp(prm)

    def invalid(airs, pvs, l=4):
        assert z.zerocheck_proof_words(lp, airs, l) == 0 == zm.proof_words(prm, airs, l)
        with pytest.raises(z.ZkhipError) as e:
            z.zerocheck_verify(lp, [], airs, pvs, l, [0] * 64)
        assert e.value.code == ERR_INVALID

    a, _, pvs = _fib(3)
    assert z.zerocheck_proof_words(lp, [a], 4) > 0
    invalid([_air(air.range_table_air(), 3)], [[]])                         # a PREP section
    b = air.AirBuilder(1, 0)
    x = b.var(0)
    e = x
    for _ in range(7):
        e = e * x
    b.assert_zero(e - x)                                                     # d = 8, D = 9
    invalid([_air(b, 3)], [[]])
    b7 = air.AirBuilder(1, 0)
    e = b7.var(0)
    for _ in range(6):
        e = e * b7.var(0)
    b7.assert_zero(e - b7.var(0))                                            # d = 7, D = 8: the cap itself is taken
    assert z.zerocheck_proof_words(lp, [_air(b7, 3)], 4) == zm.proof_words(prm, [_air(b7, 3)], 4) > 0
    one = _fib(1)
    invalid([one[0]] * 65, [one[2]] * 65)                                    # more than ZKHIP_STACK_MAX_POINTS AIRs
    assert z.zerocheck_proof_words(lp, [one[0]] * 64, 4) > 0
    invalid([dict(a, log_height=0)], [pvs])
    invalid([dict(a, log_height=27)], [pvs], l=20)
    invalid([_fib(8)[0]] * 5, [pvs] * 5, l=4)                                # 10 columns of 2^8 at l = 4: n_stack = 160
