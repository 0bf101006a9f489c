"""CPU: the keyed zero-check and AIR-set proof (docs/airset.md, docs/zerocheck.md: AIR sets with preprocessed columns under a
stacked commitment made at key generation) -- the library's host verifier (zkhip_airkey_verify) against the independent model
(tests/keyed_model.py): model proofs over a grid of AIR sets and two parameter sets are accepted with the word count of
zkhip_airkey_proof_words; forged, mis-shaped and non-canonical proofs are refused, and so are an honest proof made under a key whose
table has one cell changed (checked under the right root) and an honest proof over a changed multiplicity; refused shapes."""
import numpy as np
import pytest

import gkr_model as gm
import keyed_model as km
import whir_model as wm
from pymodel import P, Challenger

ERR_INVALID, ERR_VERIFY = -3, -7


def _params(b, k, fl, pow_bits=2, nq=3):
    return wm.Params(b, k, fl, [pow_bits] * wm.MAX_ROUNDS, [nq] * wm.MAX_ROUNDS)


PARAM_SETS = [_params(1, 1, 0), _params(2, 2, 1, pow_bits=3, nq=4)]


def _lp(p):
    import zkvm_prover_amd as z

    return z.WhirParams.make(p.b, p.k, p.final_log, p.pow_bits, p.num_queries)


def _air(builder, m):
    return {"program": builder.program(), "log_height": m, "width": builder.width, "n_pvs": builder.n_pvs}


def _item(builder, m, trace, prep=None, pvs=()):
    """(air, trace, prep, pvs) as lists"""
    return _air(builder, m), np.asarray(trace).tolist(), None if prep is None else np.asarray(prep).tolist(), list(pvs)


def _range_pair(mt, mu=4, seed=0, prep=None):
    """range_table_air (constraints on the preprocessed column with rotation, an interaction whose field is a PREP cell) + its user"""
    from zkvm_prover_amd import air

    user, mult, pr = air.range_traces(mu, mt, seed=seed)
    return [_item(air.range_table_air(), mt, mult, pr if prep is None else prep), _item(air.range_user_air(), mu, user)]


def _var_range_pair(max_bits=3, mu=3, seed=1):
    """w_p = 2, no proven constraint on the table, no rotation: u_p = v_p"""
    from zkvm_prover_amd import air

    rng = np.random.default_rng(seed)
    n = 1 << mu
    bits = rng.integers(0, max_bits + 1, size=n)
    value = rng.integers(0, 1 << 30, size=n) % (1 << bits)
    user = np.stack([value, bits, value * bits % P]).astype(np.uint32)
    prep = air.var_range_prep(max_bits)
    mult = np.bincount((1 << bits) - 1 + value, minlength=prep.shape[1]).astype(np.uint32).reshape(1, -1)
    return [_item(air.var_range_table_air(), max_bits + 1, mult, prep), _item(air.var_range_user_air(), mu, user)]


def _bitwise_pair(bits=2, mu=3, seed=2):
    """w_p = 3, two interactions on the table"""
    from zkvm_prover_amd import air

    rng = np.random.default_rng(seed)
    n = 1 << mu
    x, y, op = rng.integers(0, 1 << bits, size=n), rng.integers(0, 1 << bits, size=n), rng.integers(0, 2, size=n)
    user = np.stack([x, y, (x ^ y) * op, op]).astype(np.uint32)
    row = (x << bits) + y
    mult = np.stack([np.bincount(row[op == 0], minlength=1 << (2 * bits)), np.bincount(row[op == 1], minlength=1 << (2 * bits))]).astype(np.uint32)
    return [_item(air.bitwise_lookup_air(bits), 2 * bits, mult, air.bitwise_lookup_prep(bits)), _item(air.bitwise_user_air(), mu, user)]


def _fib(m):
    from zkvm_prover_amd import air

    tr, pvs = air.fibonacci_trace(m, 3, 5)
    return _item(air.fibonacci_air(), m, tr, None, pvs.tolist())


def _hand(m=3, seed=3):
    """w = 3, n_rot = 2 (columns 0 and 1), w_p = 3, n_rot_p = 1: the rotated preprocessed column is column 1, not 0
         p1' = p1 + 1, c0' = c0 + p0, c1' = c1 + p2 c0 on transitions; c2 = c0 p1 on every row"""
    from zkvm_prover_amd import air

    b = air.AirBuilder(3, 0, prep_width=3)
    b.when_transition(b.prep(1, 1) - b.prep(1) - 1)
    b.when_transition(b.next(0) - b.var(0) - b.prep(0))
    b.when_transition(b.next(1) - b.var(1) - b.prep(2) * b.var(0))
    b.assert_zero(b.var(2) - b.var(0) * b.prep(1))
    rng = np.random.default_rng(seed)
    n = 1 << m
    prep = np.stack([rng.integers(0, P, size=n), (np.arange(n) + 5) % P, rng.integers(0, P, size=n)]).astype(np.int64)
    c0, c1 = [int(rng.integers(0, P))], [int(rng.integers(0, P))]
    for i in range(n - 1):
        c0.append((c0[i] + int(prep[0][i])) % P)
        c1.append((c1[i] + int(prep[2][i]) * c0[i]) % P)
    tr = np.stack([np.array(c0), np.array(c1), np.array(c0) * prep[1] % P])
    assert air.check_trace(b.program(), tr.astype(np.uint32), [], prep=prep.astype(np.uint32)) == []
    return _item(b, m, tr, prep)


def _five():
    """Fibonacci between two AIRs with PREP, AIR order not the height order; Fibonacci (m = 5) is above log_stack = 4 and the variable
    range table (m = 4) above log_stack_prep = 3"""
    rt, ru = _range_pair(3)
    vt, vu = _var_range_pair(3, mu=2)
    return [rt, _fib(5), vt, ru, vu]


def _set(name):
    """(airs, traces, preps, pvs, log_stack, log_stack_prep, with_bus)"""
    sets = {
        "range3": lambda: (_range_pair(3), 4, 3, True),
        "range1": lambda: (_range_pair(1), 4, 2, True),
        "table_alone": lambda: ([_range_pair(3)[0]], 3, 3, False),
        "var_range": lambda: (_var_range_pair(), 4, 4, True),
        "bitwise": lambda: (_bitwise_pair(), 4, 4, True),
        "five": lambda: (_five(), 4, 3, True),
        "hand": lambda: ([_hand()], 4, 3, False),
    }
    items, l, lpr, wb = sets[name]()
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items], l, lpr, wb


NAMES = ["range3", "range1", "table_alone", "var_range", "bitwise", "five", "hand"]


def _prove(prm, airs, traces, preps, pvs, l, lpr, wb, prefix, key=None):
    key = key or km.Key(prm, airs, preps, lpr)
    ch = Challenger()
    ch.observe(prefix)
    root, words, info = km.prove(ch, prm, airs, traces, preps, pvs, l, key, wb)
    return key, root, words, info


def _accept(prm, airs, prep_root, lpr, pvs, l, wb, prefix, root, words):
    import zkvm_prover_amd as z

    assert len(words) == km.proof_words(prm, airs, l, lpr, wb) == z.airkey_proof_words(_lp(prm), airs, l, lpr, wb)
    ch = Challenger()
    ch.observe(prefix)
    m = km.verify(ch, prm, airs, prep_root, lpr, pvs, l, words, wb)
    got = z.airkey_verify(_lp(prm), prefix, airs, prep_root, lpr, pvs, l, words, wb)
    if wb:
        assert m[0] == root == got[0].tolist() and got[1].tolist() == m[1][0] + m[1][1] and m[1][0] == km.ZERO
    else:
        assert m == root == got.tolist()


def _refused(prm, airs, prep_root, lpr, pvs, l, wb, prefix, words, model=True, code=ERR_VERIFY):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.airkey_verify(_lp(prm), prefix, airs, prep_root, lpr, pvs, l, words, wb)
    assert e.value.code == code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject, km.Refused, IndexError)):
            km.verify(ch, prm, airs, prep_root, lpr, pvs, l, words, wb)


def test_plans_of_the_shapes():
    plans = {n: [km.Plan(a, _set(n)[6]) for a in _set(n)[0]] for n in ("range3", "var_range", "bitwise", "hand")}
    t = plans["range3"][0]
    assert (t.w, len(t.rot), t.wp, t.rot_p, t.D, len(t.proven)) == (1, 0, 1, [0], 3, 2) and t.words() == 36 + 12 + 24 + 8
    v = plans["var_range"][0]
    assert (v.wp, v.rot_p, v.proven, v.D) == (2, [], [], 2) and v.words() == 4 * 2 * 4 + 12      # no reduction: nothing further is sent
    assert (plans["bitwise"][0].wp, len(plans["bitwise"][0].ints)) == (3, 2)
    h = plans["hand"][0]
    assert (h.w, h.rot, h.wp, h.rot_p, h.D) == (3, [0, 1], 3, [1], 4)


@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_accepts_model_proofs(name, pi):
    prm = PARAM_SETS[pi]
    airs, traces, preps, pvs, l, lpr, wb = _set(name)
    prefix = [9, pi]
    key, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, prefix)
    _accept(prm, airs, key.root, lpr, pvs, l, wb, prefix, root, words)


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")
    prefix = [11, 12]
    key, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, prefix)
    _accept(prm, airs, key.root, lpr, pvs, l, wb, prefix, root, words)
    a0 = info["airs"][0]["at"]   # the table (m = 3, D = 3): rounds 36 | v 4 | v_p 4 | v_p' 4 | reduction 24 | u 4 | u_p 4
    o2 = info["open2_at"]
    spots = (a0 + 5, a0 + 30,                       # round polynomials
             a0 + 37, a0 + 41, a0 + 46,             # v, v_p, v_p'
             a0 + 48 + 9, a0 + 73, a0 + 77,         # a reduction round, u, u_p
             info["open_at"] + 1, o2 - 2,           # the main opening
             o2, o2 + 3, o2 + 4 + 5, (o2 + len(words)) // 2, len(words) - 2)   # the key's opening: value, sum-check, WHIR part
    for i in spots:
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, bad)
    wrong = list(key.root)
    wrong[3] = (wrong[3] + 1) % P
    _refused(prm, airs, wrong, lpr, pvs, l, wb, prefix, words)
    _refused(prm, airs, key.root, lpr + 1, pvs, l, wb, prefix, words)
    _refused(prm, airs, key.root, lpr - 1, pvs, l, wb, prefix, words)
    _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix + [1], words)
    _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix[:1], words)
    for bad in (words[:-1], list(words) + [0]):
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, bad)
    for i in (2, a0 + 2, a0 + 42, a0 + 78, o2 + 1, o2 + 4 + 3):
        big = list(words)
        big[i] += P
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, big)
    big = list(key.root)
    big[0] += P
    _refused(prm, airs, big, lpr, pvs, l, wb, prefix, words, model=False, code=ERR_INVALID)


def test_refuses_a_flip_in_u_p_eq_v_p_without_reduction():
    """var_range: no rotation, the key's opening must show v_p itself"""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, wb = _set("var_range")
    key, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, [4])
    a0 = info["airs"][0]["at"]
    for i in (a0 + 32 + 5, a0 + 32 + 9, info["open2_at"] + 6):   # v_p (two columns), the opened value
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key.root, lpr, pvs, l, wb, [4], bad)


def test_refuses_an_honest_proof_under_a_key_with_one_table_cell_changed():
    """The attack the key exists to stop: the prover's table has key 6 twice and no key 7 (so a user value of 6 ... passes for any
    count), its own constraints aside; every step of its proof is honest for ITS table.  Under the verifier's root it is refused."""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")
    good = km.Key(prm, airs, preps, lpr)
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][7] = 6
    key, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, wb, [5])
    assert key.root != good.root
    _refused(prm, airs, good.root, lpr, pvs, l, wb, [5], words)
    # the same prover, now lying about the key it used: the transcript is the verifier's, the key's opening is of another table
    _, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, wb, [5], key=good)
    _refused(prm, airs, good.root, lpr, pvs, l, wb, [5], words)
    # a table cell nothing constrains (var_range has no proven constraint) and nobody looks up: only the key catches it
    airs, traces, preps, pvs, l, lpr, wb = _set("var_range")
    good = km.Key(prm, airs, preps, lpr)
    row = traces[0][0].index(0)
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][row] = (bad_preps[0][0][row] + 1) % P
    _, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, wb, [6], key=good)
    _refused(prm, airs, good.root, lpr, pvs, l, wb, [6], words)
    _, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, [6], key=good)
    _accept(prm, airs, good.root, lpr, pvs, l, wb, [6], root, words)


def test_refuses_an_honest_proof_over_a_changed_multiplicity():
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, wb = _set("range3")
    traces[0][0][2] = (traces[0][0][2] + 1) % P
    key, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, [1])
    assert words[8:12] != km.ZERO   # P != 0
    _refused(prm, airs, key.root, lpr, pvs, l, wb, [1], words)


def test_refused_shapes():
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    lp = _lp(prm)

    def invalid(airs, pvs, l=4, lpr=3, wb=True):
        assert z.airkey_proof_words(lp, airs, l, lpr, wb) == 0 == km.proof_words(prm, airs, l, lpr, wb)
        with pytest.raises(z.ZkhipError) as e:
            z.airkey_verify(lp, [], airs, [0] * 8, lpr, pvs, l, [0] * 64, wb)
        assert e.value.code == ERR_INVALID

    airs, _, _, pvs, l, lpr, _ = _set("range3")
    assert z.airkey_proof_words(lp, airs, l, lpr, True) > 0 and z.airkey_proof_words(lp, airs, l, lpr, False) > 0
    invalid([airs[1]], [[]])                                  # no PREP anywhere: the unkeyed calls' case
    invalid([airs[1]], [[]], wb=False)
    assert z.airset_proof_words(lp, airs, l) == 0             # ... which still refuse PREP
    invalid(airs, pvs, lpr=1)                                 # log_stack_prep below fold_log = 2
    invalid(airs, pvs, lpr=27)
    wide = air.AirBuilder(1, 0, prep_width=65)                # 65 columns of 2^3 rows at log_stack_prep = 3: n_stack = 65 > 64
    wide.push_interaction(5, [wide.prep(64)], wide.var(0), "receive")
    invalid([_air(wide, 3), airs[1]], pvs)
    assert z.airkey_proof_words(lp, [_air(wide, 3), airs[1]], 4, 4, True) > 0
    b = air.AirBuilder(1, 0, prep_width=1)                    # D = 9
    e = b.prep(0)
    for _ in range(7):
        e = e * b.prep(0)
    b.assert_zero(e - b.var(0))
    b.push_interaction(5, [b.prep(0)], b.var(0), "receive")
    invalid([_air(b, 3), airs[1]], pvs)
    invalid([airs[0]], [[]], wb=False, l=1)                   # the main stack's shape
    invalid([dict(airs[0], log_height=0), airs[1]], pvs)
