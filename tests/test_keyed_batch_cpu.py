"""CPU: the keyed batched AIR-set proof (docs/airbatch.md, "The keyed batched form") -- the independent model
(tests/keyed_batch_model.py) against brute force over the M-cube (the batched sum with PREP leaves, every round polynomial with the
used-up AIRs' constants, the final claim) and against the library's host verifier (zkhip_airkey_batch_verify): model proofs over a grid
of AIR sets, two parameter sets and both with_bus values are accepted with the word count of zkhip_airkey_batch_proof_words; forged,
mis-shaped and non-canonical proofs are refused, and so are an honest proof made under a key whose table has one cell changed (checked
under the right root), one over a changed multiplicity, one batched without the 2^(M - m_a) weights, and proofs in the formats of
airkey_prove and airbatch_prove; refused shapes."""
import pytest

import airbatch_model as bm
import gkr_model as gm
import keyed_batch_model as kb
import keyed_model as km
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, Challenger, ext_add, ext_mul
from test_keyed_cpu import NAMES, PARAM_SETS, _air, _lp, _params, _range_pair, _set, _var_range_pair

ERR_INVALID, ERR_VERIFY = -3, -7


def _split(items, l, lpr):
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items], l, lpr


def kset(name):
    """(airs, traces, preps, pvs, log_stack, log_stack_prep, the with_bus values under which the statement holds)"""
    sets = {
        # a PREP AIR (the range table, m = 2) shorter than a non-PREP AIR (its user, m = 3) and one taller (the variable range table,
        # m = 4), in a caller order that is not the height order
        "prep_heights": lambda: _split([_range_pair(2, mu=3)[1], _var_range_pair(3, mu=2)[0], _range_pair(2, mu=3)[0], _var_range_pair(3, mu=2)[1]], 4, 3),
        # two PREP AIRs of one (D, bus, PREP) class at different heights
        "one_class": lambda: _split(_range_pair(2, mu=3, seed=1) + _range_pair(3, mu=3, seed=2), 4, 3),
    }
    if name in sets:
        return sets[name]() + ((True, False),)
    airs, traces, preps, pvs, l, lpr, wb = _set(name)
    return airs, traces, preps, pvs, l, lpr, (True, False) if wb else (False,)


OWN = ["prep_heights", "one_class"]
ZC_ONLY = ("table_alone", "hand")   # test_keyed_cpu's sets without a balanced bus: with_bus = 0 alone
CASES = [(n, wb) for n in NAMES + OWN for wb in ((False,) if n in ZC_ONLY else (True, False))]


def _prove(prm, airs, traces, preps, pvs, l, lpr, wb, prefix, key=None, **kw):
    key = key or km.Key(prm, airs, preps, lpr)
    ch = Challenger()
    ch.observe(prefix)
    root, words, info = kb.prove(ch, prm, airs, traces, preps, pvs, l, key, wb, **kw)
    return key, root, words, info


def _accept(prm, airs, prep_root, lpr, pvs, l, wb, prefix, root, words):
    import zkvm_prover_amd as z

    assert len(words) == kb.proof_words(prm, airs, l, lpr, wb) == z.airkey_batch_proof_words(_lp(prm), airs, l, lpr, wb)
    ch = Challenger()
    ch.observe(prefix)
    m = kb.verify(ch, prm, airs, prep_root, lpr, pvs, l, words, wb)
    got = z.airkey_batch_verify(_lp(prm), prefix, airs, prep_root, lpr, pvs, l, words, wb)
    if wb:
        assert m[0] == root == got[0].tolist() and got[1].tolist() == m[1][0] + m[1][1] and m[1][0] == kb.ZERO
    else:
        assert m == root == got.tolist()


def _refused(prm, airs, prep_root, lpr, pvs, l, wb, prefix, words, model=True, code=(ERR_VERIFY,)):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.airkey_batch_verify(_lp(prm), prefix, airs, prep_root, lpr, pvs, l, words, wb)
    assert e.value.code in code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject, kb.Refused, IndexError)):
            kb.verify(ch, prm, airs, prep_root, lpr, pvs, l, words, wb)


# ---- the identities, by brute force over the cube ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_bus", [("range3", True), ("range3", False), ("prep_heights", True), ("prep_heights", False)])
def test_identities_by_brute_force(name, with_bus):
    """M <= 4, PREP leaves in the constraints (range table) and in the interactions (both tables).  (1) the sum over the M-cube of
    sum_j mu^j g_a(x[0..m_a)) = sum_j mu^j 2^(M - m_a) c_a = the prover's first claim; (2) every round polynomial the model sent is the
    brute-force one, and in it a used-up AIR's part is mu^j 2^(M - 1 - i) g_a(r_a); (3) the final claim is sum_j mu^j g_a(r_a)."""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset(name)
    key, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, with_bus, [1])
    plans = info["plans"]
    act, M, D, red, M2 = kb.dims(plans)
    assert 2 <= M <= 4 and len({plans[a].m for a in act}) > 1 and any(plans[a].wp for a in act)
    mup = sm._powers(info["mu"], len(act))
    rho = info.get("rho", [])
    coef = info.get("coef", [None] * len(airs))
    tabs = {a: kb.tables(plans[a], traces[a], preps[a], info["tau"], rho) for a in act}
    apow = {a: sm._powers(info["alpha"], max(len(plans[a].proven), 1)) for a in act}

    def g(j, a, point):   # mu^j g_a at the first m_a coordinates of a point of the M-cube: the summand on the tables' extensions
        pt = point[:plans[a].m]
        return ext_mul(mup[j], kb.summand(plans[a], [gm.mle_eval(tb, pt) for tb in tabs[a]], pvs[a], apow[a], coef[a]))

    bits = lambda k, n: [gm.ext_c((k >> t) & 1) for t in range(n)]
    # (1)
    total, want = kb.ZERO, kb.ZERO
    for j, a in enumerate(act):
        for x in range(1 << M):
            total = ext_add(total, g(j, a, bits(x, M)))
        want = ext_add(want, ext_mul(ext_mul(mup[j], kb.pow2(M - plans[a].m)), info["c"].get(a, kb.ZERO)))
    assert total == want == info["claim0"]
    assert with_bus or want == kb.ZERO
    # (2)
    r = info["r"]
    for i in range(M):
        for t in (0, 1, D):
            s = kb.ZERO
            for j, a in enumerate(act):
                part = kb.ZERO
                for x in range(1 << (M - 1 - i)):
                    part = ext_add(part, g(j, a, r[:i] + [gm.ext_c(t)] + bits(x, M - 1 - i)))
                if plans[a].m <= i:   # used up: the stated constant
                    assert part == ext_mul(ext_mul(mup[j], kb.pow2(M - 1 - i)), info["g_end"][a])
                s = ext_add(s, part)
            assert s == info["rounds"][i][t]
        if i:
            assert ext_add(info["rounds"][i][0], info["rounds"][i][1]) == zm.interp(info["rounds"][i - 1], r[i - 1])
    # (3)
    last = kb.ZERO
    for j, a in enumerate(act):
        last = ext_add(last, g(j, a, r))
    assert last == zm.interp(info["rounds"][M - 1], r[M - 1])


# ---- the library's verifier on model proofs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("name,with_bus", CASES)
def test_accepts_model_proofs(name, with_bus, pi):
    prm = PARAM_SETS[pi]
    airs, traces, preps, pvs, l, lpr, _ = kset(name)
    prefix = [9, pi]
    key, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, with_bus, prefix)
    _accept(prm, airs, key.root, lpr, pvs, l, with_bus, prefix, root, words)


def test_the_shapes_are_the_ones_named():
    """what each set is there for, read off the plans"""
    prm = PARAM_SETS[0]

    def d(name, wb):
        airs, _, _, _, l, lpr, _ = kset(name)
        plans = km.Shape(prm, airs, l, lpr, wb).plans
        return (plans,) + kb.dims(plans)

    plans, act, M, D, red, M2 = d("prep_heights", True)
    assert [p.m for p in plans] == [3, 4, 2, 2] and [bool(p.wp) for p in plans] == [False, True, True, False] and act == [0, 1, 2, 3]
    plans, act, M, D, red, M2 = d("one_class", True)
    assert [(p.m, p.D, bool(p.ints), bool(p.wp)) for p in plans][::2] == [(2, 3, True, True), (3, 3, True, True)]
    plans, act, M, D, red, M2 = d("five", False)   # an inactive AIR with preprocessed columns: in the key's opening only
    assert not plans[2].active and plans[2].wp == 2 and act == [0, 1, 3, 4]
    for name, wb in (("range3", True), ("table_alone", False)):   # the only reducing AIR reduces through rot_p alone
        plans, act, M, D, red, M2 = d(name, wb)
        assert red == [0] and plans[0].rot == [] and plans[0].rot_p == [0] and M2 == plans[0].m
    for name in ("var_range", "bitwise"):   # nothing reduces: u_p = v_p, no reduction words
        plans, act, M, D, red, M2 = d(name, True)
        assert red == [] and any(plans[a].wp for a in act)
        airs, _, _, _, l, lpr, _ = kset(name)
        S = km.Shape(prm, airs, l, lpr, True)
        lay = kb.layout(S, True)
        assert lay["head"] == lay["o_red"] == lay["o_u"]


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, preps, pvs, l, lpr, _ = kset("five")
    wb, prefix = True, [11, 12]
    key, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, wb, prefix)
    _accept(prm, airs, key.root, lpr, pvs, l, wb, prefix, root, words)
    plans = info["plans"]
    g = gm.proof_words(km.Shape(prm, airs, l, lpr, wb).L)
    o_b, o_rounds, o_vals, o_red, o_u, head = (info[k] for k in ("o_b", "o_rounds", "o_vals", "o_red", "o_u", "head"))
    va, ua, o1, o2 = info["val_at"], info["u_at"], info["open_at"], info["open2_at"]
    # the table (w 1, w_p 1, rot_p [0]), Fibonacci (w 2, rot [0, 1]), the variable range table (w 1, w_p 2, no rotation), two users
    assert o_b == 8 + g and o_rounds == o_b + 16 and o_vals == o_rounds + 4 * 3 * 5 and o_u == o_red + 40 and head == o_u + 8 + 8 == o1
    assert (va[0], va[1], va[2]) == (o_vals, o_vals + 12, o_vals + 28) and (ua[0], ua[1]) == (o_u, o_u + 8)
    spots = (3, 8, 8 + g // 2, o_b - 1,                           # the root, the GKR words
             o_b + 1, o_b + 14,                                   # a B_a
             o_rounds, o_rounds + 29, o_vals - 1,                 # the batched rounds
             va[0] + 1, va[1] + 6, va[3] + 2,                     # v
             va[1] + 8 + 1, va[1] + 12 + 3,                       # v' (Fibonacci)
             va[0] + 4 + 2, va[2] + 4 + 1, va[2] + 8 + 3,         # v_p: the table's; the variable range table's, which is its u_p
             va[0] + 8 + 3,                                       # v_p'
             o_red + 3, o_u - 2,                                  # a reduction round
             ua[0] + 1, ua[1] + 5,                                # u
             ua[0] + 4 + 2,                                       # u_p
             o1 + 2, (o1 + o2) // 2, o2 - 2,                      # the main opening
             o2, o2 + 5, (o2 + len(words)) // 2, len(words) - 2)  # the key's opening: a value, the sum-check, the WHIR part
    for i in spots:
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, bad)
    either = (ERR_INVALID, ERR_VERIFY)   # a wrong shape parameter is refused as a shape or as a word count
    wrong = list(key.root)
    wrong[3] = (wrong[3] + 1) % P
    _refused(prm, airs, wrong, lpr, pvs, l, wb, prefix, words)
    for lpr2 in (lpr - 1, lpr + 1):
        _refused(prm, airs, key.root, lpr2, pvs, l, wb, prefix, words, code=either)
    for l2 in (l - 1, l + 1):
        _refused(prm, airs, key.root, lpr, pvs, l2, wb, prefix, words, code=either)
    _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix + [1], words)
    _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix[:1], words)
    _refused(prm, airs, key.root, lpr, pvs, l, False, prefix, words)
    for i, m2 in ((1, 4), (4, 3)):   # a height
        a2 = [dict(a) for a in airs]
        a2[i]["log_height"] = m2
        _refused(prm, a2, key.root, lpr, pvs, l, wb, prefix, words, code=either)
    from zkvm_prover_amd import air

    a2 = [dict(a) for a in airs]   # a program: the same table on another bus
    a2[0]["program"] = air.range_table_air(bus=6).program()
    _refused(prm, a2, key.root, lpr, pvs, l, wb, prefix, words)
    bad_pvs = [list(p) for p in pvs]   # public values (Fibonacci's)
    bad_pvs[1][0] = (bad_pvs[1][0] + 1) % P
    _refused(prm, airs, key.root, lpr, bad_pvs, l, wb, prefix, words)
    for bad in (words[:-1], list(words) + [0]):   # truncated, extended
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, bad)
    for i in (2, 20, o_b + 3, o_rounds + 2, va[0] + 5, va[0] + 9, o_red + 4, ua[0] + 6, o1 + 1, o2 + 1, o2 + 4 + 3):   # non-canonical
        big = list(words)
        big[i] += P
        _refused(prm, airs, key.root, lpr, pvs, l, wb, prefix, big)
    big = list(key.root)
    big[0] += P
    _refused(prm, airs, big, lpr, pvs, l, wb, prefix, words, model=False, code=(ERR_INVALID,))
    # the zero-check form of the same set (the variable range table inactive: in the key's opening only)
    key0, root0, words0, info0 = _prove(prm, airs, traces, preps, pvs, l, lpr, False, prefix)
    _accept(prm, airs, key0.root, lpr, pvs, l, False, prefix, root0, words0)
    _refused(prm, airs, key0.root, lpr, pvs, l, True, prefix, words0)
    for i in (8 + 5, info0["open2_at"] + 4 + 1, info0["open2_at"] + 8 + 2):   # a round; the inactive AIR's values in the key's opening
        bad = list(words0)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key0.root, lpr, pvs, l, False, prefix, bad)


def test_refuses_a_flip_in_u_p_eq_v_p_without_reduction():
    """var_range: nothing reduces, the key's opening must show v_p itself"""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset("var_range")
    key, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, True, [4])
    assert info["head"] == info["o_red"]
    va = info["val_at"][0]
    for i in (va + 4 + 1, va + 8 + 1, info["open2_at"] + 6):   # v_p (two columns), the opened value
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key.root, lpr, pvs, l, True, [4], bad)


def test_refuses_an_honest_proof_under_a_key_with_one_table_cell_changed():
    """The attack the key exists to stop (tests/test_keyed_cpu.py's): every step of the prover's proof is honest for ITS table; under
    the verifier's root it is refused."""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset("range3")
    good = km.Key(prm, airs, preps, lpr)
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][7] = 6
    key, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, True, [5])
    assert key.root != good.root
    _refused(prm, airs, good.root, lpr, pvs, l, True, [5], words)
    # the same prover, now lying about the key it used: the transcript is the verifier's, the key's opening is of another table
    _, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, True, [5], key=good)
    _refused(prm, airs, good.root, lpr, pvs, l, True, [5], words)
    # a table cell nothing constrains and nobody looks up: only the key catches it
    airs, traces, preps, pvs, l, lpr, _ = kset("var_range")
    good = km.Key(prm, airs, preps, lpr)
    row = traces[0][0].index(0)
    bad_preps = [[list(c) for c in p] if p else p for p in preps]
    bad_preps[0][0][row] = (bad_preps[0][0][row] + 1) % P
    _, root, words, _ = _prove(prm, airs, traces, bad_preps, pvs, l, lpr, True, [6], key=good)
    _refused(prm, airs, good.root, lpr, pvs, l, True, [6], words)
    _, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, True, [6], key=good)
    _accept(prm, airs, good.root, lpr, pvs, l, True, [6], root, words)


def test_refuses_an_honest_proof_over_a_changed_multiplicity():
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset("range3")
    traces[0][0][2] = (traces[0][0][2] + 1) % P
    key, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, True, [1])
    assert words[8:12] != kb.ZERO   # P != 0
    _refused(prm, airs, key.root, lpr, pvs, l, True, [1], words)


@pytest.mark.parametrize("name", ["range3", "prep_heights"])
def test_refuses_a_prover_without_the_power_of_two_weights(name):
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset(name)
    key, root, words, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, True, [3], weighted=False)
    assert len(words) == kb.proof_words(prm, airs, l, lpr)
    _refused(prm, airs, key.root, lpr, pvs, l, True, [3], words)


def test_refuses_proofs_in_the_other_formats():
    """airkey_prove's format (per AIR, same key) and airbatch_prove's (batched, unkeyed: of the set's AIRs without PREP)"""
    import zkvm_prover_amd as z

    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, _ = kset("five")
    key = km.Key(prm, airs, preps, lpr)
    n = kb.proof_words(prm, airs, l, lpr)
    ch = Challenger()
    ch.observe([4])
    root, words, _ = km.prove(ch, prm, airs, traces, preps, pvs, l, key, True)
    z.airkey_verify(_lp(prm), [4], airs, key.root, lpr, pvs, l, words, True)
    assert len(words) != n
    _refused(prm, airs, key.root, lpr, pvs, l, True, [4], words)
    _refused(prm, airs, key.root, lpr, pvs, l, True, [4], (list(words) + [0] * n)[:n])   # ... and cut or padded to the batched length
    _, _, bwords, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, True, [4], key=key)
    with pytest.raises(z.ZkhipError):
        z.airkey_verify(_lp(prm), [4], airs, key.root, lpr, pvs, l, bwords, True)
    # the unkeyed batched proof of the AIRs without PREP (with_bus = 0: their interactions are ignored)
    sub = [1, 3, 4]
    ch = Challenger()
    ch.observe([4])
    sairs, spvs = [airs[a] for a in sub], [pvs[a] for a in sub]
    root, words, _ = bm.prove(ch, prm, sairs, [traces[a] for a in sub], spvs, l, False)
    z.airbatch_verify(_lp(prm), [4], sairs, spvs, l, words, False)
    n0 = kb.proof_words(prm, airs, l, lpr, False)
    _refused(prm, airs, key.root, lpr, pvs, l, False, [4], words)
    _refused(prm, airs, key.root, lpr, pvs, l, False, [4], (list(words) + [0] * n0)[:n0])
    _, _, bwords0, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, False, [4], key=key)
    with pytest.raises(z.ZkhipError):
        z.airbatch_verify(_lp(prm), [4], sairs, spvs, l, bwords0, False)


def test_refused_shapes():
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    prm = _params(1, 2, 1)
    lp = _lp(prm)

    def invalid(airs, pvs, l=4, lpr=3, wb=True):
        assert z.airkey_batch_proof_words(lp, airs, l, lpr, wb) == 0 == kb.proof_words(prm, airs, l, lpr, wb)
        with pytest.raises(z.ZkhipError) as e:
            z.airkey_batch_verify(lp, [], airs, [0] * 8, lpr, pvs, l, [0] * 64, wb)
        assert e.value.code == ERR_INVALID

    airs, _, _, pvs, l, lpr, _ = kset("range3")
    assert z.airkey_batch_proof_words(lp, airs, l, lpr, True) > 0 and z.airkey_batch_proof_words(lp, airs, l, lpr, False) > 0
    invalid([airs[1]], [[]])                                  # no PREP anywhere: zkhip_airbatch_*'s case
    invalid([airs[1]], [[]], wb=False)
    assert z.airbatch_proof_words(lp, [airs[1]], l, False) > 0
    for wb in (True, False):                                  # ... which still refuses PREP
        assert z.airbatch_proof_words(lp, airs, l, wb) == 0
    assert z.airkey_batch_proof_words(lp, [airs[0]] + [airs[1]] * 63, 8, lpr, True) > 0
    invalid([airs[0]] + [airs[1]] * 64, [[]] * 65, l=8)      # 65 AIRs
    invalid([airs[0]] + [airs[1]] * 64, [[]] * 65, l=8, wb=False)
    b = air.AirBuilder(1, 0, prep_width=1)                    # D = 9
    e = b.prep(0)
    for _ in range(7):
        e = e * b.prep(0)
    b.assert_zero(e - b.var(0))
    b.push_interaction(5, [b.prep(0)], b.var(0), "receive")
    invalid([_air(b, 3), airs[1]], pvs)
    invalid([_air(b, 3), airs[1]], pvs, wb=False)
    invalid(airs, pvs, lpr=1)                                 # log_stack_prep below fold_log = 2
    invalid(airs, pvs, lpr=27)
    invalid([dict(airs[0], log_height=0), airs[1]], pvs)
