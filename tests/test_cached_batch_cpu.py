"""CPU: the keyed batched form with cached partitions (docs/cached_main.md) -- the independent model (tests/cached_batch_model.py)
against brute force (v, u and the cached openings' values are the MLEs of the right columns at the right prefixes, M <= 4) and against
the library's host verifier (zkhip_airkey_cached_verify): model proofs over a grid of AIR sets, two parameter sets and the with_bus
values under which the statement holds are accepted with the word count of zkhip_airkey_cached_proof_words, and the returned roots are
the model's; forged, mis-shaped and non-canonical proofs are refused, and so are cached openings exchanged between two partitions, an
honest proof over a trace whose cached column differs from the committed copy, and a proof in zkhip_airkey_batch_prove's format; a
proof about another partition is accepted only with the other root handed back; refused shapes.

The sets (`cset`), each made of test_keyed_cpu's items with air.with_cached_width and of small hand-built AIRs:
  program     a program-like AIR (m = 2, w = 3, cached width w - 1 = 2: the cached columns are received on a bus with the common column
              as multiplicity) with its sender, beside the PREP range table and its user; with_bus = 0 leaves the program AIR inactive
  five        test_keyed_cpu's `five`: Fibonacci (m = 5, log_stack_cached 3: four stacked columns) reduces through a rotation-1 read
              of its cached column 0; the variable-range user (m = 2, log_stack_cached 4: padded) does not reduce
  hand        an AIR with PREP and CACHED (both rotated columns cached), with_bus = 0
  tall_short  the cached Fibonacci is the tallest AIR (m = 4), the cached program AIR the shortest (m = 1)"""
import numpy as np
import pytest

import cached_batch_model as cm
import gkr_model as gm
import keyed_batch_model as kb
import keyed_model as km
import whir_model as wm
from pymodel import P, Challenger
from test_keyed_cpu import PARAM_SETS, _air, _fib, _hand, _lp, _params, _range_pair, _var_range_pair

ERR_INVALID, ERR_VERIFY = -3, -7


def _cached(item, cw):
    """the item with its first cw main columns declared cached"""
    from zkvm_prover_amd import air

    a, tr, pr, pv = item
    return dict(a, program=air.with_cached_width(a["program"], cw)), tr, pr, pv


def _program_pair(mp, ms, seed=0, bus=9, run=None):
    """the program-like AIR (2^mp instructions (pc, op) cached, their execution frequencies common) and the AIR that executes 2^ms of
    them: it sends (pc, op) once per row.  run: another execution of the same program (the same seed)"""
    from zkvm_prover_amd import air

    rng = np.random.default_rng(seed)
    n, ns = 1 << mp, 1 << ms
    rom = np.stack([4 * np.arange(n), rng.integers(1, 50, size=n)])
    ran = (rng if run is None else np.random.default_rng(run)).integers(0, n, size=ns)
    ran[0] = 0   # the multiplicities are not all zero, and not all equal
    freq = np.bincount(ran, minlength=n)
    b = air.AirBuilder(3, 0, cached_width=2)
    b.push_interaction(bus, [b.var(0), b.var(1)], b.var(2), "receive")
    s = air.AirBuilder(3, 0)
    s.assert_zero(s.var(2) - s.var(0) * s.var(1))
    s.push_interaction(bus, [s.var(0), s.var(1)], 1, "send")
    sent = np.stack([rom[0][ran], rom[1][ran], rom[0][ran] * rom[1][ran] % P])
    return [(_air(b, mp), np.stack([rom[0], rom[1], freq]).tolist(), None, []), (_air(s, ms), sent.tolist(), None, [])]


def cset(name):
    """(airs, traces, preps, pvs, log_stack, log_stack_prep, log_stack_cached per AIR, the with_bus values)"""
    if name == "program":
        items, l, lpr, lsc, wbs = _program_pair(2, 3) + _range_pair(2, mu=3), 4, 3, [3, None, None, None], (True, False)
    elif name == "five":
        rt, ru = _range_pair(3)
        vt, vu = _var_range_pair(3, mu=2)
        items, l, lpr, lsc, wbs = [rt, _cached(_fib(5), 1), vt, ru, _cached(vu, 2)], 4, 3, [None, 3, None, None, 4], (True, False)
    elif name == "hand":
        items, l, lpr, lsc, wbs = [_cached(_hand(), 2)], 4, 3, [3], (False,)
    elif name == "tall_short":
        items = [_cached(_fib(4), 1)] + _program_pair(1, 2, seed=1) + _range_pair(2, mu=3, seed=3)
        l, lpr, lsc, wbs = 4, 3, [2, 2, None, None, None], (True, False)
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items], [x[3] for x in items], l, lpr, lsc, wbs


NAMES = ["program", "five", "hand", "tall_short"]
CASES = [(n, wb) for n in NAMES for wb in ((False,) if n == "hand" else (True, False))]


def _handles(prm, airs, traces, lsc):
    return [cm.Cached(prm, airs, a, traces[a], lsc[a]) if lsc[a] is not None else None for a in range(len(airs))]


def _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, wb, prefix, key=None, cached=None):
    key = key or km.Key(prm, airs, preps, lpr)
    cached = cached or _handles(prm, airs, traces, lsc)
    ch = Challenger()
    ch.observe(prefix)
    root, words, info = cm.prove(ch, prm, airs, traces, preps, pvs, l, key, cached, wb)
    return key, cached, root, words, info


def _accept(prm, airs, prep_root, lpr, lsc, pvs, l, wb, prefix, root, croots, words):
    import zkvm_prover_amd as z

    assert len(words) == cm.proof_words(prm, airs, l, lpr, lsc, wb) == z.airkey_cached_proof_words(_lp(prm), airs, l, lpr, lsc, wb)
    ch = Challenger()
    ch.observe(prefix)
    m = cm.verify(ch, prm, airs, prep_root, lpr, lsc, pvs, l, words, wb)
    got = z.airkey_cached_verify(_lp(prm), prefix, airs, prep_root, lpr, lsc, pvs, l, words, wb)
    assert m[0] == root == got[0].tolist()
    assert m[-1] == croots == got[-1].tolist()   # the cached roots the proof sent, AIR order
    if wb:
        assert got[1].tolist() == m[1][0] + m[1][1] and m[1][0] == cm.ZERO
    return got


def _refused(prm, airs, prep_root, lpr, lsc, pvs, l, wb, prefix, words, model=True, code=(ERR_VERIFY,)):
    import zkvm_prover_amd as z

    with pytest.raises(z.ZkhipError) as e:
        z.airkey_cached_verify(_lp(prm), prefix, airs, prep_root, lpr, lsc, pvs, l, words, wb)
    assert e.value.code in code
    if model:
        ch = Challenger()
        ch.observe(prefix)
        with pytest.raises((wm.WhirReject, gm.GkrReject, cm.Refused, IndexError)):
            cm.verify(ch, prm, airs, prep_root, lpr, lsc, pvs, l, words, wb)


def _roots(cached):
    return [c.root for c in cached if c is not None]


# ---- the model's values, by brute force --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,with_bus", [("program", True), ("program", False), ("tall_short", True), ("hand", False)])
def test_values_are_the_mles_of_the_right_columns_at_the_right_prefixes(name, with_bus):
    """M <= 4.  v of every active AIR = the MLEs of ALL its main columns (cached first) at r[0..m_a); u of every reducing AIR = the
    same at r'[0..m_a); a cached opening's values = the MLEs of the cached columns at the AIR's point (the prefix of r' if it reduces,
    of r if it is active and does not, its own sampled point if it is inactive); the main opening's values = the MLEs of the common
    columns only.  The MLE is the sum over the m_a-cube of col[x] eq(x, point), written out."""
    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset(name)
    key, cached, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, with_bus, [1])
    plans = info["plans"]
    act, M, D, red, M2 = cm.dims(plans)
    assert 1 <= M <= 4

    def mle(col, pt):   # by brute force over the cube
        acc = cm.ZERO
        for x, c in enumerate(col):
            e = cm.ONE
            for j, z in enumerate(pt):
                e = wm.ext_mul(e, z if (x >> j) & 1 else wm.ext_sub(cm.ONE, z))
            acc = wm.ext_add(acc, wm.ext_mul(e, gm.ext_c(int(c) % P)))
        return acc

    for a in act:
        assert info["values"][a][:plans[a].w] == [mle(c, info["r"][:plans[a].m]) for c in traces[a]]
    for a in red:
        assert info["u"][a][:plans[a].w] == [mle(c, info["rp"][:plans[a].m]) for c in traces[a]]
    for a in info["cached_airs"]:
        pl, cw = plans[a], info["cw"][a]
        pt = info["rp"][:pl.m] if a in red else info["r"][:pl.m] if pl.active else info["points"][a]
        assert pt == info["points"][a] and len(pt) == pl.m
        assert info["cached_values"][a] == [mle(c, pt) for c in traces[a][:cw]]
        at = info["open3_at"][a]
        assert words[at:at + 4 * cw] == [x for e in info["cached_values"][a] for x in e]
    o, col = info["open_at"], 0
    for a, pl in enumerate(plans):   # the main opening: the common columns, AIRs in caller order
        for c in traces[a][info["cw"][a]:]:
            assert words[o + 4 * col:o + 4 * col + 4] == mle(c, info["points"][a])
            col += 1
    if name == "program" and not with_bus:
        assert not plans[0].active and info["cw"][0] == 2   # an inactive AIR with a cached partition


# ---- the library's verifier on model proofs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", [0, 1])
@pytest.mark.parametrize("name,with_bus", CASES)
def test_accepts_model_proofs(name, with_bus, pi):
    prm = PARAM_SETS[pi]
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset(name)
    prefix = [9, pi]
    key, cached, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, with_bus, prefix)
    _accept(prm, airs, key.root, lpr, lsc, pvs, l, with_bus, prefix, root, _roots(cached), words)
    assert words[:info["pre"]] == [x for r in _roots(cached) for x in r] and words[info["pre"]:info["pre"] + 8] == root


def test_the_shapes_are_the_ones_named():
    prm = PARAM_SETS[0]

    def d(name, wb):
        airs, _, _, _, l, lpr, lsc, _ = cset(name)
        S = cm.Shape(prm, airs, l, lpr, lsc, wb)
        return (S, S.plans) + cm.dims(S.plans)

    S, plans, act, M, D, red, M2 = d("program", True)
    assert S.cw == [2, 0, 0, 0] and plans[0].w == 3 and plans[0].ints and not plans[0].proven and 0 in act   # cached width w - 1
    assert any(p.wp for p in plans)
    S, plans, act, M, D, red, M2 = d("program", False)
    assert 0 not in act                                                  # inactive with a cached partition
    S, plans, act, M, D, red, M2 = d("five", True)
    assert S.cw == [0, 1, 0, 0, 2] and 1 in red and 0 in plans[1].rot    # reduces through a rotation-1 read of a cached column
    assert 4 in act and 4 not in red                                     # a cached AIR that does not reduce
    assert plans[1].m == 5 > S.l_cached[1] == 3 and plans[4].m == 2 < S.l_cached[4] == 4   # several stacked columns; padded
    S, plans, act, M, D, red, M2 = d("hand", False)
    assert S.cw == [2] and plans[0].wp == 3 and plans[0].rot == [0, 1]   # PREP and CACHED
    S, plans, act, M, D, red, M2 = d("tall_short", True)
    ms = [p.m for p in plans]
    assert S.cw[:2] == [1, 2] and ms[0] == max(ms) == 4 and ms[1] == min(ms) == 1


def test_refuses_forgeries():
    prm = _params(1, 2, 1, pow_bits=3, nq=3)
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("five")
    wb, prefix = True, [11, 12]
    key, cached, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, wb, prefix)
    croots = _roots(cached)
    _accept(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix, root, croots, words)
    pre, o_b, o_rounds, o_vals, o_red, o_u, head = (info[k] for k in ("pre", "o_b", "o_rounds", "o_vals", "o_red", "o_u", "head"))
    va, ua, o1, o2, o3 = info["val_at"], info["u_at"], info["open_at"], info["open2_at"], info["open3_at"]
    assert pre == 16 and head == o1 < o2 < o3[1] < o3[4] < len(words)
    spots = (2, 8 + 5,                                            # the two cached roots
             pre + 3,                                             # the main root
             pre + 8 + 2, o_b + 1, o_rounds + 7, va[1] + 1, va[1] + 8 + 1, va[4] + 2, o_red + 3, ua[1] + 1,   # the middle
             o1 + 2, (o1 + o2) // 2, o2 - 2,                      # the main opening
             o2, o2 + 5, (o2 + o3[1]) // 2, o3[1] - 2,            # the key's opening
             o3[1], o3[1] + 6, (o3[1] + o3[4]) // 2, o3[4] - 2,   # Fibonacci's cached opening: the value, the sum-check, the WHIR part
             o3[4] + 1, o3[4] + 5, o3[4] + 9, len(words) - 2)     # the user's cached opening
    for i in spots:
        bad = list(words)
        bad[i] = (bad[i] + 1) % P
        _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix, bad)
    either = (ERR_INVALID, ERR_VERIFY)   # a wrong shape parameter is refused as a shape or as a word count
    for a, l2 in ((1, 2), (1, 4), (4, 3), (4, 5)):   # log_stack_cached
        lsc2 = list(lsc)
        lsc2[a] = l2
        _refused(prm, airs, key.root, lpr, lsc2, pvs, l, wb, prefix, words, code=either)
    wrong = list(key.root)
    wrong[3] = (wrong[3] + 1) % P
    _refused(prm, airs, wrong, lpr, lsc, pvs, l, wb, prefix, words)
    for lpr2 in (lpr - 1, lpr + 1):
        _refused(prm, airs, key.root, lpr2, lsc, pvs, l, wb, prefix, words, code=either)
    for l2 in (l - 1, l + 1):
        _refused(prm, airs, key.root, lpr, lsc, pvs, l2, wb, prefix, words, code=either)
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix + [1], words)
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix[:1], words)
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, False, prefix, words, code=either)
    for i, m2 in ((1, 4), (4, 3)):   # a height
        a2 = [dict(a) for a in airs]
        a2[i]["log_height"] = m2
        _refused(prm, a2, key.root, lpr, lsc, pvs, l, wb, prefix, words, code=either)
    from zkvm_prover_amd import air

    a2 = [dict(a) for a in airs]   # a program: the same table on another bus
    a2[0]["program"] = air.range_table_air(bus=6).program()
    _refused(prm, a2, key.root, lpr, lsc, pvs, l, wb, prefix, words)
    a2 = [dict(a) for a in airs]   # a program: another cached width (the user's: 1 of 3 columns)
    a2[4]["program"] = air.with_cached_width(air.var_range_user_air().program(), 1)
    _refused(prm, a2, key.root, lpr, lsc, pvs, l, wb, prefix, words, code=either)
    bad_pvs = [list(p) for p in pvs]
    bad_pvs[1][0] = (bad_pvs[1][0] + 1) % P
    _refused(prm, airs, key.root, lpr, lsc, bad_pvs, l, wb, prefix, words)
    for bad in (words[:-1], list(words) + [0]):   # truncated, extended
        _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix, bad)
    for i in (1, 9, pre + 2, pre + 20, o_rounds + 2, va[1] + 5, o_red + 4, ua[1] + 2, o1 + 1, o2 + 1, o3[1] + 1, o3[4] + 6):   # non-canonical
        big = list(words)
        big[i] += P
        _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, prefix, big)


def test_refuses_cached_values_exchanged_between_two_partitions():
    """Two partitions of one shape (two program AIRs of the same height and width): the openings' words are exchanged whole, and only
    their values; each is an honest opening of the other commitment."""
    prm = PARAM_SETS[0]
    p1, s1 = _program_pair(2, 3, seed=0, bus=9)
    p2, s2 = _program_pair(2, 3, seed=5, bus=10)
    items = [p1, s1, p2, s2] + _range_pair(2, mu=3)
    airs, traces, preps, pvs = ([x[i] for x in items] for i in range(4))
    l, lpr, lsc, prefix = 4, 3, [3, None, 3, None, None, None], [2]
    key, cached, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, True, prefix)
    _accept(prm, airs, key.root, lpr, lsc, pvs, l, True, prefix, root, _roots(cached), words)
    a, b = info["open3_at"][0], info["open3_at"][2]
    n = b - a
    assert len(words) == b + n and words[a:a + 8] != words[b:b + 8]
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, prefix, words[:a] + words[b:] + words[a:b])
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, prefix, words[:a] + words[b:b + 8] + words[a + 8:b] + words[a:a + 8] + words[b + 8:])
    # ... and with the roots exchanged too, every opening fits its root: the values no longer are u's
    sw = words[8:16] + words[:8] + words[16:a] + words[b:] + words[a:b]
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, prefix, sw)


def test_a_proof_about_another_program_carries_the_other_root():
    """The prover commits another program and proves honestly about it (its sender runs that program): the verifier accepts, and the
    cached root it hands back differs from the program commitment the caller holds.  The caller's comparison is what binds the proof to
    the program."""
    import zkvm_prover_amd as z

    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("program")
    held = _handles(prm, airs, traces, lsc)[0].root   # the program commitment the caller holds
    other = _program_pair(2, 3, seed=7) + _range_pair(2, mu=3)
    traces2 = [x[1] for x in other]
    assert traces2[0][1] != traces[0][1]
    key, cached, root, words, _ = _prove(prm, airs, traces2, preps, pvs, l, lpr, lsc, True, [3])
    got = z.airkey_cached_verify(_lp(prm), [3], airs, key.root, lpr, lsc, pvs, l, words, True)
    assert got[2].tolist() == [cached[0].root] and cached[0].root != held
    # the same words with the held root put in its place: the opening is of another commitment
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, [3], held + words[8:])


def test_refuses_an_honest_proof_over_a_trace_that_differs_from_the_committed_copy():
    """The prover reads the cached columns from the traces, the commitment owns a copy.  One cell of a cached column differs: every
    step is honest for the trace, the cached opening shows the copy's values, which are not u's (v's)."""
    prm = PARAM_SETS[0]
    for name, a, wb in (("five", 1, True), ("five", 4, True), ("program", 0, False)):   # reduces; does not; inactive
        airs, traces, preps, pvs, l, lpr, lsc, _ = cset(name)
        cached = _handles(prm, airs, traces, lsc)
        traces[a][0][1] = (traces[a][0][1] + 1) % P
        key, _, root, words, info = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, wb, [5], cached=cached)
        if info["plans"][a].active:
            _refused(prm, airs, key.root, lpr, lsc, pvs, l, wb, [5], words)
        else:   # an inactive AIR states nothing about its columns: the opening's own values stand
            _accept(prm, airs, key.root, lpr, lsc, pvs, l, wb, [5], root, _roots(cached), words)


def test_refuses_a_proof_in_the_keyed_batched_format():
    import zkvm_prover_amd as z

    prm = PARAM_SETS[0]
    airs, traces, preps, pvs, l, lpr, lsc, _ = cset("five")
    key = km.Key(prm, airs, preps, lpr)
    ch = Challenger()
    ch.observe([4])
    root, words, _ = kb.prove(ch, prm, airs, traces, preps, pvs, l, key, True)
    z.airkey_batch_verify(_lp(prm), [4], airs, key.root, lpr, pvs, l, words, True)   # where the section is ignored
    n = cm.proof_words(prm, airs, l, lpr, lsc)
    assert len(words) != n
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, [4], words)
    _refused(prm, airs, key.root, lpr, lsc, pvs, l, True, [4], (list(words) + [0] * n)[:n])
    _, _, _, cwords, _ = _prove(prm, airs, traces, preps, pvs, l, lpr, lsc, True, [4], key=key)
    with pytest.raises(z.ZkhipError):
        z.airkey_batch_verify(_lp(prm), [4], airs, key.root, lpr, pvs, l, cwords, True)


def test_refused_shapes():
    import zkvm_prover_amd as z

    prm = _params(1, 2, 1)   # fold_log = 2
    lp = _lp(prm)

    def invalid(airs, pvs, lsc, l=4, lpr=3, wb=True):
        assert z.airkey_cached_proof_words(lp, airs, l, lpr, lsc, wb) == 0 == cm.proof_words(prm, airs, l, lpr, lsc, wb)
        with pytest.raises(z.ZkhipError) as e:
            z.airkey_cached_verify(lp, [], airs, [0] * 8, lpr, lsc, pvs, l, [0] * 64, wb)
        assert e.value.code == ERR_INVALID

    airs, _, _, pvs, l, lpr, lsc, _ = cset("program")
    for wb in (True, False):
        assert z.airkey_cached_proof_words(lp, airs, l, lpr, lsc, wb) > 0
    plain, ppvs = [airs[1], airs[2], airs[3]], [[], [], []]   # no CACHED anywhere: zkhip_airkey_batch_*'s case
    assert z.airkey_batch_proof_words(lp, plain, l, lpr, False) > 0
    invalid(plain, ppvs, [3, 3, 3], wb=False)
    invalid(airs, pvs, [1, None, None, None])        # log_stack_cached below fold_log
    invalid(airs, pvs, [1, None, None, None], wb=False)
    invalid(airs, pvs, [27, None, None, None])       # ... above ZKHIP_WHIR_MAX_LOG_N
    invalid(airs[:2], pvs[:2], [3, None])            # cached partitions but no PREP: the key is the carrier
    invalid(airs, pvs, lsc, l=1)                     # the common columns do not fit log_stack
    invalid(airs, pvs, lsc, lpr=1)
    invalid([dict(airs[0], log_height=0)] + airs[1:], pvs, lsc)
    # the forms that ignore the section keep ignoring it: the same word counts with and without it
    from zkvm_prover_amd import air

    b = air.AirBuilder(3, 0)
    b.push_interaction(9, [b.var(0), b.var(1)], b.var(2), "receive")
    bare = [dict(airs[0], program=b.program())] + airs[1:]
    for wb in (True, False):
        assert z.airkey_batch_proof_words(lp, airs, l, lpr, wb) == z.airkey_batch_proof_words(lp, bare, l, lpr, wb) > 0
        assert z.airkey_proof_words(lp, airs, l, lpr, wb) == z.airkey_proof_words(lp, bare, l, lpr, wb) > 0


@pytest.mark.parametrize("name", ["big", "chipset"])
def test_the_recorded_model_words_of_the_larger_sets_are_accepted(name):
    """tests/golden/cached_batch_words.npz holds the model's proofs of the two sets the GPU test compares the device with (the model
    takes minutes on them); the library's verifier replays them here, and they are refused with a word changed"""
    import cached_batch_sets as cs
    import zkvm_prover_amd as z

    prm, airs, traces, preps, pvs, l, lpr, lsc, prefix = cs.SETS[name]()
    kr, cr, root, words = cs.recorded(name)
    assert len(words) == z.airkey_cached_proof_words(_lp(prm), airs, l, lpr, lsc, True) == cm.proof_words(prm, airs, l, lpr, lsc)
    got = z.airkey_cached_verify(_lp(prm), prefix, airs, kr, lpr, lsc, pvs, l, words, True)
    assert got[0].tolist() == root.tolist() and got[2].tolist() == cr.tolist() and got[1].tolist()[:4] == [0, 0, 0, 0]
    bad = words.copy()
    bad[len(bad) - 3] = (int(bad[len(bad) - 3]) + 1) % P
    _refused(prm, airs, kr, lpr, lsc, pvs, l, True, prefix, bad, model=False)
