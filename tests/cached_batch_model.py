"""Independent Python model of the keyed batched form with cached partitions (docs/cached_main.md): the keyed batched AIR-set proof
(tests/keyed_batch_model.py) for AIR sets in which a program declares its first cached_width main columns a cached main partition.
Each partition is a stacked commitment of its own, made once (`Cached`); the proof's main commitment holds the common columns only;
the cached roots are sent and observed after the key's root and before the main root; after the main opening and the key's, every
partition's commitment is opened at its AIR's point.  Built on tests/keyed_batch_model.py (dims, layout, summand, tables), tests/
keyed_model.py (Plan, Key, the leaves) and below them the AIR-set, GKR, stacking and WHIR models.  It imports nothing from the product.

keyed_batch_model.prove / verify commit to and open every main column in one commitment and cannot be reused without editing: the
steps between the head and the openings are restated here as they stand there (a cached column is a main column to them).

Conventions as in keyed_batch_model.  `cached`: per AIR a `Cached` or None; `l_cached`: per AIR its log_stack_cached (read where the
AIR has a CACHED section)."""
import airset_model as am
import gkr_model as gm
import keyed_batch_model as kb
import keyed_model as km
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, ext_add, ext_mul

ZERO, ONE = wm.ZERO, wm.ONE
Refused = zm.Refused
Plan, Key = km.Plan, km.Key
pow2, dims, summand, tables = kb.pow2, kb.dims, kb.summand, kb.tables


def cached_width(air):
    """the cached_width of a program's CACHED section (it follows the constraints and the PREP section), 0 without one"""
    w = [int(x) for x in air["program"]]
    q = 4 + 3 * w[1] + w[2]
    if len(w) > q and w[q] == zm.PREP_MAGIC:
        q += 2
    return w[q + 1] if len(w) > q + 1 and w[q] == am.CACHED_MAGIC else 0


class Cached:
    """a cached main partition: the stacked commitment, at l_cached, of the first cached_width columns of AIR `air` (its whole trace,
    or those columns, will do).  Made once; a proof opens it and never changes it."""

    def __init__(self, params, airs, air, trace, l_cached):
        self.air, self.m, self.cw, self.l = air, int(airs[air]["log_height"]), cached_width(airs[air]), l_cached
        if not self.cw:
            raise Refused("no CACHED section")
        self.cols = [[int(v) % P for v in c] for c in trace[:self.cw]]
        if not sm.width(params, [self.m] * self.cw, l_cached):
            raise Refused("partition stack shape")
        self.com = sm.Commitment(params, self.cols, [self.m] * self.cw, l_cached)
        self.root = list(self.com.root)


class Shape:
    """keyed_model.Shape with the main commitment over the common columns: heights / col_point are the common columns', cw the cached
    widths, cached_airs the AIRs with a partition"""

    def __init__(self, params, airs, l, l_prep, l_cached, with_bus):
        if not 1 <= len(airs) <= sm.MAX_POINTS:
            raise Refused("AIR count")
        self.plans = plans = [Plan(a, with_bus) for a in airs]
        if sum(p.w for p in plans) > sm.MAX_COLS:
            raise Refused("column total")
        self.cw = [cached_width(a) for a in airs]
        if any(c >= p.w for c, p in zip(self.cw, plans)):
            raise Refused("a common part must remain")
        self.cached_airs = [a for a, c in enumerate(self.cw) if c]
        if not self.cached_airs:
            raise Refused("no CACHED: the keyed batched form's case")
        self.l_cached = [int(l_cached[a]) if self.cw[a] else None for a in range(len(airs))]
        for a in self.cached_airs:
            if not sm.width(params, [plans[a].m] * self.cw[a], self.l_cached[a]):
                raise Refused("partition stack shape")
        self.heights = [p.m for p, c in zip(plans, self.cw) for _ in range(p.w - c)]
        self.col_point = [i for i, (p, c) in enumerate(zip(plans, self.cw)) for _ in range(p.w - c)]
        if not sm.width(params, self.heights, l):
            raise Refused("stack shape")
        self.prep_airs = [a for a, p in enumerate(plans) if p.wp]
        if not self.prep_airs:
            raise Refused("no PREP: the key is the carrier")
        self.heights_p = [plans[a].m for a in self.prep_airs for _ in range(plans[a].wp)]
        self.col_point_p = [i for i, a in enumerate(self.prep_airs) for _ in range(plans[a].wp)]
        if not sm.width(params, self.heights_p, l_prep):
            raise Refused("key stack shape")
        self.blocks, self.L = [], 0
        if with_bus:
            self.blocks, _, self.L = am.layout(plans)
            if not self.blocks:
                raise Refused("no interaction")
            if self.L > am.GKR_MAX_LOG_N:
                raise Refused("too many leaves")

    def cached_words(self, params, a):
        return sm.proof_words(params, [self.plans[a].m] * self.cw[a], self.l_cached[a])


def layout(S, with_bus):
    """keyed_batch_model.layout behind the cached roots: every offset moves by pre = 8 n_c"""
    pre = 8 * len(S.cached_airs)
    lay = kb.layout(S, with_bus)
    out = {k: v + pre for k, v in lay.items() if k not in ("val_at", "u_at")}
    out.update(pre=pre, val_at={a: v + pre for a, v in lay["val_at"].items()}, u_at={a: v + pre for a, v in lay["u_at"].items()})
    return out


def proof_words(params, airs, l, l_prep, l_cached, with_bus=True):
    try:
        S = Shape(params, airs, l, l_prep, l_cached, with_bus)
    except Refused:
        return 0
    return (layout(S, with_bus)["head"] + sm.proof_words(params, S.heights, l) + sm.proof_words(params, S.heights_p, l_prep)
            + sum(S.cached_words(params, a) for a in S.cached_airs))


def prove(ch, params, airs, traces, preps, pvs, l, key, cached, with_bus=True, leaf_hook=None):
    """The proof, continuing `ch` (after the caller's prefix): (root, words, info).  The prover reads the cached columns from `traces`
    (the whole traces, cached columns first) and opens the handles' own copies.  leaf_hook: as airset_model.prove's.  info: as keyed_batch_model.prove's, plus the offsets
    of the three kinds of opening (open_at, open2_at, open3_at: AIR -> offset) and the opened cached values."""
    S = Shape(params, airs, l, key.l_prep, [c.l if c else 0 for c in cached], with_bus)
    plans, n_airs = S.plans, len(airs)
    for a in S.cached_airs:
        c = cached[a]
        if c is None or (c.air, c.m, c.cw) != (a, plans[a].m, S.cw[a]):
            raise Refused("a handle made for another AIR, height or width")
    scom = sm.Commitment(params, [[int(v) % P for v in c] for a, tr in enumerate(traces) for c in tr[S.cw[a]:]], S.heights, l)
    ch.observe(list(key.root))
    words = []
    for a in S.cached_airs:   # cached..., common
        wm._observe(ch, list(cached[a].root), words)
    wm._observe(ch, list(scom.root), words)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    rho, coef, c, info = [], [None] * n_airs, {}, {}
    if with_bus:   # steps 2 - 5 of the keyed AIR-set proof
        gamma, beta = gm.bus_challenges(ch)
        num, den = km.leaves(S, traces, preps, pvs, gamma, beta)
        if leaf_hook:
            leaf_hook(num, den)
        gw, rho, _ = gm.prove(ch, num, den)
        words += gw
        eb = am.block_eq(S.blocks, rho)
        kappa = ch.sample_ext()
        B = am.leaf_claims(plans, S.blocks, eb, rho, num, den, kappa)
        wm._observe(ch, [x for e in B for x in e], words)
        coef = am.bus_coefs(plans, S.blocks, eb, beta, kappa)
        with_ints = [a for a, p in enumerate(plans) if p.ints]
        c = {a: wm.ext_sub(B[i], am.const_of(plans[a], a, S.blocks, eb, gamma, kappa)) for i, a in enumerate(with_ints)}
        info.update(rho=rho, coef=coef)
    act, M, D, red, M2 = dims(plans)
    # 6. one batched sum-check
    tau, alpha = [], ZERO
    if any(plans[a].proven for a in act):
        tau = [ch.sample_ext() for _ in range(M)]
        alpha = ch.sample_ext()
    mu = ch.sample_ext()
    mup = sm._powers(mu, max(len(act), 1))
    apow = {a: sm._powers(alpha, max(len(plans[a].proven), 1)) for a in act}
    tabs = {a: tables(plans[a], traces[a], preps[a], tau, rho) for a in act}
    wgt = {a: ext_mul(mup[j], pow2(M - plans[a].m)) for j, a in enumerate(act)}
    g_end = {}
    claim = ZERO
    for a in act:
        claim = ext_add(claim, ext_mul(wgt[a], c.get(a, ZERO)))
    info.update(tau=tau, alpha=alpha, mu=mu, claim0=claim, rounds=[], c=c, sa={})
    r = []
    ca = {a: c.get(a, ZERO) for a in act}   # every AIR's running claim
    for i in range(M):
        s = [ZERO] * (D + 1)
        for j, a in enumerate(act):
            pl = plans[a]
            if pl.m > i:
                sa = []
                for t in range(pl.D + 1):
                    x = ZERO
                    for y in range(len(tabs[a][0]) // 2):
                        x = ext_add(x, summand(pl, [zm._at(tb[2 * y], tb[2 * y + 1], t) for tb in tabs[a]], pvs[a], apow[a], coef[a]))
                    sa.append(x)
                # the round polynomial the AIR would have sent alone is s_a(0), s_a(2), .., s_a(D_a): s_a(1) is what its running claim
                # leaves and the points above D_a follow from those D_a + 1.  On a true statement these are the sums themselves
                sa[1] = wm.ext_sub(ca[a], sa[0])
                sa += [zm.interp(sa[:pl.D + 1], gm.ext_c(t)) for t in range(pl.D + 1, D + 1)]
                info["sa"][(i, a)] = sa   # s_a(0..D) of round i, before its weight
                for t in range(D + 1):
                    s[t] = ext_add(s[t], ext_mul(wgt[a], sa[t]))
            else:   # used up: the constant mu^j 2^(M - 1 - i) g_a(r_a)
                k = ext_mul(ext_mul(mup[j], pow2(M - 1 - i)), g_end[a])
                s = [ext_add(x, k) for x in s]
        info["rounds"].append(s)
        wm._observe(ch, [x for t in [0] + list(range(2, D + 1)) for x in s[t]], words)
        ri = ch.sample_ext()
        r.append(ri)
        for a in act:
            if plans[a].m > i:
                tabs[a] = zm._fold_all(tabs[a], ri)
                ca[a] = zm.interp(info["sa"][(i, a)], ri)
                if plans[a].m == i + 1:   # g_a(r_a), as the last claim gives it (the summand on the folded tables, if the statement is true)
                    g_end[a] = ca[a]
    # 7. the values [v | v' | v_p | v_p'] of every active AIR
    vals = {a: [tabs[a][k][0] for k in range(plans[a].n_val)] for a in act}
    wm._observe(ch, [x for a in act for e in vals[a] for x in e], words)
    info.update(r=r, g_end=g_end, values=vals)
    # 8. one batched rotation reduction
    rp, us = [], {}
    if red:
        lp = sm._powers(ch.sample_ext(), sum(len(vals[a]) for a in red))
        rt, o = {}, 0
        for a in red:
            pl, n = plans[a], 1 << plans[a].m
            cols, pcols = kb._ext_cols(pl, traces[a], preps[a])
            nr = len(pl.rot)
            fa, fb = [ZERO] * n, [ZERO] * n
            for k in range(pl.w):
                fa = [ext_add(x, ext_mul(lp[o + k], y)) for x, y in zip(fa, cols[k])]
            for t, k in enumerate(pl.rot):
                fb = [ext_add(x, ext_mul(lp[o + pl.w + t], y)) for x, y in zip(fb, cols[k])]
            for k in range(pl.wp):
                fa = [ext_add(x, ext_mul(lp[o + pl.w + nr + k], y)) for x, y in zip(fa, pcols[k])]
            for t, k in enumerate(pl.rot_p):
                fb = [ext_add(x, ext_mul(lp[o + pl.w + nr + pl.wp + t], y)) for x, y in zip(fb, pcols[k])]
            e = gm.eq_table(r[:pl.m])
            rt[a] = [fa, e, fb, [e[(x - 1) % n] for x in range(n)]]
            o += len(vals[a])
        end = {}
        for i in range(M2):
            s0, s2 = ZERO, ZERO
            for a in red:
                if plans[a].m > i:
                    x0, x2 = wm._sumcheck_round(rt[a][0], rt[a][1])
                    y0, y2 = wm._sumcheck_round(rt[a][2], rt[a][3])
                    k = pow2(M2 - plans[a].m)
                    s0, s2 = ext_add(s0, ext_mul(k, ext_add(x0, y0))), ext_add(s2, ext_mul(k, ext_add(x2, y2)))
                else:
                    k = ext_mul(pow2(M2 - 1 - i), end[a])
                    s0, s2 = ext_add(s0, k), ext_add(s2, k)
            wm._observe(ch, s0 + s2, words)
            ri = ch.sample_ext()
            rp.append(ri)
            for a in red:
                if plans[a].m > i:
                    rt[a] = zm._fold_all(rt[a], ri)
                    if plans[a].m == i + 1:
                        end[a] = ext_add(ext_mul(rt[a][0][0], rt[a][1][0]), ext_mul(rt[a][2][0], rt[a][3][0]))
        for a in red:   # [u | u_p]
            cols, pcols = kb._ext_cols(plans[a], traces[a], preps[a])
            us[a] = [gm.mle_eval(col, rp[:plans[a].m]) for col in cols + pcols]
        wm._observe(ch, [x for a in red for e in us[a] for x in e], words)
    # 9. the points
    points = []
    for a, pl in enumerate(plans):
        points.append(rp[:pl.m] if a in red else r[:pl.m] if pl.active else [ch.sample_ext() for _ in range(pl.m)])
    info.update(rp=rp, points=points, u=us, plans=plans, cw=S.cw, cached_airs=S.cached_airs, **layout(S, with_bus))
    # 10. the main opening over the common columns, the key's, then every partition's (the handle's own copy of the columns)
    _, op = sm.open_(scom, ch, points, S.col_point)
    pcols = [[int(v) % P for v in col] for a in S.prep_airs for col in preps[a][:plans[a].wp]]
    pcom = key.com if pcols == key.cols else sm.Commitment(params, pcols, S.heights_p, key.l_prep)
    _, op2 = sm.open_(pcom, ch, [points[a] for a in S.prep_airs], S.col_point_p)
    info.update(open_at=len(words), open2_at=len(words) + len(op), open3_at={}, cached_values={})
    tail = op + op2
    for a in S.cached_airs:
        info["open3_at"][a] = len(words) + len(tail)
        info["cached_values"][a], op3 = sm.open_(cached[a].com, ch, [points[a]], [0] * S.cw[a])
        tail += op3
    return list(scom.root), words + tail, info


def verify(ch, params, airs, prep_root, l_prep, l_cached, pvs, l, words, with_bus=True):
    """Replays a proof on `ch` (after the caller's prefix).  Returns (root, cached roots) (with_bus: (root, (P, Q), cached roots));
    raises wm.WhirReject or gm.GkrReject (Refused for a refused shape).  Comparing the cached roots with the commitments the caller
    holds is the caller's business."""
    S = Shape(params, airs, l, l_prep, l_cached, with_bus)
    plans, n_airs = S.plans, len(airs)
    words = [int(x) for x in words]
    if len(words) != proof_words(params, airs, l, l_prep, l_cached, with_bus) or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    ch.observe([int(x) for x in prep_root])
    croots = {a: rd.take(8) for a in S.cached_airs}
    for a in S.cached_airs:
        ch.observe(croots[a])
    root = rd.take(8)
    ch.observe(root)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    rho, coef, c, pq = [], [None] * n_airs, {}, None
    if with_bus:
        gamma, beta = gm.bus_challenges(ch)
        rho, (pstar, qstar), pq = gm.verify(ch, rd.take(gm.proof_words(S.L)), S.L)
        if pq[0] != ZERO or pq[1] == ZERO:
            raise gm.GkrReject("unbalanced")
        eb = am.block_eq(S.blocks, rho)
        kappa = ch.sample_ext()
        with_ints = [a for a, p in enumerate(plans) if p.ints]
        B = {a: rd.ext() for a in with_ints}
        ch.observe([x for a in with_ints for x in B[a]])
        lhs, pad = ZERO, ONE
        for a in with_ints:
            lhs = ext_add(lhs, B[a])
        for e in eb:
            pad = wm.ext_sub(pad, e)
        if ext_add(lhs, ext_mul(kappa, pad)) != ext_add(pstar, ext_mul(kappa, qstar)):
            raise wm.WhirReject("leaf claims")
        coef = am.bus_coefs(plans, S.blocks, eb, beta, kappa)
        c = {a: wm.ext_sub(B[a], am.const_of(plans[a], a, S.blocks, eb, gamma, kappa)) for a in with_ints}
    act, M, D, red, M2 = dims(plans)
    tau, alpha = [], ZERO
    if any(plans[a].proven for a in act):
        tau = [ch.sample_ext() for _ in range(M)]
        alpha = ch.sample_ext()
    mu = ch.sample_ext()
    mup = sm._powers(mu, max(len(act), 1))
    claim = ZERO
    for j, a in enumerate(act):
        claim = ext_add(claim, ext_mul(ext_mul(mup[j], pow2(M - plans[a].m)), c.get(a, ZERO)))
    r = []
    for _ in range(M):
        s = [rd.ext() for _ in range(D)]
        ch.observe([x for e in s for x in e])
        ri = ch.sample_ext()
        claim = zm.interp([s[0], wm.ext_sub(claim, s[0])] + s[1:], ri)
        r.append(ri)
    vals = {a: [rd.ext() for _ in range(plans[a].n_val)] for a in act}
    ch.observe([x for a in act for e in vals[a] for x in e])
    rhs = ZERO
    for j, a in enumerate(act):
        pl = plans[a]
        ra = r[:pl.m]
        v = vals[a] + [zm.first_eval(ra), zm.last_eval(ra)]
        if pl.proven:
            v.append(gm.eq_eval(tau[:pl.m], ra))
        if pl.ints:
            v.append(gm.eq_eval(rho[:pl.m], ra))
        rhs = ext_add(rhs, ext_mul(mup[j], summand(pl, v, pvs[a], sm._powers(alpha, max(len(pl.proven), 1)), coef[a])))
    if rhs != claim:
        raise wm.WhirReject("batched sum-check claim")
    rp, u = [], {}
    if red:
        lp = sm._powers(ch.sample_ext(), sum(len(vals[a]) for a in red))
        claim, o, at = ZERO, 0, {}
        for a in red:
            at[a], acc = o, ZERO
            for x in vals[a]:
                acc = ext_add(acc, ext_mul(lp[o], x))
                o += 1
            claim = ext_add(claim, ext_mul(pow2(M2 - plans[a].m), acc))
        for _ in range(M2):
            s0, s2 = rd.ext(), rd.ext()
            ch.observe(s0 + s2)
            ri = ch.sample_ext()
            claim = wm._quad(s0, wm.ext_sub(claim, s0), s2, ri)
            rp.append(ri)
        for a in red:
            u[a] = [rd.ext() for _ in range(plans[a].w + plans[a].wp)]
        ch.observe([x for a in red for e in u[a] for x in e])
        want = ZERO
        for a in red:
            pl, ua, ub = plans[a], ZERO, ZERO
            w, nr, o = pl.w, len(pl.rot), at[a]
            for k in range(w):
                ua = ext_add(ua, ext_mul(lp[o + k], u[a][k]))
            for t, k in enumerate(pl.rot):
                ub = ext_add(ub, ext_mul(lp[o + w + t], u[a][k]))
            for k in range(pl.wp):
                ua = ext_add(ua, ext_mul(lp[o + w + nr + k], u[a][w + k]))
            for t, k in enumerate(pl.rot_p):
                ub = ext_add(ub, ext_mul(lp[o + w + nr + pl.wp + t], u[a][w + k]))
            ra, rpa = r[:pl.m], rp[:pl.m]
            want = ext_add(want, ext_add(ext_mul(ua, gm.eq_eval(ra, rpa)), ext_mul(ub, zm.rot_eval(ra, rpa))))
        if want != claim:
            raise wm.WhirReject("rotation claim")
    points, claimed, claimed_p = [], [], []
    for a, pl in enumerate(plans):
        nr = len(pl.rot)
        if a in red:
            points.append(rp[:pl.m]), claimed.append(u[a][:pl.w]), claimed_p.append(u[a][pl.w:])
        elif pl.active:
            points.append(r[:pl.m]), claimed.append(vals[a][:pl.w]), claimed_p.append(vals[a][pl.w + nr:pl.w + nr + pl.wp])
        else:
            points.append([ch.sample_ext() for _ in range(pl.m)]), claimed.append(None), claimed_p.append(None)
    # the main opening shows the common columns: the entries cw_a .. w_a - 1 of what is claimed
    opened = sm.verify(ch, params, root, S.heights, l, points, S.col_point, rd.take(sm.proof_words(params, S.heights, l)))
    col = 0
    for a, (pl, cl) in enumerate(zip(plans, claimed)):
        if cl is not None and opened[col:col + pl.w - S.cw[a]] != cl[S.cw[a]:]:
            raise wm.WhirReject("opened values")
        col += pl.w - S.cw[a]
    opened = sm.verify(ch, params, [int(x) for x in prep_root], S.heights_p, l_prep, [points[a] for a in S.prep_airs], S.col_point_p,
                       rd.take(sm.proof_words(params, S.heights_p, l_prep)))
    col = 0
    for a in S.prep_airs:
        pl = plans[a]
        if claimed_p[a] is not None and opened[col:col + pl.wp] != claimed_p[a]:
            raise wm.WhirReject("opened preprocessed values")
        col += pl.wp
    # every partition's opening against the root the proof sent: the first cw_a entries (an inactive AIR's own values stand)
    for a in S.cached_airs:
        opened = sm.verify(ch, params, croots[a], [plans[a].m] * S.cw[a], S.l_cached[a], [points[a]], [0] * S.cw[a],
                           rd.take(S.cached_words(params, a)))
        if claimed[a] is not None and opened != claimed[a][:S.cw[a]]:
            raise wm.WhirReject("opened cached values")
    cr = [croots[a] for a in S.cached_airs]
    return (root, pq, cr) if with_bus else (root, cr)
