"""Independent Python model of the keyed batched AIR-set proof (docs/airbatch.md, "The keyed batched form"): the statement of the keyed
AIR-set proof (with_bus) or keyed zero-check (without) of an AIR set with preprocessed columns, with ONE constraint sum-check and ONE
rotation reduction for the whole set and two stacked openings (the main commitment, then the key's).  Built on tests/keyed_model.py
(Plan, Shape, Key, the leaves), the helpers of tests/airbatch_model.py and below them the AIR-set, GKR, stacking and WHIR models.  It
imports nothing from the product.

Conventions as in zerocheck_model.  `preps` are the preprocessed columns the prover holds, per AIR (None / [] without a PREP section):
an honest prover's are the key's."""
import airbatch_model as bm
import airset_model as am
import gkr_model as gm
import keyed_model as km
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, ext_add, ext_mul

ZERO, ONE = wm.ZERO, wm.ONE
Refused = zm.Refused
Plan, Key, Shape = km.Plan, km.Key, km.Shape
pow2 = bm.pow2


def dims(plans):
    """(active AIRs, M, D, reducing AIRs, M'): an AIR reduces if n_rot + n_rot_p > 0"""
    act = [a for a, p in enumerate(plans) if p.active]
    red = [a for a in act if plans[a].reduces]
    return (act, max([plans[a].m for a in act], default=0), max([plans[a].D for a in act], default=0), red,
            max([plans[a].m for a in red], default=0))


def layout(S, with_bus):
    """word offsets of the parts before the openings: dict(o_b, o_rounds, o_vals, o_red, o_u, head, val_at, u_at)"""
    plans = S.plans
    act, M, D, red, M2 = dims(plans)
    o_b = 8 + (gm.proof_words(S.L) if with_bus else 0)
    o_rounds = o_b + (4 * sum(1 for p in plans if p.ints) if with_bus else 0)
    o_vals = o_rounds + 4 * D * M
    val_at, q = {}, o_vals
    for a in act:
        val_at[a], q = q, q + 4 * plans[a].n_val
    o_red = q
    o_u = o_red + (8 * M2 if red else 0)
    u_at, q = {}, o_u
    for a in red:
        u_at[a], q = q, q + 4 * (plans[a].w + plans[a].wp)
    return dict(o_b=o_b, o_rounds=o_rounds, o_vals=o_vals, o_red=o_red, o_u=o_u, head=q, val_at=val_at, u_at=u_at)


def proof_words(params, airs, l, l_prep, with_bus=True):
    try:
        S = Shape(params, airs, l, l_prep, with_bus)
    except Refused:
        return 0
    return layout(S, with_bus)["head"] + sm.proof_words(params, S.heights, l) + sm.proof_words(params, S.heights_p, l_prep)


def summand(plan, v, pvs, apow, coef):
    """g_a on one value of every table of the AIR: [w columns | n_rot next-row | w_p preprocessed | n_rot_p next-row | first | last |
    eq(tau_a, .) if it has proven constraints | eq(rho_a, .) if it has interactions]"""
    nv = plan.n_val
    e, acc = nv + 2, ZERO
    if plan.proven:
        acc = ext_mul(plan.combine(v, v[nv], v[nv + 1], pvs, apow), v[e])
        e += 1
    if plan.ints:
        acc = ext_add(acc, ext_mul(plan.bus_combine(v, pvs, coef), v[e]))
    return acc


def _ext_cols(plan, trace, prep):
    cols = [[gm.ext_c(int(v)) for v in c] for c in trace]
    pcols = [[gm.ext_c(int(v)) for v in c] for c in (prep or [])[:plan.wp]]
    return cols, pcols


def tables(plan, trace, prep, tau, rho):
    """the tables `summand` reads, over the AIR's own m variables (tau, rho: the common points; their prefixes are used)"""
    n = 1 << plan.m
    cols, pcols = _ext_cols(plan, trace, prep)
    tabs = cols + [cols[j][1:] + [cols[j][0]] for j in plan.rot] + pcols + [pcols[j][1:] + [pcols[j][0]] for j in plan.rot_p]
    tabs += [[ONE] + [ZERO] * (n - 1), [ZERO] * (n - 1) + [ONE]]
    if plan.proven:
        tabs.append(gm.eq_table(tau[:plan.m]))
    if plan.ints:
        tabs.append(gm.eq_table(rho[:plan.m]))
    return tabs


def prove(ch, params, airs, traces, preps, pvs, l, key, with_bus=True, weighted=True, leaf_hook=None):
    """The proof, continuing `ch` (after the caller's prefix): (root, words, info).  weighted=False (tests only): a prover that batches
    with mu^j alone, without the 2^(M - m_a) weights.  leaf_hook: as airset_model.prove's.  info: the challenges, every round polynomial at 0..D, the claims, the values,
    the layout's offsets, the offsets of the two openings."""
    S = Shape(params, airs, l, key.l_prep, with_bus)
    plans, n_airs = S.plans, len(airs)
    scom = sm.Commitment(params, [[int(v) % P for v in c] for tr in traces for c in tr], S.heights, l)
    ch.observe(list(key.root))
    words = []
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
    wgt = {a: ext_mul(mup[j], pow2(M - plans[a].m) if weighted else ONE) for j, a in enumerate(act)}
    g_end = {}   # a used-up AIR's g_a(r_a)
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
                k = ext_mul(ext_mul(mup[j], pow2(M - 1 - i) if weighted else ONE), g_end[a])
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
            cols, pcols = _ext_cols(pl, traces[a], preps[a])
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
            cols, pcols = _ext_cols(plans[a], traces[a], preps[a])
            us[a] = [gm.mle_eval(col, rp[:plans[a].m]) for col in cols + pcols]
        wm._observe(ch, [x for a in red for e in us[a] for x in e], words)
    # 9. the points
    points = []
    for a, pl in enumerate(plans):
        points.append(rp[:pl.m] if a in red else r[:pl.m] if pl.active else [ch.sample_ext() for _ in range(pl.m)])
    info.update(rp=rp, points=points, u=us, plans=plans, **layout(S, with_bus))
    # 10. the main opening, then the key's: on the PROVER's columns (a prover whose table differs from the key's commits to its own)
    _, op = sm.open_(scom, ch, points, S.col_point)
    pcols = [[int(v) % P for v in col] for a in S.prep_airs for col in preps[a][:plans[a].wp]]
    pcom = key.com if pcols == key.cols else sm.Commitment(params, pcols, S.heights_p, key.l_prep)
    _, op2 = sm.open_(pcom, ch, [points[a] for a in S.prep_airs], S.col_point_p)
    info.update(open_at=len(words), open2_at=len(words) + len(op))
    return list(scom.root), words + op + op2, info


def verify(ch, params, airs, prep_root, l_prep, pvs, l, words, with_bus=True):
    """Replays a proof on `ch` (after the caller's prefix).  Returns the root (with_bus: (root, (P, Q))); raises wm.WhirReject or
    gm.GkrReject (Refused for a refused shape)."""
    S = Shape(params, airs, l, l_prep, with_bus)
    plans, n_airs = S.plans, len(airs)
    words = [int(x) for x in words]
    if len(words) != proof_words(params, airs, l, l_prep, with_bus) or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    ch.observe([int(x) for x in prep_root])
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
    n1 = sm.proof_words(params, S.heights, l)
    opened = sm.verify(ch, params, root, S.heights, l, points, S.col_point, words[rd.pos:rd.pos + n1])
    col = 0
    for pl, cl in zip(plans, claimed):
        if cl is not None and opened[col:col + pl.w] != cl:
            raise wm.WhirReject("opened values")
        col += pl.w
    opened = sm.verify(ch, params, [int(x) for x in prep_root], S.heights_p, l_prep, [points[a] for a in S.prep_airs], S.col_point_p,
                       words[rd.pos + n1:])
    col = 0
    for a in S.prep_airs:
        pl = plans[a]
        if claimed_p[a] is not None and opened[col:col + pl.wp] != claimed_p[a]:
            raise wm.WhirReject("opened preprocessed values")
        col += pl.wp
    return (root, pq) if with_bus else root
