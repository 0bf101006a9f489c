"""Independent Python model of the keyed zero-check and AIR-set proof (docs/zerocheck.md and docs/airset.md, "keyed form"): AIR sets
with preprocessed columns under a stacked commitment made once, the key.  It parses the PREP section itself (zerocheck_model raises
Refused on it), proves a PREP leaf like a main cell, sends v_p, v_p' and u_p, and opens the key's commitment after the main one.
Built on tests/zerocheck_model.py, tests/airset_model.py, tests/stacking_model.py, tests/whir_model.py and tests/gkr_model.py; it
imports nothing from the product.

Conventions as in zerocheck_model.  A key is made from `preps`: per AIR its preprocessed columns (lists of 2^m canonical ints), or
None / [] for an AIR without a PREP section."""
import airset_model as am
import gkr_model as gm
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, ext_add, ext_mul

ZERO, ONE = wm.ZERO, wm.ONE
Refused = zm.Refused


class Plan:
    """What is proven of one AIR in the keyed form.  A PREP leaf has degree 1 and is proven; `rot_p` = the preprocessed columns the
    proven constraints read with rotation 1, increasing; wp = the preprocessed width.  with_bus: the interactions join (airset_model's
    rule for D), else `ints` is empty."""

    def __init__(self, air, with_bus):
        w = [int(x) for x in air["program"]]
        self.m, self.w = int(air["log_height"]), int(air["width"])
        if len(w) < 4 or w[0] != zm.AIR_MAGIC or not 1 <= self.m <= zm.MAX_LOG_N or self.w < 1:
            raise Refused("program or height")
        n_nodes, n_cons, self.n_pvs = w[1], w[2], w[3]
        self.nodes = [tuple(w[4 + 3 * i:7 + 3 * i]) for i in range(n_nodes)]
        q = 4 + 3 * n_nodes
        cons, q = w[q:q + n_cons], q + n_cons
        self.wp = 0
        if len(w) > q and w[q] == zm.PREP_MAGIC:
            self.wp, q = w[q + 1], q + 2
        if len(w) > q and w[q] == am.CACHED_MAGIC:
            q += 2
        self.ints = []
        if len(w) > q:
            if w[q] != am.LOGUP_MAGIC:
                raise Refused("program")
            n_int, q = w[q + 1], q + 2
            for _ in range(n_int):
                bus, sign, count, nf = w[q:q + 4]
                if with_bus:
                    self.ints.append((bus, sign, count, w[q + 4:q + 4 + nf]))
                q += 4 + nf + 1
        deg, later = [], []
        for op, a, b in self.nodes:
            if op in (zm.VAR, zm.PREP, zm.FIRST, zm.LAST, zm.TRANS):
                deg.append(1), later.append(False)
            elif op in (zm.PUB, zm.CONST):
                deg.append(0), later.append(False)
            elif op in (zm.ADD, zm.SUB):
                deg.append(max(deg[a], deg[b])), later.append(later[a] or later[b])
            elif op == zm.MUL:
                deg.append(deg[a] + deg[b]), later.append(later[a] or later[b])
            elif op == zm.NEG:
                deg.append(deg[a]), later.append(later[a])
            else:
                deg.append(0), later.append(True)
        self.proven = [c for c in cons if not later[c]]
        self.d = max([deg[c] for c in self.proven], default=0)
        self.reach = self._reach(self.proven)
        self.rot = sorted({self.nodes[i][1] for i in self.reach if self.nodes[i][0] == zm.VAR and self.nodes[i][2] == 1})
        self.rot_p = sorted({self.nodes[i][1] for i in self.reach if self.nodes[i][0] == zm.PREP and self.nodes[i][2] == 1})
        roots = [x for _, _, c, f in self.ints for x in [c] + f]
        self.d_bus = max([deg[x] for x in roots], default=0)
        self.bus_reach = self._reach(roots)
        parts = ([self.d] if self.proven else []) + ([self.d_bus] if self.ints else [])
        self.D = max(parts) + 1 if parts else 0
        if self.D > zm.MAX_DEGREE:
            raise Refused("degree")

    def _reach(self, roots):
        reach, stack = set(), list(roots)
        while stack:
            i = stack.pop()
            if i in reach:
                continue
            reach.add(i)
            op, a, b = self.nodes[i]
            if op in (zm.ADD, zm.SUB, zm.MUL):
                stack += [a, b]
            elif op == zm.NEG:
                stack.append(a)
        return sorted(reach)

    @property
    def active(self):
        return self.D > 0

    @property
    def n_val(self):
        return self.w + len(self.rot) + self.wp + len(self.rot_p)

    @property
    def reduces(self):
        return bool(self.rot or self.rot_p)

    def words(self):
        if not self.active:
            return 0
        return 4 * self.D * self.m + 4 * self.n_val + (8 * self.m + 4 * (self.w + self.wp) if self.reduces else 0)

    def split(self, v):
        """[v | v' | v_p | v_p'] of one list of n_val values"""
        a, b, c = self.w, self.w + len(self.rot), self.w + len(self.rot) + self.wp
        return v[:a], v[a:b], v[b:c], v[c:self.n_val]

    def values(self, reach, v, first, last, pvs):
        """every node in `reach` on one value of every table, v = [cols | nexts | preps | prep nexts]"""
        cols, nexts, preps, pnexts = self.split(v)
        val = {}
        for i in reach:
            op, a, b = self.nodes[i]
            if op == zm.VAR:
                val[i] = nexts[self.rot.index(a)] if b else cols[a]
            elif op == zm.PREP:
                val[i] = pnexts[self.rot_p.index(a)] if b else preps[a]
            elif op == zm.PUB:
                val[i] = gm.ext_c(int(pvs[a]))
            elif op == zm.CONST:
                val[i] = gm.ext_c(a)
            elif op == zm.FIRST:
                val[i] = first
            elif op == zm.LAST:
                val[i] = last
            elif op == zm.TRANS:
                val[i] = wm.ext_sub(ONE, last)
            elif op == zm.ADD:
                val[i] = ext_add(val[a], val[b])
            elif op == zm.SUB:
                val[i] = wm.ext_sub(val[a], val[b])
            elif op == zm.MUL:
                val[i] = ext_mul(val[a], val[b])
            else:
                val[i] = wm.ext_sub(ZERO, val[a])
        return val

    def combine(self, v, first, last, pvs, apow):
        """sum_k alpha^k C_k"""
        val = self.values(self.reach, v, first, last, pvs)
        acc = ZERO
        for ap, c in zip(apow, self.proven):
            acc = ext_add(acc, ext_mul(ap, val[c]))
        return acc

    def bus_values(self, v, pvs):
        """[(count, [fields])] per interaction; operands read the current row only, so first and last do not enter"""
        val = self.values(self.bus_reach, v, ZERO, ZERO, pvs)
        return [(val[c], [val[x] for x in f]) for _, _, c, f in self.ints]

    def bus_combine(self, v, pvs, coef):
        acc = ZERO
        for (c, fs), (cc, cfs) in zip(self.bus_values(v, pvs), coef):
            acc = ext_add(acc, ext_mul(cc, c))
            for f, cf in zip(fs, cfs):
                acc = ext_add(acc, ext_mul(cf, f))
        return acc


class Shape:
    def __init__(self, params, airs, l, l_prep, with_bus):
        if not 1 <= len(airs) <= sm.MAX_POINTS:
            raise Refused("AIR count")
        self.plans = plans = [Plan(a, with_bus) for a in airs]
        self.heights = [p.m for p in plans for _ in range(p.w)]
        self.col_point = [i for i, p in enumerate(plans) for _ in range(p.w)]
        if not sm.width(params, self.heights, l):
            raise Refused("stack shape")
        self.prep_airs = [a for a, p in enumerate(plans) if p.wp]
        if not self.prep_airs:
            raise Refused("no PREP: the unkeyed calls' case")
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
        self.words = (8 + (gm.proof_words(self.L) + 4 * sum(1 for p in plans if p.ints) if with_bus else 0) + sum(p.words() for p in plans)
                      + sm.proof_words(params, self.heights, l) + sm.proof_words(params, self.heights_p, l_prep))


def proof_words(params, airs, l, l_prep, with_bus=True):
    try:
        return Shape(params, airs, l, l_prep, with_bus).words
    except Refused:
        return 0


class Key:
    """the stacked commitment of every preprocessed column of the set, AIRs in caller order, columns in column order"""

    def __init__(self, params, airs, preps, l_prep):
        self.cols, heights = [], []
        for a, pr in zip(airs, preps):
            wp = Plan(a, False).wp
            if wp and not pr:
                raise Refused("a PREP AIR without a preprocessed trace")
            for c in (pr or [])[:wp]:
                if any(int(x) >= P for x in c):
                    raise Refused("not canonical")
                self.cols.append([int(x) for x in c]), heights.append(int(a["log_height"]))
        if not heights or not sm.width(params, heights, l_prep):
            raise Refused("key stack shape")
        self.l_prep = l_prep
        self.com = sm.Commitment(params, self.cols, heights, l_prep)
        self.root = list(self.com.root)


def leaves(S, traces, preps, pvs, gamma, beta):
    num, den = [0] * (1 << S.L), [ONE] * (1 << S.L)
    bp = sm._powers(beta, 34)
    for a, j, m, off in S.blocks:
        pl = S.plans[a]
        bus, sign, _, _ = pl.ints[j]
        for x in range(1 << m):
            v = [gm.ext_c(int(c[x])) for c in traces[a]] + [ZERO] * len(pl.rot) + [gm.ext_c(int(c[x])) for c in (preps[a] or [])[:pl.wp]]
            c, fs = pl.bus_values(v + [ZERO] * len(pl.rot_p), pvs[a])[j]
            num[off + x] = (P - c[0]) % P if sign else c[0]
            d = ext_add(gamma, gm.ext_c(bus + 1))
            for i, f in enumerate(fs):
                d = ext_add(d, ext_mul(bp[i + 1], f))
            den[off + x] = d
    return num, den


def _air_prove(ch, pl, trace, prep, pvs, words, rho_a, coef, info):
    m, w, D = pl.m, pl.w, pl.D
    n = 1 << m
    if not pl.active:
        return [ch.sample_ext() for _ in range(m)]
    cols = [[gm.ext_c(int(v)) for v in c] for c in trace]
    pcols = [[gm.ext_c(int(v)) for v in c] for c in (prep or [])[:pl.wp]]
    vals = cols + [cols[j][1:] + [cols[j][0]] for j in pl.rot] + pcols + [pcols[j][1:] + [pcols[j][0]] for j in pl.rot_p]
    nv = pl.n_val
    tabs = vals + [[ONE] + [ZERO] * (n - 1), [ZERO] * (n - 1) + [ONE]]
    if pl.proven:
        tau = [ch.sample_ext() for _ in range(m)]
        apow = sm._powers(ch.sample_ext(), len(pl.proven))
        tabs.append(gm.eq_table(tau))
    if pl.ints:
        tabs.append(gm.eq_table(rho_a))
    r = []
    for _ in range(m):
        pts = [0] + list(range(2, D + 1))
        s = [ZERO] * len(pts)
        for y in range(len(tabs[0]) // 2):
            for k, t in enumerate(pts):
                v = [zm._at(tb[2 * y], tb[2 * y + 1], t) for tb in tabs]
                e = nv + 2
                if pl.proven:
                    s[k] = ext_add(s[k], ext_mul(pl.combine(v, v[nv], v[nv + 1], pvs, apow), v[e]))
                    e += 1
                if pl.ints:
                    s[k] = ext_add(s[k], ext_mul(pl.bus_combine(v, pvs, coef), v[e]))
        wm._observe(ch, [x for e in s for x in e], words)
        ri = ch.sample_ext()
        r.append(ri)
        tabs = zm._fold_all(tabs, ri)
    v = [tabs[j][0] for j in range(nv)]
    info["v"] = v
    info["r"] = r
    wm._observe(ch, [x for e in v for x in e], words)
    if not pl.reduces:
        return r
    lp = sm._powers(ch.sample_ext(), nv)
    nr = len(pl.rot)
    fa, fb = [ZERO] * n, [ZERO] * n
    for j in range(w):
        fa = [ext_add(x, ext_mul(lp[j], c)) for x, c in zip(fa, cols[j])]
    for t, j in enumerate(pl.rot):
        fb = [ext_add(x, ext_mul(lp[w + t], c)) for x, c in zip(fb, cols[j])]
    for j in range(pl.wp):
        fa = [ext_add(x, ext_mul(lp[w + nr + j], c)) for x, c in zip(fa, pcols[j])]
    for t, j in enumerate(pl.rot_p):
        fb = [ext_add(x, ext_mul(lp[w + nr + pl.wp + t], c)) for x, c in zip(fb, pcols[j])]
    e = gm.eq_table(r)
    tabs = [fa, e, fb, [e[(x - 1) % n] for x in range(n)]]
    rp = []
    for _ in range(m):
        s0a, s2a = wm._sumcheck_round(tabs[0], tabs[1])
        s0b, s2b = wm._sumcheck_round(tabs[2], tabs[3])
        wm._observe(ch, ext_add(s0a, s0b) + ext_add(s2a, s2b), words)
        ri = ch.sample_ext()
        rp.append(ri)
        tabs = zm._fold_all(tabs, ri)
    u = [gm.mle_eval(c, rp) for c in cols + pcols]
    info["u"] = u
    wm._observe(ch, [x for e in u for x in e], words)
    return rp


def prove(ch, params, airs, traces, preps, pvs, l, key, with_bus=True):
    """The keyed proof, continuing `ch` (after the caller's prefix): (root, words, info).  `preps` are the columns the prover holds:
    an honest prover's are the key's.  info: per AIR its offset in the words, r, v (all n_val values), u (w + w_p values, if the
    reduction ran) and r'; the offsets of the two openings."""
    S = Shape(params, airs, l, key.l_prep, with_bus)
    cols = [[int(v) % P for v in c] for tr in traces for c in tr]
    scom = sm.Commitment(params, cols, S.heights, l)
    ch.observe(list(key.root))
    words = []
    wm._observe(ch, list(scom.root), words)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    rho, coef = [], [None] * len(airs)
    if with_bus:
        gamma, beta = gm.bus_challenges(ch)
        num, den = leaves(S, traces, preps, pvs, gamma, beta)
        gw, rho, _ = gm.prove(ch, num, den)
        words += gw
        eb = am.block_eq(S.blocks, rho)
        kappa = ch.sample_ext()
        B = am.leaf_claims(S.plans, S.blocks, eb, rho, num, den, kappa)
        wm._observe(ch, [x for e in B for x in e], words)
        coef = am.bus_coefs(S.plans, S.blocks, eb, beta, kappa)
    points, infos = [], []
    for pl, tr, pr, pv, cf in zip(S.plans, traces, preps, pvs, coef):
        info = {"at": len(words)}
        points.append(_air_prove(ch, pl, tr, pr, pv, words, rho[:pl.m], cf, info))
        info["rp"] = points[-1]
        infos.append(info)
    _, op = sm.open_(scom, ch, points, S.col_point)
    # the key's opening runs on the PROVER's columns: a prover whose table differs from the key's commits to its own
    pcols = [[int(v) % P for v in c] for a in S.prep_airs for c in preps[a][:S.plans[a].wp]]
    pcom = key.com if pcols == key.cols else sm.Commitment(params, pcols, S.heights_p, key.l_prep)
    _, op2 = sm.open_(pcom, ch, [points[a] for a in S.prep_airs], S.col_point_p)
    return list(scom.root), words + op + op2, dict(airs=infos, open_at=len(words), open2_at=len(words) + len(op), plans=S.plans)


def verify(ch, params, airs, prep_root, l_prep, pvs, l, words, with_bus=True):
    """Replays a keyed proof on `ch` (after the caller's prefix).  Returns the root (with_bus: (root, (P, Q))); raises wm.WhirReject
    or gm.GkrReject (Refused for a refused shape)."""
    S = Shape(params, airs, l, l_prep, with_bus)
    words = [int(x) for x in words]
    if len(words) != S.words or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    ch.observe([int(x) for x in prep_root])
    root = rd.take(8)
    ch.observe(root)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    pq = None
    if with_bus:
        gamma, beta = gm.bus_challenges(ch)
        rho, (pstar, qstar), pq = gm.verify(ch, rd.take(gm.proof_words(S.L)), S.L)
        if pq[0] != ZERO or pq[1] == ZERO:
            raise gm.GkrReject("unbalanced")
        eb = am.block_eq(S.blocks, rho)
        kappa = ch.sample_ext()
        with_ints = [a for a, p in enumerate(S.plans) if p.ints]
        B = {a: rd.ext() for a in with_ints}
        ch.observe([x for a in with_ints for x in B[a]])
        lhs, pad = ZERO, ONE
        for a in with_ints:
            lhs = ext_add(lhs, B[a])
        for e in eb:
            pad = wm.ext_sub(pad, e)
        if ext_add(lhs, ext_mul(kappa, pad)) != ext_add(pstar, ext_mul(kappa, qstar)):
            raise wm.WhirReject("leaf claims")
        coef = am.bus_coefs(S.plans, S.blocks, eb, beta, kappa)
    points, claimed, claimed_p = [], [], []
    for a, (pl, pv) in enumerate(zip(S.plans, pvs)):
        m, w, D, nv, nr = pl.m, pl.w, pl.D, pl.n_val, len(pl.rot)
        if not pl.active:
            points.append([ch.sample_ext() for _ in range(m)])
            claimed.append(None), claimed_p.append(None)
            continue
        if pl.proven:
            tau = [ch.sample_ext() for _ in range(m)]
            apow = sm._powers(ch.sample_ext(), len(pl.proven))
        claim = wm.ext_sub(B[a], am.const_of(pl, a, S.blocks, eb, gamma, kappa)) if pl.ints else ZERO
        r = []
        for _ in range(m):
            s = [rd.ext() for _ in range(D)]
            ch.observe([x for e in s for x in e])
            ri = ch.sample_ext()
            claim = zm.interp([s[0], wm.ext_sub(claim, s[0])] + s[1:], ri)
            r.append(ri)
        v = [rd.ext() for _ in range(nv)]
        ch.observe([x for e in v for x in e])
        rhs = ZERO
        if pl.proven:
            rhs = ext_mul(gm.eq_eval(tau, r), pl.combine(v, zm.first_eval(r), zm.last_eval(r), pv, apow))
        if pl.ints:
            rhs = ext_add(rhs, ext_mul(gm.eq_eval(rho[:m], r), pl.bus_combine(v, pv, coef[a])))
        if rhs != claim:
            raise wm.WhirReject("sum-check claim")
        if not pl.reduces:
            points.append(r), claimed.append(v[:w]), claimed_p.append(v[w + nr:w + nr + pl.wp])
            continue
        lp = sm._powers(ch.sample_ext(), nv)
        claim = ZERO
        for c, x in zip(lp, v):
            claim = ext_add(claim, ext_mul(c, x))
        rp = []
        for _ in range(m):
            s0, s2 = rd.ext(), rd.ext()
            ch.observe(s0 + s2)
            ri = ch.sample_ext()
            claim = wm._quad(s0, wm.ext_sub(claim, s0), s2, ri)
            rp.append(ri)
        u = [rd.ext() for _ in range(w + pl.wp)]
        ch.observe([x for e in u for x in e])
        ua, ub = ZERO, ZERO
        for j in range(w):
            ua = ext_add(ua, ext_mul(lp[j], u[j]))
        for t, j in enumerate(pl.rot):
            ub = ext_add(ub, ext_mul(lp[w + t], u[j]))
        for j in range(pl.wp):
            ua = ext_add(ua, ext_mul(lp[w + nr + j], u[w + j]))
        for t, j in enumerate(pl.rot_p):
            ub = ext_add(ub, ext_mul(lp[w + nr + pl.wp + t], u[w + j]))
        if ext_add(ext_mul(ua, gm.eq_eval(r, rp)), ext_mul(ub, zm.rot_eval(r, rp))) != claim:
            raise wm.WhirReject("rotation claim")
        points.append(rp), claimed.append(u[:w]), claimed_p.append(u[w:])
    n1 = sm.proof_words(params, S.heights, l)
    vals = sm.verify(ch, params, root, S.heights, l, points, S.col_point, words[rd.pos:rd.pos + n1])
    col = 0
    for pl, cl in zip(S.plans, claimed):
        if cl is not None and vals[col:col + pl.w] != cl:
            raise wm.WhirReject("opened values")
        col += pl.w
    vals = sm.verify(ch, params, [int(x) for x in prep_root], S.heights_p, l_prep, [points[a] for a in S.prep_airs], S.col_point_p,
                     words[rd.pos + n1:])
    col = 0
    for a in S.prep_airs:
        pl = S.plans[a]
        if claimed_p[a] is not None and vals[col:col + pl.wp] != claimed_p[a]:
            raise wm.WhirReject("opened preprocessed values")
        col += pl.wp
    return (root, pq) if with_bus else root
