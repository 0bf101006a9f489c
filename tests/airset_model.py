"""Independent Python model of the AIR-set proof (docs/airset.md): constraints and bus balance of a set of AIRs over one stacked WHIR
commitment -- the block layout of the LogUp leaves, the per-AIR leaf claims, the joint sum-check, the prover and the verifier, built on
tests/gkr_model.py, tests/stacking_model.py, tests/whir_model.py and tests/zerocheck_model.py.  It imports nothing from the product.

Conventions as in zerocheck_model: extension elements are lists of 4 canonical ints, a table of 2^m entries is indexed by
i = sum b_j 2^j (z_0 the lowest bit), variables are bound lowest first, words on the wire are canonical."""
import gkr_model as gm
import stacking_model as sm
import whir_model as wm
import zerocheck_model as zm
from pymodel import P, ext_add, ext_mul

ZERO, ONE = wm.ZERO, wm.ONE
Refused = zm.Refused
LOGUP_MAGIC, CACHED_MAGIC = 0x554C4B5A, 0x43414B5A
GKR_MAX_LOG_N = 28       # ZKHIP_GKR_MAX_LOG_N


class Plan(zm.Plan):
    """The zero-check's plan of one AIR plus its interactions: `ints` = (bus, sign, count node, field nodes) in program order, d_bus =
    the largest multilinear degree of a count or field node, D = max(d_cons, d_bus) + 1 over the parts that exist (0: not active)."""

    def __init__(self, air):
        super().__init__(air)
        w = [int(x) for x in air["program"]]
        q = 4 + 3 * w[1] + w[2]
        if len(w) > q and w[q] == CACHED_MAGIC:
            q += 2
        self.ints = []
        if len(w) > q:
            if w[q] != LOGUP_MAGIC:
                raise Refused("program")
            n_int, q = w[q + 1], q + 2
            for _ in range(n_int):
                bus, sign, count, nf = w[q:q + 4]
                self.ints.append((bus, sign, count, w[q + 4:q + 4 + nf]))
                q += 4 + nf + 1
        deg = []
        for op, a, b in self.nodes:
            if op in (zm.VAR, zm.FIRST, zm.LAST, zm.TRANS):
                deg.append(1)
            elif op in (zm.ADD, zm.SUB):
                deg.append(max(deg[a], deg[b]))
            elif op == zm.MUL:
                deg.append(deg[a] + deg[b])
            elif op == zm.NEG:
                deg.append(deg[a])
            else:
                deg.append(0)
        roots = [x for _, _, c, f in self.ints for x in [c] + f]
        self.d_bus = max([deg[x] for x in roots], default=0)
        parts = ([self.d] if self.proven else []) + ([self.d_bus] if self.ints else [])
        self.D = max(parts) + 1 if parts else 0
        if self.D > zm.MAX_DEGREE:
            raise Refused("degree")
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
        self.bus_reach = sorted(reach)

    @property
    def active(self):
        return self.D > 0

    def words(self):
        if not self.active:
            return 0
        return 4 * self.D * self.m + 4 * self.w + 4 * len(self.rot) + (8 * self.m + 4 * self.w if self.rot else 0)

    def bus_values(self, cols, pvs):
        """the value of every count and field node on one value of every column: [(count, [fields])] per interaction"""
        val = {}
        for i in self.bus_reach:
            op, a, b = self.nodes[i]
            if op == zm.VAR:
                val[i] = cols[a]
            elif op == zm.PUB:
                val[i] = gm.ext_c(int(pvs[a]))
            elif op == zm.CONST:
                val[i] = gm.ext_c(a)
            elif op == zm.ADD:
                val[i] = ext_add(val[a], val[b])
            elif op == zm.SUB:
                val[i] = wm.ext_sub(val[a], val[b])
            elif op == zm.MUL:
                val[i] = ext_mul(val[a], val[b])
            else:
                val[i] = wm.ext_sub(ZERO, val[a])
        return [(val[c], [val[x] for x in f]) for _, _, c, f in self.ints]

    def bus_combine(self, cols, pvs, coef):
        """sum_j (cc_j count_j + sum_i cf_{j,i} f_{j,i}) with coef = [(cc_j, [cf_{j,i}])]"""
        acc = ZERO
        for (c, fs), (cc, cfs) in zip(self.bus_values(cols, pvs), coef):
            acc = ext_add(acc, ext_mul(cc, c))
            for f, cf in zip(fs, cfs):
                acc = ext_add(acc, ext_mul(cf, f))
        return acc


def layout(plans):
    """Blocks (a, j, m, off), sorted stably by non-increasing height and laid end to end; T; L = max(1, ceil(log2 T))."""
    order = sorted(((a, j) for a, p in enumerate(plans) for j in range(len(p.ints))), key=lambda b: -plans[b[0]].m)
    blocks, off = [], 0
    for a, j in order:
        blocks.append((a, j, plans[a].m, off))
        off += 1 << plans[a].m
    return blocks, off, max(1, (off - 1).bit_length())


def shape(params, airs, l):
    """(plans, heights of the stacked columns, col_point, blocks, L); raises Refused"""
    if not 1 <= len(airs) <= sm.MAX_POINTS:
        raise Refused("AIR count")
    plans = [Plan(a) for a in airs]
    heights = [p.m for p in plans for _ in range(p.w)]
    col_point = [i for i, p in enumerate(plans) for _ in range(p.w)]
    if not sm.width(params, heights, l):
        raise Refused("stack shape")
    blocks, T, L = layout(plans)
    if not blocks:
        raise Refused("no interaction: zerocheck's case")
    if L > GKR_MAX_LOG_N:
        raise Refused("too many leaves")
    rows = {}
    for p in plans:
        for bus, _, _, _ in p.ints:
            rows[bus] = rows.get(bus, 0) + (1 << p.m)
            if rows[bus] >= P:
                raise Refused("bus counts")
    return plans, heights, col_point, blocks, L


def proof_words(params, airs, l):
    try:
        plans, heights, _, _, L = shape(params, airs, l)
    except Refused:
        return 0
    return 8 + gm.proof_words(L) + 4 * sum(1 for p in plans if p.ints) + sum(p.words() for p in plans) + sm.proof_words(params, heights, l)


def leaves(plans, blocks, L, traces, pvs, gamma, beta):
    """(num, den): num = +-count (canonical ints), den = gamma + (bus + 1) + sum_i beta^(i+1) f_i; padding (0, 1)"""
    num, den = [0] * (1 << L), [ONE] * (1 << L)
    bp = sm._powers(beta, 34)
    for a, j, m, off in blocks:
        pl = plans[a]
        bus, sign, _, _ = pl.ints[j]
        for x in range(1 << m):
            c, fs = pl.bus_values([gm.ext_c(int(col[x])) for col in traces[a]], pvs[a])[j]
            num[off + x] = (P - c[0]) % P if sign else c[0]
            d = ext_add(gamma, gm.ext_c(bus + 1))
            for i, f in enumerate(fs):
                d = ext_add(d, ext_mul(bp[i + 1], f))
            den[off + x] = d
    return num, den


def block_eq(blocks, rho):
    """e_b = eq(rho[m_b..L), the bits of off_b >> m_b)"""
    out = []
    for _, _, m, off in blocks:
        hi = rho[m:]
        out.append(gm.eq_eval(hi, [gm.ext_c((off >> m >> t) & 1) for t in range(len(hi))]))
    return out


def bus_coefs(plans, blocks, eb, beta, kappa):
    """per AIR [(e s_j, [kappa e beta^(i+1)])] in program order, and the constant kappa sum_j e_{a,j} (gamma-free part: bus_j + 1 and
    gamma are added by the caller through `const_of`)"""
    bp = sm._powers(beta, 34)
    coef = [[None] * len(p.ints) for p in plans]
    for (a, j, _, _), e in zip(blocks, eb):
        _, sign, _, fs = plans[a].ints[j]
        ke = ext_mul(kappa, e)
        coef[a][j] = (wm.ext_sub(ZERO, e) if sign else e, [ext_mul(ke, bp[i + 1]) for i in range(len(fs))])
    return coef


def const_of(plan, a, blocks, eb, gamma, kappa):
    """kappa sum_j e_{a,j} (gamma + bus_j + 1): the part of AIR a's denominators that leaves through the claim"""
    acc = ZERO
    for (a2, j, _, _), e in zip(blocks, eb):
        if a2 == a:
            acc = ext_add(acc, ext_mul(e, ext_add(gamma, gm.ext_c(plan.ints[j][0] + 1))))
    return ext_mul(kappa, acc)


def leaf_claims(plans, blocks, eb, rho, num, den, kappa):
    """B_a = sum_j e_{a,j} (num~_{a,j}(rho_a) + kappa den~_{a,j}(rho_a)) for every AIR with interactions, in order"""
    B = {}
    for (a, j, m, off), e in zip(blocks, eb):
        n_, d_ = gm.mle_eval(num[off:off + (1 << m)], rho[:m]), gm.mle_eval(den[off:off + (1 << m)], rho[:m])
        B[a] = ext_add(B.get(a, ZERO), ext_mul(e, ext_add(n_, ext_mul(kappa, d_))))
    return [B[a] for a in sorted(B)]


def _air_prove(ch, plan, trace, pvs, words, rho_a, coef):
    """steps 6 - 8 for one AIR; returns its point r'"""
    m, w, D = plan.m, plan.w, plan.D
    n = 1 << m
    if not plan.active:
        return [ch.sample_ext() for _ in range(m)]
    cols = [[gm.ext_c(int(v)) for v in c] for c in trace]
    nexts = [cols[j][1:] + [cols[j][0]] for j in plan.rot]
    tabs = cols + nexts + [[ONE] + [ZERO] * (n - 1), [ZERO] * (n - 1) + [ONE]]
    nr = len(plan.rot)
    if plan.proven:
        tau = [ch.sample_ext() for _ in range(m)]
        apow = sm._powers(ch.sample_ext(), len(plan.proven))
        tabs.append(gm.eq_table(tau))
    if plan.ints:
        tabs.append(gm.eq_table(rho_a))
    r = []
    for _ in range(m):
        pts = [0] + list(range(2, D + 1))
        s = [ZERO] * len(pts)
        for y in range(len(tabs[0]) // 2):
            for k, t in enumerate(pts):
                v = [zm._at(tb[2 * y], tb[2 * y + 1], t) for tb in tabs]
                e = w + nr + 2
                if plan.proven:
                    s[k] = ext_add(s[k], ext_mul(plan.combine(v[:w], v[w:w + nr], v[w + nr], v[w + nr + 1], pvs, apow), v[e]))
                    e += 1
                if plan.ints:
                    s[k] = ext_add(s[k], ext_mul(plan.bus_combine(v[:w], pvs, coef), v[e]))
        wm._observe(ch, [x for e in s for x in e], words)
        ri = ch.sample_ext()
        r.append(ri)
        tabs = zm._fold_all(tabs, ri)
    v = [tabs[j][0] for j in range(w + nr)]
    wm._observe(ch, [x for e in v for x in e], words)
    if not nr:
        return r
    lam = ch.sample_ext()
    lp = sm._powers(lam, w + nr)
    fa, fb = [ZERO] * n, [ZERO] * n
    for j in range(w):
        fa = [ext_add(x, ext_mul(lp[j], c)) for x, c in zip(fa, cols[j])]
    for t, j in enumerate(plan.rot):
        fb = [ext_add(x, ext_mul(lp[w + t], c)) for x, c in zip(fb, cols[j])]
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
    u = [gm.mle_eval(c, rp) for c in cols]
    wm._observe(ch, [x for e in u for x in e], words)
    return rp


def prove(ch, params, airs, traces, pvs, l, leaf_hook=None):
    """The proof, continuing `ch` (after the caller's prefix): (root, words, info).  leaf_hook (tests only): called with (num, den)
    before the GKR part and may change them in place -- the GKR part and the leaf claims then run on leaves that are not the
    committed traces'.  info: rho, (p*, q*), the leaf claims B_a, the leaves."""
    plans, heights, col_point, blocks, L = shape(params, airs, l)
    cols = [[int(v) % P for v in c] for tr in traces for c in tr]
    scom = sm.Commitment(params, cols, heights, l)
    words = []
    wm._observe(ch, list(scom.root), words)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    gamma, beta = gm.bus_challenges(ch)
    num, den = leaves(plans, blocks, L, traces, pvs, gamma, beta)
    if leaf_hook:
        leaf_hook(num, den)
    gw, rho, claims = gm.prove(ch, num, den)
    words += gw
    eb = block_eq(blocks, rho)
    kappa = ch.sample_ext()
    B = leaf_claims(plans, blocks, eb, rho, num, den, kappa)
    wm._observe(ch, [x for e in B for x in e], words)
    coef = bus_coefs(plans, blocks, eb, beta, kappa)
    points = [_air_prove(ch, pl, tr, pv, words, rho[:pl.m], cf) for pl, tr, pv, cf in zip(plans, traces, pvs, coef)]
    _, op = sm.open_(scom, ch, points, col_point)
    return list(scom.root), words + op, dict(rho=rho, claims=claims, B=B, num=num, den=den, L=L, blocks=blocks)


def verify(ch, params, airs, pvs, l, words):
    """Replays a proof on `ch` (after the caller's prefix).  Returns (root, (P, Q)); raises wm.WhirReject or gm.GkrReject (Refused for
    a refused shape)."""
    plans, heights, col_point, blocks, L = shape(params, airs, l)
    words = [int(x) for x in words]
    if len(words) != proof_words(params, airs, l) or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    root = rd.take(8)
    ch.observe(root)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    gamma, beta = gm.bus_challenges(ch)
    rho, (pstar, qstar), (rp_, rq_) = gm.verify(ch, rd.take(gm.proof_words(L)), L)
    if rp_ != ZERO or rq_ == ZERO:
        raise gm.GkrReject("unbalanced")
    eb = block_eq(blocks, rho)
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
    coef = bus_coefs(plans, blocks, eb, beta, kappa)
    points, claimed = [], []
    for a, (pl, pv) in enumerate(zip(plans, pvs)):
        m, w, D, nr = pl.m, pl.w, pl.D, len(pl.rot)
        if not pl.active:
            points.append([ch.sample_ext() for _ in range(m)])
            claimed.append(None)
            continue
        if pl.proven:
            tau = [ch.sample_ext() for _ in range(m)]
            apow = sm._powers(ch.sample_ext(), len(pl.proven))
        claim = wm.ext_sub(B[a], const_of(pl, a, blocks, eb, gamma, kappa)) if pl.ints else ZERO
        r = []
        for _ in range(m):
            s = [rd.ext() for _ in range(D)]
            ch.observe([x for e in s for x in e])
            ri = ch.sample_ext()
            claim = zm.interp([s[0], wm.ext_sub(claim, s[0])] + s[1:], ri)
            r.append(ri)
        v = [rd.ext() for _ in range(w + nr)]
        ch.observe([x for e in v for x in e])
        rhs = ZERO
        if pl.proven:
            rhs = ext_mul(gm.eq_eval(tau, r), pl.combine(v[:w], v[w:], zm.first_eval(r), zm.last_eval(r), pv, apow))
        if pl.ints:
            rhs = ext_add(rhs, ext_mul(gm.eq_eval(rho[:m], r), pl.bus_combine(v[:w], pv, coef[a])))
        if rhs != claim:
            raise wm.WhirReject("joint sum-check claim")
        if not nr:
            points.append(r), claimed.append(v)
            continue
        lp = sm._powers(ch.sample_ext(), w + nr)
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
        u = [rd.ext() for _ in range(w)]
        ch.observe([x for e in u for x in e])
        ua, ub = ZERO, ZERO
        for j in range(w):
            ua = ext_add(ua, ext_mul(lp[j], u[j]))
        for t, j in enumerate(pl.rot):
            ub = ext_add(ub, ext_mul(lp[w + t], u[j]))
        if ext_add(ext_mul(ua, gm.eq_eval(r, rp)), ext_mul(ub, zm.rot_eval(r, rp))) != claim:
            raise wm.WhirReject("rotation claim")
        points.append(rp), claimed.append(u)
    vals = sm.verify(ch, params, root, heights, l, points, col_point, words[rd.pos:])
    col = 0
    for pl, cl in zip(plans, claimed):
        if cl is not None and vals[col:col + pl.w] != cl:
            raise wm.WhirReject("opened values")
        col += pl.w
    return root, (rp_, rq_)
