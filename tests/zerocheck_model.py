"""Independent Python model of the AIR zero-check over the stacked WHIR commitment (docs/zerocheck.md): what is proven of a program,
the rotation MLE, the prover and the verifier, built on tests/stacking_model.py, tests/whir_model.py, tests/gkr_model.py and
pymodel.Challenger.  It imports nothing from the product.

Conventions as in whir_model: extension elements are lists of 4 canonical ints, a table of 2^m entries is indexed by i = sum b_j 2^j
(z_0 the lowest bit), variables are bound lowest first, words on the wire are canonical.  An AIR is a dict with `program` (the
bytecode words), `log_height` and `width`; a trace is `width` lists of 2^log_height canonical ints."""
import gkr_model as gm
import stacking_model as sm
import whir_model as wm
from pymodel import P, ext_add, ext_mul, inv

ZERO, ONE = wm.ZERO, wm.ONE
AIR_MAGIC, PREP_MAGIC = 0x31414B5A, 0x50504B5A
VAR, PUB, CONST, FIRST, LAST, TRANS, ADD, SUB, MUL, NEG, PERM, CHAL, EXPOSED, PREP = range(14)
MAX_DEGREE = 8           # ZKHIP_ZEROCHECK_MAX_DEGREE
MAX_LOG_N = sm.WHIR_MAX_LOG_N


class Refused(Exception):
    """a shape the protocol does not take (ZKHIP_ERR_INVALID)"""


class Plan:
    """What is proven of one AIR: `proven` = the nodes of the constraints that reach no PERM / CHAL / EXPOSED leaf, in program order;
    d = their largest multilinear degree in the row index (cells, first, last, transition count 1), D = d + 1; `rot` = the columns they
    read with rotation 1, increasing."""

    def __init__(self, air):
        w = [int(x) for x in air["program"]]
        self.m, self.w = int(air["log_height"]), int(air["width"])
        if len(w) < 4 or w[0] != AIR_MAGIC or not 1 <= self.m <= MAX_LOG_N or self.w < 1:
            raise Refused("program or height")
        n_nodes, n_cons, self.n_pvs = w[1], w[2], w[3]
        self.nodes = [tuple(w[4 + 3 * i:7 + 3 * i]) for i in range(n_nodes)]
        cons = w[4 + 3 * n_nodes:4 + 3 * n_nodes + n_cons]
        end = 4 + 3 * n_nodes + n_cons
        if len(w) > end and w[end] == PREP_MAGIC:
            raise Refused("preprocessed columns")
        deg, later = [], []
        for op, a, b in self.nodes:
            if op in (VAR, FIRST, LAST, TRANS):
                deg.append(1), later.append(False)
            elif op in (PUB, CONST):
                deg.append(0), later.append(False)
            elif op in (ADD, SUB):
                deg.append(max(deg[a], deg[b])), later.append(later[a] or later[b])
            elif op == MUL:
                deg.append(deg[a] + deg[b]), later.append(later[a] or later[b])
            elif op == NEG:
                deg.append(deg[a]), later.append(later[a])
            else:
                deg.append(0), later.append(True)
        self.proven = [c for c in cons if not later[c]]
        self.d = max([deg[c] for c in self.proven], default=0)
        self.D = self.d + 1 if self.proven else 0
        if self.D > MAX_DEGREE:
            raise Refused("degree")
        reach, stack = set(), list(self.proven)
        while stack:
            i = stack.pop()
            if i in reach:
                continue
            reach.add(i)
            op, a, b = self.nodes[i]
            if op in (ADD, SUB, MUL):
                stack += [a, b]
            elif op == NEG:
                stack.append(a)
        self.reach = sorted(reach)
        self.rot = sorted({self.nodes[i][1] for i in self.reach if self.nodes[i][0] == VAR and self.nodes[i][2] == 1})

    def words(self):
        if not self.proven:
            return 0
        return 4 * self.D * self.m + 4 * self.w + 4 * len(self.rot) + (8 * self.m + 4 * self.w if self.rot else 0)

    def combine(self, cols, nexts, first, last, pvs, apow):
        """sum_k alpha^k C_k on one value of every column, of the rotated columns (in `rot` order), of first and last"""
        val = {}
        for i in self.reach:
            op, a, b = self.nodes[i]
            if op == VAR:
                val[i] = nexts[self.rot.index(a)] if b else cols[a]
            elif op == PUB:
                val[i] = gm.ext_c(int(pvs[a]))
            elif op == CONST:
                val[i] = gm.ext_c(a)
            elif op == FIRST:
                val[i] = first
            elif op == LAST:
                val[i] = last
            elif op == TRANS:
                val[i] = wm.ext_sub(ONE, last)
            elif op == ADD:
                val[i] = ext_add(val[a], val[b])
            elif op == SUB:
                val[i] = wm.ext_sub(val[a], val[b])
            elif op == MUL:
                val[i] = ext_mul(val[a], val[b])
            else:
                val[i] = wm.ext_sub(ZERO, val[a])
        acc = ZERO
        for ap, c in zip(apow, self.proven):
            acc = ext_add(acc, ext_mul(ap, val[c]))
        return acc


def shape(params, airs, l):
    """(plans, heights of the stacked columns, col_point); raises Refused"""
    if not 1 <= len(airs) <= sm.MAX_POINTS:
        raise Refused("AIR count")
    plans = [Plan(a) for a in airs]
    heights = [p.m for p in plans for _ in range(p.w)]
    col_point = [i for i, p in enumerate(plans) for _ in range(p.w)]
    if not sm.width(params, heights, l):
        raise Refused("stack shape")
    return plans, heights, col_point


def proof_words(params, airs, l):
    try:
        plans, heights, _ = shape(params, airs, l)
    except Refused:
        return 0
    return 8 + sum(p.words() for p in plans) + sm.proof_words(params, heights, l)


def first_eval(r):
    return gm.eq_eval([ZERO] * len(r), r)


def last_eval(r):
    return gm.eq_eval([ONE] * len(r), r)


def rot_eval(a, b):
    """the multilinear extension of the successor relation b = a + 1 mod 2^m:
    sum_k [prod_{j<k} a_j (1 - b_j)] (1 - a_k) b_k [prod_{j>k} eq(a_j, b_j)] + prod_j a_j (1 - b_j)"""
    m = len(a)
    lo = [ONE]
    for j in range(m):
        lo.append(ext_mul(lo[j], ext_mul(a[j], wm.ext_sub(ONE, b[j]))))
    acc = lo[m]
    for k in range(m):
        t = ext_mul(lo[k], ext_mul(wm.ext_sub(ONE, a[k]), b[k]))
        acc = ext_add(acc, ext_mul(t, gm.eq_eval(a[k + 1:], b[k + 1:])))
    return acc


def interp(s, x):
    """the polynomial of degree <= len(s) - 1 through (j, s[j]), at x"""
    n, acc = len(s), ZERO
    for j in range(n):
        num, den = ONE, 1
        for i in range(n):
            if i != j:
                num = ext_mul(num, wm.ext_sub(x, gm.ext_c(i)))
                den = den * (j - i) % P
        acc = ext_add(acc, ext_mul(wm.ext_scale(num, inv(den)), s[j]))
    return acc


def _at(a, b, t):
    """the line through (0, a), (1, b) at the integer t"""
    return ext_add(a, wm.ext_scale(wm.ext_sub(b, a), t))


def _fold_all(tabs, r):
    return [[gm.fold(t[2 * y], t[2 * y + 1], r) for y in range(len(t) // 2)] for t in tabs]


def _air_prove(ch, plan, trace, pvs, words, cyclic=True):
    """steps 2 - 4 for one AIR; returns its point r'"""
    m, w, D = plan.m, plan.w, plan.D
    n = 1 << m
    if not plan.proven:
        return [ch.sample_ext() for _ in range(m)]
    tau = [ch.sample_ext() for _ in range(m)]
    alpha = ch.sample_ext()
    apow = sm._powers(alpha, len(plan.proven))
    cols = [[gm.ext_c(int(v)) for v in c] for c in trace]
    nexts = [cols[j][1:] + [cols[j][0] if cyclic else ZERO] for j in plan.rot]
    first = [ONE] + [ZERO] * (n - 1)
    last = [ZERO] * (n - 1) + [ONE]
    tabs = cols + nexts + [first, last, gm.eq_table(tau)]
    nr = len(plan.rot)
    r = []
    for _ in range(m):
        pts = [0] + list(range(2, D + 1))
        s = [ZERO] * len(pts)
        for y in range(len(tabs[0]) // 2):
            for k, t in enumerate(pts):
                v = [_at(tb[2 * y], tb[2 * y + 1], t) for tb in tabs]
                c = plan.combine(v[:w], v[w:w + nr], v[w + nr], v[w + nr + 1], pvs, apow)
                s[k] = ext_add(s[k], ext_mul(c, v[w + nr + 2]))
        wm._observe(ch, [x for e in s for x in e], words)
        ri = ch.sample_ext()
        r.append(ri)
        tabs = _fold_all(tabs, ri)
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
        tabs = _fold_all(tabs, ri)
    u = [gm.mle_eval(c, rp) for c in cols]
    wm._observe(ch, [x for e in u for x in e], words)
    return rp


def prove(ch, params, airs, traces, pvs, l, cyclic=True):
    """The proof, continuing `ch` (after the caller's prefix): (root, words).  cyclic=False (tests only): the next-row tables of the
    zero-check take 0 after the last row instead of row 0."""
    plans, heights, col_point = shape(params, airs, l)
    cols = [[int(v) % P for v in c] for tr in traces for c in tr]
    scom = sm.Commitment(params, cols, heights, l)
    words = []
    wm._observe(ch, list(scom.root), words)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    points = [_air_prove(ch, pl, tr, pv, words, cyclic) for pl, tr, pv in zip(plans, traces, pvs)]
    _, op = sm.open_(scom, ch, points, col_point)
    return list(scom.root), words + op


def verify(ch, params, airs, pvs, l, words):
    """Replays a proof on `ch` (after the caller's prefix).  Returns the root; raises wm.WhirReject (Refused for a refused shape)."""
    plans, heights, col_point = shape(params, airs, l)
    words = [int(x) for x in words]
    if len(words) != proof_words(params, airs, l) or any(x < 0 or x >= P for x in words):
        raise wm.WhirReject("shape")
    rd = wm._Reader(words)
    root = rd.take(8)
    ch.observe(root)
    for pv in pvs:
        ch.observe([int(x) for x in pv])
    points, claimed = [], []
    for pl, pv in zip(plans, pvs):
        m, w, D, nr = pl.m, pl.w, pl.D, len(pl.rot)
        if not pl.proven:
            points.append([ch.sample_ext() for _ in range(m)])
            claimed.append(None)
            continue
        tau = [ch.sample_ext() for _ in range(m)]
        apow = sm._powers(ch.sample_ext(), len(pl.proven))
        claim, r = ZERO, []
        for _ in range(m):
            s = [rd.ext() for _ in range(D)]
            ch.observe([x for e in s for x in e])
            ri = ch.sample_ext()
            claim = interp([s[0], wm.ext_sub(claim, s[0])] + s[1:], ri)
            r.append(ri)
        v = [rd.ext() for _ in range(w + nr)]
        ch.observe([x for e in v for x in e])
        c = pl.combine(v[:w], v[w:], first_eval(r), last_eval(r), pv, apow)
        if ext_mul(gm.eq_eval(tau, r), c) != claim:
            raise wm.WhirReject("zero-check claim")
        if not nr:
            points.append(r), claimed.append(v)
            continue
        lp = sm._powers(ch.sample_ext(), w + nr)
        claim = ZERO
        for a, x in zip(lp, v):
            claim = ext_add(claim, ext_mul(a, x))
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
        if ext_add(ext_mul(ua, gm.eq_eval(r, rp)), ext_mul(ub, rot_eval(r, rp))) != claim:
            raise wm.WhirReject("rotation claim")
        points.append(rp), claimed.append(u)
    vals = sm.verify(ch, params, root, heights, l, points, col_point, words[rd.pos:])
    col = 0
    for pl, cl in zip(plans, claimed):
        if cl is not None and vals[col:col + pl.w] != cl:
            raise wm.WhirReject("opened values")
        col += pl.w
    return root
