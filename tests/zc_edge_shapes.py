"""Edge shapes of the AIR zero-check and the AIR-set proof (docs/boundary_tests.md), built with air.AirBuilder and shared by
tests/test_zc_edges_cpu.py and tests/test_gpu_zc_boundary.py.  A zero-check builder returns (air dict, satisfying trace, pvs) like
test_zerocheck_cpu's; an AIR-set builder returns a list of such triples.  Every builder checks its own trace with air.check_trace and
the plan it was written to reach (D, n_rot) with the model's Plan."""
import numpy as np

import airset_model as am
import zerocheck_model as zm
from pymodel import P
import boundary_inputs as bi
from test_airset_cpu import _bus_mix, _lookup
from test_zerocheck_cpu import _air, _fib, _table
from zkvm_prover_amd import air


def _done(b, m, tr, pvs, D=None, n_rot=None):
    a = _air(b, m)
    tr = np.asarray(tr, dtype=np.int64) % P
    assert tr.shape == (b.width, 1 << m) and air.check_trace(a["program"], tr.astype(np.uint32), pvs) == []
    pl = am.Plan(a) if getattr(b, "interactions", None) else zm.Plan(a)
    assert D is None or pl.D == D, (pl.D, D)
    assert n_rot is None or len(pl.rot) == n_rot
    return a, tr.tolist(), [int(x) for x in pvs]


def _cells(seed, shape, lo=0):
    return np.random.default_rng(seed).integers(lo, P, size=shape, dtype=np.int64)


# ---- the zero-check ----------------------------------------------------------------------------------------------------------------
def deg0(m, c=0x12345):
    """the only constraint is pub(0) - c: multilinear degree 0, D = 1; the column is read by nothing"""
    b = air.AirBuilder(1, 1)
    b.assert_zero(b.pub(0) - b.const(c))
    return _done(b, m, _cells(10 + m, (1, 1 << m)), [c], D=1, n_rot=0)


def deg1(m):
    """col0 - col1: D = 2, no rotation"""
    b = air.AirBuilder(2, 0)
    b.assert_zero(b.var(0) - b.var(1))
    c = _cells(20 + m, 1 << m)
    return _done(b, m, [c, c], [], D=2, n_rot=0)


def prod_builder(k):
    b = air.AirBuilder(k, 0)
    e = b.var(0)
    for j in range(1, k):
        e = e * b.var(j)
    b.assert_zero(e)
    return b


def prod(k, m):
    """the product of k cells, column k // 2 zero and every other cell non-zero: D = k + 1"""
    tr = _cells(30 + k + m, (k, 1 << m), lo=1)
    tr[k // 2] = 0
    return _done(prod_builder(k), m, tr, [], D=k + 1, n_rot=0)


def sel(kind, m):
    """one selector times cell 0 (D = 3); column 0 is zero only where the selector is not, so that a selector that is wrong on any
    row breaks the proof; column 1 is free"""
    b = air.AirBuilder(2, 0)
    s = {"first": b.is_first_row, "last": b.is_last_row, "trans": b.is_transition}[kind]()
    b.assert_zero(s * b.var(0))
    n = 1 << m
    tr = _cells(40 + m, (2, n), lo=1)
    rows = np.arange(n)
    tr[0, {"first": rows == 0, "last": rows == n - 1, "trans": rows != n - 1}[kind]] = 0
    assert (tr[0] != 0).any()
    return _done(b, m, tr, [], D=3, n_rot=0)


def all_rot_builder(w=3):
    b = air.AirBuilder(w, 0)
    for j in range(w):
        b.when_transition(b.next(j) - b.var(j) - b.var((j + 1) % w))
    return b


def all_rot(w, m):
    """col_j(r + 1) = col_j(r) + col_{j+1 mod w}(r) on the transition rows: every column is read at both rotations, n_rot = w"""
    n = 1 << m
    tr = np.zeros((w, n), dtype=np.int64)
    tr[:, 0] = _cells(50 + m, w)
    for r in range(1, n):
        tr[:, r] = (tr[:, r - 1] + np.roll(tr[:, r - 1], -1)) % P
    return _done(all_rot_builder(w), m, tr, [], D=3, n_rot=w)


def only_rot(m):
    """column 1 appears only as next(1), column 0 only at rotation 0: rot = [1]"""
    b = air.AirBuilder(2, 0)
    b.when_transition(b.next(1) - b.var(0))
    tr = _cells(60 + m, (2, 1 << m))
    tr[1, 1:] = tr[0, :-1]
    a = _done(b, m, tr, [], D=3, n_rot=1)
    assert zm.Plan(a[0]).rot == [1]
    return a


def width1(m, c=P - 2):
    """next(0) - var(0) on every row (the last one wraps to row 0): a constant column, w = n_rot = 1, D = 2"""
    b = air.AirBuilder(1, 0)
    b.assert_zero(b.next(0) - b.var(0))
    return _done(b, m, np.full((1, 1 << m), c), [], D=2, n_rot=1)


def _slots_expr(b, k):
    """x_i = var(0) + (i + 1); sum_i x_i^2 is computed first and every x_i is used again by sum_i x_i after it, so all k stay alive"""
    xs = [b.var(0) + (i + 1) for i in range(k)]
    sq, lin = xs[0] * xs[0], xs[0]
    for x in xs[1:]:
        sq, lin = sq + x * x, lin + x
    return sq + lin


def _slots_value(x, k):
    x = np.asarray(x, dtype=object)
    return sum((x + i + 1) ** 2 + (x + i + 1) for i in range(k)) % P


def slots(k, m=1):
    """a program that keeps about k intermediates alive: col1 = sum_i (x_i^2 + x_i), x_i = col0 + i + 1 (D = 3)"""
    b = air.AirBuilder(2, 0)
    b.assert_zero(_slots_expr(b, k) - b.var(1))
    c = _cells(70 + m, 1 << m)
    return _done(b, m, [c, _slots_value(c, k).astype(np.int64)], [], D=3, n_rot=0)


def slots_bus(k, m=1):
    """the same expression as the one field of a message the AIR sends and receives once per row: an interaction's operand program
    with about k live intermediates (d_bus = 2, D = 3), no constraint"""
    b = air.AirBuilder(1, 0)
    b.push_interaction(5, [_slots_expr(b, k)], 1, "send")
    b.push_interaction(5, [_slots_expr(b, k)], 1, "receive")
    return _done(b, m, _cells(80 + m, (1, 1 << m)), [], D=3, n_rot=0)


def many(count=64):
    """`count` AIRs of m in {1, 2, 3}, cycling Fibonacci, deg0, a lookup table (no proven constraint) and width1"""
    kinds = [_fib, deg0, _table, width1]
    items = [kinds[i % 4](1 + (i // 4) % 3) for i in range(count)]
    return [list(x) for x in zip(*items)]


ZC_SHAPES = {
    "deg0-m1": lambda: deg0(1), "deg0-m3": lambda: deg0(3), "deg1-m1": lambda: deg1(1), "deg1-m4": lambda: deg1(4),
    "prod6-m2": lambda: prod(6, 2), "prod7-m1": lambda: prod(7, 1), "prod7-m3": lambda: prod(7, 3),
    "all_rot3-m1": lambda: all_rot(3, 1), "all_rot3-m4": lambda: all_rot(3, 4),
    "only_rot-m1": lambda: only_rot(1), "only_rot-m3": lambda: only_rot(3),
    "width1-m1": lambda: width1(1), "width1-m4": lambda: width1(4),
    "slots40-m2": lambda: slots(40, 2),
}
ZC_SHAPES.update({"sel_%s-m%d" % (k, m): (lambda k=k, m=m: sel(k, m)) for k in ("first", "last", "trans") for m in (1, 2, 3)})


# ---- the AIR-set proof ---------------------------------------------------------------------------------------------------------------
def self_balanced(m, n_fields=1, bus=4):
    """ONE interaction that balances against itself: rows 2 i and 2 i + 1 send the same message with counts c_i and -c_i.  Columns:
    the fields, then the count"""
    b = air.AirBuilder(n_fields + 1, 0)
    b.push_interaction(bus, [b.var(i) for i in range(n_fields)], b.var(n_fields), "send")
    n = 1 << m
    tr = np.zeros((n_fields + 1, n), dtype=np.int64)
    tr[:n_fields] = np.repeat(_cells(90 + m + n_fields, (n_fields, n // 2)), 2, axis=1)
    c = _cells(91 + m, n // 2, lo=1)
    tr[n_fields, 0::2], tr[n_fields, 1::2] = c, P - c
    return _done(b, m, tr, [], D=2, n_rot=0)


def fields33_air(m=1):
    """an interaction of 33 fields (the builder itself refuses it, so it is appended past its check)"""
    b = air.AirBuilder(34, 0)
    b.push_interaction(4, [b.var(i) for i in range(32)], b.var(33), "send")
    bus, sign, count, fields = b.interactions[0]
    b.interactions[0] = (bus, sign, count, fields + [b.var(32)])
    return _air(b, m)


def lookup_heights(sender_ms, mt, order, seed=7):
    """senders of the given heights looking up one table of 2^mt rows; `order` places the AIRs (index len(sender_ms) is the table)"""
    rng = np.random.default_rng(seed)
    nt = 1 << mt
    keys = rng.permutation(1 << 20)[:nt].astype(np.int64)
    vals = (keys * keys + 1) % P
    mult = np.zeros(nt, dtype=np.int64)
    items = []
    for ms in sender_ms:
        pick = rng.integers(0, nt, size=1 << ms)
        mult += np.bincount(pick, minlength=nt)
        items.append(_done(air.lookup_sender_air(), ms, [keys[pick], vals[pick], rng.integers(0, P, size=1 << ms)], []))
    items.append(_done(air.lookup_table_air(), mt, [keys, vals, mult], []))
    return [items[i] for i in order]


def blocks_set():
    """heights 9, 8, 8, 7, 7, 7 (a block of 512 leaves, two of 256 and three of 128) in an AIR order that is not the block order"""
    return lookup_heights([8, 8, 7, 7, 7], 9, [2, 0, 5, 3, 1, 4])


AS_SHAPES = {
    # name: (items, log_stack, L, T)
    "L1": lambda: ([self_balanced(1)], 2, 1, 2),
    "no_pad": lambda: (_lookup(3, 3), 4, 4, 16),
    "blocks": lambda: (blocks_set(), 9, 11, 1408),
    "fields32-m1": lambda: ([self_balanced(1, 32)], 4, 1, 2),
    "fields32-m2": lambda: ([self_balanced(2, 32)], 4, 2, 4),
    "split": lambda: ([_fib(3), self_balanced(2), deg0(1)], 4, 2, 4),   # only constraints / only an interaction / D = 1 beside them
    "slots_bus20": lambda: ([slots_bus(20, 2)], 4, 3, 8),
}


def as_shape(name):
    """(airs, traces, pvs, log_stack, L); the layout is checked against what the shape was written to reach"""
    items, l, L, T = AS_SHAPES[name]()
    airs, traces, pvs = [list(x) for x in zip(*items)]
    blocks, T_, L_ = am.layout([am.Plan(a) for a in airs])
    assert (T_, L_) == (T, L), (T_, L_)
    if name == "blocks":
        assert sorted((b[2] for b in blocks), reverse=True) == [9, 8, 8, 7, 7, 7] and [b[0] for b in blocks] != sorted(b[0] for b in blocks)
    return airs, traces, pvs, l, L


# ---- operand families of the AIR-set proof (the GPU test and the CPU count of zero denominators run the same list) -------------------
SEED = 20240611
PV_POOL = [0, 1, P - 1, int(bi.raw_words([P - 1])[0])]   # canonical 0, 1, p-1 and the value whose Montgomery word is p-1
AS_FAMILY_CASES = [("bus_mix", 1), ("bus_mix", 3), ("bus_mix", 5), ("lookup", 1), ("lookup", 2), ("lookup", 5)]


class ZeroDenominator(Exception):
    pass


def no_zero_den(num, den):
    """am.prove's leaf hook: the model's GKR cannot invert a zero denominator"""
    if any(d == am.ZERO for d in den):
        raise ZeroDenominator()


def _count_variants(tr, col):
    """the trace with its count column at raw p-1 (multiplicity -1 on every row), canonical p-1 and zero"""
    out = []
    for name, v in (("raw p-1", PV_POOL[3]), ("canonical p-1", P - 1), ("zero", 0)):
        t = np.array(tr, dtype=np.uint32)
        t[col] = v
        out.append(("count " + name, t))
    return out


def as_family_case(kind, m):
    """(airs, index of the parameter set, [(name, traces, pvs, prefix)]) at log_stack 4"""
    if kind == "bus_mix":
        a, tr, _ = _bus_mix(m)
        rng = np.random.default_rng(SEED + 100 + m)
        fams = bi.families(rng, a["width"], 1 << m) + _count_variants(tr, 3)
        return [a], m % 2, [(name, [t], [[PV_POOL[i % 4]]], [m, i]) for i, (name, t) in enumerate(fams)]
    items = _lookup(m, m)
    rng = np.random.default_rng(SEED + 200 + m)
    fams = [(name, [t[:3], t[3:]]) for name, t in bi.families(rng, 6, 1 << m)]
    fams += [(name, [np.array(items[0][1], dtype=np.uint32), t]) for name, t in _count_variants(items[1][1], 2)]
    return [items[0][0], items[1][0]], (m + 1) % 2, [(name, [np.ascontiguousarray(t) for t in ts], [[], []], [m, i]) for i, (name, ts) in enumerate(fams)]
