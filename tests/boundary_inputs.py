"""Structured inputs for the stage tests: what uniform random cells show a kernel about once in 2^31.

The device holds Montgomery words; upload() takes canonical values.  raw_words(r) gives the canonical values whose device words
are exactly r, so a test can put p-1, (p+-1)/2, MONTY_ONE or a multiple of 2^27 INTO device memory and still compare with the
canonical-form oracle."""
import numpy as np

from field_probe_ref import B, MONTY_ONE, P, RINV

CONST_WORDS = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, MONTY_ONE, P - MONTY_ONE]
_B = np.array(B, dtype=np.uint64)


def raw_words(r):
    """canonical c = r * 2^-32 mod p for raw words r in [0, p): upload(c) leaves exactly r in device memory"""
    r = np.asarray(r, dtype=np.uint64)
    assert (r < P).all()
    return ((r * np.uint64(RINV)) % np.uint64(P)).astype(np.uint32)


def boundary_cells(rng, shape):
    """raw words drawn from the boundary set B, as canonical values"""
    return raw_words(_B[rng.integers(0, len(_B), size=shape)])


def families(rng, width, n, small=False):
    """(name, [width, n] canonical uint32) pairs.  small=True keeps one member of each family (for the largest sizes)."""
    out = []
    for c in (CONST_WORDS[2:3] if small else CONST_WORDS):
        out.append(("const raw 0x%08x" % c, raw_words(np.full((width, n), c))))
    idx = np.arange(n)
    periods = sorted({2, 4, max(2, n // 2)} if n >= 2 else {2})
    for per in (periods[:1] if small else periods):
        hi = (idx % per) < max(1, per // 2)   # first half of each period p-1, second half 0
        raw = np.where(hi, P - 1, 0)
        out.append(("alternate raw p-1/0 period %d" % per, raw_words(np.broadcast_to(raw, (width, n)))))
    if not small:
        for per in (periods[0], periods[-1]):   # the canonical analogues: the oracle's own extremes
            hi = (idx % per) < max(1, per // 2)
            out.append(("alternate canonical p-1/0 period %d" % per, np.broadcast_to(np.where(hi, P - 1, 0), (width, n)).astype(np.uint32).copy()))
        for pos in sorted({0, n // 2, n - 1}):
            m = np.zeros((width, n), np.uint32)
            m[:, pos] = raw_words(np.full(width, P - 1))
            out.append(("delta at %d" % pos, m))
        m = np.zeros((width, n), np.uint32)
        m[width // 2] = boundary_cells(rng, n)
        out.append(("one non-zero column", m))
    out.append(("boundary", boundary_cells(rng, (width, n))))
    sp = rng.integers(0, P, size=(width, n), dtype=np.uint64).astype(np.uint32)
    sp[rng.random((width, n)) < 0.9] = 0
    out.append(("sparse", sp))
    return [(name, np.ascontiguousarray(m, dtype=np.uint32)) for name, m in out]


def ext_families(rng, n):
    """(name, [n, 4] canonical) tables of extension elements: all four coefficients raw p-1, constants, boundary coefficients, sparse"""
    out = [("all coefficients raw p-1", raw_words(np.full((n, 4), P - 1))),
           ("all coefficients canonical p-1", np.full((n, 4), P - 1, np.uint32)),
           ("constant raw (p+1)/2", raw_words(np.full((n, 4), (P + 1) // 2))),
           ("boundary", boundary_cells(rng, (n, 4)))]
    sp = rng.integers(0, P, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    sp[rng.random(n) < 0.9] = 0
    out.append(("sparse", sp))
    return out


def challenges(rng):
    """extension challenges with coefficients from B: all p-1, zero, one, a base-field element, random draws"""
    return [raw_words(np.full(4, P - 1)), np.zeros(4, np.uint32), np.array([1, 0, 0, 0], np.uint32), np.array([P - 1, 0, 0, 0], np.uint32),
            np.full(4, P - 1, np.uint32), boundary_cells(rng, 4), boundary_cells(rng, 4)]
