"""CPU: the FRI final-polynomial chip (air.fri_final_air: a query's last check, Horner over the final polynomial's coefficients at the
query's point).  The host function equals the twin and refuses what it must with nothing written; its point is the inverse square of what
the domain-point chip holds; the twin's traces satisfy the AIR and every constraint family refuses the trace that breaks it, a call of
L - 1 or L + 1 rows included; the honest low-degree FRI instance ends on its own interpolated final polynomial; the C++ twin of the AIR
emits the same program; the host function runs clean under the sanitizers as a stand-alone program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_final_util as ff  # noqa: E402
import fri_query_util as fq  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOPV = np.zeros(0, np.uint32)
P = ff.P
SETS = ff.call_sets("cpu")
BUSES = (14, 17)


def _prog(lfp, coeff_bus=18):
    return air.fri_final_air(lfp, *BUSES, coeff_bus).program()


def test_widths_agree():
    assert air.FRI_FINAL_WIDTH == z.FRI_FINAL_WIDTH == ff.WIDTH == 19


def _host_cases():
    rng = np.random.default_rng(1)
    for lfp in (0, 1, 3, 8):
        L = 1 << lfp
        seeded = rng.integers(0, P, (L, 4), dtype=np.int64)
        for lvl in (1, 12, 26):
            for k in sorted({0, 1, (1 << lvl) - 1, int(rng.integers(0, 1 << lvl))}):
                for coef in (np.zeros((L, 4), np.int64), np.full((L, 4), P - 1), seeded):
                    yield lfp, lvl, k, coef


def test_host_function_equals_the_twin():
    n = 0
    for lfp, lvl, k, coef in _host_cases():
        x, val = z.fri_final_host(lfp, lvl, k, coef)
        wx, wval = ff.value_int(coef, lvl, k)
        assert (x, val.tolist()) == (wx, wval), (lfp, lvl, k)
        if k == 0:
            assert x == 1
        if k == 1:
            assert x == P - 1
        n += 1
    assert n >= 4 * 3 * 3 * 3 - 12


def test_host_function_refuses_with_the_outputs_untouched():
    lib = z.load_library()
    u = lambda v: np.ascontiguousarray(v, dtype=np.uint32).reshape(-1).ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    rng = np.random.default_rng(2)
    coef = rng.integers(0, P, (8, 4), dtype=np.int64).astype(np.uint32)
    big = rng.integers(0, P, (512, 4), dtype=np.int64).astype(np.uint32)
    x, val = np.full(1, 77, np.uint32), np.full(4, 78, np.uint32)

    def call(lfp=3, lvl=5, k=19, coef=coef, x=x, val=val):
        return lib.zkhip_fri_final_host(lfp, lvl, k, None if coef is None else u(coef), None if x is None else u(x), None if val is None else u(val))
    assert call(coef=None) == -3 and call(x=None) == -3 and call(val=None) == -3
    assert call(lfp=9, coef=big) == -3 and call(lfp=(1 << 32) - 1, coef=big) == -3
    assert call(lvl=0, k=0) == -3 and call(lvl=27) == -3 and call(lvl=(1 << 32) - 1) == -3
    assert call(k=32) == -3 and call(k=1 << 32) == -3 and call(k=(1 << 64) - 1) == -3 and call(lvl=26, k=1 << 26) == -3
    for pos, v in ((0, P), (31, P), (13, 0xFFFFFFFF)):
        w = coef.copy()
        w.reshape(-1)[pos] = v
        assert call(coef=w) == -3
    assert x[0] == 77 and (val == 78).all()                       # nothing written by any refusal
    assert call(k=31) == 0 and call(lvl=26, k=(1 << 26) - 1) == 0 and call(lfp=8, coef=big) == 0
    assert call() == 0 and (int(x[0]), val.tolist()) == ff.value_int(coef, 5, 19)
    with pytest.raises(z.ZkhipError):
        z.fri_final_host(3, 5, 32, coef)
    with pytest.raises(z.ZkhipError):
        z.fri_final_host(2, 5, 3, coef)                           # eight coefficients are not 2^2


def test_the_point_is_the_inverse_square_of_the_domain_point_chips():
    """x from the host function times (the domain-point twin's x_inv)^2 is 1 at every lvl: the squaring identity the chip's line 8 states"""
    rng = np.random.default_rng(3)
    assert fq.WINV == air.domain_point_inverse_roots()
    for lvl in range(1, 27):
        for k in {0, 1, (1 << lvl) - 1, int(rng.integers(0, 1 << lvl)), int(rng.integers(0, 1 << lvl))}:
            x, _ = z.fri_final_host(0, lvl, k, [1, 2, 3, 4])
            assert x == ff.point(k, lvl) and x * fq.x_inv(k) ** 2 % P == 1, (lvl, k)


def test_the_two_forms_of_the_twin_agree_with_the_host_function():
    for name, s in ff.call_sets().items():
        tr, val = ff.trace(s)
        L = 1 << s["lfp"]
        calls = range(len(s["k"])) if len(s["k"]) <= 32 else range(0, len(s["k"]), 17)
        for c in calls:
            k, lvl, coef = int(s["k"][c]), int(s["lvl"][c]), s["coef"][int(s["poly"][c])]
            x, want = ff.value_int(coef, lvl, k)
            hx, hval = z.fri_final_host(s["lfp"], lvl, k, coef)
            assert (hx, hval.tolist()) == (x, want) and val[c].tolist() == want, (name, c)
            r = c * L + L - 1
            assert tr[ff.ACC:ff.ACC + 4, r].tolist() == want and int(tr[ff.X, r]) == x and int(tr[ff.XINV, r]) == fq.x_inv(k)
            assert tr[ff.COEF:ff.COEF + 4, c * L].tolist() == [int(v) for v in coef[L - 1]] and int(tr[ff.J, c * L]) == L - 1 and int(tr[ff.J, r]) == 0


@pytest.mark.parametrize("name", sorted(SETS))
def test_twin_traces_satisfy_the_air(name):
    s = SETS[name]
    tr, _ = ff.trace(s)
    assert air.check_trace(_prog(s["lfp"]), tr, NOPV) == []
    assert air.check_trace(_prog(s["lfp"], None), tr, NOPV) == []
    assert (tr[:, len(s["k"]) << s["lfp"]:] == 0).all()


def test_degree_chunks_widths_and_padding():
    for lfp in (0, 1, 3, 8):
        for b in (air.fri_final_air(lfp, *BUSES), air.fri_final_air(lfp, *BUSES, 18)):
            assert b.max_degree() == 3 and air.quotient_chunks(b.program()) == 2
        b = air.fri_final_air(lfp, *BUSES, 18)
        assert [(bus, kind, len(f)) for (bus, kind, _, f) in b.interactions] == [(14, 0, 2), (17, 1, 7), (18, 0, 6)]
        assert air.check_trace(b.program(), np.zeros((19, 8), np.uint32), NOPV) == []      # an all-zero row satisfies every line
    for lfp in (-1, 9):
        with pytest.raises(AssertionError):
            air.fri_final_air(lfp, *BUSES)


def test_the_call_sets_reach_the_shapes_they_are_meant_for():
    full = ff.call_sets()
    rows = lambda s: len(s["k"]) << s["lfp"]  # noqa: E731
    assert rows(full["lfp0_one_call"]) == 1 == 1 << full["lfp0_one_call"]["lh"]
    assert rows(full["lfp0_past_a_workgroup"]) == 300 and full["lfp0_past_a_workgroup"]["lh"] == 9
    assert rows(full["lfp3_five_calls"]) == 40 and rows(full["lfp3_full"]) == 64 == 1 << full["lfp3_full"]["lh"]
    assert rows(full["lfp6_three_calls"]) == 192 and rows(full["lfp7_three_calls"]) == 384
    assert rows(full["lfp8_one_call"]) == 256 == 1 << full["lfp8_one_call"]["lh"] and rows(full["lfp8_three_calls"]) == 768 and full["lfp8_three_calls"]["lh"] == 10
    for name in ("lfp0_boundary", "lfp1_boundary", "lfp3_boundary", "lfp8_boundary"):
        s = full[name]
        got = {(int(k), int(lvl)) for k, lvl in zip(s["k"], s["lvl"])}
        assert {(0, 1), (1, 1), (0, 26), (1, 26), ((1 << 26) - 1, 26), ((1 << 12) - 1, 12)} <= got
        assert (s["coef"][0] == 0).all() and (s["coef"][1] == P - 1).all() and sorted(set(s["poly"].tolist())) == [0, 1, 2]
        assert any(s["poly"][c] != s["poly"][c + 1] for c in range(len(s["poly"]) - 1))
    for name, s in full.items():
        assert rows(s) <= 1 << s["lh"], name


def _bump(t, col, row):
    w = t.copy()
    w[col][row] = (int(w[col][row]) + 1) % P
    return w


def test_every_constraint_family_refuses_its_mutation():
    rng = np.random.default_rng(5)
    s = ff.call_set(rng, 2, 4, 3, 2)                      # rows 0..3 | 4..7 | 8..11, padding from 12
    s["k"], s["lvl"] = np.array([5, 0, 1]), np.array([3, 7, 1])
    prog = _prog(2)
    t, _ = ff.trace(s)
    assert air.check_trace(prog, t, NOPV) == []
    bad = lambda w: air.check_trace(prog, w, NOPV) != []  # noqa: E731
    # each flag: set on padding; not boolean; first / last moved or cleared
    for col in (ff.FIRST, ff.LAST, ff.REAL):
        w = t.copy()
        w[col][13] = 1
        assert bad(w)
        w = t.copy()
        w[col][{ff.FIRST: 4, ff.LAST: 7, ff.REAL: 5}[col]] = 2
        assert bad(w)
    for col, row, v in ((ff.LAST, 3, 0), (ff.LAST, 11, 0), (ff.LAST, 5, 1), (ff.FIRST, 6, 1), (ff.FIRST, 0, 0), (ff.FIRST, 4, 0), (ff.REAL, 6, 0)):
        w = t.copy()
        w[col][row] = v
        assert bad(w), (col, row)
    w = t.copy()
    w[:, 12:16] = t[:, 4:8]                               # a whole call behind ... nothing wrong: padding starts later
    w[ff.CALL, 12:16] = 3
    assert not bad(w)
    w[:, 12] = 0                                        # ... but real rows behind a padding row
    assert bad(w)
    # j on the first row, on the last, inside a call
    assert bad(_bump(t, ff.J, 0)) and bad(_bump(t, ff.J, 4)) and bad(_bump(t, ff.J, 3)) and bad(_bump(t, ff.J, 11)) and bad(_bump(t, ff.J, 5)) and bad(_bump(t, ff.J, 9))
    # a coef word on the first row (acc = coef there), on a later row (the Horner step); an acc word on a later row
    assert bad(_bump(t, ff.COEF + 1, 0)) and bad(_bump(t, ff.COEF + 3, 8)) and bad(_bump(t, ff.COEF, 6))
    assert bad(_bump(t, ff.ACC + 2, 1)) and bad(_bump(t, ff.ACC, 7)) and bad(_bump(t, ff.ACC + 3, 10)) and bad(_bump(t, ff.ACC + 1, 4))
    # x, x_inv, xi2 -- on one row, and x on every row of a call at once (line 8 still names it)
    assert bad(_bump(t, ff.X, 2)) and bad(_bump(t, ff.XINV, 5)) and bad(_bump(t, ff.XI2, 9)) and bad(_bump(t, ff.XI2, 0))
    w = t.copy()
    w[ff.X, 0:4] = (int(t[ff.X, 0]) + 1) % P
    assert bad(w)
    w = t.copy()
    w[ff.XINV, 4:8] = (int(t[ff.XINV, 4]) + 1) % P
    assert bad(w)
    # k, lvl, poly, call inside a call
    for col in (ff.K, ff.LVL, ff.POLY, ff.CALL):
        assert bad(_bump(t, col, 1)) and bad(_bump(t, col, 7)) and bad(_bump(t, col, 10)), col
    # ... while the same value on every row of a call is free for the constraints: the buses bind it
    for col in (ff.K, ff.LVL, ff.POLY, ff.CALL):
        w = t.copy()
        w[col, 4:8] = (int(t[col, 4]) + 1) % P
        assert not bad(w), col


def _rows(s, per_call):
    """the twin's trace with call c cut or stretched to per_call[c] rows, flags and j as an honest prover of that length would set them"""
    L = 1 << s["lfp"]
    t, _ = ff.trace(s)
    cols = []
    for c, n in enumerate(per_call):
        blk = t[:, c * L:(c + 1) * L]
        blk = blk[:, :n] if n <= L else np.concatenate([blk, np.repeat(blk[:, -1:], n - L, axis=1)], axis=1)
        blk = blk.copy()
        blk[ff.FIRST], blk[ff.LAST] = 0, 0
        blk[ff.FIRST, 0], blk[ff.LAST, n - 1] = 1, 1
        cols.append(blk)
    w = np.concatenate(cols, axis=1)
    out = np.zeros((19, 1 << s["lh"]), np.uint32)
    out[:, :w.shape[1]] = w
    return out


def test_a_call_of_another_length_is_refused():
    rng = np.random.default_rng(6)
    for lfp in (1, 2, 3):
        L = 1 << lfp
        s = ff.call_set(rng, lfp, lfp + 2, 3)
        prog = _prog(lfp)
        assert air.check_trace(prog, _rows(s, [L, L, L]), NOPV) == []
        for per_call in ([L, L - 1, L], [L - 1, L, L], [L, L, L - 1]):
            w = _rows(s, per_call)
            assert air.check_trace(prog, w, NOPV) != []           # is_last meets j = 1
            # ... and with j renumbered to end on 0 the first row no longer holds L - 1
            for c, n in enumerate(per_call):
                r0 = sum(per_call[:c])
                w[ff.J, r0:r0 + n] = np.arange(n - 1, -1, -1)
            assert air.check_trace(prog, w, NOPV) != []
        for per_call in ([L, L + 1, L], [L + 1, L, L]):
            w = _rows(s, per_call)
            r0 = sum(per_call[:per_call.index(L + 1)])
            # an honest Horner step onto the extra row, with j running on to p - 1: every transition line holds, is_last meets j != 0
            w[ff.J, r0 + L] = P - 1
            x = int(w[ff.X, r0])
            w[ff.ACC:ff.ACC + 4, r0 + L] = [(int(a) * x + int(cf)) % P for a, cf in zip(w[ff.ACC:ff.ACC + 4, r0 + L - 1], w[ff.COEF:ff.COEF + 4, r0 + L])]
            got = air.check_trace(prog, w, NOPV)
            assert got != []
            w[ff.J, r0 + L] = 0                                    # j forced to 0 there: the step j' = j - 1 breaks instead
            assert air.check_trace(prog, w, NOPV) != []


@pytest.mark.parametrize("shape", [(5, 1, 0), (6, 1, 2), (6, 2, 3)])
def test_the_honest_instance_ends_on_its_final_polynomial(ora, shape):
    log_max, log_blowup, lfp = shape
    inst = ff.final_instance(ora, z, log_max, log_blowup, lfp)     # (asserts the interpolant's degree and every query's last eval)
    assert inst.n_layers == log_max - log_blowup - lfp and inst.lvl == log_blowup + lfp and inst.coef.shape == (1 << lfp, 4)
    assert len(inst.calls) == 12 and inst.indices[0] >> 2 == inst.indices[1] >> 2 == inst.indices[2] >> 2
    assert (inst.coef[-1] != 0).any()                             # the degree bound is tight
    k, lvl, poly = ff.final_records(inst)
    lh = max(1, int(np.ceil(np.log2(len(k) << lfp))))
    tr, val = ff.trace_np(lfp, k, lvl, poly, inst.coef[None], lh)
    assert air.check_trace(_prog(lfp), tr, NOPV) == []
    # the chip's value is what the query chip's last row sends: the fold loop's last eval
    tq, _, _, fin = fq.trace(ora, inst.calls, max(1, int(np.ceil(np.log2(fq.n_rows(inst.calls))))))
    assert (val == fin).all()
    last_rows = np.nonzero(tq[fq.LAST])[0]
    for c, r in enumerate(last_rows):
        rf = (c << lfp) + (1 << lfp) - 1
        sent = [int(tq[fq.CALL, r]), int(tq[fq.LVL, r]), int(tq[fq.K, r])] + tq[fq.EVAL:fq.EVAL + 4, r].tolist()
        assert sent == [int(tr[ff.CALL, rf]), int(tr[ff.LVL, rf]), int(tr[ff.K, rf])] + tr[ff.ACC:ff.ACC + 4, rf].tolist()


def test_cpp_twin_emits_the_same_program(tmp_path):
    exe = str(tmp_path / "fri_final_cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fri_final_cpp.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["fri_final_0", "fri_final_3", "fri_final_8", "fri_final_2_coeff"]
    for line, b in zip(lines, (air.fri_final_air(0, *BUSES), air.fri_final_air(3, *BUSES), air.fri_final_air(8, *BUSES), air.fri_final_air(2, *BUSES, 18))):
        _, deg, *words = line.split()
        want = b.program()
        got = np.array([int(x) for x in words], dtype=np.uint32)
        assert len(got) == len(want), (len(got), len(want))
        assert (got == want).all(), "first difference at word %d" % int(np.nonzero(got != want)[0][0])
        assert int(deg) == b.max_degree() == 3


def test_host_function_alone_under_the_sanitizers(tmp_path):
    """csrc/fri_final_host.hpp with the verifier whose helpers it calls and tests/fri_final_host_main.cpp, a program of its own (nothing
    loaded into this interpreter runs under a sanitizer): clean on heap blocks of exactly 2^lfp coefficients, and what it prints is the twin's."""
    exe = str(tmp_path / "fri_final_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DZK_NO_HOST_AVX512",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fri_final_host_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert [tuple(int(x) for x in ln.split("|")[0].split()) for ln in lines] == [(0, 1, 0), (0, 1, 1), (1, 2, 3), (3, 12, 0xABC), (8, 26, (1 << 26) - 1), (8, 9, 1), (5, 26, 0)]
    words = []
    for ln in lines:
        (lfp, lvl, k), coef, (x,), val = [[int(v) for v in p.split()] for p in ln.split("|")]
        assert (x, val) == ff.value_int(np.array(coef).reshape(1 << lfp, 4), lvl, k)
        words += coef
    assert 0 in words and P - 1 in words
