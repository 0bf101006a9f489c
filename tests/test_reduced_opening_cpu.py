"""CPU: the reduced-opening chip (air.reduced_opening_air: ro = sum_i alpha^i (b_i - a_i) of one query at one height class, one element
per row, Horner from the call's last element).  The host entry point equals the direct power sum at every boundary operand; the twin's
traces satisfy the AIR and every constraint family refuses the trace that breaks it; the C++ twin of the AIR emits the same program.

(The first call set is 1 + 1 + 2 + 60 rows: the 2^6 rows are exactly full.)"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduced_opening_util as ru  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOPV = np.zeros(0, np.uint32)
P = ru.P
SETS = ru.call_sets(z.REDUCED_OPENING_BLOCK_ROWS, "cpu")


@pytest.fixture(scope="module")
def prog():
    return air.reduced_opening_air().program()


def _host(alpha, a, b):
    return tuple(int(x) for x in z.reduced_opening_host(alpha, a, b))


def test_widths_agree():
    assert air.REDUCED_OPENING_WIDTH == z.REDUCED_OPENING_WIDTH == ru.WIDTH == 18


def test_host_equals_the_power_sum_at_boundary_operands():
    calls = ru.boundary_calls()
    assert sorted({len(c[1]) for c in calls}) == [1, 2, 5, 300]
    assert {c[0] for c in calls} >= {(0, 0, 0, 0), (1, 0, 0, 0), ru.PMAX}
    cells = [(ai, tuple(bi)) for c in calls for ai, bi in zip(c[1], c[2])]
    assert any(ai == 0 for ai, _ in cells) and any(ai == P - 1 and bi[0] == 0 for ai, bi in cells) and any(bi == ru.PMAX for _, bi in cells)
    for alpha, a, b in calls:
        assert _host(alpha, a, b) == ru.power_sum(alpha, a, b)


def test_host_equals_the_power_sum_on_seeded_operands():
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 5, 17, 64, 65, 300):
        alpha, a, b = ru.random_call(rng, L)
        assert _host(alpha, a, b) == ru.power_sum(alpha, a, b)
    # alpha = 0 keeps element 0 only, alpha = 1 is the plain sum
    alpha, a, b = ru.random_call(rng, 5, (0, 0, 0, 0))
    assert _host(alpha, a, b) == ru.term(a[0], b[0])
    alpha, a, b = ru.random_call(rng, 5, (1, 0, 0, 0))
    assert _host(alpha, a, b) == tuple((sum(bi[q] for bi in b) - (sum(a) if q == 0 else 0)) % P for q in range(4))


def test_host_refuses_an_operand_equal_to_p_and_an_empty_call():
    lib = z.load_library()
    u = lambda v: np.ascontiguousarray(v, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    out = np.zeros(4, np.uint32)
    good = ([1, 2, 3, 4], [5, 6], [[1, 2, 3, 4], [5, 6, 7, 8]])
    assert lib.zkhip_reduced_opening_host(u(good[0]), u(good[1]), u(good[2]), 2, u(out)) == 0
    assert lib.zkhip_reduced_opening_host(u(good[0]), u(good[1]), u(good[2]), 0, u(out)) == -3   # ZKHIP_ERR_INVALID
    for alpha, a, b in (([1, P, 3, 4], good[1], good[2]), (good[0], [5, P], good[2]), (good[0], good[1], [[1, 2, 3, 4], [5, 6, P, 8]])):
        assert lib.zkhip_reduced_opening_host(u(alpha), u(a), u(b), 2, u(out)) == -3
    with pytest.raises(z.ZkhipError):
        z.reduced_opening_host([1, 2, 3, P], good[1], good[2])


@pytest.mark.parametrize("name", sorted(SETS))
def test_twin_traces_satisfy_the_air(prog, name):
    lh, calls = SETS[name]
    assert air.check_trace(prog, ru.trace(calls, lh), NOPV) == []
    assert air.quotient_chunks(prog) == 2
    assert air.quotient_chunks(air.reduced_opening_air(12).program()) == 2


def test_padding_only_and_boundary_operand_traces_satisfy_the_air(prog):
    assert air.check_trace(prog, np.zeros((18, 8), np.uint32), NOPV) == []
    assert air.check_trace(prog, ru.trace(ru.boundary_calls(), 11), NOPV) == []


def test_the_numpy_twin_equals_the_integer_twin():
    for lh, calls in list(SETS.values()) + [(11, ru.boundary_calls())]:
        assert (ru.trace_np(*ru.records(calls), lh) == ru.trace(calls, lh)).all()
    alpha, lens, a, b = ru.many_short_calls(500)
    calls = [(alpha[c], a[o:o + l], b[o:o + l]) for c, (o, l) in enumerate(zip(np.cumsum(lens) - lens, lens))]
    assert sorted(set(lens.tolist())) == [1, 2, 3] and (ru.trace_np(alpha, lens, a, b, 10) == ru.trace(calls, 10)).all()


def _bump(t, col, row):
    w = t.copy()
    w[col][row] = (int(w[col][row]) + 1) % P
    return w


def test_every_constraint_family_refuses_its_mutation(prog):
    rng = np.random.default_rng(5)
    calls = ru.random_calls(rng, [4, 1, 6])          # rows 0..3 | 4 | 5..10, padding from 11
    t = ru.trace(calls, 4)
    assert air.check_trace(prog, t, NOPV) == []
    bad = lambda w: air.check_trace(prog, w, NOPV) != []  # noqa: E731
    # one cell of acc on a first, a middle and a last row
    assert bad(_bump(t, ru.ACC + 1, 5)) and bad(_bump(t, ru.ACC + 2, 7)) and bad(_bump(t, ru.ACC + 3, 10))
    assert bad(_bump(t, ru.ACC, 4))                  # the one-row call: first and last at once
    assert bad(_bump(t, ru.ALPHA + 2, 7))            # alpha changed mid-call
    assert bad(_bump(t, ru.IDX, 8)) and bad(_bump(t, ru.IDX, 0))   # idx off by one (mid-call; on a first row)
    assert bad(_bump(t, ru.CALL, 2))                 # call changed mid-call
    w = t.copy()
    w[ru.LAST][3] = 0                                # is_last cleared on a call's last row
    assert bad(w)
    w = t.copy()
    w[ru.FIRST][7] = 1                               # is_first set mid-call
    assert bad(w)
    w = t.copy()
    w[:, 13] = t[:, 4]                               # a real row (a whole one-row call) after a padding row
    assert bad(w)
    w = t.copy()
    w[ru.REAL][6] = 0                                # a hole inside a call
    assert bad(w)
    w = t.copy()
    w[ru.FIRST][0] = 0                               # the first trace row is real but not first
    assert bad(w)
    for col in (ru.FIRST, ru.LAST, ru.REAL):         # flags are boolean; first and last imply real
        w = t.copy()
        w[col][12] = 1
        assert bad(w)
        w = t.copy()
        w[col][5 if col != ru.LAST else 10] = 2
        assert bad(w)
    # a call that runs into the last trace row without is_last: 16 rows, the last call 5 rows long and not closed
    full = ru.trace(ru.random_calls(rng, [11, 5]), 4)
    assert air.check_trace(prog, full, NOPV) == []
    w = full.copy()
    w[ru.LAST][15] = 0
    assert bad(w)


def test_opened_rows_of_the_reference_proofs_as_base_cells(prog):
    """a = real opened rows of the reference's stored proofs (openings[*].batches of the fixture: one call per opened matrix, its row as
    the base cells).  The fixture holds neither the batching challenge nor the values at zeta, so alpha and b are SEEDED here."""
    with open(os.path.join(HERE, "golden", "ref_v1_vectors.json")) as f:
        vec = json.load(f)
    rng = np.random.default_rng(11)
    calls = []
    for q in vec["openings"][:2]:
        alpha = tuple(int(x) for x in rng.integers(0, P, 4))
        for bt in q["batches"]:
            offs = np.concatenate([[0], np.cumsum(bt["widths"])])
            for m, w in enumerate(bt["widths"]):
                a = [int(x) for x in bt["opening"][offs[m]:offs[m + 1]]]
                calls.append((alpha, a, rng.integers(0, P, (w, 4)).tolist()))
    calls = calls[:24]
    assert len(calls) >= 6 and max(len(c[1]) for c in calls) > 1
    for alpha, a, b in calls:
        assert _host(alpha, a, b) == ru.power_sum(alpha, a, b)
    rows = sum(len(c[1]) for c in calls)
    lh = int(np.ceil(np.log2(rows + 1)))
    assert air.check_trace(prog, ru.trace(calls, lh), NOPV) == []


def test_cpp_twin_emits_the_same_program(tmp_path):
    exe = str(tmp_path / "reduced_opening_cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "reduced_opening_cpp.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["reduced_opening", "reduced_opening_bus"]
    for line, b in zip(lines, (air.reduced_opening_air(), air.reduced_opening_air(12))):
        _, deg, *words = line.split()
        want = b.program()
        got = np.array([int(x) for x in words], dtype=np.uint32)
        assert len(got) == len(want), (len(got), len(want))
        assert (got == want).all(), "first difference at word %d" % int(np.nonzero(got != want)[0][0])
        assert int(deg) == b.max_degree() == 3
