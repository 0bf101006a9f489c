"""CPU: the row-digest chip (air.mmcs_rows_air: the sponge between the opened words of one query at one height class and the row digest
the MMCS path chip claims, one permutation per row).  The host sponge equals the oracle's at every block boundary; the twin's traces
satisfy the AIR and every constraint family refuses the trace that breaks it; the calls of the reference's stored openings give exactly
the claims the path chip sends; the C++ twin of the AIR emits the same program; the host sponge runs clean under the sanitizers as a
stand-alone program."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmcs_path_util as mu  # noqa: E402
import mmcs_rows_util as mr  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOPV = np.zeros(0, np.uint32)
P = mr.P
SETS = mr.call_sets("cpu")
LENGTHS = (1, 7, 8, 9, 16, 17, 438)


@pytest.fixture(scope="module")
def prog():
    return air.mmcs_rows_air(11, 10).program()


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(HERE, "golden", "ref_v1_vectors.json")) as f:
        return json.load(f)


def test_widths_agree():
    assert air.MMCS_ROWS_WIDTH == z.MMCS_ROWS_WIDTH == mr.WIDTH == 56


def test_host_sponge_equals_the_oracle(ora):
    rng = np.random.default_rng(1)
    for L in LENGTHS:
        for kind in ("seeded", "zeros", "pmax", "mixed"):
            w = rng.integers(0, P, L, dtype=np.int64)
            if kind == "zeros":
                w[:] = 0
            elif kind == "pmax":
                w[:] = P - 1
            elif kind == "mixed":
                w[::2], w[1::2] = 0, P - 1
            assert (z.hash_slice_host(w) == mr.hash_slice(ora, w)).all(), (L, kind)
    assert (z.hash_slice_host([]) == 0).all()


def test_host_sponge_refuses_a_word_equal_to_p():
    lib = z.load_library()
    u = lambda v: np.ascontiguousarray(v, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    out = np.zeros(8, np.uint32)
    assert lib.zkhip_hash_slice_host(u([1, 2, 3]), 3, u(out)) == 0
    for L in LENGTHS:
        for pos in {0, L - 1, L // 2}:
            w = np.ones(L, np.uint32)
            w[pos] = P
            assert lib.zkhip_hash_slice_host(u(w), L, u(out)) == -3   # ZKHIP_ERR_INVALID
    assert lib.zkhip_hash_slice_host(u([1]), 1, None) == -3
    with pytest.raises(z.ZkhipError):
        z.hash_slice_host([1, 0xFFFFFFFF])


@pytest.mark.parametrize("name", sorted(SETS))
def test_twin_traces_satisfy_the_air(ora, prog, name):
    lh, calls = SETS[name]
    t, hin, dg = mr.trace(ora, calls, lh)      # (asserts row-wise walk == ora_hash_slice on every call)
    assert air.check_trace(prog, t, NOPV) == []
    assert (hin.T == t[:16]).all()
    for c, d in zip(calls, dg):
        assert (z.hash_slice_host(c[0]) == d).all()


def test_degree_and_padding(prog):
    for b in (air.mmcs_rows_air(11, 10), air.mmcs_rows_air(11, 10, 12)):
        assert b.max_degree() == 3 and air.quotient_chunks(b.program()) == 2
    assert air.check_trace(prog, np.zeros((56, 8), np.uint32), NOPV) == []      # an all-zero row satisfies every line


def test_the_call_sets_reach_the_shapes_they_are_meant_for():
    rows = lambda name: sum((len(c[0]) + 7) // 8 for c in SETS[name][1])  # noqa: E731
    assert rows("full_16") == 16 == 1 << SETS["full_16"][0]
    assert rows("one_word") == 1 == 1 << SETS["one_word"][0]
    assert rows("short_padded") < (1 << SETS["short_padded"][0]) // 2
    words = [w for c in SETS["boundary_words"][1] for w in c[0]]
    assert 0 in words and P - 1 in words
    full = mr.call_sets()
    assert sorted(len(full["calls_%d" % n][1]) for n in (3, 4, 5, 65)) == [3, 4, 5, 65]
    lens = [len(c[0]) for c in full["imbalance"][1]]
    assert max(lens) == 8 << 10 and lens.count(1) == 200


def _bump(t, col, row):
    w = t.copy()
    w[col][row] = (int(w[col][row]) + 1) % P
    return w


def test_every_constraint_family_refuses_its_mutation(ora, prog):
    rng = np.random.default_rng(5)
    calls = [mr.random_call(rng, L, m) for L, m in ((29, 2), (3, 1), (48, 0))]      # rows 0..3 | 4 | 5..10, padding from 11
    t, _, _ = mr.trace(ora, calls, 4)
    assert air.check_trace(prog, t, NOPV) == []
    bad = lambda w: air.check_trace(prog, w, NOPV) != []  # noqa: E731
    assert [int(x) for x in t[mr.F:mr.F + 8, 3]] == [1] * 5 + [0] * 3 and int(t[mr.MULT][3]) == 2
    # a flag: not boolean; set on padding; first / last moved
    for col in (mr.FIRST, mr.LAST, mr.REAL, mr.F + 2):
        w = t.copy()
        w[col][12] = 1
        assert bad(w)
        w = t.copy()
        w[col][5 if col != mr.LAST else 10] = 2
        assert bad(w)
    w = t.copy()
    w[mr.LAST][3] = 0                                   # is_last cleared on a call's last row
    assert bad(w)
    w = t.copy()
    w[mr.FIRST][7] = 1                                  # is_first set mid-call
    assert bad(w)
    w = t.copy()
    w[mr.FIRST][0] = 0                                  # the first trace row is real but not first
    assert bad(w)
    w = t.copy()
    w[mr.REAL][6], w[mr.F:mr.F + 8, 6] = 0, 0          # a hole inside a call
    assert bad(w)
    w = t.copy()
    w[:, 13] = t[:, 4]                                  # a real row (a whole one-row call) after a padding row
    assert bad(w)
    # f is a prefix, and f[0] = is_real
    w = t.copy()
    w[mr.F + 6][3] = 1                                  # 1 1 1 1 1 0 1 0
    assert bad(w)
    w = t.copy()
    w[mr.F][4] = 0                                      # a real row that overwrites nothing
    assert bad(w)
    # a partial row in the middle of a call (the prefix itself stays a prefix)
    w = t.copy()
    w[mr.F + 7][6] = 0
    assert bad(w)
    # a capacity lane, and a rate lane that no word overwrote, on a first row
    assert bad(_bump(t, mr.ST_IN + 8, 0)) and bad(_bump(t, mr.ST_IN + 15, 5)) and bad(_bump(t, mr.ST_IN + 3, 4))
    # a carried lane: capacity mid-call, and a rate lane of the partial last row
    assert bad(_bump(t, mr.ST_IN + 9, 2)) and bad(_bump(t, mr.ST_IN + 6, 3)) and bad(_bump(t, mr.ST_OUT + 12, 7))
    # ... while an overwritten lane is free (it is the word), and so is st_out of a last row (the hash bus binds both)
    assert not bad(_bump(t, mr.ST_IN + 2, 2)) and not bad(_bump(t, mr.ST_OUT + 5, 3))
    # root, lvl, idx, call change inside a call
    assert bad(_bump(t, mr.ROOT + 4, 2)) and bad(_bump(t, mr.LVL, 8)) and bad(_bump(t, mr.IDX, 1)) and bad(_bump(t, mr.CALL, 9))
    # blk: off by one mid-call; not zero on a first row
    assert bad(_bump(t, mr.BLK, 6)) and bad(_bump(t, mr.BLK, 4))
    # mult on a row that is not last; on padding
    assert bad(_bump(t, mr.MULT, 1)) and bad(_bump(t, mr.MULT, 14))
    # ... while mult on a last row is a free count, 0 included
    w = t.copy()
    w[mr.MULT][3] = 0
    assert not bad(w) and int(t[mr.MULT][10]) == 0
    # a call that runs into the last trace row without is_last
    full, _, _ = mr.trace(ora, [mr.random_call(rng, 8 * 11), mr.random_call(rng, 8 * 5 - 3)], 4)
    assert air.check_trace(prog, full, NOPV) == []
    w = full.copy()
    w[mr.LAST][15], w[mr.MULT][15] = 0, 0
    assert bad(w)


def test_the_fixture_calls_give_exactly_the_claims_the_path_chip_sends(ora, vec):
    want = mu.records_of_fixture(ora, vec)[5]
    plain = mr.calls_of_fixture(ora, vec, merge=False)
    assert len(plain) == 336 and sum((len(c[0]) + 7) // 8 for c in plain) == 2124
    assert min((len(c[0]) + 7) // 8 for c in plain) == 1 and max((len(c[0]) + 7) // 8 for c in plain) == 55
    calls = mr.calls_of_fixture(ora, vec)
    assert len(calls) == 319 == len(set(want)) and sum(c[4] for c in calls) == 336 == len(want) and max(c[4] for c in calls) > 1
    for cs in (plain, calls):
        t, _, dg = mr.trace(ora, cs, 12)
        assert air.check_trace(air.mmcs_rows_air(11, 10).program(), t, NOPV) == []
        assert sorted(mr.claims_of(cs, dg)) == sorted(want)
        # ... and read back from the trace: the is_last rows' (root, lvl, idx, st_out[0..8]) x mult
        got = []
        for r in np.nonzero(t[mr.LAST])[0]:
            got += [(tuple(t[mr.ROOT:mr.ROOT + 8, r].tolist()), int(t[mr.LVL][r]), int(t[mr.IDX][r]), tuple(t[mr.ST_OUT:mr.ST_OUT + 8, r].tolist()))] * int(t[mr.MULT][r])
        assert sorted(got) == sorted(want)


def test_cpp_twin_emits_the_same_program(tmp_path):
    exe = str(tmp_path / "mmcs_rows_cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "mmcs_rows_cpp.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["mmcs_rows", "mmcs_rows_values"]
    for line, b in zip(lines, (air.mmcs_rows_air(11, 10), air.mmcs_rows_air(11, 10, 12))):
        _, deg, *words = line.split()
        want = b.program()
        got = np.array([int(x) for x in words], dtype=np.uint32)
        assert len(got) == len(want), (len(got), len(want))
        assert (got == want).all(), "first difference at word %d" % int(np.nonzero(got != want)[0][0])
        assert int(deg) == b.max_degree() == 3


def test_host_sponge_alone_under_the_sanitizers(ora, tmp_path):
    """csrc/hash_slice_host.hpp with tests/mmcs_rows_sponge_main.cpp, a program of its own (nothing loaded into this interpreter runs
    under a sanitizer): clean at every block boundary on heap blocks of exactly `len` words, and the digests it prints are the oracle's."""
    exe = str(tmp_path / "mmcs_rows_sponge")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DZK_NO_HOST_AVX512",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mmcs_rows_sponge_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert [int(ln.split()[0]) for ln in lines] == [0] + list(LENGTHS)
    for ln in lines:
        left, right = ln.split(":")
        words = [int(x) for x in left.split()[1:]]
        assert len(words) == int(left.split()[0])
        assert [int(x) for x in right.split()] == mr.hash_slice(ora, np.array(words, np.uint32)).tolist()
        if len(words) > 1:
            assert 0 in words and P - 1 in words
