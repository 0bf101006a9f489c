"""CPU: the FRI query chip (air.fri_query_air: one query's fold loop, a row per commit-phase layer).  The host function equals the twin and
repeated zkhip_fri_fold_row; the twin's two forms agree; its traces satisfy the AIR and every constraint family refuses the trace that
breaks it, while the cells the buses bind stay free; the reference's own stored fold rows satisfy the fold lines; the honest FRI instance
chains into its own layers; the C++ twin of the AIR emits the same program; the host function runs clean under the sanitizers as a
stand-alone program."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_query_util as fq  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOPV = np.zeros(0, np.uint32)
P = fq.P
SETS = fq.call_sets("cpu")
BUSES = (14, 11, 10, 15)


@pytest.fixture(scope="module")
def prog():
    return air.fri_query_air(*BUSES, 16, 17).program()


def test_widths_agree():
    assert air.FRI_QUERY_WIDTH == z.FRI_QUERY_WIDTH == fq.WIDTH == 61
    assert fq.WINV == air.domain_point_inverse_roots()


def _host_cases():
    rng = np.random.default_rng(1)
    cases = []
    for n, lm in ((1, 2), (2, 3), (2, 27), (26, 27), (1, 27), (13, 20)):
        for index in (0, (1 << lm) - 1, int(rng.integers(0, 1 << lm))):
            for has in (0, 1, None):
                cases.append(fq.random_call(rng, n, lm, index, has))
    return cases + fq.boundary_calls()


def test_host_function_equals_the_twin_and_repeated_fold_row():
    for index, lm, beta, _, sib, has, ro, top in _host_cases():
        e0, e1, ev = z.fri_query_host(index, lm, beta, sib, has, ro, top)
        want = fq.chain_int(index, lm, beta, sib, has, ro, top)
        assert e0.tolist() == [w[0] for w in want] and e1.tolist() == [w[1] for w in want] and ev.tolist() == [w[2] for w in want]
        cur = [int(v) for v in top]
        for t in range(len(has)):                       # the same walk over the verifier's exposed fold step
            pair = [sib[t].tolist(), cur] if (index >> t) & 1 else [cur, sib[t].tolist()]
            cur = [int(v) for v in z.fri_fold_row(index >> (t + 1), lm - 1 - t, beta[t], pair[0], pair[1])]
            if has[t]:
                cur = [(a + b) % P for a, b in zip(cur, fq.emul(fq.emul(beta[t].tolist(), beta[t].tolist()), ro[t].tolist()))]
            assert cur == ev[t].tolist()


def test_host_function_refuses():
    lib = z.load_library()
    u = lambda v: np.ascontiguousarray(v, dtype=np.uint32).reshape(-1).ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    rng = np.random.default_rng(2)
    index, lm, beta, _, sib, has, ro, top = fq.random_call(rng, 3, 6, 37, has=1)
    out = [np.zeros((3, 4), np.uint32) for _ in range(3)]
    arrs = [beta, sib, has, ro, top]
    call = lambda index=index, lm=lm, n=3, arrs=arrs, outs=out: lib.zkhip_fri_query_host(index, lm, n, *[None if a is None else u(a) for a in list(arrs) + list(outs)])  # noqa: E731
    assert call() == 0
    for i in range(5):
        assert call(arrs=[None if j == i else a for j, a in enumerate(arrs)]) == -3
    for i in range(3):
        assert call(outs=[None if j == i else a for j, a in enumerate(out)]) == -3
    assert call(lm=28) == -3 and call(n=0) == -3
    assert call(lm=3, index=5) == -3                     # n_layers = 3 > log_max - 1 = 2
    assert call(lm=4, index=5) == 0                      # n_layers = log_max - 1
    for n in (6, 7, 27, 1 << 31, (1 << 32) - 2, (1 << 32) - 1):   # n_layers >= log_max = 6, up to the counts at which n_layers + 1 wraps
        assert call(n=n) == -3
    assert call(lm=0, index=0, n=(1 << 32) - 1) == -3 and call(lm=27, n=(1 << 32) - 1) == -3
    assert call(index=64) == -3 and call(index=63) == 0  # index >= 2^log_max
    assert lib.zkhip_fri_query_host((1 << 27) - 1, 27, 3, *[u(a) for a in arrs + out]) == 0
    assert lib.zkhip_fri_query_host(1 << 27, 27, 3, *[u(a) for a in arrs + out]) == -3
    for i in (0, 1, 3, 4):                               # a word equal to p, first and last position
        for pos in (0, arrs[i].size - 1):
            w = np.array(arrs[i], np.uint32)
            w.reshape(-1)[pos] = P
            assert call(arrs=[w if j == i else a for j, a in enumerate(arrs)]) == -3
    h = np.array(has, np.uint32)
    h[1] = 2
    assert call(arrs=[beta, sib, h, ro, top]) == -3      # has_ro outside {0, 1}
    h[1] = 0
    assert call(arrs=[beta, sib, h, ro, top]) == -3      # a non-zero ro under has_ro = 0
    r = np.array(ro, np.uint32)
    r[1] = 0
    assert call(arrs=[beta, sib, h, r, top]) == 0
    keep = [o.copy() for o in out]
    assert call(arrs=[beta, sib, h, ro, top]) == -3 and all((a == b).all() for a, b in zip(keep, out))   # nothing written
    with pytest.raises(z.ZkhipError):
        z.fri_query_host(0, 2, beta[:1], sib[:1], [1], ro[:1], [0, 0, 0, P])


def test_the_two_forms_of_the_twin_agree(ora):
    for name, (lh, calls) in SETS.items():
        tr, hin, leaf, fin = fq.trace(ora, calls, lh)
        r = 0
        for c, (index, lm, beta, root, sib, has, ro, top) in enumerate(calls):
            walk = fq.chain_int(index, lm, beta, sib, has, ro, top)
            h0, h1, hev = z.fri_query_host(index, lm, beta, sib, has, ro, top)   # and the host definition, on the very calls the device is given
            assert h0.tolist() == [x[0] for x in walk] and h1.tolist() == [x[1] for x in walk] and hev.tolist() == [x[2] for x in walk], (name, c)
            for t, (e0, e1, ev) in enumerate(walk):
                assert tr[fq.E0:fq.E0 + 4, r].tolist() == e0 and tr[fq.E1:fq.E1 + 4, r].tolist() == e1 and tr[fq.EVAL:fq.EVAL + 4, r].tolist() == ev, (name, c, t)
                assert int(tr[fq.XINV, r]) == fq.x_inv(index >> (t + 1)) and int(tr[fq.K, r]) == index >> (t + 1) and int(tr[fq.LVL, r]) == lm - 1 - t
                assert tr[fq.BSQ:fq.BSQ + 4, r].tolist() == fq.emul(beta[t].tolist(), beta[t].tolist())
                assert (ora.permute(hin[r])[:8] == leaf[r]).all() and (hin[r, 8:] == 0).all()
                r += 1
            assert fin[c].tolist() == walk[-1][2]
        assert r == fq.n_rows(calls)


@pytest.mark.parametrize("name", sorted(SETS))
def test_twin_traces_satisfy_the_air(ora, prog, name):
    lh, calls = SETS[name]
    tr, hin, _, _ = fq.trace(ora, calls, lh)
    assert air.check_trace(prog, tr, NOPV) == []
    assert air.check_trace(air.fri_query_air(*BUSES).program(), tr, NOPV) == []
    assert (hin[:, :4].T == tr[fq.E0:fq.E0 + 4]).all() and (hin[:, 4:8].T == tr[fq.E1:fq.E1 + 4]).all()


def test_degree_and_padding(prog):
    for b in (air.fri_query_air(*BUSES), air.fri_query_air(*BUSES, 16), air.fri_query_air(*BUSES, None, 17), air.fri_query_air(*BUSES, 16, 17)):
        assert b.max_degree() == 3 and air.quotient_chunks(b.program()) == 2
        assert max(len(f) for (_, _, _, f) in b.interactions) == 32
    assert air.check_trace(prog, np.zeros((61, 8), np.uint32), NOPV) == []      # an all-zero row satisfies every line


def test_the_call_sets_reach_the_shapes_they_are_meant_for():
    assert fq.n_rows(SETS["full_16"][1]) == 16 == 1 << SETS["full_16"][0]
    assert fq.n_rows(SETS["one_row"][1]) == 1 == 1 << SETS["one_row"][0]
    assert fq.n_rows(SETS["rows_26"][1]) == 26 and SETS["rows_26"][1][0][1] == 27
    assert fq.n_rows(SETS["short_padded"][1]) < (1 << SETS["short_padded"][0]) // 2
    words = [int(w) for c in SETS["boundary_operands"][1] for k in (2, 4, 6, 7) for w in np.asarray(c[k]).reshape(-1)]
    assert 0 in words and P - 1 in words
    full = fq.call_sets()
    assert sorted(len(full["calls_%d" % n][1]) for n in (3, 4, 5, 65)) == [3, 4, 5, 65]
    assert [len(c[5]) for c in full["rows_15_16_17"][1]] == [15, 16, 17] and len(full["seventeen_one_row"][1]) == 17
    for name, (lh, calls) in full.items():               # every set is one the host definition accepts and the trace has room for
        assert fq.n_rows(calls) <= 1 << lh, name
        for index, lm, beta, _, sib, has, ro, top in calls[:70]:
            z.fri_query_host(index, lm, beta, sib, has, ro, top)


def _bump(t, col, row):
    w = t.copy()
    w[col][row] = (int(w[col][row]) + 1) % P
    return w


def test_every_constraint_family_refuses_its_mutation(ora, prog):
    rng = np.random.default_rng(5)
    calls = [fq.random_call(rng, 4, 9, 0b101101101, has=1), fq.random_call(rng, 1, 5, 9, has=0), fq.random_call(rng, 6, 12, None, has=None)]
    calls[2][5][:] = (1, 0, 1, 0, 0, 1)
    calls[2][6][:] = calls[2][6] * 0 + np.arange(1, 25).reshape(6, 4) * calls[2][5][:, None]   # rows 0..3 | 4 | 5..10, padding from 11
    t, _, _, _ = fq.trace(ora, calls, 4)
    assert air.check_trace(prog, t, NOPV) == []
    bad = lambda w: air.check_trace(prog, w, NOPV) != []  # noqa: E731
    # a flag: set on padding; not boolean; first / last moved
    for col in (fq.FIRST, fq.LAST, fq.REAL, fq.HAS_RO):
        w = t.copy()
        w[col][12] = 1
        assert bad(w)
        w = t.copy()
        w[col][7 if col != fq.LAST else 10] = 2
        assert bad(w)
    for col, row, v in ((fq.LAST, 3, 0), (fq.FIRST, 7, 1), (fq.FIRST, 0, 0), (fq.REAL, 6, 0)):
        w = t.copy()
        w[col][row] = v
        assert bad(w)
    w = t.copy()
    w[:, 13] = t[:, 4]                                  # a real row (a whole one-row call) after a padding row
    assert bad(w)
    # bit: not boolean; flipped (the chain and k = 2 k' + bit' both name it)
    w = t.copy()
    w[fq.BIT][2] = 2
    assert bad(w)
    w = t.copy()
    w[fq.BIT][2] = 1 - int(w[fq.BIT][2])
    assert bad(w)
    # k, lvl, call inside a call
    assert bad(_bump(t, fq.K, 1)) and bad(_bump(t, fq.K, 8)) and bad(_bump(t, fq.LVL, 2)) and bad(_bump(t, fq.LVL, 9)) and bad(_bump(t, fq.CALL, 6))
    # a bsq word, a folded word, an eval word -- on a last row too
    assert bad(_bump(t, fq.BSQ + 1, 2)) and bad(_bump(t, fq.FOLDED + 3, 6)) and bad(_bump(t, fq.EVAL, 5)) and bad(_bump(t, fq.EVAL + 2, 3))
    assert bad(_bump(t, fq.XINV, 4)) and bad(_bump(t, fq.BETA + 2, 7))
    # ro under has_ro = 0; has_ro cleared over a non-zero ro
    assert int(t[fq.HAS_RO][6]) == 0 and bad(_bump(t, fq.RO + 1, 6)) and bad(_bump(t, fq.RO, 4))
    w = t.copy()
    w[fq.HAS_RO][5] = 0
    assert bad(w)
    # the chained e word of a later row: the side the bit names
    for row in (1, 2, 3, 6, 10):
        side = fq.E1 if int(t[fq.BIT][row]) else fq.E0
        assert bad(_bump(t, side + 1, row))
    # the siblings swapped: e0 <-> e1 on a later row
    w = t.copy()
    w[fq.E0:fq.E0 + 4, 7], w[fq.E1:fq.E1 + 4, 7] = t[fq.E1:fq.E1 + 4, 7], t[fq.E0:fq.E0 + 4, 7]
    assert bad(w)
    # ... while the cells the buses bind are free for the constraints: the sibling (with folded and eval redone from it the row lines hold,
    # and on a last row nothing chains out of it), st_out, root, and the pair of a first row
    for row in (3, 4, 10):
        side = fq.E0 if int(t[fq.BIT][row]) else fq.E1
        w = _bump(t, side + 2, row)
        e0, e1 = w[fq.E0:fq.E0 + 4, row].tolist(), w[fq.E1:fq.E1 + 4, row].tolist()
        f = fq.fold(e0, e1, w[fq.BETA:fq.BETA + 4, row].tolist(), int(w[fq.XINV][row]))
        w[fq.FOLDED:fq.FOLDED + 4, row] = f
        w[fq.EVAL:fq.EVAL + 4, row] = [(a + b) % P for a, b in zip(f, fq.emul(w[fq.BSQ:fq.BSQ + 4, row].tolist(), w[fq.RO:fq.RO + 4, row].tolist()))]
        assert not bad(w)
    assert not bad(_bump(t, fq.ST_OUT + 5, 2)) and not bad(_bump(t, fq.ST_OUT + 12, 10)) and not bad(_bump(t, fq.ROOT + 3, 1)) and not bad(_bump(t, fq.ROOT, 4))
    # a call that runs into the last trace row without is_last
    full, _, _, _ = fq.trace(ora, [fq.random_call(rng, 11), fq.random_call(rng, 5)], 4)
    assert air.check_trace(prog, full, NOPV) == []
    w = full.copy()
    w[fq.LAST][15] = 0
    assert bad(w)


def test_the_reference_fold_rows_as_one_row_calls(prog):
    """tests/golden/ref_v1_vectors.json `fri_layers`: the reference's own (k, log_n_out, beta, e0, e1, folded), laid out as one-row
    calls with ro = 0 -- the fold and bsq lines on numbers this code base did not produce"""
    with open(os.path.join(HERE, "golden", "ref_v1_vectors.json")) as f:
        vec = json.load(f)
    rows = [(t_["k"], lay["log_n_out"], lay["beta"], t_["e0"], t_["e1"], t_["folded"]) for lay in vec["fri_layers"] for t_ in lay["triples"]]
    assert len(rows) >= 16 and len({r[1] for r in rows}) >= 3
    lh = int(np.ceil(np.log2(len(rows))))
    t = np.zeros((61, 1 << lh), np.uint32)
    for r, (k, h, beta, e0, e1, folded) in enumerate(rows):
        t[fq.E0:fq.E0 + 4, r], t[fq.E1:fq.E1 + 4, r], t[fq.BETA:fq.BETA + 4, r] = e0, e1, beta
        t[fq.BSQ:fq.BSQ + 4, r] = fq.emul(beta, beta)
        t[fq.XINV, r], t[fq.FOLDED:fq.FOLDED + 4, r], t[fq.EVAL:fq.EVAL + 4, r] = fq.x_inv(k), folded, folded
        t[fq.K, r], t[fq.LVL, r], t[fq.FIRST, r], t[fq.LAST, r], t[fq.REAL, r], t[fq.CALL, r] = k, h, 1, 1, 1, r
    assert air.check_trace(prog, t, NOPV) == []
    assert air.check_trace(prog, _bump(t, fq.FOLDED, 1), NOPV) != []


def test_the_honest_instance_chains_into_its_own_layers(ora, prog):
    for lm, seed in ((5, 7), (6, 8)):
        inst = fq.fri_instance(ora, z, lm, seed)          # (asserts eval = the next layer's value and every opening against zkhip_mmcs_verify)
        assert len(inst.calls) == 12 and inst.indices[0] >> 2 == inst.indices[1] >> 2 == inst.indices[2] >> 2
        lh = int(np.ceil(np.log2(fq.n_rows(inst.calls))))
        tr, _, leaf, fin = fq.trace(ora, inst.calls, lh)
        assert air.check_trace(prog, tr, NOPV) == []
        for c, idx in enumerate(inst.indices):
            assert (fin[c] == inst.layers[inst.n_layers][idx >> inst.n_layers]).all()
        # the leaf digests are what the trees hold: layer 0 of every commitment at k
        for r, (l, h, k, op) in enumerate(inst.openings):
            assert (inst.trees[l].layer(0)[k] == leaf[r]).all()


def test_cpp_twin_emits_the_same_program(tmp_path):
    exe = str(tmp_path / "fri_query_cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fri_query_cpp.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [ln.split()[0] for ln in lines] == ["fri_query", "fri_query_all", "fri_query_final"]
    for line, b in zip(lines, (air.fri_query_air(*BUSES), air.fri_query_air(*BUSES, 16, 17), air.fri_query_air(*BUSES, None, 17))):
        _, deg, *words = line.split()
        want = b.program()
        got = np.array([int(x) for x in words], dtype=np.uint32)
        assert len(got) == len(want), (len(got), len(want))
        assert (got == want).all(), "first difference at word %d" % int(np.nonzero(got != want)[0][0])
        assert int(deg) == b.max_degree() == 3


def test_host_function_alone_under_the_sanitizers(tmp_path):
    """csrc/fri_query_host.hpp with the verifier whose fold_row it calls and tests/fri_query_host_main.cpp, a program of its own (nothing
    loaded into this interpreter runs under a sanitizer): clean on heap blocks of exactly n_layers records, and what it prints is the twin's."""
    exe = str(tmp_path / "fri_query_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DZK_NO_HOST_AVX512",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fri_query_host_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert [tuple(int(x) for x in ln.split("|")[0].split()) for ln in lines] == [(0, 2, 1), (3, 2, 1), (5, 3, 2), ((1 << 27) - 1, 27, 26), (0, 27, 26), (0x2A5A5A5, 27, 13), (77, 7, 6)]
    for ln in lines:
        head, *parts = [[int(x) for x in p.split()] for p in ln.split("|")]
        index, lm, n = head
        beta, sib, has, ro, top, e0, e1, ev = parts
        sh = lambda v: np.array(v).reshape(n, 4)  # noqa: E731
        want = fq.chain_int(index, lm, sh(beta), sh(sib), has, sh(ro), top)
        assert sh(e0).tolist() == [w[0] for w in want] and sh(e1).tolist() == [w[1] for w in want] and sh(ev).tolist() == [w[2] for w in want]
        assert 0 in beta + sib and P - 1 in beta + sib
