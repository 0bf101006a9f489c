"""GPU: the row-digest chip's device generator (csrc/mmcs_rows.hip: 16 lanes per call, four calls per wave, one flat loop with the next
call from a device counter, rows staged through LDS) against the twin over the oracle's permutation, word for word, at every shape where
the kernel takes another path; the refusals, at once and deferred; and the composition the chip exists for: row-digest chip + MMCS path
chip + two Poseidon2 chips prove that the opened words of the reference's stored proofs lead to the roots those proofs carry, with no
claims table."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmcs_path_util as mu  # noqa: E402
import mmcs_rows_util as mr  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NOPV = np.zeros(0, np.uint32)
PARAMS = (1, 0, 12, 4, 4)
P = mr.P
SETS = mr.call_sets()


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(HERE, "golden", "ref_v1_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def prog():
    return air.mmcs_rows_air(11, 10).program()


def _dev(zk, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)


def _generate(zk, arrays, lh, digests=True):
    return zk.mmcs_rows_tracegen(*[_dev(zk, a) for a in arrays], lh, digests=digests)


def _same(got, want, what):
    if not (got == want).all():
        where = [int(x[0]) for x in np.nonzero(got != want)]
        pytest.fail("%s: first difference at %s (%d cells differ)" % (what, where, int((got != want).sum())))


def _check_shape(zk, ora, prog, arrays, lh):
    """device trace and hash inputs == the twin word for word, digests == ora_hash_slice (the twin asserts its own against it), and
    check_trace empty on the DEVICE trace"""
    want, want_hin, want_dg = mr.trace_np(ora, *arrays, lh)
    d_tr, d_hin, d_dg = _generate(zk, arrays, lh)
    got = zk.download(d_tr).reshape(56, -1)
    _same(got, want, "trace [column, row]")
    _same(zk.download(d_hin).reshape(-1, 16), want_hin, "hash inputs [row, lane]")
    zk.sync()
    _same(d_dg.cpu().numpy().view(np.uint32).reshape(-1, 8), want_dg, "digests [call, word]")
    assert air.check_trace(prog, got, NOPV) == []
    return got


@pytest.mark.parametrize("name", list(SETS))
def test_device_trace_equals_the_twin(zk, ora, prog, name):
    lh, calls = SETS[name]
    got = _check_shape(zk, ora, prog, mr.records(calls), lh)
    rows = sum((len(c[0]) + 7) // 8 for c in calls)
    assert (got[:, rows:] == 0).all()          # padding rows zero


def test_a_call_count_at_which_the_offset_kernels_loop(zk, ora, prog):
    """2^18 + 4096 calls of one word: a workgroup of the shared offset kernels covers 512 calls (two rounds of its scan) and 513 workgroups
    have slices in front of them -- for both scans, of the words and of the rows."""
    n_calls = (1 << 18) + 4096
    assert n_calls > 1024 * z.REDUCED_OPENING_BLOCK_ROWS
    _check_shape(zk, ora, prog, mr.many_one_word_calls(n_calls), 19)


def test_two_runs_give_identical_words(zk):
    lh, calls = SETS["imbalance"]
    one, two = _generate(zk, mr.records(calls), lh), _generate(zk, mr.records(calls), lh)
    zk.sync()
    assert all(torch.equal(a, b) for a, b in zip(one, two))


def test_no_calls_is_padding_only(zk):
    e = torch.empty(0, dtype=torch.int32, device=zk.device)
    tr, hin, dg = zk.mmcs_rows_tracegen(e, e, e, e, e, e, 3)
    assert (zk.download(tr) == 0).all() and (zk.download(hin) == 0).all() and dg.numel() == 0


def test_a_null_digest_pointer_is_accepted(zk, ora):
    lh, calls = SETS["calls_5"]
    tr, hin, dg = _generate(zk, mr.records(calls), lh, digests=False)
    assert dg is None
    want, want_hin, _ = mr.trace(ora, calls, lh)
    assert (zk.download(tr).reshape(56, -1) == want).all() and (zk.download(hin).reshape(-1, 16) == want_hin).all()


def _refusal_cases():
    rng = np.random.default_rng(2)
    calls = mr.random_calls(rng, [3, 20, 1, 70])
    lens, root, lvl, idx, mult, values = mr.records(calls)
    good = dict(lens=lens, root=root, lvl=lvl, idx=idx, mult=mult, values=values, lh=4)
    u = lambda *v: np.array(v, np.uint32)  # noqa: E731
    device = [dict(lens=u(3, 20, 0, 71)),              # a length of 0 (the sum still n_words)
              dict(lens=u(3, 20, 1, 69)),              # the lengths fall short of n_words
              dict(lens=u(3, 20, 1, 71)),              # ... run past it
              dict(lens=u(3, 20, 1, 0xFFFFFFFF)),      # ... by far
              dict(lens=np.ones(9, np.uint32), root=np.zeros((9, 8), np.uint32), lvl=np.zeros(9, np.uint32), idx=np.zeros(9, np.uint32),
                   mult=np.zeros(9, np.uint32), values=np.ones(9, np.uint32), lh=3)]   # 9 rows > 2^3 (9 words <= 8 * 2^3: not refused on the host)
    for i in (0, 23, 93):
        w = values.copy()
        w[i] = P
        device.append(dict(values=w))
    for name, arr in (("root", root), ("lvl", lvl), ("idx", idx), ("mult", mult)):
        w = arr.copy()
        w.reshape(-1)[-1] = P
        device.append({name: w})
        w = arr.copy()
        w.reshape(-1)[0] = 0xFFFFFFFF
        device.append({name: w})
    host = [dict(lens=np.zeros(0, np.uint32), root=np.zeros((0, 8), np.uint32), lvl=np.zeros(0, np.uint32), idx=np.zeros(0, np.uint32),
                 mult=np.zeros(0, np.uint32)),         # words but no call
            dict(lh=3),                                # 94 words > 8 * 2^3
            dict(lens=np.ones(95, np.uint32), root=np.zeros((95, 8), np.uint32), lvl=np.zeros(95, np.uint32), idx=np.zeros(95, np.uint32),
                 mult=np.zeros(95, np.uint32))]        # n_calls > n_words
    return calls, good, device, host


def _call(zk, good, case):
    a = dict(good, **case)
    return _generate(zk, [a[k] for k in ("lens", "root", "lvl", "idx", "mult", "values")], a["lh"])


def test_refusals(zk, ora):
    calls, good, device, host = _refusal_cases()
    _call(zk, good, {})
    for case in device + host:
        with pytest.raises(z.ZkhipError) as e:
            _call(zk, good, case)
        assert e.value.code == -3, case   # ZKHIP_ERR_INVALID
    # on the host before any launch: NULL pointers and log_height > 27 (called below the binding, which would allocate the trace)
    t = [_dev(zk, good[k]) for k in ("lens", "root", "lvl", "idx", "mult", "values")]
    ptr = [t_.data_ptr() for t_ in t]
    out = torch.empty(56 << 4, dtype=torch.int32, device=zk.device)
    hin = torch.empty(16 << 4, dtype=torch.int32, device=zk.device)
    f = zk.lib.zkhip_mmcs_rows_tracegen
    assert f(zk.h, *ptr, 4, 94, 4, out.data_ptr(), hin.data_ptr(), None) == 0
    assert f(zk.h, *ptr, 4, 94, 28, out.data_ptr(), hin.data_ptr(), None) == -3
    assert f(zk.h, *ptr, 4, 94, 4, None, hin.data_ptr(), None) == -3
    assert f(zk.h, *ptr, 4, 94, 4, out.data_ptr(), None, None) == -3
    for i in range(6):
        assert f(zk.h, *[None if j == i else p for j, p in enumerate(ptr)], 4, 94, 4, out.data_ptr(), hin.data_ptr(), None) == -3
    assert f(None, *ptr, 4, 94, 4, out.data_ptr(), hin.data_ptr(), None) == -3
    # and the generator is as it was
    tr, _, _ = _call(zk, good, {})
    assert (zk.download(tr).reshape(56, -1) == mr.trace(ora, calls, 4)[0]).all()


def test_refusals_with_deferred_checks(zk, ora):
    """under zkhip_tracegen_defer_checks the call itself returns OK and zkhip_tracegen_check reports, once, and resets"""
    calls, good, device, _ = _refusal_cases()
    assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 1) == 0
    try:
        _call(zk, good, {})
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        for case in device:
            _call(zk, good, case)                                 # no verdict yet
            assert zk.lib.zkhip_tracegen_check(zk.h) == -3, case
            assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        tr, _, _ = _call(zk, good, {})
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        assert (zk.download(tr).reshape(56, -1) == mr.trace(ora, calls, 4)[0]).all()
    finally:
        zk.lib.zkhip_tracegen_check(zk.h)
        assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 0) == 0


def test_the_call_has_its_profile_scope(zk):
    lh, calls = SETS["calls_5"]
    zk.profile_enable(True)
    zk.profile_reset()
    _generate(zk, mr.records(calls), lh)
    zk.sync()
    stats = zk.profile_read()
    zk.profile_enable(False)
    assert stats["mmcs_rows_tracegen"][0] == 1


# ---- the composition: opened words -> row digests -> paths -> roots, four AIRs, no claims table ------------------------------------------
def _lh(rows):
    return max(1, int(np.ceil(np.log2(max(rows, 2)))))


def _poseidon_chip(zk, d_hin, lh, rows):
    """the Poseidon2 chip's trace on the device from a generator's hash inputs, mult = 1 on the real rows"""
    N = 1 << lh
    d = torch.empty(299 * N, dtype=torch.int32, device=zk.device)
    zk.poseidon2_air_tracegen(d_hin, lh, d)
    m = np.zeros(N, np.uint32)
    m[:rows] = 1
    d[298 * N:] = zk.upload(m)
    return d


def _device_traces(zk, vec, limit, calls, path, lh_rows, lh_path):
    """row-digest rows from the calls; the path chip's leaf and injected digests taken on the DEVICE from the generator's d_digest (the
    sibling digests are the proof's); both Poseidon2 chips from the two generators' hash inputs"""
    leaf, idx, starts, kinds, digs = path
    rows = sum((len(c[0]) + 7) // 8 for c in calls)
    d_rows, d_hin_rows, d_dg = _generate(zk, mr.records(calls), lh_rows)
    lc, ip, ic = mr.path_digest_sources(vec, calls, limit)
    dg = d_dg.view(-1, 8)
    as_idx = lambda v: torch.from_numpy(v).to(zk.device)  # noqa: E731
    d_leaf = dg[as_idx(lc)].contiguous()
    d_digs = _dev(zk, digs).view(-1, 8).clone()
    d_digs[as_idx(ip)] = dg[as_idx(ic)]
    d_path, d_hin_path = zk.mmcs_path_tracegen(d_leaf.view(-1), _dev(zk, idx), _dev(zk, starts), _dev(zk, kinds), d_digs.view(-1), lh_path)
    return [d_rows, d_path, _poseidon_chip(zk, d_hin_path, lh_path, int(starts[-1])), _poseidon_chip(zk, d_hin_rows, lh_rows, rows)]


def _composition(zk, ora, vec, limit):
    calls = mr.calls_of_fixture(ora, vec, limit)
    leaf, idx, starts, kinds, digs, want = mu.records_of_fixture(ora, vec, limit)
    rows, prow = sum((len(c[0]) + 7) // 8 for c in calls), int(starts[-1])
    lh_rows, lh_path = _lh(rows), _lh(prow)
    t_rows, hin_rows, dg = mr.trace(ora, calls, lh_rows)
    assert sorted(mr.claims_of(calls, dg)) == sorted(want)
    t_path, hin_path, claims, bad = ora.mmcs_path_trace(leaf, idx, starts, kinds, digs, lh_path)
    assert bad == 0
    roots = {tuple(int(x) for x in b["root"]) for q in vec["openings"][:limit] for b in q["batches"]}
    assert {tuple(t_path[:8, r].tolist()) for r in range(prow)} <= roots      # the walks end in the roots the reference's proofs carry

    def chip(hin, lh, n):
        full = np.zeros((1 << lh, 16), np.uint32)
        full[:n] = hin[:n]
        t = np.zeros((299, 1 << lh), np.uint32)
        t[:298] = ora.poseidon2_air_trace(full, lh)
        t[298, :n] = 1
        return t

    A = lambda prog, w, t: dict(program=prog, log_height=int(np.log2(t.shape[1])), width=w, n_pvs=0, trace=t, pvs=NOPV)  # noqa: E731
    airs = [A(air.mmcs_rows_air(11, 10).program(), 56, t_rows), A(air.mmcs_path_air(9, 10).program(), 39, t_path),
            A(air.poseidon2_air(9).program(), 299, chip(hin_path, lh_path, prow)), A(air.poseidon2_air(11, out_lanes=16).program(), 299, chip(hin_rows, lh_rows, rows))]
    path = (leaf, idx, starts, kinds, digs)
    d = _device_traces(zk, vec, limit, calls, path, lh_rows, lh_path)
    for dt, a in zip(d, airs):
        assert (zk.download(dt).reshape(a["width"], -1) == a["trace"]).all()
    return calls, path, airs, d, lh_rows, lh_path


def test_opened_words_lead_to_the_roots_in_circuit(zk, ora, vec):
    """the fixture's first two queries: proof bytes == the oracle's, the host verifier accepts; one changed opened word or one changed
    mult and the claims bus no longer balances"""
    calls, path, airs, d, lh_rows, lh_path = _composition(zk, ora, vec, 2)
    pk = z.ProvingKey(zk, PARAMS, airs)
    proof = pk.prove(d, [NOPV] * 4)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 4, proof) == 0
    assert proof == ora.stark_prove(PARAMS, airs).tobytes()
    # one opened word changed: the generators produce another digest, the path chip walks from it to another root
    c = next(i for i, x in enumerate(calls) if len(x[0]) > 9)
    words = list(calls[c][0])
    words[9] = (words[9] + 1) % P
    wrong = calls[:c] + [(words,) + tuple(calls[c][1:])] + calls[c + 1:]
    d2 = _device_traces(zk, vec, 2, wrong, path, lh_rows, lh_path)
    assert not torch.equal(d2[1], d[1])
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 4, pk.prove(d2, [NOPV] * 4)) != 0
    # one mult changed
    wrong = [tuple(x[:4]) + (x[4] + 1,) if i == 3 else x for i, x in enumerate(calls)]
    d3 = _device_traces(zk, vec, 2, wrong, path, lh_rows, lh_path)
    assert torch.equal(d3[1], d[1]) and not torch.equal(d3[0], d[0])
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 4, pk.prove(d3, [NOPV] * 4)) != 0
    pk.close()


def test_all_twelve_queries_with_the_host_verifier(zk, ora, vec):
    calls, path, airs, d, _, _ = _composition(zk, ora, vec, None)
    assert len(vec["openings"]) == 12 and len(calls) == 319 and max(c[4] for c in calls) > 1
    pk = z.ProvingKey(zk, PARAMS, airs)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 4, pk.prove(d, [NOPV] * 4)) == 0
    pk.close()


def _values_receiver_air(bus):
    """test-local: columns call | pos | value | mult; takes each row `mult` times from the chip's values bus"""
    b = air.AirBuilder(4, 0)
    b.push_interaction(bus, [b.var(i) for i in range(3)], b.var(3), "receive")
    return b


def test_values_bus_against_a_receiver(zk, ora):
    """mmcs_rows_air(11, 10, 12) on the DEVICE trace, the Poseidon2 chip serving its hash bus, and a table of (call, position, word) rows:
    accepted; refused after one table word changes.  Every mult is 0 here: nobody sends claims, and mult = 0 is harmless."""
    rng = np.random.default_rng(13)
    calls = [mr.random_call(rng, L, 0) for L in (1, 8, 9, 17, 40, 3, 16)]
    rows, n_words = sum((len(c[0]) + 7) // 8 for c in calls), sum(len(c[0]) for c in calls)
    lh, lt = _lh(rows), _lh(n_words)
    table = mr.values_table(calls, lt)
    d_tr, d_hin, _ = _generate(zk, mr.records(calls), lh)
    tr = zk.download(d_tr).reshape(56, -1)
    assert (tr == mr.trace(ora, calls, lh)[0]).all()
    d_chip = _poseidon_chip(zk, d_hin, lh, rows)
    airs = [dict(program=air.mmcs_rows_air(11, 10, 12).program(), log_height=lh, width=56, n_pvs=0, trace=tr, pvs=NOPV),
            dict(program=air.poseidon2_air(11, out_lanes=16).program(), log_height=lh, width=299, n_pvs=0, trace=zk.download(d_chip).reshape(299, -1), pvs=NOPV),
            dict(program=_values_receiver_air(12).program(), log_height=lt, width=4, n_pvs=0, trace=table, pvs=NOPV)]
    pk = z.ProvingKey(zk, PARAMS, airs)
    proof = pk.prove([d_tr, d_chip, zk.upload(table.reshape(-1))], [NOPV] * 3)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 3, proof) == 0
    wrong = table.copy()
    wrong[2][11] = (int(wrong[2][11]) + 1) % P
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 3, pk.prove([d_tr, d_chip, zk.upload(wrong.reshape(-1))], [NOPV] * 3)) != 0
    pk.close()


def test_an_unrelated_key_proves_the_same_bytes_around_a_generator_call(zk):
    fa = air.fibonacci_air()
    ftr, fpv = air.fibonacci_trace(8)
    airs = [dict(program=fa.program(), log_height=8, width=2, n_pvs=3, trace=ftr, pvs=fpv)]
    pk = z.ProvingKey(zk, (1, 0, 8, 3, 4), airs)
    d = zk.upload(ftr.reshape(-1))
    before = pk.prove([d], [fpv])
    lh, calls = SETS["stage_boundaries"]
    _generate(zk, mr.records(calls), lh)
    after = pk.prove([d], [fpv])
    assert before == after and z.verify((1, 0, 8, 3, 4), pk.verifying_airs(), [fpv], after) == 0
    pk.close()
