"""GPU: the FRI query chip's device generator (csrc/fri_query.hip: a chain kernel with one lane per call, then one lane per row for the
fold lines and the permutation) against the twin, word for word, at every shape where the kernels take another path; the refusals, at once
and deferred; and the composition the chip exists for: on an honest FRI instance built from the oracle's primitives, the query chip, the
MMCS path chip, the two Poseidon2 chips and the domain-point chip prove that every query's fold loop runs from the reduced openings through
leaves of the committed layers to the final layer's value."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_query_util as fq  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

pytestmark = pytest.mark.gpu
NOPV = np.zeros(0, np.uint32)
PARAMS = (1, 0, 12, 4, 4)
P = fq.P
SETS = fq.call_sets()
NAMES = ("n_layers", "log_max", "index", "ro_top", "beta", "root", "sibling", "has_ro", "ro")


@pytest.fixture(scope="module")
def prog():
    return air.fri_query_air(14, 11, 10, 15, 16, 17).program()


def _dev(zk, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)


def _generate(zk, arrays, lh, **kw):
    return zk.fri_query_tracegen(*[_dev(zk, a) for a in arrays], lh, **kw)


def _same(got, want, what):
    if not (got == want).all():
        where = [int(x[0]) for x in np.nonzero(got != want)]
        pytest.fail("%s: first difference at %s (%d cells differ)" % (what, where, int((got != want).sum())))


def _check_shape(zk, ora, prog, arrays, lh):
    """device trace, hash inputs, leaf digests and final evals == the twin word for word, and check_trace empty on the DEVICE trace"""
    want, want_hin, want_leaf, want_fin = fq.trace_np(ora, *arrays, lh)
    d_tr, d_hin, d_leaf, d_fin = _generate(zk, arrays, lh)
    got = zk.download(d_tr).reshape(61, -1)
    _same(got, want, "trace [column, row]")
    _same(zk.download(d_hin).reshape(-1, 16), want_hin, "hash inputs [row, lane]")
    zk.sync()
    _same(d_leaf.cpu().numpy().view(np.uint32).reshape(-1, 8), want_leaf, "leaf digests [row, word]")
    _same(d_fin.cpu().numpy().view(np.uint32).reshape(-1, 4), want_fin, "final evals [call, word]")
    assert air.check_trace(prog, got, NOPV) == []
    return got


@pytest.mark.parametrize("name", list(SETS))
def test_device_trace_equals_the_twin(zk, ora, prog, name):
    lh, calls = SETS[name]
    got = _check_shape(zk, ora, prog, fq.records(calls), lh)
    assert (got[:, fq.n_rows(calls):] == 0).all()          # padding rows zero


def test_a_call_count_at_which_the_offset_kernels_loop(zk, ora, prog):
    """2^18 + 4096 calls of one row: a workgroup of the shared offset kernels covers 512 calls (two rounds of its scan) and 513 workgroups
    have slices in front of them; the row kernel's search runs over 2^18 + 4097 offsets"""
    n_calls = (1 << 18) + 4096
    assert n_calls > 1024 * z.REDUCED_OPENING_BLOCK_ROWS
    _check_shape(zk, ora, prog, fq.many_one_row_calls(n_calls), 19)


def test_two_runs_give_identical_words(zk):
    lh, calls = SETS["calls_65"]
    one, two = _generate(zk, fq.records(calls), lh), _generate(zk, fq.records(calls), lh)
    zk.sync()
    assert all(torch.equal(a, b) for a, b in zip(one, two))


def test_no_calls_is_padding_only(zk):
    e = torch.empty(0, dtype=torch.int32, device=zk.device)
    tr, hin, leaf, fin = zk.fri_query_tracegen(e, e, e, e, e, e, e, e, e, 3)
    assert (zk.download(tr) == 0).all() and (zk.download(hin) == 0).all() and leaf.numel() == 0 and fin.numel() == 0


@pytest.mark.parametrize("leaf_digests,final", [(False, True), (True, False), (False, False)])
def test_null_output_pointers_are_accepted(zk, ora, leaf_digests, final):
    lh, calls = SETS["calls_5"]
    tr, hin, leaf, fin = _generate(zk, fq.records(calls), lh, leaf_digests=leaf_digests, final=final)
    assert (leaf is None) == (not leaf_digests) and (fin is None) == (not final)
    want, want_hin, want_leaf, want_fin = fq.trace(ora, calls, lh)
    assert (zk.download(tr).reshape(61, -1) == want).all() and (zk.download(hin).reshape(-1, 16) == want_hin).all()
    zk.sync()
    if leaf is not None:
        assert (leaf.cpu().numpy().view(np.uint32).reshape(-1, 8) == want_leaf).all()
    if fin is not None:
        assert (fin.cpu().numpy().view(np.uint32).reshape(-1, 4) == want_fin).all()


def _refusal_cases():
    rng = np.random.default_rng(2)
    calls = [fq.random_call(rng, 3, 9, has=1), fq.random_call(rng, 5, 6, has=0), fq.random_call(rng, 1, 2, has=1), fq.random_call(rng, 4, 20)]
    good = dict(zip(NAMES, fq.records(calls)), lh=4)
    u = lambda *v: np.array(v, np.uint32)  # noqa: E731
    one = [np.ones(9, np.uint32), np.full(9, 5, np.uint32), np.zeros(9, np.uint32), np.zeros((9, 4), np.uint32), np.zeros((9, 4), np.uint32),
           np.zeros((9, 8), np.uint32), np.zeros((9, 4), np.uint32), np.zeros(9, np.uint32), np.zeros((9, 4), np.uint32)]
    device = [dict(n_layers=u(3, 5, 0, 5)),            # a length of 0 (the sum still n_rows)
              dict(n_layers=u(3, 5, 1, 3)),            # the lengths fall short of n_rows
              dict(n_layers=u(3, 5, 1, 5)),            # ... run past it
              dict(n_layers=u(3, 5, 1, 0xFFFFFFFF)),   # ... by far
              dict(n_layers=u(2, 6, 1, 4)),            # the sum is n_rows, but 6 layers > log_max - 1 = 5
              dict(zip(NAMES, one), lh=3),             # 9 rows > 2^3
              dict(log_max=u(9, 6, 2, 28)), dict(log_max=u(9, 6, 2, 0xFFFFFFFF)), dict(log_max=u(9, 5, 2, 20)), dict(log_max=u(3, 6, 2, 20)),
              dict(index=u(1 << 9, 0, 0, 0)), dict(index=u(0, 0, 4, 0)), dict(index=u(0, 0, 0, 0xFFFFFFFF)),
              dict(has_ro=np.where(np.arange(13) == 7, 2, good["has_ro"]).astype(np.uint32)),
              dict(has_ro=np.where(np.arange(13) == 0, 0xFFFFFFFF, good["has_ro"]).astype(np.uint32)),
              dict(has_ro=np.where(np.arange(13) == 1, 0, good["has_ro"]).astype(np.uint32)),    # a non-zero ro under has_ro = 0
              dict(zip(NAMES, [a[:0] for a in fq.records(calls)[:4]] + list(fq.records(calls)[4:])))]   # rows but no call
    for name in ("ro_top", "beta", "root", "sibling", "ro"):
        for pos, v in ((-1, P), (0, 0xFFFFFFFF)):
            w = good[name].copy()
            w.reshape(-1)[pos] = v
            device.append({name: w})
    host = [dict(zip(NAMES, [np.ones(2, np.uint32), u(5, 5), u(0, 0), np.zeros((2, 4), np.uint32)] + [a[:1] for a in one[4:]]))]   # n_calls > n_rows
    return calls, good, device, host


def _call(zk, good, case):
    a = dict(good, **case)
    return _generate(zk, [a[k] for k in NAMES], a["lh"])


def test_refusals(zk, ora):
    calls, good, device, host = _refusal_cases()
    _call(zk, good, {})
    for case in device + host:
        with pytest.raises(z.ZkhipError) as e:
            _call(zk, good, case)
        assert e.value.code == -3, case   # ZKHIP_ERR_INVALID
    # on the host before any launch: NULL pointers and log_height > 27 (called below the binding, which would allocate the trace)
    t = [_dev(zk, good[k]) for k in NAMES]
    ptr = [t_.data_ptr() for t_ in t]
    out = torch.empty(61 << 4, dtype=torch.int32, device=zk.device)
    hin = torch.empty(16 << 4, dtype=torch.int32, device=zk.device)
    f = zk.lib.zkhip_fri_query_tracegen
    assert f(zk.h, *ptr, 4, 13, 4, out.data_ptr(), hin.data_ptr(), None, None) == 0
    assert f(zk.h, *ptr, 4, 13, 28, out.data_ptr(), hin.data_ptr(), None, None) == -3
    assert f(zk.h, *ptr, 4, 13, 4, None, hin.data_ptr(), None, None) == -3
    assert f(zk.h, *ptr, 4, 13, 4, out.data_ptr(), None, None, None) == -3
    for i in range(9):
        assert f(zk.h, *[None if j == i else p for j, p in enumerate(ptr)], 4, 13, 4, out.data_ptr(), hin.data_ptr(), None, None) == -3
    assert f(None, *ptr, 4, 13, 4, out.data_ptr(), hin.data_ptr(), None, None) == -3
    assert f(zk.h, *ptr, 14, 13, 4, out.data_ptr(), hin.data_ptr(), None, None) == -3     # n_calls > n_rows
    # and the generator is as it was
    tr = _call(zk, good, {})[0]
    assert (zk.download(tr).reshape(61, -1) == fq.trace(ora, calls, 4)[0]).all()


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
        tr = _call(zk, good, {})[0]
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        assert (zk.download(tr).reshape(61, -1) == fq.trace(ora, calls, 4)[0]).all()
    finally:
        zk.lib.zkhip_tracegen_check(zk.h)
        assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 0) == 0


def test_the_call_has_its_profile_scope(zk):
    lh, calls = SETS["calls_5"]
    zk.profile_enable(True)
    zk.profile_reset()
    _generate(zk, fq.records(calls), lh)
    zk.sync()
    stats = zk.profile_read()
    zk.profile_enable(False)
    assert stats["fri_query_tracegen"][0] == 1


# ---- the composition: reduced openings -> fold loop -> leaves of the committed layers -> the final layer's value ---------------------------
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


def _sender_air(bus, width):
    """test-local: a plain table that SENDS its first width - 1 columns with multiplicity the last (the reduced openings' side)"""
    b = air.AirBuilder(width, 0)
    b.push_interaction(bus, [b.var(i) for i in range(width - 1)], b.var(width - 1), "send")
    return b


def _receiver_air(bus, width):
    b = air.AirBuilder(width, 0)
    b.push_interaction(bus, [b.var(i) for i in range(width - 1)], b.var(width - 1), "receive")
    return b


def _domain_point_records(tr, rows):
    ks, counts = np.unique(tr[fq.K, :rows], return_counts=True)
    return ks.astype(np.uint32), counts.astype(np.uint32)


def _domain_point_trace(ks, mults, lh):
    t = np.zeros((54, 1 << lh), np.uint32)
    t[27:53] = 1                                            # acc of a padding row: k = 0, the empty product
    for r, (k, m) in enumerate(zip(ks.tolist(), mults.tolist())):
        acc = 1
        t[0, r], t[53, r] = k, m
        for j in range(26):
            bit = (k >> j) & 1
            acc = acc * (fq.WINV[j] if bit else 1) % P
            t[1 + j, r], t[27 + j, r] = bit, acc
    return t


def _device_traces(zk, inst, calls, lh_q, lh_p, ks, mults, lh_d):
    """query rows from the calls; the path chip's leaves taken on the DEVICE from the generator's d_leaf_digest (the sibling digests are
    the openings'); both Poseidon2 chips from the two generators' hash inputs; the domain points from the pair indices"""
    rows = fq.n_rows(calls)
    d_q, d_hin_q, d_leaf, d_fin = _generate(zk, fq.records(calls), lh_q)
    idx, starts, kinds, digs = fq.path_records(inst)
    d_path, d_hin_path = zk.mmcs_path_tracegen(d_leaf, _dev(zk, idx), _dev(zk, starts), _dev(zk, kinds), _dev(zk, digs.reshape(-1)), lh_p)
    d_dp = zk.domain_point_tracegen(_dev(zk, ks), _dev(zk, mults), lh_d)
    return [d_q, d_path, _poseidon_chip(zk, d_hin_path, lh_p, int(starts[-1])), _poseidon_chip(zk, d_hin_q, lh_q, rows), d_dp], d_fin


def test_the_fold_loop_in_circuit_on_an_honest_instance(zk, ora):
    """proof bytes == the oracle's, the host verifier accepts; one changed sibling word, one changed ro word or one changed word of the
    final table and a bus no longer balances"""
    inst = fq.fri_instance(ora, z, 5, 7)
    calls, rows = inst.calls, fq.n_rows(inst.calls)
    idx, starts, kinds, digs = fq.path_records(inst)
    lh_q, lh_p = _lh(rows), _lh(int(starts[-1]))
    t_q, hin_q, leaf, fin = fq.trace(ora, calls, lh_q)
    t_path, hin_path, claims, bad = ora.mmcs_path_trace(leaf, idx, starts, kinds, digs, lh_p)
    assert bad == 0
    ks, mults = _domain_point_records(t_q, rows)
    lh_d = _lh(len(ks))
    t_dp = _domain_point_trace(ks, mults, lh_d)
    t_ro, t_layer, t_final = fq.bus_tables(inst)

    def chip(hin, lh, n):
        full = np.zeros((1 << lh, 16), np.uint32)
        full[:n] = hin[:n]
        t = np.zeros((299, 1 << lh), np.uint32)
        t[:298] = ora.poseidon2_air_trace(full, lh)
        t[298, :n] = 1
        return t

    A = lambda b, t: dict(program=b.program(), log_height=int(np.log2(t.shape[1])), width=t.shape[0], n_pvs=0, trace=t, pvs=NOPV)  # noqa: E731
    airs = [A(air.fri_query_air(14, 11, 10, 15, 16, 17), t_q), A(air.mmcs_path_air(9, 10), t_path), A(air.poseidon2_air(9), chip(hin_path, lh_p, int(starts[-1]))),
            A(air.poseidon2_air(11, out_lanes=16), chip(hin_q, lh_q, rows)), A(air.domain_point_air(14), t_dp),
            A(_sender_air(15, 7), t_ro), A(_receiver_air(16, 15), t_layer), A(_receiver_air(17, 8), t_final)]
    for a in airs:
        assert a["width"] == 299 or air.check_trace(a["program"], a["trace"], NOPV) == []
    tables = lambda ro=t_ro, final=t_final: [zk.upload(t.reshape(-1)) for t in (ro, t_layer, final)]  # noqa: E731
    d, d_fin = _device_traces(zk, inst, calls, lh_q, lh_p, ks, mults, lh_d)
    for dt, a in zip(d, airs):
        assert (zk.download(dt).reshape(a["width"], -1) == a["trace"]).all(), a["width"]
    zk.sync()
    assert (d_fin.cpu().numpy().view(np.uint32).reshape(-1, 4) == fin).all() and (fin == t_final[3:7, :len(calls)].T).all()
    n = len(airs)
    pk = z.ProvingKey(zk, PARAMS, airs)
    proof = pk.prove(d + tables(), [NOPV] * n)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * n, proof) == 0
    assert proof == ora.stark_prove(PARAMS, airs).tobytes()

    def refused(calls2, **kw):
        d2, _ = _device_traces(zk, inst, calls2, lh_q, lh_p, ks, mults, lh_d)
        return d2, z.verify(PARAMS, pk.verifying_airs(), [NOPV] * n, pk.prove(d2 + tables(**kw), [NOPV] * n)) != 0

    def changed(c, field, t, w):
        call = list(calls[c])
        arr = np.array(call[field]).copy()
        arr[t][w] = (int(arr[t][w]) + 1) % P
        call[field] = arr
        return calls[:c] + [tuple(call)] + calls[c + 1:]
    # one sibling word: another pair, another leaf, and the path chip walks from it to another root
    d2, no = refused(changed(3, 4, 1, 2))
    assert no and not torch.equal(d2[1], d[1])
    # one ro word: the ro bus no longer balances (the table still sends the honest one), and the chain leaves the committed layers
    t = int(np.nonzero(calls[7][5])[0][0])
    d3, no = refused(changed(7, 6, t, 3))
    assert no and not torch.equal(d3[0], d[0])
    # one word of the final table
    wrong = t_final.copy()
    wrong[4][5] = (int(wrong[4][5]) + 1) % P
    assert refused(calls, final=wrong)[1]
    assert not refused(calls)[1]
    pk.close()


def test_an_unrelated_key_proves_the_same_bytes_around_a_generator_call(zk):
    fa = air.fibonacci_air()
    ftr, fpv = air.fibonacci_trace(8)
    airs = [dict(program=fa.program(), log_height=8, width=2, n_pvs=3, trace=ftr, pvs=fpv)]
    pk = z.ProvingKey(zk, (1, 0, 8, 3, 4), airs)
    d = zk.upload(ftr.reshape(-1))
    before = pk.prove([d], [fpv])
    lh, calls = SETS["calls_65"]
    _generate(zk, fq.records(calls), lh)
    after = pk.prove([d], [fpv])
    assert before == after and z.verify((1, 0, 8, 3, 4), pk.verifying_airs(), [fpv], after) == 0
    pk.close()
