"""GPU: the FRI final-polynomial chip's device generator (csrc/fri_final.hip: one lane per trace row, the accumulator column a segmented scan
inside a wave and, for calls of 128 and 256 rows, across waves through LDS) against the twin, word for word, at every shape where the kernel
takes another path; the refusals, at once and deferred; and the composition the chip exists for: on an honest low-degree FRI instance the
query chip's final bus ends in this chip instead of a table, so the proof states that every query folds down to the final polynomial at
the query's point."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fri_final_util as ff  # noqa: E402
import fri_query_util as fq  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

pytestmark = pytest.mark.gpu
NOPV = np.zeros(0, np.uint32)
PARAMS = (1, 0, 12, 4, 4)
P = ff.P
SETS = ff.call_sets()
NAMES = ("k", "lvl", "poly", "coef")


def _dev(zk, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32).reshape(-1)).to(zk.device)


def _generate(zk, s, **kw):
    return zk.fri_final_tracegen(*[_dev(zk, s[n]) for n in NAMES], s["lfp"], s["lh"], **kw)


def _same(got, want, what):
    if not (got == want).all():
        where = [int(x[0]) for x in np.nonzero(got != want)]
        pytest.fail("%s: first difference at %s (%d cells differ)" % (what, where, int((got != want).sum())))


def _values(zk, d_val):
    zk.sync()
    return d_val.cpu().numpy().view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("name", list(SETS))
def test_device_trace_equals_the_twin(zk, name):
    """device trace and d_value == the twin word for word, and check_trace empty on the DEVICE trace"""
    s = SETS[name]
    want, want_val = ff.trace(s)
    d_tr, d_val = _generate(zk, s)
    got = zk.download(d_tr).reshape(19, -1)
    _same(got, want, "trace [column, row]")
    _same(_values(zk, d_val), want_val, "values [call, word]")
    assert air.check_trace(air.fri_final_air(s["lfp"], 14, 17, 18).program(), got, NOPV) == []
    assert (got[:, len(s["k"]) << s["lfp"]:] == 0).all()          # padding rows zero


def test_two_runs_give_identical_words(zk):
    s = SETS["lfp7_three_calls"]
    one, two = _generate(zk, s), _generate(zk, s)
    zk.sync()
    assert all(torch.equal(a, b) for a, b in zip(one, two))


@pytest.mark.parametrize("lfp,lh", [(0, 3), (3, 2), (8, 9)])
def test_no_calls_is_padding_only(zk, lfp, lh):
    e = torch.empty(0, dtype=torch.int32, device=zk.device)
    tr, val = zk.fri_final_tracegen(e, e, e, e, lfp, lh)
    assert (zk.download(tr) == 0).all() and tr.numel() == 19 << lh and val.numel() == 0


def test_a_null_value_pointer_is_accepted(zk):
    s = SETS["lfp3_five_calls"]
    tr, val = _generate(zk, s, value=False)
    assert val is None and (zk.download(tr).reshape(19, -1) == ff.trace(s)[0]).all()


def _refusal_cases():
    rng = np.random.default_rng(2)
    good = ff.call_set(rng, 3, 6, 5, 2)
    good["poly"] = np.array([0, 1, 0, 1, 1])
    u = lambda *v: np.array(v, np.uint32)  # noqa: E731
    k, lvl = good["k"].astype(np.uint32), good["lvl"].astype(np.uint32)
    put = lambda a, c, v: np.where(np.arange(5) == c, v, a).astype(np.uint32)  # noqa: E731
    # (the refused call, or None where a coefficient word is refused and the call's rows are still written) and what changes
    device = [(1, dict(lvl=put(lvl, 1, 0))), (4, dict(lvl=put(lvl, 4, 27))), (0, dict(lvl=put(lvl, 0, 0xFFFFFFFF))), (2, dict(lvl=put(lvl, 2, 32))),
              (3, dict(k=put(k, 3, 1 << int(lvl[3])))), (0, dict(k=put(k, 0, 0xFFFFFFFF))), (4, dict(lvl=put(lvl, 4, 26), k=put(k, 4, 1 << 26))),
              (2, dict(poly=u(0, 1, 2, 1, 1))), (4, dict(poly=u(0, 1, 0, 1, 0xFFFFFFFF)))]
    for pos, v in ((-1, P), (0, 0xFFFFFFFF), (37, P)):
        w = good["coef"].astype(np.uint32).copy()
        w.reshape(-1)[pos] = v
        device.append((None, dict(coef=w)))
    return good, device


def _zeroed(want, lfp, c):
    w = want.copy()
    w[:, c << lfp:(c + 1) << lfp] = 0
    return w


def test_refusals(zk):
    good, device = _refusal_cases()
    want = ff.trace(good)[0]
    _generate(zk, good)
    for _, case in device:
        with pytest.raises(z.ZkhipError) as e:
            _generate(zk, dict(good, **case))
        assert e.value.code == -3, case   # ZKHIP_ERR_INVALID
    # on the host before any launch (called below the binding, which would allocate the trace)
    t = [_dev(zk, good[n]) for n in NAMES]
    ptr = [t_.data_ptr() for t_ in t]
    out = torch.empty(19 << 6, dtype=torch.int32, device=zk.device)
    f = zk.lib.zkhip_fri_final_tracegen
    assert f(zk.h, 3, *ptr, 2, 5, 6, out.data_ptr(), None) == 0
    assert f(None, 3, *ptr, 2, 5, 6, out.data_ptr(), None) == -3
    assert f(zk.h, 3, *ptr, 2, 5, 6, None, None) == -3
    for i in range(4):
        assert f(zk.h, 3, *[None if j == i else p for j, p in enumerate(ptr)], 2, 5, 6, out.data_ptr(), None) == -3
    assert f(zk.h, 3, *ptr, 2, 5, 28, out.data_ptr(), None) == -3
    assert f(zk.h, 9, *ptr, 2, 5, 6, out.data_ptr(), None) == -3 and f(zk.h, 0xFFFFFFFF, *ptr, 2, 5, 6, out.data_ptr(), None) == -3
    assert f(zk.h, 3, *ptr, 2, 5, 5, out.data_ptr(), None) == -3          # 5 calls of 8 rows > 2^5
    assert f(zk.h, 3, *ptr, 2, 4, 5, out.data_ptr(), None) == 0           # 4 calls of 8 rows = 2^5
    assert f(zk.h, 3, *ptr, 2, 1, 2, out.data_ptr(), None) == -3          # a trace shorter than one call
    assert f(zk.h, 3, *ptr, 2, 1 << 62, 6, out.data_ptr(), None) == -3    # a count whose product with L wraps
    assert f(zk.h, 3, None, None, None, None, 0, 0, 6, out.data_ptr(), None) == 0   # no calls: no records
    # and the generator is as it was
    assert (zk.download(_generate(zk, good)[0]).reshape(19, -1) == want).all()


def test_refusals_with_deferred_checks(zk):
    """under zkhip_tracegen_defer_checks the call itself returns OK and zkhip_tracegen_check reports, once, and resets; a refused call's
    rows are zeros and every other call's are right"""
    good, device = _refusal_cases()
    want, want_val = ff.trace(good)
    assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 1) == 0
    try:
        _generate(zk, good)
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        for c, case in device:
            tr, val = _generate(zk, dict(good, **case))           # no verdict yet
            assert zk.lib.zkhip_tracegen_check(zk.h) == -3, case
            assert zk.lib.zkhip_tracegen_check(zk.h) == 0
            if c is not None:
                _same(zk.download(tr).reshape(19, -1), _zeroed(want, 3, c), "trace around the refused call %d" % c)
                wv = want_val.copy()
                wv[c] = 0
                _same(_values(zk, val), wv, "values around the refused call %d" % c)
        tr = _generate(zk, good)[0]
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        assert (zk.download(tr).reshape(19, -1) == want).all()
    finally:
        zk.lib.zkhip_tracegen_check(zk.h)
        assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 0) == 0


def test_the_call_has_its_profile_scope(zk):
    zk.profile_enable(True)
    zk.profile_reset()
    _generate(zk, SETS["lfp3_five_calls"])
    zk.sync()
    stats = zk.profile_read()
    zk.profile_enable(False)
    assert stats["fri_final_tracegen"][0] == 1


def test_an_unrelated_key_proves_the_same_bytes_around_a_generator_call(zk):
    fa = air.fibonacci_air()
    ftr, fpv = air.fibonacci_trace(8)
    airs = [dict(program=fa.program(), log_height=8, width=2, n_pvs=3, trace=ftr, pvs=fpv)]
    pk = z.ProvingKey(zk, (1, 0, 8, 3, 4), airs)
    d = zk.upload(ftr.reshape(-1))
    before = pk.prove([d], [fpv])
    _generate(zk, SETS["lfp8_three_calls"])
    after = pk.prove([d], [fpv])
    assert before == after and z.verify((1, 0, 8, 3, 4), pk.verifying_airs(), [fpv], after) == 0
    pk.close()


# ---- the composition: reduced openings -> fold loop -> the final polynomial at the query's point ---------------------------------------------
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


def _table_air(bus, width, kind):
    """test-local: a plain table that sends or receives its first width - 1 columns with multiplicity the last"""
    b = air.AirBuilder(width, 0)
    b.push_interaction(bus, [b.var(i) for i in range(width - 1)], b.var(width - 1), kind)
    return b


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


def test_the_final_bus_ends_in_the_chip_on_an_honest_instance(zk, ora):
    """proof bytes == the oracle's, the host verifier accepts; one changed sibling word, one changed coefficient word or one changed k of
    the final chip's records and a bus no longer balances"""
    inst = ff.final_instance(ora, z, 6, 1, 2)
    calls, rows, lfp = inst.calls, fq.n_rows(inst.calls), inst.lfp
    idx, starts, kinds, digs = fq.path_records(inst)
    fk, flvl, fpoly = ff.final_records(inst)
    lh_q, lh_p, lh_f = _lh(rows), _lh(int(starts[-1])), _lh(len(fk) << lfp)
    t_q, hin_q, leaf, fin = fq.trace(ora, calls, lh_q)
    t_f, val = ff.trace_np(lfp, fk, flvl, fpoly, inst.coef[None], lh_f)
    assert (val == fin).all()
    t_path, hin_path, claims, bad = ora.mmcs_path_trace(leaf, idx, starts, kinds, digs, lh_p)
    assert bad == 0
    # the point chip serves both senders: every row of the query chip, and the first row of every call of the final chip
    ks, mults = np.unique(np.concatenate([t_q[fq.K, :rows], fk]), return_counts=True)
    ks, mults = ks.astype(np.uint32), mults.astype(np.uint32)
    assert int(mults.sum()) == rows + len(fk) and set(fk.tolist()) <= set(ks.tolist())
    lh_d = _lh(len(ks))
    t_dp = _domain_point_trace(ks, mults, lh_d)
    t_ro, t_layer, _ = fq.bus_tables(inst)
    t_coef = ff.coeff_table(inst)

    def chip(hin, lh, n):
        full = np.zeros((1 << lh, 16), np.uint32)
        full[:n] = hin[:n]
        t = np.zeros((299, 1 << lh), np.uint32)
        t[:298] = ora.poseidon2_air_trace(full, lh)
        t[298, :n] = 1
        return t

    A = lambda b, t: dict(program=b.program(), log_height=int(np.log2(t.shape[1])), width=t.shape[0], n_pvs=0, trace=t, pvs=NOPV)  # noqa: E731
    airs = [A(air.fri_query_air(14, 11, 10, 15, 16, 17), t_q), A(air.fri_final_air(2, 14, 17, 18), t_f), A(air.mmcs_path_air(9, 10), t_path),
            A(air.poseidon2_air(9), chip(hin_path, lh_p, int(starts[-1]))), A(air.poseidon2_air(11, out_lanes=16), chip(hin_q, lh_q, rows)),
            A(air.domain_point_air(14), t_dp), A(_table_air(15, 7, "send"), t_ro), A(_table_air(16, 15, "receive"), t_layer), A(_table_air(18, 7, "receive"), t_coef)]
    for a in airs:
        assert a["width"] == 299 or air.check_trace(a["program"], a["trace"], NOPV) == []
    tables = [zk.upload(t.reshape(-1)) for t in (t_ro, t_layer, t_coef)]

    def device_traces(calls2, fk2=fk, coef2=inst.coef):
        d_q, d_hin_q, d_leaf, _ = zk.fri_query_tracegen(*[_dev(zk, a) for a in fq.records(calls2)], lh_q)
        d_path, d_hin_path = zk.mmcs_path_tracegen(d_leaf, _dev(zk, idx), _dev(zk, starts), _dev(zk, kinds), _dev(zk, digs.reshape(-1)), lh_p)
        d_f, d_val = zk.fri_final_tracegen(_dev(zk, fk2), _dev(zk, flvl), _dev(zk, fpoly), _dev(zk, coef2), lfp, lh_f)
        d_dp = zk.domain_point_tracegen(_dev(zk, ks), _dev(zk, mults), lh_d)
        return [d_q, d_f, d_path, _poseidon_chip(zk, d_hin_path, lh_p, int(starts[-1])), _poseidon_chip(zk, d_hin_q, lh_q, rows), d_dp], d_val

    d, d_val = device_traces(calls)
    for dt, a in zip(d, airs):
        assert (zk.download(dt).reshape(a["width"], -1) == a["trace"]).all(), a["width"]
    assert (_values(zk, d_val) == fin).all()
    n = len(airs)
    pk = z.ProvingKey(zk, PARAMS, airs)
    proof = pk.prove(d + tables, [NOPV] * n)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * n, proof) == 0
    assert proof == ora.stark_prove(PARAMS, airs).tobytes()

    def refused(*a, **kw):
        d2, _ = device_traces(*a, **kw)
        return d2, z.verify(PARAMS, pk.verifying_airs(), [NOPV] * n, pk.prove(d2 + tables, [NOPV] * n)) != 0

    # one sibling word: another pair, another leaf, another root under the path chip -- and another value on the final bus
    call = list(calls[3])
    sib = np.array(call[4]).copy()
    sib[1][2] = (int(sib[1][2]) + 1) % P
    call[4] = sib
    d2, no = refused(calls[:3] + [tuple(call)] + calls[4:])
    assert no and not torch.equal(d2[0], d[0]) and torch.equal(d2[1], d[1])
    # one coefficient word: the chip evaluates another polynomial than the coefficient table holds and than the queries fold down to
    coef2 = inst.coef.copy()
    coef2[1][3] = (int(coef2[1][3]) + 1) % P
    d3, no = refused(calls, coef2=coef2)
    assert no and not torch.equal(d3[1], d[1]) and torch.equal(d3[0], d[0])
    # one k of the final chip's records: another point than the one the query ended on
    fk2 = fk.copy()
    fk2[5] ^= 1
    d4, no = refused(calls, fk2=fk2)
    assert no and not torch.equal(d4[1], d[1])
    assert not refused(calls)[1]
    pk.close()
