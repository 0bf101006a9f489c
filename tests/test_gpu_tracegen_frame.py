"""GPU: what the trace generators' launch frame (csrc/tracegen_common.hpp tracegen_frame) does for every generator, pinned on one
generator per shape of call -- a plain row generator, a row generator that bumps a table, a count table with accumulate 0 and 1, a jump
chip, and program_freq, which counts from zero: the verdict at once and deferred, the count table's representation around the call in both
table modes, and the profile scope.  Three records in four rows, one of them refused: the frame is host code."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LH = 2
SUFFIX = " (requests outside the table)"


def _dev(zk, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Case:
    """One generator: `records(bad)` are three records (the middle one refused if bad), `run` the raw call (rc, trace or None),
    `trace` the model's rows, `counts` what the accepted records add to the table, in numpy."""
    table_words = 0        # the table the generator counts into (0: none)
    fresh = False          # the table is counted from zero, whatever it held
    always_monty = False   # ... and left in Montgomery form in either table mode
    accumulate = 0

    def trace(self, ora, recs):
        return None


class FieldArith(Case):
    name = scope = "field_arith_tracegen"

    def records(self, bad):
        return np.array([0, 4 if bad else 2, 3], np.uint32), np.array([5, 6, 7], np.uint32), np.array([1, 2, 3], np.uint32)

    def run(self, zk, recs, table):
        out = torch.empty(8 << LH, dtype=torch.int32, device=zk.device)
        d = [_dev(zk, v) for v in recs]
        return zk.lib.zkhip_field_arith_tracegen(zk.h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), 3, LH, _ptr(out)), out

    def trace(self, ora, recs):
        return ora.field_arith_trace(*recs, LH)[0]


class Rv32Alu(Case):
    name = scope = "rv32_alu_tracegen"
    table_words = 2 << 16

    def records(self, bad):
        return (np.array([0, 5 if bad else 2, 4], np.uint32), np.array([0xFFFFFFFF, 0x12345678, 0xFF00FF00], np.uint32),
                np.array([1, 0x0F0F0F0F, 0x0FF00FF0], np.uint32))

    def run(self, zk, recs, table):
        out = torch.empty(18 << LH, dtype=torch.int32, device=zk.device)
        d = [_dev(zk, v) for v in recs]
        return zk.lib.zkhip_rv32_alu_tracegen(zk.h, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), 3, LH, _ptr(out), _ptr(table)), out

    def trace(self, ora, recs):
        return ora.rv32_alu_trace(*recs, LH)[0]

    def counts(self, recs):
        """per limb (b_i, c_i) for XOR / OR / AND, (a_i, a_i) for ADD / SUB, into the XOR column"""
        t = np.zeros(2 << 16, np.int64)
        for op, b, c in zip(*(v.tolist() for v in recs)):
            if op > 4:
                continue
            a = ((b + c) if op == 0 else (b - c) if op == 1 else (b ^ c) if op == 2 else (b | c) if op == 3 else (b & c)) & 0xFFFFFFFF
            for i in range(4):
                ai, bi, ci = (a >> 8 * i) & 255, (b >> 8 * i) & 255, (c >> 8 * i) & 255
                x, y = (bi, ci) if op >= 2 else (ai, ai)
                t[(1 << 16) + (x << 8) + y] += 1
        return t


class RangeTuple(Case):
    name, scope = "range_tuple_counts_tracegen", "range_tuple_tracegen"
    table_words = 4 * 8

    def __init__(self, accumulate):
        self.accumulate, self.fresh = accumulate, not accumulate

    def records(self, bad):
        return np.array([1, 4 if bad else 2, 3], np.uint32), np.array([4, 5, 6], np.uint32)

    def run(self, zk, recs, table):
        dx, dy = zk.upload(recs[0]), zk.upload(recs[1])   # requests are Montgomery words where they lie
        return zk.lib.zkhip_range_tuple_counts_tracegen(zk.h, _ptr(dx), _ptr(dy), 3, 4, 8, _ptr(table), self.accumulate), None

    def counts(self, recs):
        t = np.zeros(4 * 8, np.int64)
        for x, y in zip(*(v.tolist() for v in recs)):
            if x < 4 and y < 8:
                t[x * 8 + y] += 1
        return t


class Rv32Auipc(Case):
    name = scope = "rv32_auipc_tracegen"
    table_words = 2 << 16

    def records(self, bad):
        return np.array([0, 0x3FFFFFFC, 0x1000], np.uint32), np.array([1, (1 << 20) if bad else 0xFFFFF, 0x80000], np.uint32)

    def run(self, zk, recs, table):
        out = torch.empty(14 << LH, dtype=torch.int32, device=zk.device)
        d = [_dev(zk, v) for v in recs]
        return zk.lib.zkhip_rv32_auipc_tracegen(zk.h, _ptr(d[0]), _ptr(d[1]), 3, LH, _ptr(out), _ptr(table)), out

    def trace(self, ora, recs):
        return ora.rv32_auipc_trace(*recs, LH)[0]

    def counts(self, recs):
        """the five range pairs of a row, into the range column"""
        t = np.zeros(2 << 16, np.int64)
        for pc, imm in zip(*(v.tolist() for v in recs)):
            if pc >= 1 << 30 or imm >> 20:
                continue
            rd, im16 = (pc + (imm << 12)) & 0xFFFFFFFF, imm << 4
            pl, dl = [(pc >> 8 * i) & 255 for i in range(4)], [(rd >> 8 * i) & 255 for i in range(4)]
            il = [(im16 >> 8 * i) & 255 for i in range(3)]
            for x, y in ((pl[0], pl[1]), (pl[2], 4 * pl[3]), (il[0], il[1]), (il[2], dl[1]), (dl[2], dl[3])):
                t[(x << 8) + y] += 1
        return t


class ProgramFreq(Case):
    name = scope = "program_freq_tracegen"
    table_words = 1 << LH
    fresh = always_monty = True

    def records(self, bad):
        return (np.array([0, 4 if bad else 1, 1], np.uint32),)

    def run(self, zk, recs, table):
        d = _dev(zk, recs[0])
        return zk.lib.zkhip_program_freq_tracegen(zk.h, _ptr(d), 3, LH, _ptr(table)), None

    def counts(self, recs):
        return np.bincount([k for k in recs[0].tolist() if k < 1 << LH], minlength=1 << LH).astype(np.int64)


CASES = [FieldArith(), Rv32Alu(), RangeTuple(0), RangeTuple(1), Rv32Auipc(), ProgramFreq()]
IDS = ["field_arith", "rv32_alu", "range_tuple_counts-fresh", "range_tuple_counts-accumulate", "rv32_auipc", "program_freq"]
WITH_TABLE = [i for i, c in enumerate(CASES) if c.table_words]


def _prior(case):
    return np.random.default_rng(case.table_words).integers(0, 1000, case.table_words).astype(np.uint32)


def _table(zk, case, canonical=False):
    """the table as the call finds it: counts it must keep (or, counting from zero, forget), in the representation of the table mode"""
    if not case.table_words:
        return None
    return _dev(zk, _prior(case)) if canonical else zk.upload(_prior(case))


def _read(zk, case, table, canonical):
    if canonical and not case.always_monty:
        zk.sync()
        return table.cpu().numpy().view(np.uint32)
    return zk.download(table)


def _expected_table(case, recs):
    return (case.counts(recs) + (0 if case.fresh else _prior(case).astype(np.int64))).astype(np.uint32)


def _good_call_matches_the_model(zk, ora, case):
    recs, table = case.records(False), _table(zk, case)
    rc, out = case.run(zk, recs, table)
    assert rc == 0
    exp = case.trace(ora, recs)
    if exp is not None:
        assert (zk.download(out).reshape(exp.shape[0], -1) == exp).all()
    if table is not None:
        assert (_read(zk, case, table, False) == _expected_table(case, recs)).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_refusal_at_once(zk, ora, case):
    """the call returns ZKHIP_ERR_INVALID, the text names the generator and the count; the table is back in its form by then, with the
    accepted records counted; the next good call is as ever"""
    recs, table = case.records(True), _table(zk, case)
    rc, _ = case.run(zk, recs, table)
    text = zk.lib.zkhip_last_error(zk.h).decode()
    assert rc == -3
    assert text.startswith(case.name) and SUFFIX in text and text.endswith(": 1 bad records"), text
    if table is not None:
        assert (_read(zk, case, table, False) == _expected_table(case, recs)).all()
    _good_call_matches_the_model(zk, ora, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_refusal_with_deferred_checks(zk, ora, case):
    """under zkhip_tracegen_defer_checks the call itself returns OK and zkhip_tracegen_check reports, once, and resets"""
    assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 1) == 0
    try:
        _good_call_matches_the_model(zk, ora, case)
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        rc, _ = case.run(zk, case.records(True), _table(zk, case))   # no verdict yet
        assert rc == 0
        assert zk.lib.zkhip_tracegen_check(zk.h) == -3
        assert "1 bad records" in zk.lib.zkhip_last_error(zk.h).decode()
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
        _good_call_matches_the_model(zk, ora, case)
        assert zk.lib.zkhip_tracegen_check(zk.h) == 0
    finally:
        zk.lib.zkhip_tracegen_check(zk.h)
        assert zk.lib.zkhip_tracegen_defer_checks(zk.h, 0) == 0


@pytest.mark.parametrize("canonical", [0, 1], ids=["monty", "canonical"])
@pytest.mark.parametrize("case", [CASES[i] for i in WITH_TABLE], ids=[IDS[i] for i in WITH_TABLE])
def test_table_representation_is_kept(zk, case, canonical):
    """the table is in the same representation after the call as before it, in both table modes: the counts of before (unless the
    generator counts from zero) plus the records', read back without (canonical mode) or with the conversion from Montgomery form"""
    recs = case.records(False)
    assert zk.lib.zkhip_tables_canonical(zk.h, canonical) == 0
    try:
        table = _table(zk, case, canonical)
        rc, _ = case.run(zk, recs, table)
        assert rc == 0
        got = _read(zk, case, table, canonical)
    finally:
        assert zk.lib.zkhip_tables_canonical(zk.h, 0) == 0
    assert (got == _expected_table(case, recs)).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_call_has_its_profile_scope(zk, case):
    zk.profile_enable(True)
    zk.profile_reset()
    rc, _ = case.run(zk, case.records(False), _table(zk, case))
    zk.sync()
    stats = zk.profile_read()
    zk.profile_enable(False)
    assert rc == 0 and stats[case.scope][0] == 1
