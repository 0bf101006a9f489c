"""GPU: the reduced-opening chip's device generator (csrc/reduced_opening.hip: offsets by a device scan of the lengths, the accumulator
column by a segmented scan over affine maps of the extension field) against the twin in Python integers, word for word, at every shape
where the kernels take another path: inside a wave, across waves, across the passes of a workgroup, across workgroups, more than one
round of the carry scan; the refusals; one proof with a receiver of the results; and no trace left in an unrelated key's proof.

(The first call set is 1 + 1 + 2 + 60 rows: the 2^6 rows are exactly full.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduced_opening_util as ru  # noqa: E402

import zkvm_prover_amd as z  # noqa: E402
from zkvm_prover_amd import air  # noqa: E402

pytestmark = pytest.mark.gpu
NOPV = np.zeros(0, np.uint32)
PARAMS = (1, 0, 12, 4, 4)
P = ru.P
W = z.REDUCED_OPENING_BLOCK_ROWS   # rows a workgroup of the generator covers at a time (include/zkhip.h)
SETS = ru.call_sets(W)


def _dev(zk, v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(zk.device)


def _generate(zk, calls, lh):
    alpha, lens, a, b = ru.records(calls)
    return zk.reduced_opening_tracegen(_dev(zk, alpha), _dev(zk, lens), _dev(zk, a), _dev(zk, b), lh)


@pytest.fixture(scope="module")
def prog():
    return air.reduced_opening_air().program()


def test_the_call_sets_reach_the_paths_they_are_meant_for():
    rows = lambda name: np.cumsum([0] + [len(c[1]) for c in SETS[name][1]])  # noqa: E731
    assert rows("full_64")[-1] == 64
    r = rows("block_crossing")
    assert r[1] < W < 2 * W < r[2] and r[2] - r[1] == 2 * W + 3 and r[3] == 3 * W and r[4] == 4 * W and r[5] > 5 * W
    assert rows("seeded_2_17")[-1] > 2 * W * 64 and (1 << 17) // (2 * W) > 64    # several rounds of the one-wave carry scan, two passes a workgroup


@pytest.mark.parametrize("name", sorted(SETS))
def test_device_trace_equals_the_twin(zk, prog, name):
    lh, calls = SETS[name]
    want = ru.trace(calls, lh)
    got = zk.download(_generate(zk, calls, lh)).reshape(18, -1)
    assert got.shape == want.shape
    if not (got == want).all():
        col, row = (int(x[0]) for x in np.nonzero(got != want))
        pytest.fail("first difference in column %d at row %d (%d cells differ)" % (col, row, int((got != want).sum())))
    assert air.check_trace(prog, got, NOPV) == []


def test_a_call_count_at_which_the_offset_kernels_loop(zk, prog):
    """2^18 + 4096 calls of 1 to 3 elements: a workgroup of the offset kernels covers 512 calls (two rounds of its scan, the sum carried
    from one to the next) and 513 workgroups have slices in front of them (the second round of the 256-lane sum over those)."""
    n_calls = (1 << 18) + 4096
    assert n_calls > 1024 * W
    alpha, lens, a, b = ru.many_short_calls(n_calls)
    lh = 19
    assert len(a) <= 1 << lh
    want = ru.trace_np(alpha, lens, a, b, lh)
    got = zk.download(zk.reduced_opening_tracegen(_dev(zk, alpha), _dev(zk, lens), _dev(zk, a), _dev(zk, b), lh)).reshape(18, -1)
    if not (got == want).all():
        col, row = (int(x[0]) for x in np.nonzero(got != want))
        pytest.fail("first difference in column %d at row %d (%d cells differ)" % (col, row, int((got != want).sum())))
    assert air.check_trace(prog, got, NOPV) == []


def test_two_runs_give_identical_words(zk):
    lh, calls = SETS["block_crossing"]
    one, two = _generate(zk, calls, lh), _generate(zk, calls, lh)
    zk.sync()
    assert torch.equal(one, two)


def test_no_calls_is_padding_only(zk):
    e = torch.empty(0, dtype=torch.int32, device=zk.device)
    assert (zk.download(zk.reduced_opening_tracegen(e, e, e, e, 3)) == 0).all()


def test_refusals(zk):
    rng = np.random.default_rng(2)
    calls = ru.random_calls(rng, [3, 70, 1, 300])
    alpha, lens, a, b = ru.records(calls)
    n = len(a)

    def refused(alpha=alpha, lens=lens, a=a, b=b, lh=9):
        with pytest.raises(z.ZkhipError) as e:
            zk.reduced_opening_tracegen(_dev(zk, alpha), _dev(zk, lens), _dev(zk, a), _dev(zk, b), lh)
        assert e.value.code == -3   # ZKHIP_ERR_INVALID
        return True

    zk.reduced_opening_tracegen(_dev(zk, alpha), _dev(zk, lens), _dev(zk, a), _dev(zk, b), 9)
    assert refused(lens=np.array([3, 70, 0, 301], np.uint32))          # a length of 0 (the sum still n_elems)
    assert refused(lens=np.array([3, 70, 1, 299], np.uint32))          # the lengths fall short of n_elems
    assert refused(lens=np.array([3, 70, 1, 301], np.uint32))          # ... run past it
    assert refused(lens=np.array([3, 70, 1, 0xFFFFFFFF], np.uint32))   # ... by far
    assert refused(alpha=np.zeros((0, 4), np.uint32), lens=np.zeros(0, np.uint32))   # elements but no call: the (empty) sum is not n_elems
    assert refused(lh=8)                                               # n_elems > 2^log_height
    assert refused(alpha=np.zeros((n + 1, 4), np.uint32), lens=np.ones(n + 1, np.uint32))   # n_calls > n_elems
    for c, q in ((0, 0), (3, 3)):
        w = alpha.copy()
        w[c][q] = P
        assert refused(alpha=w)
    for i in (0, 73, n - 1):
        w = a.copy()
        w[i] = P
        assert refused(a=w)
        w = b.copy()
        w[i][i % 4] = P
        assert refused(b=w)
    # and the generator is as it was
    got = zk.download(zk.reduced_opening_tracegen(_dev(zk, alpha), _dev(zk, lens), _dev(zk, a), _dev(zk, b), 9)).reshape(18, -1)
    assert (got == ru.trace(calls, 9)).all()


def test_the_call_has_its_profile_scope(zk):
    lh, calls = SETS["wave_crossing"]
    zk.profile_enable(True)
    zk.profile_reset()
    _generate(zk, calls, lh)
    zk.sync()
    stats = zk.profile_read()
    zk.profile_enable(False)
    assert stats["reduced_opening_tracegen"][0] == 1


def _receiver_air(bus):
    """test-local: columns call | len | alpha[4] | ro[4] | mult; takes each row `mult` times from the chip's result bus"""
    b = air.AirBuilder(11, 0)
    b.push_interaction(bus, [b.var(i) for i in range(10)], b.var(10), "receive")
    return b


def test_results_proven_against_a_receiver(zk):
    """reduced_opening_air(result_bus) on the DEVICE trace with a table of (call, len, alpha, ro) rows whose ro is the power sum: the two
    prove together and the host verifier accepts; with one ro word changed in the table the bus no longer balances and the verifier
    refuses (as in the other chips' bus tests, proving goes through and verification is the refusing side)."""
    rng = np.random.default_rng(13)
    lens = [1, 2, 65, 300, 5, 1, 2 * W + 3, 64]
    calls = ru.random_calls(rng, lens)
    lh, lt, bus = 10, 3, 12
    assert sum(lens) < 1 << lh and len(calls) <= 1 << lt
    table = np.zeros((11, 1 << lt), np.uint32)
    for c, (alpha, a, b) in enumerate(calls):
        table[:, c] = [c, len(a)] + list(alpha) + list(ru.power_sum(alpha, a, b)) + [1]
    d_tr = _generate(zk, calls, lh)
    tr = zk.download(d_tr).reshape(18, -1)
    assert (tr == ru.trace(calls, lh)).all()
    airs = [dict(program=air.reduced_opening_air(bus).program(), log_height=lh, width=18, n_pvs=0, trace=tr, pvs=NOPV),
            dict(program=_receiver_air(bus).program(), log_height=lt, width=11, n_pvs=0, trace=table, pvs=NOPV)]
    pk = z.ProvingKey(zk, PARAMS, airs)
    proof = pk.prove([d_tr, zk.upload(table.reshape(-1))], [NOPV] * 2)
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 2, proof) == 0
    wrong = table.copy()
    wrong[6 + 2][3] = (int(wrong[6 + 2][3]) + 1) % P
    assert z.verify(PARAMS, pk.verifying_airs(), [NOPV] * 2, pk.prove([d_tr, zk.upload(wrong.reshape(-1))], [NOPV] * 2)) != 0
    pk.close()


def test_an_unrelated_key_proves_the_same_bytes_around_a_generator_call(zk):
    fa = air.fibonacci_air()
    ftr, fpv = air.fibonacci_trace(8)
    airs = [dict(program=fa.program(), log_height=8, width=2, n_pvs=3, trace=ftr, pvs=fpv)]
    pk = z.ProvingKey(zk, (1, 0, 8, 3, 4), airs)
    d = zk.upload(ftr.reshape(-1))
    before = pk.prove([d], [fpv])
    lh, calls = SETS["block_crossing"]
    _generate(zk, calls, lh)
    after = pk.prove([d], [fpv])
    assert before == after and z.verify((1, 0, 8, 3, 4), pk.verifying_airs(), [fpv], after) == 0
    pk.close()
