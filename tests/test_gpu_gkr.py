"""GPU: LogUp-GKR (docs/logup_gkr.md) -- the device prover's words equal the independent model's (tests/gkr_model.py); the host
verifier accepts device proofs up to 2^22 leaves and its claims are the leaves' multilinear extensions at the returned point
(evaluated here with numpy); the bus argument of a key balances, and its leaves are recomputed from the AIR programs' interaction
nodes on the host traces; an interleaved bus proof leaves zkhip_prove's bytes unchanged."""
import numpy as np
import pytest

import gkr_model as gm
import pymodel_verify as pv
import zkvm_prover_amd as z
from pymodel import Challenger
from zkvm_prover_amd import air

pytestmark = pytest.mark.gpu
P = z.P
NOPV = np.zeros(0, np.uint32)


# ---- numpy extension arithmetic (independent of the product) -------------------------------------------------------------------
def np_ext_mul(a, b):
    """a: (n, 4) int64 canonical, b: (4,) or (n, 4) -> (n, 4)"""
    a = a.astype(np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    c = [np.zeros(len(a), dtype=np.uint64) for _ in range(7)]
    for i in range(4):
        for j in range(4):
            bj = b[..., j]
            c[i + j] = (c[i + j] + (a[:, i] * bj) % P) % P
    out = np.empty((len(a), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = (c[k] + 11 * c[k + 4] % P) % P if k < 3 else c[k]
    return out.astype(np.int64)


def np_mle(vals, point):
    """vals: (n, 4) canonical, point: list of extension elements (z_0 first)"""
    t = np.asarray(vals, dtype=np.int64)
    for r in point:
        a, b = t[0::2], t[1::2]
        t = (a + np_ext_mul((b - a) % P, [int(x) for x in r])) % P
    return t[0].tolist()


def _leaves(rng, log_n, ext_num):
    n = 1 << log_n
    num = rng.integers(0, P, size=(n, 4) if ext_num else n, dtype=np.uint32)
    den = rng.integers(0, P, size=(n, 4), dtype=np.uint32)
    return num, den


def _gpu_proof(zk, num, den, log_n, prefix, ext_num):
    return zk.gkr_prove(zk.upload(num.reshape(-1)), zk.upload(den.reshape(-1)), log_n, prefix, num_is_ext=ext_num)


@pytest.mark.parametrize("log_n", list(range(1, 15)))
@pytest.mark.parametrize("ext_num", [False, True])
def test_gpu_words_equal_model(zk, log_n, ext_num):
    rng = np.random.default_rng(1000 + 2 * log_n + ext_num)
    prefix = rng.integers(0, P, size=int(rng.integers(0, 20)), dtype=np.uint32)
    num, den = _leaves(rng, log_n, ext_num)
    proof, point, claims = _gpu_proof(zk, num, den, log_n, prefix, ext_num)
    ch = Challenger()
    ch.observe([int(x) for x in prefix])
    words, mpoint, mclaims = gm.prove(ch, [x.tolist() if ext_num else int(x) for x in num], den.tolist())
    assert len(proof) == gm.proof_words(log_n)
    if proof.tolist() != words:
        pytest.fail("proof differs from the model at word %d of %d" % (int(np.nonzero(proof != np.array(words))[0][0]), len(words)))
    assert point.tolist() == mpoint and claims.tolist() == [list(c) for c in mclaims]


@pytest.mark.parametrize("log_n,ext_num", [(13, False), (14, True), (17, False), (22, False), (22, True)])
def test_host_verifier_accepts_gpu_proofs_and_claims_are_the_mle(zk, log_n, ext_num):
    rng = np.random.default_rng(log_n)
    prefix = rng.integers(0, P, size=9, dtype=np.uint32)
    num, den = _leaves(rng, log_n, ext_num)
    proof, point, claims = _gpu_proof(zk, num, den, log_n, prefix, ext_num)
    vpoint, vclaims = z.gkr_verify(prefix, proof, log_n)
    assert (vpoint == point).all() and (vclaims == claims).all()
    num4 = num.astype(np.int64) if ext_num else np.stack([num.astype(np.int64)] + [np.zeros(len(num), np.int64)] * 3, axis=1)
    assert np_mle(num4, point.tolist()) == claims[0].tolist()
    assert np_mle(den.astype(np.int64), point.tolist()) == claims[1].tolist()
    bad = proof.copy()
    bad[len(bad) // 2] = (int(bad[len(bad) // 2]) + 1) % P
    with pytest.raises(z.ZkhipError):
        z.gkr_verify(prefix, bad, log_n)


def test_two_runs_give_identical_words(zk):
    rng = np.random.default_rng(5)
    num, den = _leaves(rng, 15, False)
    d_num, d_den = zk.upload(num), zk.upload(den.reshape(-1))
    a = zk.gkr_prove(d_num, d_den, 15, [1, 2, 3])
    b = zk.gkr_prove(d_num, d_den, 15, [1, 2, 3])
    for x, y in zip(a, b):
        assert (x == y).all()
    # the leaves are untouched
    assert (zk.download(d_den).reshape(-1, 4) == den).all()


def test_zero_denominator_gives_q_zero(zk):
    rng = np.random.default_rng(6)
    for log_n in (5, 12):
        num, den = _leaves(rng, log_n, False)
        den[(1 << log_n) // 3] = 0
        proof, point, claims = _gpu_proof(zk, num, den, log_n, [], False)
        assert proof[4:8].tolist() == [0, 0, 0, 0]
        z.gkr_verify([], proof, log_n)   # a valid proof of a tree whose root has Q = 0


# ---- the bus argument of a key ---------------------------------------------------------------------------------------------------
def _fib(log_n):
    tr, pvv = air.fibonacci_trace(log_n)
    return dict(program=air.fibonacci_air().program(), log_height=log_n, width=2, n_pvs=3, trace=tr, pvs=pvv)


def _lookup(log_s, log_t, seed=1, sender_width=3):
    s, t = air.lookup_traces(log_s, log_t, seed=seed, sender_width=sender_width)
    return (dict(program=air.lookup_sender_air(sender_width).program(), log_height=log_s, width=sender_width, n_pvs=0,
                 trace=s, pvs=NOPV),
            dict(program=air.lookup_table_air().program(), log_height=log_t, width=3, n_pvs=0, trace=t, pvs=NOPV))


def _mix(log_n, seed=3):
    tr, pvv = air.bus_mix_trace(log_n, seed)
    return dict(program=air.bus_mix_air().program(), log_height=log_n, width=6, n_pvs=1, trace=tr, pvs=pvv)


def _limb(log_n, seed=3):
    return dict(program=air.limb_air().program(), log_height=log_n, width=4, n_pvs=0, trace=air.limb_trace(log_n, seed), pvs=NOPV)


def _cases():
    s, t = _lookup(6, 4)
    s2, t2 = _lookup(9, 5, seed=2, sender_width=5)
    return {
        "lookup_pair": [s, t],
        "lookup_tall_table_last": [s, _fib(8), t],
        "mix_only": [_mix(5)],
        "mix_and_lookup": [_mix(7), s2, _fib(4), t2],
        "mix_min_height": [_mix(1)],
        "compound_messages": [_limb(6), s, t],
        "compound_and_mix": [_mix(4), _limb(8, seed=5), _fib(6)],
        "twelve_fields": [dict(program=air.program_bus_air().program(), log_height=5, width=13, n_pvs=0,
                               trace=air.program_bus_trace(5, 2), pvs=NOPV), _fib(3)],
    }


def _eval_nodes(prog, trace, pvs, n):
    """every node of the program on rows 0..n-1 (row-local operands only), canonical int64 arrays"""
    vals = []
    for op, a, b in prog.nodes:
        if op == pv.VAR:
            v = trace[a].astype(np.int64) if b == 0 else None
        elif op == pv.PUB:
            v = np.full(n, int(pvs[a]), np.int64)
        elif op == pv.CONST:
            v = np.full(n, a, np.int64)
        elif op == pv.ADD:
            v = None if vals[a] is None or vals[b] is None else (vals[a] + vals[b]) % P
        elif op == pv.SUB:
            v = None if vals[a] is None or vals[b] is None else (vals[a] - vals[b]) % P
        elif op == pv.MUL:
            v = None if vals[a] is None or vals[b] is None else (vals[a].astype(object) * vals[b] % P).astype(np.int64)
        elif op == pv.NEG:
            v = None if vals[a] is None else (-vals[a]) % P
        else:
            v = None   # not row-local: never an interaction operand
        vals.append(v)
    return vals


def _bus_leaves(airs, gamma, beta):
    """(num, den) of every interaction row, chips in key order, interactions in program order, rows 0..N-1; padded to 2^L"""
    bpow = [beta]
    for _ in range(pv.MAX_FIELDS):
        bpow.append(gm.ext_mul(bpow[-1], beta))
    nums, dens = [], []
    for a in airs:
        prog = pv.Program(a["program"], a["width"])
        if not prog.ints:
            continue
        n = 1 << a["log_height"]
        vals = _eval_nodes(prog, a["trace"], a["pvs"], n)
        for bus, sign, count, fields in prog.ints:
            cnt = vals[count] if not sign else (-vals[count]) % P
            den = np.tile(np.array(gm.ext_add(gamma, gm.ext_c(bus + 1)), np.int64), (n, 1))
            for i, f in enumerate(fields):
                den = (den + np_ext_mul(np.stack([vals[f]] + [np.zeros(n, np.int64)] * 3, axis=1), bpow[i])) % P
            nums.append(cnt)
            dens.append(den)
    num, den = np.concatenate(nums), np.concatenate(dens)
    L = max(1, int(len(num) - 1).bit_length())
    pad = (1 << L) - len(num)
    num = np.concatenate([num, np.zeros(pad, np.int64)])
    den = np.concatenate([den, np.tile(np.array([1, 0, 0, 0], np.int64), (pad, 1))])
    return num, den, L


def _bus_prove(zk, airs, prefix, params=(1, 0, 8, 3, 4)):
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    proof = pk.bus_gkr_prove(d_traces, [a["pvs"] for a in airs], prefix)
    return pk, d_traces, proof


@pytest.mark.parametrize("name", sorted(_cases()))
def test_bus_balances_and_claims_are_the_recomputed_leaves(zk, name):
    airs = _cases()[name]
    prefix = [7, 11, 13, len(name)]
    pk, d_traces, proof = _bus_prove(zk, airs, prefix)
    L = pk.bus_gkr_log_leaves()
    assert len(proof) == gm.proof_words(L)
    chal, point, claims = z.bus_gkr_verify(prefix, proof, L)
    assert proof[0:4].tolist() == [0, 0, 0, 0]
    gamma, beta = chal[0].tolist(), chal[1].tolist()
    num, den, L2 = _bus_leaves(airs, gamma, beta)
    assert L2 == L
    num4 = np.stack([num] + [np.zeros(len(num), np.int64)] * 3, axis=1)
    assert np_mle(num4, point.tolist()) == claims[0].tolist()
    assert np_mle(den, point.tolist()) == claims[1].tolist()
    if L <= 10:   # the model proves the same leaves to the same words
        ch = Challenger()
        ch.observe(prefix)
        assert list(gm.bus_challenges(ch)) == [gamma, beta]
        words, _, _ = gm.prove(ch, [int(x) for x in num], den.tolist())
        assert proof.tolist() == words


@pytest.mark.parametrize("name", ["lookup_pair", "mix_and_lookup"])
def test_one_cell_change_unbalances_the_bus(zk, name):
    airs = [dict(a) for a in _cases()[name]]
    t = airs[-1]
    t["trace"] = t["trace"].copy()
    t["trace"][2, 1] = (int(t["trace"][2, 1]) + 1) % P
    pk, _, proof = _bus_prove(zk, airs, [1])
    assert proof[0:4].tolist() != [0, 0, 0, 0]
    with pytest.raises(z.ZkhipError):
        z.bus_gkr_verify([1], proof, pk.bus_gkr_log_leaves())


def test_interleaved_bus_proof_leaves_prove_unchanged(zk):
    airs = _cases()["mix_and_lookup"]
    params = (1, 0, 8, 3, 4)
    pk = z.ProvingKey(zk, params, airs)
    d_traces = [zk.upload(a["trace"].reshape(-1)) for a in airs]
    pvs = [a["pvs"] for a in airs]
    before = pk.prove(d_traces, pvs)
    gkr1 = pk.bus_gkr_prove(d_traces, pvs, [3])
    after = pk.prove(d_traces, pvs)
    gkr2 = pk.bus_gkr_prove(d_traces, pvs, [3])
    assert before == after
    assert (gkr1 == gkr2).all()
    assert z.verify(params, airs, pvs, after) == 0
