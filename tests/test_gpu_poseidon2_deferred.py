"""GPU: every bulk Poseidon2 kernel shares poseidon2_permute_rolled, whose thirteen partial rounds run with the linear layer deferred
(csrc/poseidon2.hpp).  Row sponges, mixed-height trees and one whole proof against the CPU oracle (plain C, canonical form, round-wise
rounds), with the boundary words of the field in every ragged position of the rows.

The Python surface hashes rows through merkle_commit, whose heights are powers of two: a case of n_rows rows is the first n_rows
leaves of the tree of the next power of two (the rows behind them are hashed and compared as well), so that the rows 62..65 and
255..257 around a wave's and a workgroup's end carry the boundary words."""
import numpy as np
import pytest

from boundary_inputs import raw_words

pytestmark = pytest.mark.gpu
P = 2013265921
# device (Montgomery) words a uniform draw shows about never
WORDS = [0, P - 1, 1, (P - 1) // 2, (P + 1) // 2, 1 << 27, (1 << 31) % P]


def _matrix(ora, rng, width, n_rows, height):
    """[width, height] canonical values whose device words are boundary words in the ragged block of every row (the columns behind the
    last full block of eight), in the whole last row and the rows around it, and random elsewhere"""
    raw = ((ora.rand_field(rng, (width, height)).astype(np.uint64) << np.uint64(32)) % np.uint64(P))
    first_ragged = 8 * ((width - 1) // 8)
    for c in range(first_ragged, width):
        raw[c, :] = [WORDS[(r + c) % len(WORDS)] for r in range(height)]
    for k, r in enumerate(range(max(0, n_rows - 2), min(height, n_rows + 1))):
        raw[:, r] = WORDS[(k + 1) % len(WORDS)] if k != 1 else P - 1     # row n_rows - 1: every device word p - 1
    return raw_words(raw)


def _check_tree(zk, ora, mats, shapes):
    ot = ora.Tree(mats)
    t = zk.merkle_commit([(zk.upload(m.reshape(-1)), lh, w) for m, (lh, w) in zip(mats, shapes)])
    assert t.root.tolist() == ot.root.tolist()
    for l in range(t.log_height + 1):
        assert (t.layer(l) == ot.layer(l)).all(), l
    return t, ot


@pytest.mark.parametrize("n_cols", [1, 7, 8, 9, 16, 302])
def test_row_sponge_digests(zk, ora, n_cols):
    for n_rows in (1, 63, 64, 65, 257):
        lh = int(np.ceil(np.log2(n_rows))) if n_rows > 1 else 0
        rng = np.random.default_rng(1000 * n_cols + n_rows)
        m = _matrix(ora, rng, n_cols, n_rows, 1 << lh)
        t, ot = _check_tree(zk, ora, [m], [(lh, n_cols)])
        assert (t.layer(0)[:n_rows] == ot.layer(0)[:n_rows]).all(), n_rows      # the leaves: the row digests themselves


def test_mixed_height_tree(zk, ora):
    """three matrices of heights 2^6, 2^4, 2^3 and widths 9, 1, 17: the injected levels through k_hash_rows_multi (one lane per row and
    the cooperative form) and through the layer kernels that hash the injected rows themselves"""
    shapes = [(6, 9), (4, 1), (3, 17)]
    rng = np.random.default_rng(77)
    mats = [_matrix(ora, rng, w, 1 << lh, 1 << lh) for lh, w in shapes]
    cfg0 = zk.config()
    try:
        for bulk, coop_log in ((1, 15), (1, 0), (0, 15), (0, 0)):
            zk.set_config(rows_in_bulk=bulk, rows_coop_max_log=coop_log)
            _check_tree(zk, ora, mats, shapes)
    finally:
        zk.set_config(cfg0)


def test_small_proof_equals_the_oracle(zk, ora):
    """one whole proof (2^10 rows, width 20): every kernel that shares the permutation's body -- row sponges, compression layers,
    the pair hashes of the openings -- ends in the proof bytes"""
    import zkvm_prover_amd as z
    from zkvm_prover_amd import air

    params = (1, 0, 8, 4, 4)
    sa = air.SyntheticAir(width=20, n_free=8, n_bool=4, n_boundary=3, seed=3)
    tr, pv = sa.gen_trace(10, seed=4)
    airs = [dict(program=sa.program(), log_height=10, width=20, n_pvs=len(pv), trace=tr, pvs=pv)]
    pk = z.ProvingKey(zk, params, airs)
    proof = pk.prove([zk.upload(tr.reshape(-1))], [pv])
    assert proof == ora.stark_prove(params, airs).tobytes()
    assert z.verify(params, airs, [pv], proof) == 0
