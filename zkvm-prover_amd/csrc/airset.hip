// airset.hip -- the host side of two proofs over ONE stacked WHIR commitment of the main traces of a set of AIRs.  The AIR zero-check
// (zkhip_zerocheck_*, docs/zerocheck.md, model tests/zerocheck_model.py): the main-trace constraints hold on every row.  The AIR-set
// proof (zkhip_airset_*, docs/airset.md, model tests/airset_model.py): the zero-check's steps plus a bus part that an AIR may lack;
// the LogUp-GKR leaves are computed from the committed traces, and per AIR one sum-check carries the constraint zero-check and the
// reduction of the GKR's leaf claims to column values.  Protocols, layouts, limits and measurements are in the two documents.
//
// Device side, per AIR (zc_prove_air, zerocheck_dev.hpp): eq(tau, .) (k_whir_weight); round 0 of the sum-check straight from the
// base-field trace, the constraint program interpreted in the base field once per point (k_zc_round0); the later rounds as one
// streaming pass each that folds every table with the previous challenge and interprets the program in the extension field
// (k_zc_pass), to the last round; the values from the last fold; the rotation reduction on the sum-check core (k_sc_pass,
// sc_small_round) and the columns' values at its point (k_zc_dot).  Then one stacked opening (stacking.hip).
// The bus part, before the AIRs: the leaves of all blocks in one launch (k_as_leaves), the fraction-sum proof (gkr_prove_device, its
// result stays on the device), the blocks' eq factors and the roots' coefficients from rho, kappa and beta (k_as_coefs), the per-AIR
// leaf claims in one pass over the leaf buffers (k_as_claims, k_as_claims_out); an AIR with interactions then runs
// zc_prove_air<true>.  One prover frame, one host verifier (at the end of the file) and one shape serve both proofs.
//
// The keyed form of both (zkhip_airkey_*, with_bus = 0 / 1): the preprocessed columns of the set are ONE stacked WHIR commitment made at
// key generation (zkhip_airkey: the columns resident in Montgomery form, the commitment, its root); both sides observe the root before
// the main root; a PREP leaf is proven like a main cell (the kernels' PREP form reads the key's columns); the values v_p, v_p' and u_p
// follow v, v' and u; a second stacked opening, of the key's commitment, follows the main one.  Keyed proof words:
//   [root 8 | with_bus: GKR words for L | with_bus: 4 per AIR with interactions |
//    per active AIR 4 D_a m + 4 (w + n_rot + w_p + n_rot_p) (+ 8 m + 4 (w + w_p) if n_rot + n_rot_p > 0) |
//    zkhip_stack_proof_words(main columns, log_stack) | zkhip_stack_proof_words(preprocessed columns, log_stack_prep)]
//
// The batched form of both (zkhip_airbatch_*, docs/airbatch.md, model tests/airbatch_model.py; kernels: airbatch_dev.hpp, airbatch_pass.hip): the same
// statements with ONE constraint sum-check and ONE rotation reduction for the whole set, every AIR's point a prefix of the same r (r');
// shape(), prove_bus(), the provers' frame (check_inputs .. open_and_finish) and the verifiers' pieces (verify_start .. verify_openings)
// are shared; prove() / verify() and prove_batch() / verify_batch() are the two step lists over them.
//
// The keyed batched form with cached partitions (zkhip_airkey_cached_*, docs/cached_main.md, model tests/cached_batch_model.py): an AIR's
// leading cached_width main columns are a stacked commitment of their own, made once (zkhip_cached_main); the main commitment holds the
// common columns, the cached roots lead the transcript and the proof, and each partition is opened at its AIR's point after the key's
// opening.  It is prove_batch() and verify_batch() with the handles / log_stack_cached as data; every other form ignores the section.
#include <map>

#include "airbatch_dev.hpp"

// the key of the keyed proofs: made once by zkhip_airkey_create, read by every zkhip_airkey_prove
struct zkhip_airkey {
    zkhip_whir_params params{};
    unsigned l_prep = 0;
    std::vector<std::vector<uint32_t>> programs;   // copies: the caller's need not outlive the call
    std::vector<zkhip_air> airs;                   // program -> programs[a]; prep_trace and prep_commit null
    uint32_t* d_prep = nullptr;                    // every preprocessed column end to end, Montgomery, AIRs in caller order
    std::vector<size_t> prep_at;                   // AIR -> its first word in d_prep
    zkhip_stack_commitment* sc = nullptr;          // the stacked commitment of those columns at l_prep
    uint32_t root[8] = {};
};

// a cached main partition (docs/cached_main.md): the stacked commitment of the first cw main columns of one AIR of a key, made once by
// zkhip_airkey_commit_cached and opened, never modified, by every zkhip_airkey_cached_prove that is handed it
struct zkhip_cached_main {
    zkhip_whir_params params{};
    size_t air = 0;                       // the AIR of the key it was made for
    unsigned m = 0, cw = 0, l = 0;        // that AIR's log height, its cached width, log_stack_cached
    zkhip_stack_commitment* sc = nullptr; // owns the gathered copy of the columns
    uint32_t root[8] = {};
};

namespace zk {

constexpr unsigned AS_BS = 256;          // threads of a leaf workgroup: 256 rows of one block
constexpr unsigned AS_CLAIM_NB = 64;     // workgroups per AIR of the leaf-claim pass

// one block of leaves: interaction j of an AIR, 2^m leaves from `off` on; the last descriptor is the padding (pad = 1)
struct AsBlock {
    const uint32_t* trace;   // the AIR's columns, stride 2^m, Montgomery
    const uint32_t* pvs;     // Montgomery
    const uint32_t* code;    // the interaction's operand program: roots = its fields, then its count
    const uint32_t* consts;
    const uint32_t* prep;    // PREP: the AIR's preprocessed columns in the key, stride 2^m, Montgomery (null: none)
    uint64_t off, n;         // first leaf, leaves
    uint32_t n_ins, bus1, sign, n_fields, pad;
    uint32_t first_wg;       // its first workgroup in the flattened grid
};

// gamma, beta^1 .. beta^LOGUP_MAX_FIELDS (k_logup_chal's layout)
__global__ void k_as_chal(const uint32_t* __restrict__ gb, uint32_t* __restrict__ lchal) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    sc_st(lchal, 0, sc_ld(gb, 0));
    const Ext beta = sc_ld(gb, 1);
    Ext cur = beta;
    for (unsigned i = 1; i <= LOGUP_MAX_FIELDS; i++) sc_st(lchal, i, cur), cur = ext_mul(cur, beta);
}

// the block of a workgroup: the last one whose first_wg is <= wg (prover.hip's chip_of_block on the descriptors themselves)
__device__ __forceinline__ uint32_t as_block_of(const AsBlock* __restrict__ blk, uint32_t n, uint32_t wg) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (blk[mid].first_wg <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// num = +-count and den = gamma + bus + 1 + sum_i beta^(i+1) f_i of one row of one block, straight into the sorted layout; the
// padding's leaves are (0, 1).  The operand program is k_logup_denoms' form: ASSERT k < n_fields is field k, the last one the count.
// PREP (the keyed proofs): an operand may be a cell of the key's columns.
template <bool PREP>
__global__ __launch_bounds__(AS_BS) void k_as_leaves(const AsBlock* __restrict__ blk, uint32_t n_blk, const uint32_t* __restrict__ lchal,
                                                     uint32_t* __restrict__ num, uint32_t* __restrict__ den) {
    extern __shared__ uint32_t as_slots[];   // [slot][lane]
    const AsBlock& b = blk[as_block_of(blk, n_blk, blockIdx.x)];
    const unsigned tid = threadIdx.x;
    const uint64_t r = (uint64_t)(blockIdx.x - b.first_wg) * AS_BS + tid;
    if (r >= b.n) return;
    if (b.pad) {
        num[b.off + r] = 0;
        sc_st(den, b.off + r, ext_one());
        return;
    }
    Ext d = sc_ld(lchal, 0);
    d.c[0] = madd(d.c[0], b.bus1);
    uint32_t cnt = 0;
    auto fetch = [&](uint32_t w) -> uint32_t {
        const uint32_t idx = w & 0x07ffffffu;
        if (PREP && (w >> 28) == K_PREP) return b.prep[(size_t)idx * b.n + r];
        switch (w >> 28) {
            case K_SLOT: return as_slots[idx * AS_BS + tid];
            case K_VAR: return b.trace[(size_t)idx * b.n + r];
            case K_PUB: return b.pvs[idx];
            default: return b.consts[idx];
        }
    };
    for (uint32_t pc = 0; pc < b.n_ins; pc++) {
        const uint32_t w0 = b.code[3 * pc], op = w0 & 0xffu, dst = w0 >> 8;
        const uint32_t va = fetch(b.code[3 * pc + 1]);
        if (op == Q_ASSERT) {
            if (dst < b.n_fields) d = ext_add(d, ext_mul_base(sc_ld(lchal, dst + 1), va));
            else cnt = b.sign ? mneg(va) : va;
        } else if (op == Q_NEG) {
            as_slots[dst * AS_BS + tid] = mneg(va);
        } else {
            const uint32_t vb = fetch(b.code[3 * pc + 2]);
            as_slots[dst * AS_BS + tid] = op == Q_ADD ? madd(va, vb) : op == Q_SUB ? msub(va, vb) : mmul(va, vb);
        }
    }
    num[b.off + r] = cnt;
    sc_st(den, b.off + r, d);
}

// what the coefficient kernel knows of a block / of a root of an AIR's joint program
struct AsBlockPos {
    uint32_t m, hi;   // height, off >> m
};
struct AsRoot {
    uint32_t block, kind;   // kind 0: a count sent (+), 1: a count received (-), 2 + i: field i
};
// From the GKR's point (canonical, at `point`), kappa and the beta powers: rho in Montgomery form, e_b = eq(rho[m_b..L), bits of
// off_b >> m_b) per block, and per root e s (count) or kappa e beta^(i+1) (field i).
__global__ __launch_bounds__(256) void k_as_coefs(const uint32_t* __restrict__ point, unsigned L, const uint32_t* __restrict__ kappa,
                                                  const uint32_t* __restrict__ lchal, const AsBlockPos* __restrict__ pos, unsigned n_blk,
                                                  const AsRoot* __restrict__ roots, unsigned n_roots, uint32_t* __restrict__ rho,
                                                  uint32_t* __restrict__ eb, uint32_t* __restrict__ coef) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * L) rho[i] = to_monty(point[i]);
    auto e_of = [&](unsigned b) {
        const AsBlockPos p = pos[b];
        const Ext one = ext_one();
        Ext e = one;
        for (unsigned t = 0; p.m + t < L; t++) {
            Ext x;
            for (int q = 0; q < 4; q++) x.c[q] = to_monty(point[4 * (p.m + t) + q]);
            e = ext_mul(e, (p.hi >> t) & 1u ? x : ext_sub(one, x));
        }
        return e;
    };
    if (i < n_blk) sc_st(eb, i, e_of(i));
    if (i < n_roots) {
        const AsRoot r = roots[i];
        const Ext e = e_of(r.block);
        sc_st(coef, i, r.kind == 0 ? e : r.kind == 1 ? ext_neg(e) : ext_mul(ext_mul(sc_ld(kappa, 0), e), sc_ld(lchal, r.kind - 1)));
    }
}

// an AIR with interactions in the leaf-claim pass: its blocks ids[first .. first + n), eq(rho[0..m), .) at E
struct AsClaim {
    const uint32_t* E;
    uint32_t m, first, n;
};
// stage 1: workgroup (x, a) sums e_b eq(rho_a, r) (num + kappa den) over its share of AIR a's leaves: 4 words at
// partial[(4 a + q) AS_CLAIM_NB + x]
__global__ __launch_bounds__(256) void k_as_claims(const AsClaim* __restrict__ cl, const uint32_t* __restrict__ ids, const AsBlock* __restrict__ blk,
                                                   const uint32_t* __restrict__ eb, const uint32_t* __restrict__ kappa,
                                                   const uint32_t* __restrict__ num, const uint32_t* __restrict__ den, uint32_t* __restrict__ partial) {
    const AsClaim c = cl[blockIdx.y];
    const Ext k = sc_ld(kappa, 0);
    const uint64_t n = (uint64_t)1 << c.m, total = (uint64_t)c.n << c.m;
    Ext acc[1] = {ext_zero()};
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)AS_CLAIM_NB * 256) {
        const uint32_t b = ids[c.first + (uint32_t)(i >> c.m)];
        const uint64_t r = i & (n - 1), at = blk[b].off + r;
        Ext v = ext_mul(k, sc_ld(den, at));
        v.c[0] = madd(v.c[0], num[at]);
        acc[0] = ext_add(acc[0], ext_mul(sc_ld(eb, b), ext_mul(sc_ld(c.E, r), v)));
    }
    sc_block_sum(acc, partial + (size_t)4 * blockIdx.y * AS_CLAIM_NB + blockIdx.x, AS_CLAIM_NB);
}
// stage 2: wave a adds AIR a's partial sums up; B_a, canonical, to out[4 a ..]
__global__ __launch_bounds__(64) void k_as_claims_out(const uint32_t* __restrict__ partial, uint32_t* __restrict__ out) {
    for (int q = 0; q < 4; q++) {
        const uint32_t x = sc_wave_sum(partial[(size_t)(4 * blockIdx.x + q) * AS_CLAIM_NB + threadIdx.x]);
        if (threadIdx.x == 0) out[4 * blockIdx.x + q] = from_monty(x);
    }
}

namespace {
// ---- host side: the shape ---------------------------------------------------------------------------------------------------------
struct AsBlk {
    unsigned a, j, m;
    uint64_t off;
};
// the whole shape of either proof: plans, the stacked columns' heights and AIRs, the words before the stacked opening
struct Shape {
    std::vector<ZcPlan> plans;
    std::vector<unsigned> lh, col_point, dims;
    size_t head = 8, total = 0;   // head: the words before the stacked opening
    // with_bus only
    std::vector<AsBlk> blocks;   // sorted stably by non-increasing height, laid end to end
    std::vector<size_t> b_at;    // per AIR: its place among the AIRs with interactions, or -1
    unsigned L = 0;
    size_t n_bus = 0, gkr_words = 0;
    // keyed only: the key's stacked columns (the preprocessed columns, AIRs in caller order), one point per AIR that has some
    std::vector<unsigned> lh_p, col_point_p, dims_p;
    std::vector<size_t> prep_airs;   // the AIRs with preprocessed columns
    size_t main_words = 0;           // the main stacked opening's words (the key's opening follows it)
    // the cached form only (docs/cached_main.md); elsewhere a CACHED section is ignored: cw is 0 everywhere and pre is 0
    std::vector<size_t> cw;            // AIR -> its cached width: those leading columns are not in the main commitment
    std::vector<size_t> cached_airs;   // the AIRs with a cached partition
    std::vector<size_t> cached_words;  // per such AIR: the words of its partition's stacked opening (they follow the key's)
    size_t pre = 0, prep_words = 0;    // the cached roots' words before the main root; the key's opening's words
};
// false = refused.  Without with_bus the AIRs' interactions are ignored: their plans have no bus roots (and another D).
// l_prep >= 0: the keyed form at log_stack_prep = l_prep
// l_cached (per AIR, read where the AIR has a CACHED section): the keyed form with cached partitions
bool shape(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, bool with_bus, Shape* S, int l_prep = -1,
           const unsigned* l_cached = nullptr) {
    const bool keyed = l_prep >= 0;
    if (!prm || !airs || n_airs < 1 || n_airs > ZKHIP_STACK_MAX_POINTS) return false;
    S->plans.resize(n_airs);
    std::vector<AirProgram> progs;
    size_t n_cols = 0;
    for (size_t a = 0; a < n_airs; a++) {
        ZcPlan& pl = S->plans[a];
        if (!zc_plan(airs[a], &pl, with_bus, keyed)) return false;
        if (pl.wp) {
            S->dims_p.push_back(pl.m);
            for (size_t c = 0; c < pl.wp; c++) S->lh_p.push_back(pl.m), S->col_point_p.push_back((unsigned)S->prep_airs.size());
            S->prep_airs.push_back(a);
        }
        n_cols += airs[a].width;
        if (n_cols > ZKHIP_STACK_MAX_COLS) return false;
        S->head += pl.active() ? pl.words() : 0;
        S->dims.push_back(airs[a].log_height);
        S->cw.push_back(l_cached ? pl.prog.cached_width : 0);
        if (S->cw[a]) S->cached_airs.push_back(a);
        for (size_t c = S->cw[a]; c < airs[a].width; c++) S->lh.push_back(airs[a].log_height), S->col_point.push_back((unsigned)a);
        if (!with_bus) continue;
        S->b_at.push_back(pl.prog.ints.empty() ? (size_t)-1 : S->n_bus++);
        for (size_t j = 0; j < pl.prog.ints.size(); j++) S->blocks.push_back({(unsigned)a, (unsigned)j, pl.m, 0});
        progs.push_back(pl.prog);
    }
    if (with_bus) {
        if (S->blocks.empty()) return false;   // no interaction anywhere: zkhip_zerocheck_prove's case
        if (!logup_bus_counts_bounded(progs.data(), S->dims.data(), n_airs)) return false;
        std::stable_sort(S->blocks.begin(), S->blocks.end(), [](const AsBlk& x, const AsBlk& y) { return x.m > y.m; });
        uint64_t T = 0;
        for (AsBlk& b : S->blocks) b.off = T, T += (uint64_t)1 << b.m;
        S->L = 1;
        while (((uint64_t)1 << S->L) < T) S->L++;
        if (S->L > ZKHIP_GKR_MAX_LOG_N) return false;
        S->gkr_words = zkhip_gkr_proof_words(S->L);
        S->head += S->gkr_words + 4 * S->n_bus;
    }
    const size_t sw = zkhip_stack_proof_words(prm, S->lh.data(), S->lh.size(), l);
    if (!sw) return false;
    S->main_words = sw, S->total = S->head + sw;
    if (keyed) {
        if (S->prep_airs.empty()) return false;   // no PREP anywhere: the unkeyed calls' case
        const size_t sp = zkhip_stack_proof_words(prm, S->lh_p.data(), S->lh_p.size(), (unsigned)l_prep);
        if (!sp) return false;
        S->prep_words = sp, S->total += sp;
    }
    if (l_cached) {
        if (!keyed || S->cached_airs.empty()) return false;   // no CACHED anywhere: zkhip_airkey_batch_*'s case
        for (size_t a : S->cached_airs) {
            const std::vector<unsigned> lhc(S->cw[a], S->plans[a].m);
            const size_t sc = zkhip_stack_proof_words(prm, lhc.data(), lhc.size(), l_cached[a]);
            if (!sc) return false;
            S->cached_words.push_back(sc), S->total += sc;
        }
        S->pre = 8 * S->cached_airs.size(), S->head += S->pre, S->total += S->pre;
    }
    return true;
}

// ---- the device prover ---------------------------------------------------------------------------------------------------------
// The bus part of the AIR-set proof (docs/airset.md, steps 2 - 5), after the root and the public values were observed: the leaves,
// the fraction-sum proof (its words to dP + 8), the leaf claims B_a (after them), and per AIR with interactions what its joint
// sum-check needs (bus[a]).  Its buffers are B's: they live until the caller's per-AIR loop is done.
int prove_bus(zkhip_ctx* ctx, const Shape& S, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces, const uint32_t* const* pvs,
              DevTranscript* d_t, DevBufs& B, uint32_t* dP, std::vector<ZcBus>* bus, const zkhip_airkey* key,
              const uint32_t** chal_out = nullptr) {
    hipStream_t st = ctx->stream;
    const unsigned L = S.L;
    const size_t n_blk = S.blocks.size(), NL = (size_t)1 << L;
    // the interactions' operand programs, the descriptors and the roots of the joint programs: one upload
    //   words: [code | consts | pvs (Montgomery) | ids]; then the three descriptor arrays in buffers of their own
    std::vector<uint32_t> code, consts, pvm, ids;
    std::vector<size_t> pv_at(n_airs);
    for (size_t a = 0; a < n_airs; a++) {
        pv_at[a] = pvm.size();
        for (size_t i = 0; i < airs[a].n_pvs; i++) pvm.push_back(to_monty(pvs[a][i]));
    }
    struct Lowered {
        size_t code_at, const_at, n_ins;
    };
    std::vector<Lowered> low(n_blk);
    unsigned max_slots = 1;
    for (size_t b = 0; b < n_blk; b++) {
        const AsBlk& k = S.blocks[b];
        const Interaction& it = S.plans[k.a].prog.ints[k.j];
        std::vector<uint32_t> roots(it.fields, it.fields + it.n_fields);
        roots.push_back(it.count);
        CompiledAir ca;
        std::string err;
        if (compile_air(S.plans[k.a].prog, &ca, &err, &roots) != 0 || ca.n_slots > ZC_MAX_SLOTS)
            return set_error(ctx, ZKHIP_ERR_INVALID, "airset: " + (err.empty() ? "an interaction needs more than 64 live intermediates" : err));
        low[b] = {code.size() / 3, consts.size(), ca.code.size() / 3};
        code.insert(code.end(), ca.code.begin(), ca.code.end());
        consts.insert(consts.end(), ca.consts.begin(), ca.consts.end());
        max_slots = std::max(max_slots, ca.n_slots);
    }
    // per AIR with interactions: its blocks in program order (ids), the roots of its bus part (count, then fields, per interaction)
    std::vector<AsRoot> roots;
    std::vector<size_t> root_at(n_airs, 0), ids_at(n_airs, 0);
    {
        std::vector<std::vector<uint32_t>> of(n_airs);
        for (size_t a = 0; a < n_airs; a++) of[a].resize(S.plans[a].prog.ints.size());
        for (size_t b = 0; b < n_blk; b++) of[S.blocks[b].a][S.blocks[b].j] = (uint32_t)b;
        for (size_t a = 0; a < n_airs; a++) {
            root_at[a] = roots.size(), ids_at[a] = ids.size();
            for (size_t j = 0; j < of[a].size(); j++) {
                const Interaction& it = S.plans[a].prog.ints[j];
                ids.push_back(of[a][j]);
                roots.push_back({of[a][j], it.sign});
                for (uint32_t i = 0; i < it.n_fields; i++) roots.push_back({of[a][j], 2 + i});
            }
        }
    }
    std::vector<uint32_t> up(code);
    const size_t o_consts = up.size();
    up.insert(up.end(), consts.begin(), consts.end());
    const size_t o_pvs = up.size();
    up.insert(up.end(), pvm.begin(), pvm.end());
    const size_t o_ids = up.size();
    up.insert(up.end(), ids.begin(), ids.end());
    // device: challenges [gamma | beta | kappa]; the beta powers; rho (Montgomery); e_b; the roots' coefficients; the leaves (20 B each)
    uint32_t *d_up = B.get(up.size()), *ch = B.get(12);
    uint32_t *lchal = B.get(4 * (LOGUP_MAX_FIELDS + 1)), *rho = B.get(4 * (size_t)L), *eb = B.get(4 * n_blk), *coef = B.get(4 * roots.size());
    uint32_t *d_num = B.get(NL), *d_den = B.get(4 * NL), *partial = B.get(4 * S.n_bus * AS_CLAIM_NB);
    AsBlock* d_blk = (AsBlock*)B.get((n_blk + 1) * sizeof(AsBlock) / 4);
    AsBlockPos* d_pos = (AsBlockPos*)B.get(n_blk * sizeof(AsBlockPos) / 4);
    AsRoot* d_roots = (AsRoot*)B.get(roots.size() * sizeof(AsRoot) / 4);
    AsClaim* d_cl = (AsClaim*)B.get(S.n_bus * sizeof(AsClaim) / 4);
    if (!d_up || !ch || !lchal || !rho || !eb || !coef || !d_num || !d_den || !partial || !d_blk || !d_pos || !d_roots || !d_cl)
        return set_error(ctx, ZKHIP_ERR_NOMEM, "airset: the leaves do not fit");
    if (chal_out) *chal_out = ch;   // the batched proof's round kernel reads gamma and kappa
    // one eq(rho[0..m), .) table per distinct height of an AIR with interactions
    std::map<unsigned, uint32_t*> eq_of;
    for (const AsBlk& k : S.blocks)
        if (!eq_of.count(k.m) && !(eq_of[k.m] = B.get(4 * ((size_t)1 << k.m)))) return set_error(ctx, ZKHIP_ERR_NOMEM, "airset: the eq tables do not fit");
    std::vector<AsBlock> hb(n_blk + 1);
    std::vector<AsBlockPos> hpos(n_blk);
    uint64_t wg = 0;
    for (size_t b = 0; b <= n_blk; b++) {
        AsBlock& d = hb[b];
        d = AsBlock{};
        d.first_wg = (uint32_t)wg;
        if (b == n_blk) {   // the padding [T, 2^L)
            const uint64_t T = S.blocks.back().off + ((uint64_t)1 << S.blocks.back().m);
            d.off = T, d.n = NL - T, d.pad = 1;
        } else {
            const AsBlk& k = S.blocks[b];
            const Interaction& it = S.plans[k.a].prog.ints[k.j];
            d.trace = d_traces[k.a], d.pvs = d_up + o_pvs + pv_at[k.a];
            d.prep = key && S.plans[k.a].wp ? key->d_prep + key->prep_at[k.a] : nullptr;
            d.code = d_up + 3 * low[b].code_at, d.consts = d_up + o_consts + low[b].const_at;
            d.off = k.off, d.n = (uint64_t)1 << k.m;
            d.n_ins = (uint32_t)low[b].n_ins, d.bus1 = to_monty(it.bus + 1), d.sign = it.sign, d.n_fields = it.n_fields;
            hpos[b] = {k.m, (uint32_t)(k.off >> k.m)};
        }
        wg += (d.n + AS_BS - 1) / AS_BS;
    }
    std::vector<AsClaim> hcl;
    for (size_t a = 0; a < n_airs; a++)
        if (!S.plans[a].prog.ints.empty()) hcl.push_back({eq_of[S.plans[a].m], S.plans[a].m, (uint32_t)ids_at[a], (uint32_t)S.plans[a].prog.ints.size()});
    ZK_TRY(zkhip_h2d(ctx, d_up, up.data(), up.size() * 4));
    ZK_TRY(zkhip_h2d(ctx, d_blk, hb.data(), hb.size() * sizeof(AsBlock)));
    ZK_TRY(zkhip_h2d(ctx, d_pos, hpos.data(), hpos.size() * sizeof(AsBlockPos)));
    ZK_TRY(zkhip_h2d(ctx, d_roots, roots.data(), roots.size() * sizeof(AsRoot)));
    ZK_TRY(zkhip_h2d(ctx, d_cl, hcl.data(), hcl.size() * sizeof(AsClaim)));
    // 2. gamma, beta   3. the leaves
    ZK_TRY(transcript_sample(ctx, d_t, ch, nullptr, 4));
    ZK_TRY(transcript_sample(ctx, d_t, ch + 4, nullptr, 4));
    {
        KernelScope ks(ctx, "as_chal");
        hipLaunchKernelGGL(k_as_chal, dim3(1), dim3(64), 0, st, (const uint32_t*)ch, lchal);
    }
    {
        KernelScope ks(ctx, "as_leaves");
        if (key)
            hipLaunchKernelGGL(k_as_leaves<true>, dim3((unsigned)wg), dim3(AS_BS), (size_t)max_slots * AS_BS * 4, st, (const AsBlock*)d_blk,
                               (uint32_t)(n_blk + 1), (const uint32_t*)lchal, d_num, d_den);
        else
            hipLaunchKernelGGL(k_as_leaves<false>, dim3((unsigned)wg), dim3(AS_BS), (size_t)max_slots * AS_BS * 4, st, (const AsBlock*)d_blk,
                               (uint32_t)(n_blk + 1), (const uint32_t*)lchal, d_num, d_den);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    // 4. the fraction-sum proof; its words, rho and the claims stay on the device
    const uint32_t* d_res = nullptr;
    ZK_TRY(gkr_prove_device(ctx, d_t, d_num, false, d_den, L, &d_res));
    ZK_HIP_CHECK(ctx, hipMemcpyAsync(dP + 8, d_res, S.gkr_words * 4, hipMemcpyDeviceToDevice, st));
    // 5. kappa, the coefficients, the eq tables, the leaf claims
    uint32_t* kappa = ch + 8;
    ZK_TRY(transcript_sample(ctx, d_t, kappa, nullptr, 4));
    {
        KernelScope ks(ctx, "as_coefs");
        const size_t nthr = std::max<size_t>(std::max<size_t>(4 * L, n_blk), roots.size());
        hipLaunchKernelGGL(k_as_coefs, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, d_res + S.gkr_words, L, (const uint32_t*)kappa,
                           (const uint32_t*)lchal, (const AsBlockPos*)d_pos, (unsigned)n_blk, (const AsRoot*)d_roots, (unsigned)roots.size(), rho, eb,
                           coef);
    }
    for (auto& e : eq_of) {
        KernelScope ks(ctx, "as_eq");
        whir_eq_launch(st, e.second, e.first, rho);
    }
    uint32_t* dB = dP + 8 + S.gkr_words;
    {
        KernelScope ks(ctx, "as_claims");
        hipLaunchKernelGGL(k_as_claims, dim3(AS_CLAIM_NB, (unsigned)S.n_bus), dim3(256), 0, st, (const AsClaim*)d_cl, (const uint32_t*)(d_up + o_ids),
                           (const AsBlock*)d_blk, (const uint32_t*)eb, (const uint32_t*)kappa, (const uint32_t*)d_num, (const uint32_t*)d_den, partial);
    }
    {
        KernelScope ks(ctx, "as_claims");
        hipLaunchKernelGGL(k_as_claims_out, dim3((unsigned)S.n_bus), dim3(64), 0, st, (const uint32_t*)partial, dB);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ZK_TRY(transcript_observe(ctx, d_t, dB, (uint32_t)(4 * S.n_bus), true));
    for (size_t a = 0; a < n_airs; a++)
        if (!S.plans[a].prog.ints.empty()) (*bus)[a] = ZcBus{eq_of[S.plans[a].m], coef + 4 * root_at[a]};
    return ZKHIP_OK;
}

// ---- what prove() and prove_batch() share ---------------------------------------------------------------------------------------
// what a prove call was handed; key: the keyed form (prm, airs and n_airs are the key's), cached: the cached form (prove_batch only)
struct ProveIn {
    zkhip_ctx* ctx; const zkhip_whir_params* prm; const zkhip_air* airs; size_t n_airs; const uint32_t* const* d_traces; const uint32_t* const* pvs;
    unsigned l; bool with_bus; DevTranscript* d_t; uint32_t* proof_out; size_t cap; uint32_t* root_out; const zkhip_airkey* key;
    zkhip_cached_main* const* cached;
};
// the main commitment of one prove call, destroyed on every way out
struct MainCom {
    zkhip_ctx* ctx;
    zkhip_stack_commitment* sc = nullptr;
    uint32_t root[8] = {};
    ~MainCom() { stack_destroy(ctx, sc); }
};
// n_pv: the public values of the whole set
int check_inputs(const ProveIn& in, const std::string& who, size_t* n_pv) {
    *n_pv = 0;
    for (size_t a = 0; a < in.n_airs; a++) {
        if (!in.d_traces[a] || (in.airs[a].n_pvs && !in.pvs[a])) return set_error(in.ctx, ZKHIP_ERR_INVALID, who + "null trace or public values");
        for (size_t i = 0; i < in.airs[a].n_pvs; i++)
            if (in.pvs[a][i] >= P) return set_error(in.ctx, ZKHIP_ERR_INVALID, who + "public value not canonical");
        *n_pv += in.airs[a].n_pvs;
    }
    return ZKHIP_OK;
}
// 1. commit: every main column from S.cw[a] on (0 outside the cached form, whose partitions were committed before), AIRs in caller order
int commit_main(const ProveIn& in, const Shape& S, MainCom* com) {
    std::vector<const uint32_t*> cols;
    for (size_t a = 0; a < in.n_airs; a++)
        for (size_t c = S.cw[a]; c < in.airs[a].width; c++) cols.push_back(in.d_traces[a] + (c << in.airs[a].log_height));
    return stack_commit(in.ctx, in.prm, cols.data(), S.lh.data(), cols.size(), in.l, &com->sc, com->root);
}
// observed before anything is sampled, through d_obs (obs_words() words): [the key's root (observed, not sent) | the cached roots |
// the main root | the public values]
size_t obs_words(const ProveIn& in, const Shape& S, size_t n_pv) { return (in.key ? 16 : 8) + S.pre + n_pv; }
int observe_start(const ProveIn& in, const Shape& S, uint32_t* d_obs, const uint32_t* root) {
    std::vector<uint32_t> obs;
    if (in.key) obs.assign(in.key->root, in.key->root + 8);
    for (size_t a : S.cached_airs) obs.insert(obs.end(), in.cached[a]->root, in.cached[a]->root + 8);
    obs.insert(obs.end(), root, root + 8);
    for (size_t a = 0; a < in.n_airs; a++) obs.insert(obs.end(), in.pvs[a], in.pvs[a] + in.airs[a].n_pvs);
    ZK_TRY(zkhip_h2d(in.ctx, d_obs, obs.data(), obs.size() * 4));
    return transcript_observe(in.ctx, in.d_t, d_obs, (uint32_t)obs.size(), true);
}
// The closing openings, on one transcript, in this order: the main commitment at every AIR's point, the key's at the points of the
// AIRs that have preprocessed columns, each cached partition's at its AIR's point.  h: the read-back (the points canonical), pt_at:
// AIR -> its point in h, head: the words before the main opening.  Then the roots and the head's words go to the proof.
int open_and_finish(const ProveIn& in, const Shape& S, const MainCom& com, const std::vector<uint32_t>& h, const std::vector<size_t>& pt_at,
                    size_t head) {
    std::vector<uint32_t> points, points_p;
    for (size_t a = 0; a < in.n_airs; a++) {
        const auto from = h.begin() + pt_at[a], to = from + 4 * (size_t)S.plans[a].m;
        points.insert(points.end(), from, to);
        if (in.key && S.plans[a].wp) points_p.insert(points_p.end(), from, to);
    }
    uint32_t* out = in.proof_out;
    size_t o = head;
    ZK_TRY(stack_open(in.ctx, com.sc, in.d_t, points.data(), S.dims.data(), S.dims.size(), S.col_point.data(), nullptr, out + o, in.cap - o));
    o += S.main_words;
    if (in.key)
        ZK_TRY(stack_open(in.ctx, in.key->sc, in.d_t, points_p.data(), S.dims_p.data(), S.dims_p.size(), S.col_point_p.data(), nullptr, out + o, in.cap - o));
    o += S.prep_words;
    for (size_t k = 0; k < S.cached_airs.size(); o += S.cached_words[k], k++) {
        const size_t a = S.cached_airs[k];
        const std::vector<unsigned> zero(S.cw[a], 0);
        ZK_TRY(stack_open(in.ctx, in.cached[a]->sc, in.d_t, h.data() + pt_at[a], &S.dims[a], 1, zero.data(), nullptr, out + o, in.cap - o));
        memcpy(out + 8 * k, in.cached[a]->root, 32);
    }
    memcpy(out + S.pre, com.root, 32);
    memcpy(out + S.pre + 8, h.data() + S.pre + 8, (head - S.pre - 8) * 4);
    if (in.root_out) memcpy(in.root_out, com.root, 32);
    return ZKHIP_OK;
}
// either proof: with_bus, the AIR-set proof of docs/airset.md (its step numbers below); without, the zero-check of docs/zerocheck.md
int prove(const ProveIn& in) {
    zkhip_ctx* ctx = in.ctx;
    const size_t n_airs = in.n_airs;
    const zkhip_airkey* key = in.key;
    const std::string who = key ? "airkey: " : in.with_bus ? "airset: " : "zerocheck: ";
    Shape S;
    if (!shape(in.prm, in.airs, n_airs, in.l, in.with_bus, &S, key ? (int)key->l_prep : -1))
        return set_error(ctx, ZKHIP_ERR_INVALID, who + "the shape does not fit the limits");
    if (in.cap < S.total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, who + "proof buffer too small");
    size_t n_pv = 0;
    ZK_TRY(check_inputs(in, who, &n_pv));
    std::vector<size_t> pt_at(n_airs);   // AIR -> its point r'_a, after the words before the opening
    size_t back_words = S.head;
    for (size_t a = 0; a < n_airs; a++) pt_at[a] = back_words, back_words += 4 * (size_t)in.airs[a].log_height;
    MainCom com{ctx};
    ZK_TRY(commit_main(in, S, &com));   // 1.
    DevBufs B(ctx);
    // device: [the words before the opening | the points r'_a (Montgomery)], then the roots and the public values to observe
    uint32_t *dP = B.get(back_words), *d_obs = B.get(obs_words(in, S, n_pv));
    if (!dP || !d_obs) return set_error(ctx, ZKHIP_ERR_NOMEM, who + "proof staging");
    ZK_TRY(observe_start(in, S, d_obs, com.root));
    // 2. - 5. the bus part
    std::vector<ZcBus> bus(n_airs);   // E2 null: an AIR without interactions, or the zero-check
    if (in.with_bus) ZK_TRY(prove_bus(ctx, S, in.airs, n_airs, in.d_traces, in.pvs, in.d_t, B, dP, &bus, key));
    // 6. - 8. per AIR
    size_t off = 8 + S.gkr_words + 4 * S.n_bus;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        const uint32_t *tr = in.d_traces[a], *pv = in.pvs[a];
        uint32_t *out = dP + off, *pt = dP + pt_at[a];
        if (key && pl.wp) {   // the kernels' PREP form, on the key's resident columns
            const uint32_t* prep = key->d_prep + key->prep_at[a];
            if (bus[a].E2) ZK_TRY((zc_prove_air<true, true>(ctx, in.d_t, pl, tr, pv, out, pt, bus[a], prep)));
            else ZK_TRY((zc_prove_air<false, true>(ctx, in.d_t, pl, tr, pv, out, pt, ZcBus{}, prep)));
        } else if (bus[a].E2) ZK_TRY(zc_prove_air<true>(ctx, in.d_t, pl, tr, pv, out, pt, bus[a]));
        else ZK_TRY(zc_prove_air<false>(ctx, in.d_t, pl, tr, pv, out, pt));
        off += pl.active() ? pl.words() : 0;
    }
    // 9. the one read-back before the openings: the words so far and the points
    std::vector<uint32_t> h(back_words);
    ZK_TRY(zkhip_d2h(ctx, h.data(), dP, h.size() * 4));
    for (size_t i = S.head; i < h.size(); i++) h[i] = from_monty(h[i]);
    return open_and_finish(in, S, com, h, pt_at, S.head);
}

// ---- the host verifier: the pieces verify() and verify_batch() share --------------------------------------------------------------
// what a verify call was handed; prep_root: the keyed form, l_cached: the cached form (verify_batch only)
struct VerIn {
    const zkhip_whir_params* prm; const uint32_t* prefix; size_t n_prefix; const zkhip_air* airs; size_t n_airs; const uint32_t* const* pvs;
    unsigned l; const uint32_t* proof; size_t words; bool with_bus; const uint32_t* prep_root; unsigned l_prep; const unsigned* l_cached;
};
// The checks after shape(), refusing in this order: prep_root, the public values, the prefix (ZKHIP_ERR_INVALID), the length, the
// head's words (ZKHIP_ERR_VERIFY); then the transcript's start.  head, total: the form's words before the main opening and in all.
int verify_start(HostChallenger& ch, const VerIn& in, const Shape& S, size_t head, size_t total) {
    for (size_t i = 0; in.prep_root && i < 8; i++)
        if (in.prep_root[i] >= P) return ZKHIP_ERR_INVALID;
    for (size_t a = 0; a < in.n_airs; a++) {
        if (in.airs[a].n_pvs && !in.pvs[a]) return ZKHIP_ERR_INVALID;
        for (size_t i = 0; i < in.airs[a].n_pvs; i++)
            if (in.pvs[a][i] >= P) return ZKHIP_ERR_INVALID;
    }
    for (size_t i = 0; i < in.n_prefix; i++)
        if (in.prefix[i] >= P) return ZKHIP_ERR_INVALID;
    if (in.words != total) return ZKHIP_ERR_VERIFY;
    for (size_t i = 0; i < head; i++)
        if (in.proof[i] >= P) return ZKHIP_ERR_VERIFY;
    ch.observe_canon(in.prefix, in.n_prefix);
    if (in.prep_root) ch.observe_canon(in.prep_root, 8);
    ch.observe_canon(in.proof, S.pre + 8);   // the cached roots (none in the per-AIR form), then the main root
    for (size_t a = 0; a < in.n_airs; a++) ch.observe_canon(in.pvs[a], in.airs[a].n_pvs);
    return ZKHIP_OK;
}
// what the bus part leaves for the later steps; without a bus part it stays as constructed and nothing reads it
struct BusV {
    Ext gamma = ext_zero(), kappa = ext_zero();
    std::vector<Ext> rho, eb, bpow;             // the GKR's point, e_b per block, beta^0 .. beta^LOGUP_MAX_FIELDS
    std::vector<std::vector<size_t>> blk_of;    // AIR -> its blocks in program order
    const uint32_t* qB = nullptr;               // the leaf claims B_a
};
// the bus part (docs/airset.md, steps 2 - 5), q at the fraction-sum proof's words
int verify_bus(HostChallenger& ch, const Shape& S, const uint32_t* q, BusV* V) {
    const Ext one = ext_one();
    const size_t n_blk = S.blocks.size();
    // 2. - 4. gamma, beta, the fraction-sum proof: rho, (p*, q*), balance
    V->gamma = ch.sample_ext();
    const Ext beta = ch.sample_ext();
    std::vector<uint32_t> pt(4 * (size_t)S.L);
    uint32_t cl8[8];
    Ext pq[2];
    ZK_TRY(gkr_verify_host(ch, q, S.gkr_words, S.L, pt.data(), cl8, pq));
    if (!ext_eq(pq[0], ext_zero()) || ext_eq(pq[1], ext_zero())) return ZKHIP_ERR_VERIFY;
    V->rho.resize(S.L);
    for (unsigned j = 0; j < S.L; j++) V->rho[j] = ext_from_canon(pt.data() + 4 * j);
    const Ext pstar = ext_from_canon(cl8), qstar = ext_from_canon(cl8 + 4);
    // 5. the leaf claims: sum_a B_a + kappa (the padding's share) = p* + kappa q*
    Ext pad = one;
    V->eb.resize(n_blk);
    for (size_t b = 0; b < n_blk; b++) {
        const AsBlk& k = S.blocks[b];
        Ext e = one;
        for (unsigned t = 0; k.m + t < S.L; t++) e = ext_mul(e, ((k.off >> k.m) >> t) & 1u ? V->rho[k.m + t] : ext_sub(one, V->rho[k.m + t]));
        V->eb[b] = e, pad = ext_sub(pad, e);
    }
    V->kappa = ch.sample_ext();
    V->qB = q + S.gkr_words;
    Ext lhs = ext_mul(V->kappa, pad);
    for (size_t i = 0; i < S.n_bus; i++) lhs = ext_add(lhs, ext_from_canon(V->qB + 4 * i));
    ch.observe_canon(V->qB, 4 * S.n_bus);
    if (!ext_eq(lhs, ext_add(pstar, ext_mul(V->kappa, qstar)))) return ZKHIP_ERR_VERIFY;
    V->bpow.assign(LOGUP_MAX_FIELDS + 1, one);
    for (unsigned i = 1; i <= LOGUP_MAX_FIELDS; i++) V->bpow[i] = ext_mul(V->bpow[i - 1], beta);
    V->blk_of.resize(S.plans.size());
    for (size_t a = 0; a < S.plans.size(); a++) V->blk_of[a].resize(S.plans[a].prog.ints.size());
    for (size_t b = 0; b < n_blk; b++) V->blk_of[S.blocks[b].a][S.blocks[b].j] = b;
    return ZKHIP_OK;
}
// AIR a's bus claim B_a - kappa sum_j e_{a,j} (gamma + bus_j + 1), and the coefficients of its bus roots in pl.bus_roots' order:
// per interaction +-e (its count), then kappa e beta^(i+1) (field i)
Ext bus_claim(const Shape& S, const BusV& V, size_t a, std::vector<Ext>* coef) {
    const ZcPlan& pl = S.plans[a];
    Ext cst = ext_zero();
    for (size_t j = 0; j < V.blk_of[a].size(); j++) {
        const Interaction& it = pl.prog.ints[j];
        const Ext e = V.eb[V.blk_of[a][j]], ke = ext_mul(V.kappa, e);
        Ext g1 = V.gamma;
        g1.c[0] = madd(g1.c[0], to_monty(it.bus + 1));
        cst = ext_add(cst, ext_mul(e, g1));
        coef->push_back(it.sign ? ext_neg(e) : e);
        for (uint32_t i = 0; i < it.n_fields; i++) coef->push_back(ext_mul(ke, V.bpow[i + 1]));
    }
    return ext_sub(ext_from_canon(V.qB + 4 * S.b_at[a]), ext_mul(V.kappa, cst));
}
// m rounds of a sum-check of degree D from q on: a round sends s(0), s(2), .., s(D) (s(1) = claim - s(0)), is observed and answered
// by r[i]; returns the last claim, q after the rounds
Ext rounds_host(HostChallenger& ch, const uint32_t*& q, unsigned m, unsigned D, Ext claim, Ext* r) {
    for (unsigned i = 0; i < m; i++, q += 4 * D) {
        Ext s[ZKHIP_ZEROCHECK_MAX_DEGREE + 1];
        s[0] = ext_from_canon(q), s[1] = ext_sub(claim, s[0]);
        for (unsigned e = 1; e < D; e++) s[e + 1] = ext_from_canon(q + 4 * e);
        ch.observe_canon(q, 4 * D);
        r[i] = ch.sample_ext();
        claim = poly_at(s, D, r[i]);
    }
    return claim;
}
// One AIR's summand at r[0..m), from its values [v | v' | v_p | v_p'] at q:
//   eq(tau, r) sum_k alpha^k C_k  (if it has proven constraints)  +  eq(rho, r) sum_k coef_k root_k  (if it has bus roots)
// parse_air: interaction operands read the current row only, so neither v' nor first / last enters the bus half
Ext air_summand(const ZcPlan& pl, const uint32_t* q, const uint32_t* pvs, const Ext* tau, const Ext& alpha, const Ext* rho, const std::vector<Ext>& coef,
                const Ext* r) {
    const Ext one = ext_one();
    const size_t w = pl.w, n_rot = pl.rot.size(), wp = pl.wp, n_rot_p = pl.rot_p.size();
    std::vector<Ext> v(w), vn(n_rot), vp(wp), vpn(n_rot_p);
    for (size_t j = 0; j < w; j++) v[j] = ext_from_canon(q + 4 * j);
    for (size_t t = 0; t < n_rot; t++) vn[t] = ext_from_canon(q + 4 * (w + t));
    for (size_t j = 0; j < wp; j++) vp[j] = ext_from_canon(q + 4 * (w + n_rot + j));
    for (size_t t = 0; t < n_rot_p; t++) vpn[t] = ext_from_canon(q + 4 * (w + n_rot + wp + t));
    Ext first = one, last = one, g = ext_zero();
    for (unsigned j = 0; j < pl.m; j++) first = ext_mul(first, ext_sub(one, r[j])), last = ext_mul(last, r[j]);
    if (!pl.proven.empty()) {
        const std::vector<Ext> val = zc_eval_host(pl, pl.reach, v.data(), vn.data(), first, last, pvs, vp.data(), vpn.data());
        Ext c = ext_zero(), ap = one;
        for (uint32_t k : pl.proven) c = ext_add(c, ext_mul(ap, val[k])), ap = ext_mul(ap, alpha);
        g = ext_mul(eq_eval(tau, r, pl.m), c);
    }
    if (!pl.bus_roots.empty()) {
        const std::vector<Ext> val = zc_eval_host(pl, pl.bus_reach, v.data(), vn.data(), first, last, pvs, vp.data(), vpn.data());
        Ext c = ext_zero();
        for (size_t k = 0; k < coef.size(); k++) c = ext_add(c, ext_mul(coef[k], val[pl.bus_roots[k]]));
        g = ext_add(g, ext_mul(eq_eval(rho, r, pl.m), c));
    }
    return g;
}
// the rotation reduction's start for one AIR: lp = lambda^(o + k) over its n_val values at q, from *x = lambda^o on (left at the
// next AIR's first power); returns sum_k lp_k value_k
Ext lambda_comb(const uint32_t* q, size_t n_val, const Ext& lambda, Ext* x, std::vector<Ext>* lp) {
    Ext acc = ext_zero();
    for (size_t k = 0; k < n_val; k++) lp->push_back(*x), acc = ext_add(acc, ext_mul(*x, ext_from_canon(q + 4 * k))), *x = ext_mul(*x, lambda);
    return acc;
}
// the rotation reduction's end for one AIR: ua eq(r, rp) + ub rot(r, rp) from [u | u_p] at q and its lambda powers lp over
// [v | v' | v_p | v_p']: ua takes u and u_p with v's and v_p's powers, ub the rotated columns' entries with v''s and v_p''s
Ext u_term(const ZcPlan& pl, const Ext* lp, const uint32_t* q, const Ext* r, const Ext* rp) {
    const size_t w = pl.w, n_rot = pl.rot.size(), wp = pl.wp;
    const uint32_t* qp = q + 4 * w;   // u_p
    Ext ua = ext_zero(), ub = ext_zero();
    for (size_t j = 0; j < w; j++) ua = ext_add(ua, ext_mul(lp[j], ext_from_canon(q + 4 * j)));
    for (size_t t = 0; t < n_rot; t++) ub = ext_add(ub, ext_mul(lp[w + t], ext_from_canon(q + 4 * pl.rot[t])));
    for (size_t j = 0; j < wp; j++) ua = ext_add(ua, ext_mul(lp[w + n_rot + j], ext_from_canon(qp + 4 * j)));
    for (size_t t = 0; t < pl.rot_p.size(); t++) ub = ext_add(ub, ext_mul(lp[w + n_rot + wp + t], ext_from_canon(qp + 4 * pl.rot_p[t])));
    return ext_add(ext_mul(ua, eq_eval(r, rp, pl.m)), ext_mul(ub, zc_rot_eval(r, rp, pl.m)));
}
// The openings, from the proof's word `head` on: the main commitment at every AIR's point; the key's, against the verifier's own
// root, at the points of the AIRs that have preprocessed columns (an inactive one too); each partition's, against the root the proof
// sent, at its AIR's point.  points: canonical, AIRs end to end.  claimed[a] (null: none, an inactive AIR's values stand): AIR a's w
// values, the first S.cw[a] the partition's, the rest the main opening's; claimed_p[a]: its w_p values in the key's opening.
int verify_openings(HostChallenger& ch, const VerIn& in, const Shape& S, size_t head, const std::vector<uint32_t>& points,
                    const std::vector<const uint32_t*>& claimed, const std::vector<const uint32_t*>& claimed_p) {
    const size_t n_airs = in.n_airs;
    const uint32_t* op = in.proof + head;
    ZK_TRY(stack_verify_host(ch, in.prm, in.proof + S.pre, S.lh.data(), S.lh.size(), in.l, points.data(), S.dims.data(), n_airs, S.col_point.data(),
                             op, S.main_words));
    size_t col = 0;
    for (size_t a = 0; a < n_airs; col += in.airs[a].width - S.cw[a], a++)
        if (claimed[a] && memcmp(claimed[a] + 4 * S.cw[a], op + 4 * col, 16 * (in.airs[a].width - S.cw[a])) != 0) return ZKHIP_ERR_VERIFY;
    op += S.main_words;
    if (in.prep_root) {
        std::vector<uint32_t> pts;
        size_t at = 0;
        for (size_t a = 0; a < n_airs; at += 4 * (size_t)S.plans[a].m, a++)
            if (S.plans[a].wp) pts.insert(pts.end(), points.begin() + at, points.begin() + at + 4 * (size_t)S.plans[a].m);
        ZK_TRY(stack_verify_host(ch, in.prm, in.prep_root, S.lh_p.data(), S.lh_p.size(), in.l_prep, pts.data(), S.dims_p.data(), S.dims_p.size(),
                                 S.col_point_p.data(), op, S.prep_words));
        col = 0;
        for (size_t a = 0; a < n_airs; col += S.plans[a].wp, a++)
            if (claimed_p[a] && memcmp(claimed_p[a], op + 4 * col, 16 * S.plans[a].wp) != 0) return ZKHIP_ERR_VERIFY;
    }
    op += S.prep_words;
    size_t at = 0;
    for (size_t a = 0, k = 0; a < n_airs; at += 4 * (size_t)S.plans[a].m, a++) {
        if (!S.cw[a]) continue;   // every AIR outside the cached form: in.l_cached is not read
        const std::vector<unsigned> lhc(S.cw[a], S.plans[a].m), zero(S.cw[a], 0);
        ZK_TRY(stack_verify_host(ch, in.prm, in.proof + 8 * k, lhc.data(), lhc.size(), in.l_cached[a], points.data() + at, &S.dims[a], 1, zero.data(),
                                 op, S.cached_words[k]));
        if (claimed[a] && memcmp(claimed[a], op, 16 * S.cw[a]) != 0) return ZKHIP_ERR_VERIFY;
        op += S.cached_words[k++];
    }
    return ZKHIP_OK;
}
// the host verifier of either per-AIR proof (docs/airset.md's step numbers; without with_bus docs/zerocheck.md's statement)
// pq_out: the fraction sum's (P, Q), written whenever non-null: the callers pass null without with_bus (verify_batch tests with_bus itself)
int verify(const VerIn& in, uint32_t* root_out, uint32_t* pq_out) {
    const size_t n_airs = in.n_airs;
    const uint32_t* const* pvs = in.pvs;
    Shape S;
    if (!shape(in.prm, in.airs, n_airs, in.l, in.with_bus, &S, in.prep_root ? (int)in.l_prep : -1)) return ZKHIP_ERR_INVALID;
    HostChallenger ch;
    ZK_TRY(verify_start(ch, in, S, S.head, S.total));   // 1.
    const Ext one = ext_one();
    BusV V;
    const uint32_t* q = in.proof + 8;
    if (in.with_bus) {   // 2. - 5.
        ZK_TRY(verify_bus(ch, S, q, &V));
        q = V.qB + 4 * S.n_bus;
    }
    std::vector<uint32_t> points;                            // r'_a, canonical, end to end
    std::vector<const uint32_t*> claimed(n_airs, nullptr);   // the w values the opening must show (null: none claimed)
    std::vector<const uint32_t*> claimed_p(n_airs, nullptr); // keyed: the w_p values the key's opening must show
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        const unsigned m = pl.m;
        const size_t w = pl.w, n_rot = pl.rot.size(), wp = pl.wp, n_val = w + n_rot + wp + pl.rot_p.size();
        std::vector<Ext> rp(m);
        if (!pl.active()) {
            for (unsigned j = 0; j < m; j++) rp[j] = ch.sample_ext();
        } else {
            // 6. the (joint) sum-check: tau and alpha if it has proven constraints, the bus claim if it has bus roots (the zero-check's
            // plans have none)
            std::vector<Ext> tau(m), r(m), coef;
            Ext alpha = ext_zero(), claim = ext_zero();
            if (!pl.proven.empty()) {
                for (unsigned j = 0; j < m; j++) tau[j] = ch.sample_ext();
                alpha = ch.sample_ext();
            }
            if (!pl.bus_roots.empty()) claim = bus_claim(S, V, a, &coef);
            claim = rounds_host(ch, q, m, pl.D, claim, r.data());
            // 7. the values
            const uint32_t* qv = q;
            ch.observe_canon(qv, 4 * n_val);
            q += 4 * n_val;
            if (!ext_eq(air_summand(pl, qv, pvs[a], tau.data(), alpha, V.rho.data(), coef, r.data()), claim)) return ZKHIP_ERR_VERIFY;
            // 8. the rotation reduction
            if (!pl.reduces()) {
                rp = r, claimed[a] = qv, claimed_p[a] = wp ? qv + 4 * (w + n_rot) : nullptr;
            } else {
                const Ext lambda = ch.sample_ext();
                std::vector<Ext> lp;
                Ext x = one;
                claim = lambda_comb(qv, n_val, lambda, &x, &lp);
                claim = rounds_host(ch, q, m, 2, claim, rp.data());
                ch.observe_canon(q, 4 * (w + wp));
                claimed[a] = q, claimed_p[a] = wp ? q + 4 * w : nullptr;
                if (!ext_eq(u_term(pl, lp.data(), q, r.data(), rp.data()), claim)) return ZKHIP_ERR_VERIFY;
                q += 4 * (w + wp);
            }
        }
        for (unsigned j = 0; j < m; j++) {
            uint32_t c4[4];
            ext_to_canon(c4, rp[j]);
            points.insert(points.end(), c4, c4 + 4);
        }
    }
    // 9. the stacked opening, then the key's.  The key's opening takes S.prep_words words: once verify_start has passed the length
    // check that is the remaining length words - S.head - S.main_words.
    ZK_TRY(verify_openings(ch, in, S, S.head, points, claimed, claimed_p));
    if (root_out) memcpy(root_out, in.proof, 32);
    if (pq_out) memcpy(pq_out, in.proof + 8, 32);
    return ZKHIP_OK;
}

size_t proof_words(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, bool with_bus, int l_prep = -1) {
    Shape S;
    return shape(prm, airs, n_airs, l, with_bus, &S, l_prep) ? S.total : 0;
}

// ---- the batched proof (docs/airbatch.md) ---------------------------------------------------------------------------------------
// The statement of either proof above with ONE constraint sum-check and ONE rotation reduction for the set: every AIR's point is a
// prefix of the same r (r').  Steps 0 - 5 (plan, commit, the bus part) are the code above; the step numbers below are the document's.
struct BatchShape {
    Shape S;
    std::vector<size_t> act, red;   // the active AIRs, the reducing ones among them, caller order
    unsigned M = 0, D = 0, M2 = 0;  // the largest height and degree of an active AIR, the largest height of a reducing one
    bool any_cons = false;
    size_t o_rounds = 0, o_vals = 0, o_red = 0, o_u = 0, head = 0, total = 0;   // words; head: before the stacked opening
};
// l_prep >= 0: the keyed form (shape()'s pass-through); its values and u carry the preprocessed parts, and the key's opening follows
// l_cached: the cached form (shape()'s pass-through): the cached roots lead the proof, the partitions' openings end it
bool batch_shape(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, bool with_bus, BatchShape* T, int l_prep = -1,
                 const unsigned* l_cached = nullptr) {
    if (!shape(prm, airs, n_airs, l, with_bus, &T->S, l_prep, l_cached)) return false;
    size_t vals = 0, us = 0;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = T->S.plans[a];
        if (!pl.active()) continue;
        T->act.push_back(a);
        T->M = std::max(T->M, pl.m), T->D = std::max(T->D, pl.D), T->any_cons |= !pl.proven.empty();
        vals += 4 * (pl.w + pl.rot.size() + pl.wp + pl.rot_p.size());   // wp = 0 and rot_p empty in the unkeyed form
        if (pl.reduces()) T->red.push_back(a), T->M2 = std::max(T->M2, pl.m), us += 4 * (pl.w + pl.wp);
    }
    T->o_rounds = T->S.pre + 8 + (with_bus ? T->S.gkr_words + 4 * T->S.n_bus : 0);
    T->o_vals = T->o_rounds + 4 * (size_t)T->D * T->M;
    T->o_red = T->o_vals + vals;
    T->o_u = T->o_red + (T->red.empty() ? 0 : 8 * (size_t)T->M2);
    T->head = T->o_u + us;
    T->total = T->head + (T->S.total - T->S.head);   // the main opening (keyed: then the key's; cached: then the partitions')
    return true;
}

// ---- the batched device prover: one upload, one workspace, launches that do not grow with the number of AIRs --------------------
// One job (an active AIR): its lowered program and its footprint in the workspace.  batch_plan() places every piece at the running
// total and moves the total on: each size is written there once, so the workspace's size and the pieces' places cannot disagree.
struct ZbSlot {
    size_t a = 0;
    CompiledAir ca;                // roots: the proven constraints, then (with_bus) the bus roots
    bool has_bus = false;
    size_t up_at = 0;              // in the upload: [code | the extension passes' copy | consts | pvs | rot | rot_p], padded to 4 words
    size_t partial = 0, tA = 0, tB = 0;   // among the tables (words from o_tabs): 4 D SC_NB; nt tables of n / 2; nt of max(n / 4, 1)
    size_t red = 0;                // a reducing AIR: [F_a (4 n) | F_b (4 n) | partial (8 SC_NB)], after its tables
    uint32_t first_wg = 0, n_wg = 0;      // its workgroups, counted from its class's first job
};
struct ZbCls {   // a (D, BUS, PREP) class: a run of the job table, tallest first
    size_t lo, n;
    unsigned D, slots;
    bool bus, prep;
};
struct BatchPlan {
    std::vector<ZbSlot> slots;   // class order
    std::vector<ZbCls> classes;
    std::map<unsigned, size_t> eq_at;   // height of an AIR with proven constraints -> its eq table (words from d_ws)
    size_t n_cons_max = 1, n_cst = 0, n_ucols = 0, red_vals = 0, inact_words = 0;
    // the workspace (words from d_ws): [upload: the jobs' slices | lagx | lagw | ZbJob, ZbCst, ZbRot, ZbCol tables] [tau, alpha, mu,
    // lambda | alpha powers | lambda powers | weights | claims | states | eq tables | the jobs' tables]
    size_t o_lagx = 0, o_lagw = 0, o_job = 0, o_cst = 0, o_rot = 0, o_col = 0, up_total = 0;
    size_t o_chal = 0, o_apow = 0, o_lpow = 0, o_wgt = 0, o_claim = 0, o_state = 0, o_tabs = 0, ws_words = 0;
    // read back at once (words from dP): [the words before the opening | r (4 M) | r' (4 M') | the inactive AIRs' points]
    size_t o_r = 0, o_rp = 0, o_inact = 0, back_words = 0;
};
size_t pad4(size_t x) { return (x + 3) & ~(size_t)3; }
// the plan: the classes, the lowered programs, the layout
int batch_plan(zkhip_ctx* ctx, const std::string& who, const BatchShape& T, bool with_bus, BatchPlan* Q) {
    const Shape& S = T.S;
    const size_t n_jobs = T.act.size(), n_red = T.red.size();
    std::vector<size_t> order(T.act);
    auto cls = [&](size_t a) { return 4 * S.plans[a].D + (with_bus && !S.plans[a].prog.ints.empty() ? 2u : 0u) + (S.plans[a].wp ? 1u : 0u); };
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cls(x) != cls(y) ? cls(x) < cls(y) : S.plans[x].m > S.plans[y].m; });
    Q->slots.resize(n_jobs);
    size_t up_words = 0, tab_words = 0;
    auto take = [](size_t& at, size_t n) { return (at += n) - n; };   // n words at the running total
    uint64_t wg = 0;
    for (size_t k = 0; k < n_jobs; k++) {
        ZbSlot& J = Q->slots[k];
        const ZcPlan& pl = S.plans[J.a = order[k]];
        J.has_bus = with_bus && !pl.prog.ints.empty();
        std::vector<uint32_t> roots = pl.proven;
        if (with_bus) roots.insert(roots.end(), pl.bus_roots.begin(), pl.bus_roots.end());
        std::string err;
        if (compile_air(pl.prog, &J.ca, &err, &roots) != 0 || J.ca.n_slots > ZC_MAX_SLOTS)
            return set_error(ctx, ZKHIP_ERR_INVALID, who + (err.empty() ? "an AIR needs more than 64 live intermediates" : err));
        if (Q->classes.empty() || cls(order[Q->classes.back().lo]) != cls(J.a)) Q->classes.push_back({k, 0, pl.D, 1, J.has_bus, pl.wp != 0}), wg = 0;
        Q->classes.back().n++, Q->classes.back().slots = std::max(Q->classes.back().slots, J.ca.n_slots);
        const size_t n = (size_t)1 << pl.m, n_val = pl.w + pl.rot.size() + pl.wp + pl.rot_p.size();   // wp = 0, rot_p empty without a key
        const size_t nt = n_val + (J.has_bus ? 4 : 3);
        J.first_wg = (uint32_t)wg, J.n_wg = grid_w(n / 2), wg += J.n_wg;
        J.up_at = take(up_words, pad4(2 * J.ca.code.size() + J.ca.consts.size() + pl.prog.n_pvs + pl.rot.size() + pl.rot_p.size()));
        J.partial = take(tab_words, 4 * (size_t)pl.D * SC_NB);
        J.tA = take(tab_words, 4 * nt * (n / 2));
        J.tB = take(tab_words, 4 * nt * std::max<size_t>(n / 4, 1));
        if (pl.reduces()) J.red = take(tab_words, 8 * n + 8 * SC_NB), Q->n_ucols += pl.w + pl.wp, Q->red_vals += n_val;
        Q->n_cons_max = std::max(Q->n_cons_max, pl.proven.size());
        if (J.has_bus) Q->n_cst += pl.prog.ints.size();
    }
    size_t at = up_words;   // the rest of the upload, then what the device alone writes
    Q->o_lagx = take(at, pad4(ZB_PTS * ZB_PTS * ZB_PTS)), Q->o_lagw = take(at, pad4(ZB_PTS));
    Q->o_job = take(at, pad4(n_jobs * sizeof(ZbJob) / 4 + 1)), Q->o_cst = take(at, pad4(Q->n_cst * sizeof(ZbCst) / 4 + 1));
    Q->o_rot = take(at, pad4(n_red * sizeof(ZbRot) / 4 + 1)), Q->o_col = take(at, pad4(Q->n_ucols * sizeof(ZbCol) / 4 + 1));
    Q->up_total = at;
    Q->o_chal = take(at, 4 * (size_t)T.M + 12), Q->o_apow = take(at, 4 * Q->n_cons_max), Q->o_lpow = take(at, 4 * std::max<size_t>(Q->red_vals, 1));
    Q->o_wgt = take(at, 4 * std::max<size_t>(n_jobs, 1)), Q->o_claim = take(at, 4 * std::max<size_t>(n_jobs, 1));
    Q->o_state = take(at, 4 * std::max<size_t>(n_red, 1));
    for (size_t a : T.act)
        if (!S.plans[a].proven.empty() && !Q->eq_at.count(S.plans[a].m)) Q->eq_at[S.plans[a].m] = take(at, 4 * ((size_t)1 << S.plans[a].m));
    Q->o_tabs = at, Q->ws_words = at + tab_words;
    at = T.head;   // the read-back
    Q->o_r = take(at, 4 * (size_t)T.M), Q->o_rp = take(at, 4 * (size_t)T.M2), Q->o_inact = at;
    for (const ZcPlan& pl : S.plans)
        if (!pl.active()) at += 4 * (size_t)pl.m;
    Q->inact_words = at - Q->o_inact, Q->back_words = at;
    return ZKHIP_OK;
}
// s(t), t > d, from s(0..d) at lagx; and 1 / prod_{i != t} (t - i) over 0..D at lagw
void zb_lagrange(uint32_t* lagx, uint32_t* lagw, unsigned D) {
    auto small = [](unsigned x) { return to_monty(x); };
    for (unsigned d = 1; d < ZB_PTS; d++)
        for (unsigned t = d + 1; t < ZB_PTS; t++)
            for (unsigned j = 0; j <= d; j++) {
                uint32_t num = MONTY_ONE, den = MONTY_ONE;
                for (unsigned i = 0; i <= d; i++)
                    if (i != j) num = mmul(num, msub(small(t), small(i))), den = mmul(den, msub(small(j), small(i)));
                lagx[(d * ZB_PTS + t) * ZB_PTS + j] = mmul(num, minv(den));
            }
    for (unsigned t = 0; t <= D; t++) {
        uint32_t den = MONTY_ONE;
        for (unsigned i = 0; i <= D; i++)
            if (i != t) den = mmul(den, msub(small(t), small(i)));
        lagw[t] = minv(den);
    }
}
// the one upload: programs, constants, public values, rotation lists, the interpolation weights, the job tables; jobs: the host's
// copy of the job table, class order (the round loop reads heights and grids from it)
void batch_fill(const ProveIn& in, const BatchShape& T, const BatchPlan& Q, const std::vector<ZcBus>& bus, uint32_t* d_ws, std::vector<uint32_t>* up,
                std::vector<ZbJob>* jobs) {
    const Shape& S = T.S;
    const uint32_t *const *d_traces = in.d_traces, *const *pvs = in.pvs;
    const zkhip_airkey* key = in.key;
    const size_t n_airs = S.plans.size(), n_jobs = Q.slots.size();
    up->assign(Q.up_total, 0);
    jobs->assign(n_jobs, ZbJob{});
    std::vector<ZbCst> cst;
    std::vector<ZbRot> rots(T.red.size());
    std::vector<ZbCol> ucols;
    std::vector<size_t> val_at(n_airs, 0), u_at(n_airs, 0), lam_at(n_airs, 0);   // caller order: the proof's value and u sections, the lambda powers
    size_t v = 0, u = 0, o = 0;
    for (size_t a : T.act) {
        const ZcPlan& pl = S.plans[a];
        const size_t n_val = pl.w + pl.rot.size() + pl.wp + pl.rot_p.size();
        val_at[a] = v, v += 4 * n_val;
        if (pl.reduces()) u_at[a] = u, u += 4 * (pl.w + pl.wp), lam_at[a] = o, o += n_val;
    }
    auto eq_of = [&](unsigned m) { return d_ws + Q.eq_at.at(m); };   // of an AIR with proven constraints: batch_plan gave its height a table
    uint32_t* tabs = d_ws + Q.o_tabs;
    for (size_t k = 0; k < n_jobs; k++) {
        const ZbSlot& J = Q.slots[k];
        const size_t a = J.a;
        const ZcPlan& pl = S.plans[a];
        const unsigned w = (unsigned)pl.w, n_rot = (unsigned)pl.rot.size(), wp = (unsigned)pl.wp, n_rot_p = (unsigned)pl.rot_p.size();
        const size_t n_code = J.ca.code.size(), n_ins = n_code / 3, n = (size_t)1 << pl.m;
        uint32_t* h = up->data() + J.up_at;
        std::copy(J.ca.code.begin(), J.ca.code.end(), h);
        for (size_t i = 0; i < n_ins; i++) {   // the extension passes' copy names tables in its VAR operands (zc_prove_air's remap)
            uint32_t* x = h + n_code + 3 * i;
            x[0] = J.ca.code[3 * i];
            for (int q = 1; q < 3; q++) {
                const uint32_t op = J.ca.code[3 * i + q];
                x[q] = (op >> 28) != K_VAR ? op : (K_VAR << 28) | (((op >> 27) & 1u) ? w + (uint32_t)pl.rot_of[op & 0x07ffffffu] : (op & 0x07ffffffu));
                if (wp && (op >> 28) == K_PREP)   // the preprocessed tables follow the main ones
                    x[q] = (K_VAR << 28) | (w + n_rot + (((op >> 27) & 1u) ? wp + (uint32_t)pl.rot_p_of[op & 0x07ffffffu] : (op & 0x07ffffffu)));
            }
        }
        uint32_t* hp = h + 2 * n_code;
        hp = std::copy(J.ca.consts.begin(), J.ca.consts.end(), hp);
        for (uint32_t i = 0; i < pl.prog.n_pvs; i++) *hp++ = to_monty(pvs[a][i]);
        hp = std::copy(pl.rot.begin(), pl.rot.end(), hp);
        std::copy(pl.rot_p.begin(), pl.rot_p.end(), hp);
        const uint32_t* d = d_ws + J.up_at;
        ZbJob& jb = (*jobs)[k];
        jb.pg = ZcProg{d, (unsigned)n_ins, d + 2 * n_code, d + 2 * n_code + J.ca.consts.size(), d_ws + Q.o_apow, bus[a].coef, (unsigned)pl.proven.size()};
        jb.xcode = d + n_code, jb.trace = d_traces[a], jb.rot = d + 2 * n_code + J.ca.consts.size() + pl.prog.n_pvs;
        if (wp) jb.pp = ZcPrep{key->d_prep + key->prep_at[a], jb.rot + n_rot, wp, n_rot_p};   // the key's columns of this AIR
        jb.E2 = bus[a].E2, jb.E = pl.proven.empty() ? bus[a].E2 : eq_of(pl.m);
        jb.partial = tabs + J.partial, jb.tA = tabs + J.tA, jb.tB = tabs + J.tB;
        jb.m = pl.m, jb.w = w, jb.n_rot = n_rot, jb.D = pl.D;
        jb.j = (uint32_t)(std::find(T.act.begin(), T.act.end(), a) - T.act.begin());
        jb.first_wg = J.first_wg, jb.n_wg = J.n_wg;
        jb.val_at = (uint32_t)val_at[a];
        if (J.has_bus) {
            jb.cst_at = (uint32_t)cst.size(), jb.cst_n = (uint32_t)pl.prog.ints.size(), jb.b_at = (uint32_t)S.b_at[a];
            uint32_t root_at = 0;   // pl.bus_roots: per interaction its count, then its fields
            for (const Interaction& it : pl.prog.ints) cst.push_back({root_at, to_monty(it.bus + 1), it.sign}), root_at += 1 + it.n_fields;
        }
        if (pl.reduces()) {
            ZbRot& rj = rots[std::find(T.red.begin(), T.red.end(), a) - T.red.begin()];
            rj = ZbRot{};
            rj.trace = d_traces[a], rj.rot = jb.rot, rj.lpow = d_ws + Q.o_lpow + 4 * lam_at[a], rj.E = eq_of(pl.m);
            rj.fa = tabs + J.red, rj.fb = rj.fa + 4 * n, rj.partial = rj.fb + 4 * n;   // ZbSlot::red's layout
            rj.tA = jb.tA, rj.tB = jb.tB, rj.m = pl.m, rj.w = w, rj.n_rot = n_rot, rj.pp = jb.pp;
            rj.wgt = mpow(to_monty(2), T.M2 - pl.m), rj.u_at = (uint32_t)u_at[a];
        }
    }
    for (size_t a : T.red) {   // u, then u_p from the key's columns
        const ZcPlan& pl = S.plans[a];
        for (size_t c = 0; c < pl.w; c++) ucols.push_back({d_traces[a] + (c << pl.m), eq_of(pl.m), pl.m, (uint32_t)(u_at[a] + 4 * c)});
        for (size_t c = 0; c < pl.wp; c++)
            ucols.push_back({key->d_prep + key->prep_at[a] + (c << pl.m), eq_of(pl.m), pl.m, (uint32_t)(u_at[a] + 4 * (pl.w + c))});
    }
    zb_lagrange(up->data() + Q.o_lagx, up->data() + Q.o_lagw, T.D);
    if (n_jobs) memcpy(up->data() + Q.o_job, jobs->data(), n_jobs * sizeof(ZbJob));
    if (!cst.empty()) memcpy(up->data() + Q.o_cst, cst.data(), cst.size() * sizeof(ZbCst));
    if (!rots.empty()) memcpy(up->data() + Q.o_rot, rots.data(), rots.size() * sizeof(ZbRot));
    if (!ucols.empty()) memcpy(up->data() + Q.o_col, ucols.data(), ucols.size() * sizeof(ZbCol));
}
// 6. the batched sum-check: tau and alpha (if some AIR has proven constraints), then mu; M rounds and the tallest AIRs' last fold
// 7. the values of every active AIR at its prefix of r
// chal: prove_bus's [gamma | beta | kappa] (null without with_bus)
int batch_rounds(const ProveIn& in, const BatchShape& T, const BatchPlan& Q, const std::vector<ZbJob>& jobs, uint32_t* d_ws, uint32_t* dP,
                 const uint32_t* chal) {
    zkhip_ctx* ctx = in.ctx;
    DevTranscript* d_t = in.d_t;
    hipStream_t st = ctx->stream;
    const unsigned M = T.M;
    const size_t n_jobs = jobs.size();
    uint32_t *tau = d_ws + Q.o_chal, *alpha = tau + 4 * M, *mu = alpha + 4, *d_r = dP + Q.o_r;
    const ZbJob* d_jobs = (const ZbJob*)(d_ws + Q.o_job);
    if (T.any_cons) ZK_TRY(transcript_sample(ctx, d_t, tau, nullptr, 4 * M + 8));
    else ZK_TRY(transcript_sample(ctx, d_t, mu, nullptr, 4));
    for (auto& e : Q.eq_at) {
        KernelScope ks(ctx, "zb_eq");
        whir_eq_launch(st, d_ws + e.second, e.first, tau);
    }
    if (T.any_cons) {
        KernelScope ks(ctx, "zb_pows");
        hipLaunchKernelGGL(k_zc_pows, dim3(1), dim3(256), 0, st, (const uint32_t*)alpha, (unsigned)Q.n_cons_max, d_ws + Q.o_apow);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ZbTr ztr{};
    ztr.mu = mu, ztr.lagx = d_ws + Q.o_lagx, ztr.lagw = d_ws + Q.o_lagw, ztr.cst = (const ZbCst*)(d_ws + Q.o_cst), ztr.chal = chal;
    ztr.dB = dP + T.S.pre + 8 + T.S.gkr_words, ztr.wgt = d_ws + Q.o_wgt, ztr.claim = d_ws + Q.o_claim, ztr.proof = dP + T.o_rounds, ztr.r = d_r;
    for (unsigned i = 0; i <= M; i++) {   // round i; i = M: the tallest AIRs' last fold only
        for (const ZbCls& c : Q.classes) {
            size_t alive = 0;   // the class's jobs are sorted tallest first: the ones with m >= i are a prefix
            while (alive < c.n && jobs[c.lo + alive].m >= i) alive++;
            if (!alive) continue;
            const ZbJob& last = jobs[c.lo + alive - 1];
            KernelScope ks(ctx, i ? "zb_pass" : "zb_round0");
            zb_launch(c.D, c.bus, c.prep, st, last.first_wg + last.n_wg, (size_t)c.slots * ZC_W * (i ? 16 : 4), d_jobs + c.lo, (uint32_t)alive, i,
                      i ? d_r + 4 * (i - 1) : nullptr);
        }
        if (i < M) {
            KernelScope ks(ctx, "zb_round_tr");
            hipLaunchKernelGGL(k_zb_round_tr, dim3(1), dim3(ZB_TR), 0, st, d_t, d_jobs, (unsigned)n_jobs, i, M, T.D, ztr);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    if (n_jobs) {
        {
            KernelScope ks(ctx, "zb_emit");
            hipLaunchKernelGGL(k_zb_emit, dim3((unsigned)n_jobs), dim3(64), 0, st, d_jobs, dP + T.o_vals);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
        ZK_TRY(transcript_observe(ctx, d_t, dP + T.o_vals, (uint32_t)(T.o_red - T.o_vals), true));
    }
    return ZKHIP_OK;
}
// 8. the batched rotation reduction (some AIR reduces); the keyed form's combine reads the key's columns too
int batch_reduce(const ProveIn& in, const BatchShape& T, const BatchPlan& Q, uint32_t* d_ws, uint32_t* dP) {
    zkhip_ctx* ctx = in.ctx;
    DevTranscript* d_t = in.d_t;
    hipStream_t st = ctx->stream;
    const unsigned M2 = T.M2, n_red = (unsigned)T.red.size();
    uint32_t *lambda = d_ws + Q.o_chal + 4 * T.M + 8, *d_r = dP + Q.o_r, *d_rp = dP + Q.o_rp;
    const ZbRot* d_rots = (const ZbRot*)(d_ws + Q.o_rot);
    // the reducing AIRs' distinct heights -> their eq tables: zc_plan takes rot and rot_p from the proven constraints, so a reducing
    // AIR has some and batch_plan gave its height a table
    std::map<unsigned, size_t> heights;
    for (size_t a : T.red) heights[T.S.plans[a].m] = Q.eq_at.at(T.S.plans[a].m);
    ZK_TRY(transcript_sample(ctx, d_t, lambda, nullptr, 4));
    {
        KernelScope ks(ctx, "zb_pows");
        hipLaunchKernelGGL(k_zc_pows, dim3(1), dim3(256), 0, st, (const uint32_t*)lambda, (unsigned)Q.red_vals, d_ws + Q.o_lpow);
    }
    for (auto& e : heights) {
        KernelScope ks(ctx, "zb_eq");
        whir_eq_launch(st, d_ws + e.second, e.first, d_r);
    }
    {
        KernelScope ks(ctx, "zb_combine");
        if (in.key) hipLaunchKernelGGL(k_zb_combine_p, dim3(grid_of((size_t)1 << M2), n_red), dim3(256), 0, st, d_rots);
        else hipLaunchKernelGGL(k_zb_combine, dim3(grid_of((size_t)1 << M2), n_red), dim3(256), 0, st, d_rots);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    const ZbRotTr rtr{d_ws + Q.o_state, dP + T.o_red, d_rp};
    for (unsigned t = 0; t < M2; t++) {
        {
            KernelScope ks(ctx, "zb_rot_pass");
            hipLaunchKernelGGL(k_zb_rot_pass, dim3(grid_of(((size_t)1 << (M2 - t)) >> 1), n_red), dim3(256), 0, st, d_rots, t,
                               t ? (const uint32_t*)(d_rp + 4 * (t - 1)) : nullptr);
        }
        {
            KernelScope ks(ctx, "zb_round_tr");
            hipLaunchKernelGGL(k_zb_rot_tr, dim3(1), dim3(ZB_TR), 0, st, d_t, d_rots, n_red, t, rtr);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    for (auto& e : heights) {
        KernelScope ks(ctx, "zb_eq");
        whir_eq_launch(st, d_ws + e.second, e.first, d_rp);
    }
    {
        KernelScope ks(ctx, "zb_dot");
        hipLaunchKernelGGL(k_zb_dot, dim3((unsigned)Q.n_ucols), dim3(256), 0, st, (const ZbCol*)(d_ws + Q.o_col), dP + T.o_u);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return transcript_observe(ctx, d_t, dP + T.o_u, (uint32_t)(T.head - T.o_u), true);
}
// the batched proof (docs/airbatch.md's step numbers); in.cached: per AIR, null where the AIR has no CACHED section
int prove_batch(const ProveIn& in) {
    zkhip_ctx* ctx = in.ctx;
    const size_t n_airs = in.n_airs;
    const std::string who = in.cached ? "airkey cached: " : in.key ? "airkey batch: " : "airbatch: ";
    BatchShape T;
    std::vector<unsigned> l_cached;
    for (size_t a = 0; in.cached && a < n_airs; a++) l_cached.push_back(in.cached[a] ? in.cached[a]->l : 0);
    if (!batch_shape(in.prm, in.airs, n_airs, in.l, in.with_bus, &T, in.key ? (int)in.key->l_prep : -1, in.cached ? l_cached.data() : nullptr))
        return set_error(ctx, ZKHIP_ERR_INVALID, who + "the shape does not fit the limits");
    const Shape& S = T.S;
    for (size_t a : S.cached_airs) {
        const zkhip_cached_main* c = in.cached[a];
        if (!c || !c->sc || c->air != a || c->m != S.plans[a].m || c->cw != S.cw[a] || memcmp(&c->params, in.prm, sizeof(*in.prm)) != 0)
            return set_error(ctx, ZKHIP_ERR_INVALID, who + "a cached partition's handle is null or was made for another AIR, height or width");
    }
    if (in.cap < T.total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, who + "proof buffer too small");
    size_t n_pv = 0;
    ZK_TRY(check_inputs(in, who, &n_pv));
    BatchPlan Q;
    ZK_TRY(batch_plan(ctx, who, T, in.with_bus, &Q));
    MainCom com{ctx};
    ZK_TRY(commit_main(in, S, &com));   // 1.
    DevBufs B(ctx);
    uint32_t *dP = B.get(Q.back_words), *d_obs = B.get(obs_words(in, S, n_pv)), *d_ws = B.get(Q.ws_words);
    if (!dP || !d_obs || !d_ws) return set_error(ctx, ZKHIP_ERR_NOMEM, who + "the workspace does not fit");
    ZK_TRY(observe_start(in, S, d_obs, com.root));
    // 2. - 5. the bus part
    std::vector<ZcBus> bus(n_airs);
    const uint32_t* chal = nullptr;
    if (in.with_bus) ZK_TRY(prove_bus(ctx, S, in.airs, n_airs, in.d_traces, in.pvs, in.d_t, B, dP + S.pre, &bus, in.key, &chal));
    std::vector<uint32_t> up;
    std::vector<ZbJob> jobs;
    batch_fill(in, T, Q, bus, d_ws, &up, &jobs);
    ZK_TRY(zkhip_h2d(ctx, d_ws, up.data(), up.size() * 4));
    ZK_TRY(batch_rounds(in, T, Q, jobs, d_ws, dP, chal));               // 6., 7.
    if (!T.red.empty()) ZK_TRY(batch_reduce(in, T, Q, d_ws, dP));       // 8.
    // 9. the points: an inactive AIR samples its own, all of them in one launch; then the one read-back
    if (Q.inact_words) ZK_TRY(transcript_sample(ctx, in.d_t, dP + Q.o_inact, nullptr, (uint32_t)Q.inact_words));
    std::vector<uint32_t> h(Q.back_words);
    ZK_TRY(zkhip_d2h(ctx, h.data(), dP, h.size() * 4));
    for (size_t i = T.head; i < h.size(); i++) h[i] = from_monty(h[i]);
    std::vector<size_t> pt_at(n_airs);   // AIR -> its point in h: its own if inactive, else its prefix of r' if it reduces, of r if not
    size_t in_at = Q.o_inact;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        pt_at[a] = !pl.active() ? in_at : pl.reduces() ? Q.o_rp : Q.o_r;
        if (!pl.active()) in_at += 4 * (size_t)pl.m;
    }
    // 10. the openings
    return open_and_finish(in, S, com, h, pt_at, T.head);
}
// the host verifier of the batched proof
// pq_out: written under with_bus only: these entry points hand the caller's pointer through in either form (verify()'s callers
// pass null without with_bus instead)
int verify_batch(const VerIn& in, uint32_t* root_out, uint32_t* pq_out, uint32_t* cached_roots_out = nullptr) {
    const size_t n_airs = in.n_airs;
    const uint32_t *const *pvs = in.pvs, *proof = in.proof;
    BatchShape T;
    if (!batch_shape(in.prm, in.airs, n_airs, in.l, in.with_bus, &T, in.prep_root ? (int)in.l_prep : -1, in.l_cached)) return ZKHIP_ERR_INVALID;
    const Shape& S = T.S;
    const uint32_t* root = proof + S.pre;   // the cached form: the partitions' roots are sent before the main root
    HostChallenger ch;
    ZK_TRY(verify_start(ch, in, S, T.head, T.total));   // 1.
    const Ext one = ext_one();
    BusV V;
    if (in.with_bus) ZK_TRY(verify_bus(ch, S, root + 8, &V));   // 2. - 5.
    // 6. the batched sum-check: the claim is sum_j mu^j 2^(M - m_a) (AIR a's bus claim), j over the active AIRs
    const unsigned M = T.M, M2 = T.M2;
    std::vector<Ext> tau(M), r(M), rp(M2);
    Ext alpha = ext_zero();
    if (T.any_cons) {
        for (unsigned j = 0; j < M; j++) tau[j] = ch.sample_ext();
        alpha = ch.sample_ext();
    }
    const Ext mu = ch.sample_ext();
    const Ext two = ext_from_base(to_monty(2));
    std::vector<std::vector<Ext>> coef(n_airs);   // per AIR with interactions: the coefficients of pl.bus_roots
    Ext claim = ext_zero(), mup = one;
    for (size_t a : T.act) {
        const ZcPlan& pl = S.plans[a];
        if (!pl.bus_roots.empty()) claim = ext_add(claim, ext_mul(ext_mul(mup, ext_pow(two, M - pl.m)), bus_claim(S, V, a, &coef[a])));
        mup = ext_mul(mup, mu);
    }
    const uint32_t* q = proof + T.o_rounds;
    claim = rounds_host(ch, q, M, T.D, claim, r.data());
    // 7. the values: sum_j mu^j (AIR a's summand at its prefix of r) = the last claim
    ch.observe_canon(q, T.o_red - T.o_vals);
    std::vector<const uint32_t*> vals(n_airs, nullptr);
    Ext rhs = ext_zero();
    mup = one;
    for (size_t a : T.act) {
        const ZcPlan& pl = S.plans[a];
        vals[a] = q, q += 4 * (pl.w + pl.rot.size() + pl.wp + pl.rot_p.size());
        rhs = ext_add(rhs, ext_mul(mup, air_summand(pl, vals[a], pvs[a], tau.data(), alpha, V.rho.data(), coef[a], r.data())));
        mup = ext_mul(mup, mu);
    }
    if (!ext_eq(rhs, claim)) return ZKHIP_ERR_VERIFY;
    // 8. the batched rotation reduction: one lambda, its powers running through the reducing AIRs' values, weights 2^(M' - m_a)
    std::vector<const uint32_t*> claimed(n_airs, nullptr), claimed_p(n_airs, nullptr);   // as in verify()
    if (!T.red.empty()) {
        const Ext lambda = ch.sample_ext();
        std::vector<std::vector<Ext>> lp(n_airs);
        Ext x = one;
        claim = ext_zero();
        for (size_t a : T.red) {
            const ZcPlan& pl = S.plans[a];
            const Ext acc = lambda_comb(vals[a], pl.w + pl.rot.size() + pl.wp + pl.rot_p.size(), lambda, &x, &lp[a]);
            claim = ext_add(claim, ext_mul(ext_pow(two, M2 - pl.m), acc));
        }
        claim = rounds_host(ch, q, M2, 2, claim, rp.data());
        ch.observe_canon(q, T.head - T.o_u);
        Ext want = ext_zero();
        for (size_t a : T.red) {
            const ZcPlan& pl = S.plans[a];
            want = ext_add(want, u_term(pl, lp[a].data(), q, r.data(), rp.data()));
            claimed[a] = q, claimed_p[a] = pl.wp ? q + 4 * pl.w : nullptr, q += 4 * (pl.w + pl.wp);
        }
        if (!ext_eq(want, claim)) return ZKHIP_ERR_VERIFY;
    }
    // 9. the points: an inactive AIR samples its own; the others take their prefix of r' if they reduce, of r if not
    std::vector<uint32_t> points;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        if (pl.active() && !pl.reduces()) claimed[a] = vals[a], claimed_p[a] = pl.wp ? vals[a] + 4 * (pl.w + pl.rot.size()) : nullptr;
        for (unsigned j = 0; j < pl.m; j++) {
            uint32_t c4[4];
            ext_to_canon(c4, !pl.active() ? ch.sample_ext() : pl.reduces() ? rp[j] : r[j]);
            points.insert(points.end(), c4, c4 + 4);
        }
    }
    // 10. the openings: main, the key's, the partitions'
    ZK_TRY(verify_openings(ch, in, S, T.head, points, claimed, claimed_p));
    if (cached_roots_out) memcpy(cached_roots_out, proof, 4 * S.pre);
    if (root_out) memcpy(root_out, root, 32);
    if (pq_out && in.with_bus) memcpy(pq_out, root + 8, 32);
    return ZKHIP_OK;
}

// ---- the key ---------------------------------------------------------------------------------------------------------------------
void airkey_destroy(zkhip_ctx* ctx, zkhip_airkey* key) {
    if (!key) return;
    stack_destroy(ctx, key->sc);   // synchronises
    if (key->d_prep) (void)hipFree(key->d_prep);
    delete key;
}

// reads zkhip_air::prep_trace (host, canonical, column-major), as zkhip_keygen does; the columns stay on the device in Montgomery form
int airkey_create(zkhip_ctx* ctx, const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l_prep, zkhip_airkey** out,
                  uint32_t* root_out) {
    if (n_airs < 1 || n_airs > ZKHIP_STACK_MAX_POINTS) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: AIR count");
    zkhip_airkey* key = new zkhip_airkey();
    struct Guard {
        zkhip_ctx* ctx;
        zkhip_airkey* key;
        ~Guard() { airkey_destroy(ctx, key); }
    } guard{ctx, key};
    key->params = *prm, key->l_prep = l_prep;
    key->programs.resize(n_airs), key->airs.resize(n_airs), key->prep_at.assign(n_airs, 0);
    std::vector<unsigned> lh;
    std::vector<uint32_t> host;   // Montgomery
    for (size_t a = 0; a < n_airs; a++) {
        ZcPlan pl;   // the zero-check's plan: a set the bus form alone refuses (D, no interaction) is refused by the prove call
        if (!zc_plan(airs[a], &pl, false, true)) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: the shape does not fit the limits");
        key->programs[a].assign(airs[a].program, airs[a].program + airs[a].program_len);
        key->airs[a] = airs[a];
        key->airs[a].program = key->programs[a].data(), key->airs[a].prep_trace = nullptr, key->airs[a].prep_commit = nullptr;
        key->prep_at[a] = host.size();
        if (!pl.wp) continue;
        if (!airs[a].prep_trace) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: a PREP AIR without a preprocessed trace");
        const size_t cnt = pl.wp << pl.m;
        for (size_t i = 0; i < cnt; i++) {
            if (airs[a].prep_trace[i] >= P) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: preprocessed word not canonical");
            host.push_back(to_monty(airs[a].prep_trace[i]));
        }
        lh.insert(lh.end(), pl.wp, pl.m);
    }
    if (lh.empty()) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: no AIR has a PREP section: use the unkeyed calls");
    if (!zkhip_stack_width(prm, lh.data(), lh.size(), l_prep)) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey: the preprocessed columns do not fit log_stack_prep");
    if (hipMalloc(&key->d_prep, host.size() * 4) != hipSuccess) return set_error(ctx, ZKHIP_ERR_NOMEM, "airkey: the preprocessed columns do not fit");
    ZK_TRY(zkhip_h2d(ctx, key->d_prep, host.data(), host.size() * 4));
    std::vector<const uint32_t*> cols;
    for (size_t a = 0, j = 0; a < n_airs; a++) {
        ZcPlan pl;
        (void)zc_plan(key->airs[a], &pl, false, true);
        for (size_t c = 0; c < pl.wp; c++, j++) cols.push_back(key->d_prep + key->prep_at[a] + (c << pl.m));
    }
    ZK_TRY(stack_commit(ctx, prm, cols.data(), lh.data(), cols.size(), l_prep, &key->sc, key->root));   // synchronises
    if (root_out) memcpy(root_out, key->root, 32);
    guard.key = nullptr;
    *out = key;
    return ZKHIP_OK;
}

void cached_main_destroy(zkhip_ctx* ctx, zkhip_cached_main* c) {
    if (!c) return;
    stack_destroy(ctx, c->sc);   // synchronises
    delete c;
}

// the first cached_width columns of the key's AIR `air` as ONE stacked commitment at l_cached; stack_commit gathers a copy it owns
int commit_cached(zkhip_ctx* ctx, const zkhip_airkey* key, size_t air, const uint32_t* d_cols, unsigned l_cached, zkhip_cached_main** out,
                  uint32_t* root_out) {
    if (air >= key->airs.size()) return set_error(ctx, ZKHIP_ERR_INVALID, "airkey cached: AIR index");
    ZcPlan pl;
    if (!zc_plan(key->airs[air], &pl, false, true) || !pl.prog.cached_width)
        return set_error(ctx, ZKHIP_ERR_INVALID, "airkey cached: the AIR has no CACHED section");
    zkhip_cached_main* c = new zkhip_cached_main();
    c->params = key->params, c->air = air, c->m = pl.m, c->cw = (unsigned)pl.prog.cached_width, c->l = l_cached;
    std::vector<const uint32_t*> cols;
    for (size_t k = 0; k < c->cw; k++) cols.push_back(d_cols + (k << pl.m));
    const std::vector<unsigned> lh(c->cw, pl.m);
    const int rc = stack_commit(ctx, &key->params, cols.data(), lh.data(), cols.size(), l_cached, &c->sc, c->root);   // synchronises
    if (rc != ZKHIP_OK) {
        cached_main_destroy(ctx, c);
        return rc;
    }
    if (root_out) memcpy(root_out, c->root, 32);
    *out = c;
    return ZKHIP_OK;
}
}  // namespace

}  // namespace zk

using namespace zk;

extern "C" {

size_t zkhip_zerocheck_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack) {
    return proof_words(params, airs, n_airs, log_stack, false);
}

size_t zkhip_airset_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack) {
    return proof_words(params, airs, n_airs, log_stack, true);
}

int zkhip_zerocheck_prove(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
                          const uint32_t* const* pvs, unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap,
                          uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove({ctx, params, airs, n_airs, d_traces, pvs, log_stack, false, transcript->d, proof_out, cap, root_out});
}

int zkhip_airset_prove(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
                       const uint32_t* const* pvs, unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap,
                       uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove({ctx, params, airs, n_airs, d_traces, pvs, log_stack, true, transcript->d, proof_out, cap, root_out});
}

int zkhip_airkey_create(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack_prep,
                        zkhip_airkey** key_out, uint32_t* prep_root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !key_out) return ZKHIP_ERR_INVALID;
    return airkey_create(ctx, params, airs, n_airs, log_stack_prep, key_out, prep_root_out);
}

void zkhip_airkey_destroy(zkhip_ctx* ctx, zkhip_airkey* key) {
    ZK_BIND_DEVICE(ctx);
    airkey_destroy(ctx, key);
}

size_t zkhip_airkey_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack, unsigned log_stack_prep,
                                int with_bus) {
    if (log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return 0;
    return proof_words(params, airs, n_airs, log_stack, with_bus != 0, (int)log_stack_prep);
}

int zkhip_airkey_prove(zkhip_ctx* ctx, zkhip_airkey* key, int with_bus, const uint32_t* const* d_traces, const uint32_t* const* pvs,
                       unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !key || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove({ctx, &key->params, key->airs.data(), key->airs.size(), d_traces, pvs, log_stack, with_bus != 0, transcript->d, proof_out, cap,
                  root_out, key});
}

int zkhip_airkey_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                        const uint32_t* prep_root, unsigned log_stack_prep, const uint32_t* const* pvs, unsigned log_stack, int with_bus,
                        const uint32_t* proof, size_t words, uint32_t* root_out, uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !prep_root || !pvs || !proof || log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return ZKHIP_ERR_INVALID;
    return verify({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, with_bus != 0, prep_root, log_stack_prep}, root_out,
                  with_bus ? pq_out : nullptr);
}

size_t zkhip_airkey_batch_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack,
                                      unsigned log_stack_prep, int with_bus) {
    if (log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return 0;
    BatchShape T;
    return batch_shape(params, airs, n_airs, log_stack, with_bus != 0, &T, (int)log_stack_prep) ? T.total : 0;
}

int zkhip_airkey_batch_prove(zkhip_ctx* ctx, zkhip_airkey* key, int with_bus, const uint32_t* const* d_traces, const uint32_t* const* pvs,
                             unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !key || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove_batch({ctx, &key->params, key->airs.data(), key->airs.size(), d_traces, pvs, log_stack, with_bus != 0, transcript->d, proof_out,
                        cap, root_out, key});
}

int zkhip_airkey_batch_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                              const uint32_t* prep_root, unsigned log_stack_prep, const uint32_t* const* pvs, unsigned log_stack, int with_bus,
                              const uint32_t* proof, size_t words, uint32_t* root_out, uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !prep_root || !pvs || !proof || log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return ZKHIP_ERR_INVALID;
    return verify_batch({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, with_bus != 0, prep_root, log_stack_prep}, root_out,
                        pq_out);
}

int zkhip_airkey_commit_cached(zkhip_ctx* ctx, zkhip_airkey* key, size_t air, const uint32_t* d_cols, unsigned log_stack_cached,
                               zkhip_cached_main** out, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !key || !d_cols || !out) return ZKHIP_ERR_INVALID;
    return commit_cached(ctx, key, air, d_cols, log_stack_cached, out, root_out);
}

void zkhip_cached_main_destroy(zkhip_ctx* ctx, zkhip_cached_main* cached) {
    ZK_BIND_DEVICE(ctx);
    cached_main_destroy(ctx, cached);
}

size_t zkhip_airkey_cached_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack,
                                       unsigned log_stack_prep, const unsigned* log_stack_cached, int with_bus) {
    if (!log_stack_cached || log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return 0;
    BatchShape T;
    return batch_shape(params, airs, n_airs, log_stack, with_bus != 0, &T, (int)log_stack_prep, log_stack_cached) ? T.total : 0;
}

int zkhip_airkey_cached_prove(zkhip_ctx* ctx, zkhip_airkey* key, int with_bus, const uint32_t* const* d_traces, const uint32_t* const* pvs,
                              zkhip_cached_main* const* cached, unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out,
                              size_t cap, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !key || !d_traces || !pvs || !cached || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove_batch({ctx, &key->params, key->airs.data(), key->airs.size(), d_traces, pvs, log_stack, with_bus != 0, transcript->d, proof_out,
                        cap, root_out, key, cached});
}

int zkhip_airkey_cached_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                               const uint32_t* prep_root, unsigned log_stack_prep, const unsigned* log_stack_cached, const uint32_t* const* pvs,
                               unsigned log_stack, int with_bus, const uint32_t* proof, size_t words, uint32_t* root_out, uint32_t* pq_out,
                               uint32_t* cached_roots_out) {
    if (!params || (n_prefix && !prefix) || !airs || !prep_root || !log_stack_cached || !pvs || !proof || log_stack_prep > ZKHIP_WHIR_MAX_LOG_N)
        return ZKHIP_ERR_INVALID;
    return verify_batch({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, with_bus != 0, prep_root, log_stack_prep,
                         log_stack_cached}, root_out, pq_out, cached_roots_out);
}

int zkhip_zerocheck_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                           const uint32_t* const* pvs, unsigned log_stack, const uint32_t* proof, size_t words, uint32_t* root_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return verify({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, false}, root_out, nullptr);
}

int zkhip_airset_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                        const uint32_t* const* pvs, unsigned log_stack, const uint32_t* proof, size_t words, uint32_t* root_out,
                        uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return verify({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, true}, root_out, pq_out);
}

size_t zkhip_airbatch_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack, int with_bus) {
    BatchShape T;
    return batch_shape(params, airs, n_airs, log_stack, with_bus != 0, &T) ? T.total : 0;
}

int zkhip_airbatch_prove(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
                         const uint32_t* const* pvs, unsigned log_stack, int with_bus, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap,
                         uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove_batch({ctx, params, airs, n_airs, d_traces, pvs, log_stack, with_bus != 0, transcript->d, proof_out, cap, root_out});
}

int zkhip_airbatch_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                          const uint32_t* const* pvs, unsigned log_stack, int with_bus, const uint32_t* proof, size_t words, uint32_t* root_out,
                          uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return verify_batch({params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, with_bus != 0}, root_out, pq_out);
}

}  // extern "C"
