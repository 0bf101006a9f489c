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
#include <map>

#include "zerocheck_dev.hpp"

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
};
// false = refused.  Without with_bus the AIRs' interactions are ignored: their plans have no bus roots (and another D).
// l_prep >= 0: the keyed form at log_stack_prep = l_prep
bool shape(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, bool with_bus, Shape* S, int l_prep = -1) {
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
        for (size_t c = 0; c < airs[a].width; c++) S->lh.push_back(airs[a].log_height), S->col_point.push_back((unsigned)a);
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
        S->total += sp;
    }
    return true;
}

// ---- the device prover ---------------------------------------------------------------------------------------------------------
// The bus part of the AIR-set proof (docs/airset.md, steps 2 - 5), after the root and the public values were observed: the leaves,
// the fraction-sum proof (its words to dP + 8), the leaf claims B_a (after them), and per AIR with interactions what its joint
// sum-check needs (bus[a]).  Its buffers are B's: they live until the caller's per-AIR loop is done.
int prove_bus(zkhip_ctx* ctx, const Shape& S, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces, const uint32_t* const* pvs,
              DevTranscript* d_t, DevBufs& B, uint32_t* dP, std::vector<ZcBus>* bus, const zkhip_airkey* key) {
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

// either proof: with_bus, the AIR-set proof of docs/airset.md (its step numbers below); without, the zero-check of docs/zerocheck.md.
// key: the keyed form (prm, airs and n_airs are the key's)
int prove(zkhip_ctx* ctx, const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
          const uint32_t* const* pvs, unsigned l, bool with_bus, DevTranscript* d_t, uint32_t* proof_out, size_t cap, uint32_t* root_out,
          const zkhip_airkey* key = nullptr) {
    const std::string who = key ? "airkey: " : with_bus ? "airset: " : "zerocheck: ";
    Shape S;
    if (!shape(prm, airs, n_airs, l, with_bus, &S, key ? (int)key->l_prep : -1))
        return set_error(ctx, ZKHIP_ERR_INVALID, who + "the shape does not fit the limits");
    if (cap < S.total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, who + "proof buffer too small");
    size_t n_pv = 0, pt_words = 0;
    for (size_t a = 0; a < n_airs; a++) {
        if (!d_traces[a] || (airs[a].n_pvs && !pvs[a])) return set_error(ctx, ZKHIP_ERR_INVALID, who + "null trace or public values");
        for (size_t i = 0; i < airs[a].n_pvs; i++)
            if (pvs[a][i] >= P) return set_error(ctx, ZKHIP_ERR_INVALID, who + "public value not canonical");
        n_pv += airs[a].n_pvs, pt_words += 4 * (size_t)airs[a].log_height;
    }
    // 1. commit: every main column, AIRs in caller order
    std::vector<const uint32_t*> cols;
    for (size_t a = 0; a < n_airs; a++)
        for (size_t c = 0; c < airs[a].width; c++) cols.push_back(d_traces[a] + (c << airs[a].log_height));
    struct Com {
        zkhip_ctx* ctx;
        zkhip_stack_commitment* sc = nullptr;
        ~Com() { stack_destroy(ctx, sc); }
    } com{ctx};
    uint32_t root[8];
    ZK_TRY(stack_commit(ctx, prm, cols.data(), S.lh.data(), cols.size(), l, &com.sc, root));
    DevBufs B(ctx);
    // device: [the words before the opening | the points r'_a (Montgomery)], then the root and the public values to observe
    uint32_t *dP = B.get(S.head + pt_words), *d_obs = B.get((key ? 16 : 8) + n_pv);
    if (!dP || !d_obs) return set_error(ctx, ZKHIP_ERR_NOMEM, who + "proof staging");
    std::vector<uint32_t> obs;
    if (key) obs.assign(key->root, key->root + 8);   // the key's root is observed, not sent
    obs.insert(obs.end(), root, root + 8);
    for (size_t a = 0; a < n_airs; a++) obs.insert(obs.end(), pvs[a], pvs[a] + airs[a].n_pvs);
    ZK_TRY(zkhip_h2d(ctx, d_obs, obs.data(), obs.size() * 4));
    ZK_TRY(transcript_observe(ctx, d_t, d_obs, (uint32_t)obs.size(), true));
    // 2. - 5. the bus part
    std::vector<ZcBus> bus(n_airs);   // E2 null: an AIR without interactions, or the zero-check
    if (with_bus) ZK_TRY(prove_bus(ctx, S, airs, n_airs, d_traces, pvs, d_t, B, dP, &bus, key));
    // 6. - 8. per AIR
    size_t off = 8 + S.gkr_words + 4 * S.n_bus, poff = S.head;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        if (key && pl.wp) {   // the kernels' PREP form, on the key's resident columns
            const uint32_t* prep = key->d_prep + key->prep_at[a];
            if (bus[a].E2) ZK_TRY((zc_prove_air<true, true>(ctx, d_t, pl, d_traces[a], pvs[a], dP + off, dP + poff, bus[a], prep)));
            else ZK_TRY((zc_prove_air<false, true>(ctx, d_t, pl, d_traces[a], pvs[a], dP + off, dP + poff, ZcBus{}, prep)));
        } else if (bus[a].E2) ZK_TRY(zc_prove_air<true>(ctx, d_t, pl, d_traces[a], pvs[a], dP + off, dP + poff, bus[a]));
        else ZK_TRY(zc_prove_air<false>(ctx, d_t, pl, d_traces[a], pvs[a], dP + off, dP + poff));
        off += pl.active() ? pl.words() : 0;
        poff += 4 * (size_t)pl.m;
    }
    // 9. the one read-back before the opening: the words so far and the points
    std::vector<uint32_t> h(S.head + pt_words);
    ZK_TRY(zkhip_d2h(ctx, h.data(), dP, h.size() * 4));
    for (size_t i = S.head; i < h.size(); i++) h[i] = from_monty(h[i]);
    ZK_TRY(stack_open(ctx, com.sc, d_t, h.data() + S.head, S.dims.data(), n_airs, S.col_point.data(), nullptr, proof_out + S.head, cap - S.head));
    if (key) {   // the key's commitment at the points of the AIRs that have preprocessed columns
        std::vector<uint32_t> pts;
        size_t at = S.head;
        for (size_t a = 0; a < n_airs; at += 4 * (size_t)S.plans[a].m, a++)
            if (S.plans[a].wp) pts.insert(pts.end(), h.begin() + at, h.begin() + at + 4 * (size_t)S.plans[a].m);
        const size_t o = S.head + S.main_words;
        ZK_TRY(stack_open(ctx, key->sc, d_t, pts.data(), S.dims_p.data(), S.dims_p.size(), S.col_point_p.data(), nullptr, proof_out + o, cap - o));
    }
    memcpy(proof_out, root, 32);
    memcpy(proof_out + 8, h.data() + 8, (S.head - 8) * 4);
    if (root_out) memcpy(root_out, root, 32);
    return ZKHIP_OK;
}

// ---- the host verifier ---------------------------------------------------------------------------------------------------------
// of either proof; pq_out: the fraction sum's (P, Q), with_bus only
// prep_root: the keyed form, checked against the key's root at l_prep
int verify(const zkhip_whir_params* prm, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs, const uint32_t* const* pvs,
           unsigned l, const uint32_t* proof, size_t words, bool with_bus, uint32_t* root_out, uint32_t* pq_out, const uint32_t* prep_root = nullptr,
           unsigned l_prep = 0) {
    Shape S;
    if (!shape(prm, airs, n_airs, l, with_bus, &S, prep_root ? (int)l_prep : -1)) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; prep_root && i < 8; i++)
        if (prep_root[i] >= P) return ZKHIP_ERR_INVALID;
    for (size_t a = 0; a < n_airs; a++) {
        if (airs[a].n_pvs && !pvs[a]) return ZKHIP_ERR_INVALID;
        for (size_t i = 0; i < airs[a].n_pvs; i++)
            if (pvs[a][i] >= P) return ZKHIP_ERR_INVALID;
    }
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    if (words != S.total) return ZKHIP_ERR_VERIFY;
    for (size_t i = 0; i < S.head; i++)
        if (proof[i] >= P) return ZKHIP_ERR_VERIFY;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    if (prep_root) ch.observe_canon(prep_root, 8);
    ch.observe_canon(proof, 8);
    for (size_t a = 0; a < n_airs; a++) ch.observe_canon(pvs[a], airs[a].n_pvs);
    const Ext one = ext_one();
    const size_t n_blk = S.blocks.size();
    const uint32_t *q = proof + 8, *qB = nullptr;   // qB: the leaf claims B_a
    Ext gamma = ext_zero(), kappa = ext_zero();
    std::vector<Ext> rho(S.L), eb(n_blk), bpow(LOGUP_MAX_FIELDS + 1, one);
    std::vector<std::vector<size_t>> blk_of(n_airs);   // AIR -> its blocks in program order
    if (with_bus) {
        // 2. - 4. gamma, beta, the fraction-sum proof: rho, (p*, q*), balance
        gamma = ch.sample_ext();
        const Ext beta = ch.sample_ext();
        std::vector<uint32_t> pt(4 * (size_t)S.L);
        uint32_t cl8[8];
        Ext pq[2];
        ZK_TRY(gkr_verify_host(ch, q, S.gkr_words, S.L, pt.data(), cl8, pq));
        if (!ext_eq(pq[0], ext_zero()) || ext_eq(pq[1], ext_zero())) return ZKHIP_ERR_VERIFY;
        for (unsigned j = 0; j < S.L; j++) rho[j] = ext_from_canon(pt.data() + 4 * j);
        const Ext pstar = ext_from_canon(cl8), qstar = ext_from_canon(cl8 + 4);
        // 5. the leaf claims
        Ext pad = one;
        for (size_t b = 0; b < n_blk; b++) {
            const AsBlk& k = S.blocks[b];
            Ext e = one;
            for (unsigned t = 0; k.m + t < S.L; t++) e = ext_mul(e, ((k.off >> k.m) >> t) & 1u ? rho[k.m + t] : ext_sub(one, rho[k.m + t]));
            eb[b] = e, pad = ext_sub(pad, e);
        }
        kappa = ch.sample_ext();
        qB = q + S.gkr_words;
        Ext lhs = ext_mul(kappa, pad);
        for (size_t i = 0; i < S.n_bus; i++) lhs = ext_add(lhs, ext_from_canon(qB + 4 * i));
        ch.observe_canon(qB, 4 * S.n_bus);
        if (!ext_eq(lhs, ext_add(pstar, ext_mul(kappa, qstar)))) return ZKHIP_ERR_VERIFY;
        q = qB + 4 * S.n_bus;
        for (unsigned i = 1; i <= LOGUP_MAX_FIELDS; i++) bpow[i] = ext_mul(bpow[i - 1], beta);
        for (size_t a = 0; a < n_airs; a++) blk_of[a].resize(S.plans[a].prog.ints.size());
        for (size_t b = 0; b < n_blk; b++) blk_of[S.blocks[b].a][S.blocks[b].j] = b;
    }
    std::vector<uint32_t> points;                            // r'_a, canonical, end to end
    std::vector<const uint32_t*> claimed(n_airs, nullptr);   // the w values the opening must show (null: none claimed)
    std::vector<const uint32_t*> claimed_p(n_airs, nullptr); // keyed: the w_p values the key's opening must show
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        const unsigned m = pl.m, D = pl.D;
        const size_t w = pl.w, n_rot = pl.rot.size(), wp = pl.wp, n_rot_p = pl.rot_p.size(), n_val = w + n_rot + wp + n_rot_p;
        const bool has_cons = !pl.proven.empty(), has_bus = !pl.bus_roots.empty();   // the zero-check's plans have no bus roots
        std::vector<Ext> rp(m);
        if (!pl.active()) {
            for (unsigned j = 0; j < m; j++) rp[j] = ch.sample_ext();
        } else {
            // 6. the (joint) sum-check
            std::vector<Ext> tau(m), r(m), coef;
            Ext alpha = ext_zero(), claim = ext_zero();
            if (has_cons) {
                for (unsigned j = 0; j < m; j++) tau[j] = ch.sample_ext();
                alpha = ch.sample_ext();
            }
            if (has_bus) {
                Ext cst = ext_zero();   // sum_j e_{a,j} (gamma + bus_j + 1)
                for (size_t j = 0; j < blk_of[a].size(); j++) {
                    const Interaction& it = pl.prog.ints[j];
                    const Ext e = eb[blk_of[a][j]], ke = ext_mul(kappa, e);
                    Ext g1 = gamma;
                    g1.c[0] = madd(g1.c[0], to_monty(it.bus + 1));
                    cst = ext_add(cst, ext_mul(e, g1));
                    coef.push_back(it.sign ? ext_neg(e) : e);
                    for (uint32_t i = 0; i < it.n_fields; i++) coef.push_back(ext_mul(ke, bpow[i + 1]));
                }
                claim = ext_sub(ext_from_canon(qB + 4 * S.b_at[a]), ext_mul(kappa, cst));
            }
            for (unsigned i = 0; i < m; i++, q += 4 * D) {
                Ext s[ZKHIP_ZEROCHECK_MAX_DEGREE + 1];
                s[0] = ext_from_canon(q), s[1] = ext_sub(claim, s[0]);
                for (unsigned e = 1; e < D; e++) s[e + 1] = ext_from_canon(q + 4 * e);
                ch.observe_canon(q, 4 * D);
                r[i] = ch.sample_ext();
                claim = poly_at(s, D, r[i]);
            }
            // 7. the values
            std::vector<Ext> v(w), vn(n_rot), vp(wp), vpn(n_rot_p);   // v, v', v_p, v_p'
            for (size_t j = 0; j < w; j++) v[j] = ext_from_canon(q + 4 * j);
            for (size_t t = 0; t < n_rot; t++) vn[t] = ext_from_canon(q + 4 * (w + t));
            for (size_t j = 0; j < wp; j++) vp[j] = ext_from_canon(q + 4 * (w + n_rot + j));
            for (size_t t = 0; t < n_rot_p; t++) vpn[t] = ext_from_canon(q + 4 * (w + n_rot + wp + t));
            ch.observe_canon(q, 4 * n_val);
            const uint32_t* qv = q;
            q += 4 * n_val;
            Ext first = one, last = one;
            for (unsigned j = 0; j < m; j++) first = ext_mul(first, ext_sub(one, r[j])), last = ext_mul(last, r[j]);
            Ext rhs = ext_zero();
            if (has_cons) {   // eq(tau, r) sum_k alpha^k C_k
                const std::vector<Ext> val = zc_eval_host(pl, pl.reach, v.data(), vn.data(), first, last, pvs[a], vp.data(), vpn.data());
                Ext c = ext_zero(), ap = one;
                for (uint32_t k : pl.proven) c = ext_add(c, ext_mul(ap, val[k])), ap = ext_mul(ap, alpha);
                rhs = ext_mul(eq_eval(tau.data(), r.data(), m), c);
            }
            if (has_bus) {   // eq(rho_a, r) sum_j (cc_j count_j + sum_i cf_{j,i} f_{j,i}), coef in pl.bus_roots' order
                // parse_air: interaction operands read the current row only, so neither v' nor first / last enters
                const std::vector<Ext> val = zc_eval_host(pl, pl.bus_reach, v.data(), vn.data(), first, last, pvs[a], vp.data(), vpn.data());
                Ext c = ext_zero();
                for (size_t k = 0; k < coef.size(); k++) c = ext_add(c, ext_mul(coef[k], val[pl.bus_roots[k]]));
                rhs = ext_add(rhs, ext_mul(eq_eval(rho.data(), r.data(), m), c));
            }
            if (!ext_eq(rhs, claim)) return ZKHIP_ERR_VERIFY;
            // 8. the rotation reduction
            if (!pl.reduces()) {
                rp = r, claimed[a] = qv, claimed_p[a] = wp ? qv + 4 * (w + n_rot) : nullptr;
            } else {
                const Ext lambda = ch.sample_ext();
                std::vector<Ext> lp(n_val);   // over [v | v' | v_p | v_p']
                Ext x = one;
                claim = ext_zero();
                for (size_t j = 0; j < n_val; j++) lp[j] = x, claim = ext_add(claim, ext_mul(x, ext_from_canon(qv + 4 * j))), x = ext_mul(x, lambda);
                for (unsigned i = 0; i < m; i++, q += 8) {
                    const Ext s0 = ext_from_canon(q), s2 = ext_from_canon(q + 4);
                    ch.observe_canon(q, 8);
                    rp[i] = ch.sample_ext();
                    const Ext sv[3] = {s0, ext_sub(claim, s0), s2};
                    claim = poly_at(sv, 2, rp[i]);
                }
                Ext ua = ext_zero(), ub = ext_zero();
                for (size_t j = 0; j < w; j++) ua = ext_add(ua, ext_mul(lp[j], ext_from_canon(q + 4 * j)));
                for (size_t t = 0; t < n_rot; t++) ub = ext_add(ub, ext_mul(lp[w + t], ext_from_canon(q + 4 * pl.rot[t])));
                const uint32_t* qp = q + 4 * w;   // u_p
                for (size_t j = 0; j < wp; j++) ua = ext_add(ua, ext_mul(lp[w + n_rot + j], ext_from_canon(qp + 4 * j)));
                for (size_t t = 0; t < n_rot_p; t++) ub = ext_add(ub, ext_mul(lp[w + n_rot + wp + t], ext_from_canon(qp + 4 * pl.rot_p[t])));
                ch.observe_canon(q, 4 * (w + wp));
                claimed[a] = q, claimed_p[a] = wp ? qp : nullptr, q += 4 * (w + wp);
                const Ext want = ext_add(ext_mul(ua, eq_eval(r.data(), rp.data(), m)), ext_mul(ub, zc_rot_eval(r.data(), rp.data(), m)));
                if (!ext_eq(want, claim)) return ZKHIP_ERR_VERIFY;
            }
        }
        for (unsigned j = 0; j < m; j++) {
            uint32_t c4[4];
            ext_to_canon(c4, rp[j]);
            points.insert(points.end(), c4, c4 + 4);
        }
    }
    // 9. the stacked opening
    const uint32_t* op = proof + S.head;
    ZK_TRY(stack_verify_host(ch, prm, proof, S.lh.data(), S.lh.size(), l, points.data(), S.dims.data(), n_airs, S.col_point.data(), op, S.main_words));
    size_t col = 0;
    for (size_t a = 0; a < n_airs; col += airs[a].width, a++)
        if (claimed[a] && memcmp(claimed[a], op + 4 * col, 16 * airs[a].width) != 0) return ZKHIP_ERR_VERIFY;
    if (prep_root) {   // the key's opening, against the verifier's own root
        std::vector<uint32_t> pts;
        size_t at = 0;
        for (size_t a = 0; a < n_airs; at += 4 * (size_t)S.plans[a].m, a++)
            if (S.plans[a].wp) pts.insert(pts.end(), points.begin() + at, points.begin() + at + 4 * (size_t)S.plans[a].m);
        const uint32_t* op2 = op + S.main_words;
        ZK_TRY(stack_verify_host(ch, prm, prep_root, S.lh_p.data(), S.lh_p.size(), l_prep, pts.data(), S.dims_p.data(), S.dims_p.size(),
                                 S.col_point_p.data(), op2, words - S.head - S.main_words));
        col = 0;
        for (size_t a = 0; a < n_airs; col += S.plans[a].wp, a++)
            if (claimed_p[a] && memcmp(claimed_p[a], op2 + 4 * col, 16 * S.plans[a].wp) != 0) return ZKHIP_ERR_VERIFY;
    }
    if (root_out) memcpy(root_out, proof, 32);
    if (pq_out) memcpy(pq_out, proof + 8, 32);
    return ZKHIP_OK;
}

size_t proof_words(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, bool with_bus, int l_prep = -1) {
    Shape S;
    return shape(prm, airs, n_airs, l, with_bus, &S, l_prep) ? S.total : 0;
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
    return prove(ctx, params, airs, n_airs, d_traces, pvs, log_stack, false, transcript->d, proof_out, cap, root_out);
}

int zkhip_airset_prove(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
                       const uint32_t* const* pvs, unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap,
                       uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return prove(ctx, params, airs, n_airs, d_traces, pvs, log_stack, true, transcript->d, proof_out, cap, root_out);
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
    return prove(ctx, &key->params, key->airs.data(), key->airs.size(), d_traces, pvs, log_stack, with_bus != 0, transcript->d, proof_out, cap,
                 root_out, key);
}

int zkhip_airkey_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                        const uint32_t* prep_root, unsigned log_stack_prep, const uint32_t* const* pvs, unsigned log_stack, int with_bus,
                        const uint32_t* proof, size_t words, uint32_t* root_out, uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !prep_root || !pvs || !proof || log_stack_prep > ZKHIP_WHIR_MAX_LOG_N) return ZKHIP_ERR_INVALID;
    return verify(params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, with_bus != 0, root_out, with_bus ? pq_out : nullptr, prep_root,
                  log_stack_prep);
}

int zkhip_zerocheck_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                           const uint32_t* const* pvs, unsigned log_stack, const uint32_t* proof, size_t words, uint32_t* root_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return verify(params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, false, root_out, nullptr);
}

int zkhip_airset_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                        const uint32_t* const* pvs, unsigned log_stack, const uint32_t* proof, size_t words, uint32_t* root_out,
                        uint32_t* pq_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return verify(params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, true, root_out, pq_out);
}

}  // extern "C"
