// logup_gkr.hip -- LogUp-GKR: the fractional-sum GKR proof (Papini-Habock, "Improving logarithmic derivative lookups using GKR",
// 2023) of a binary tree of fractions, the bus argument of the pinned backend's v2 form, in this library's
// own transcript.  Protocol, leaf layout and measurements: docs/logup_gkr.md.
//
// Device side, per proof of 2^L leaves:
//   * the fraction tree: every layer is written (each layer's sum-check reads the layer below it); a workgroup reduces a block of
//     512 entries nine layers deep through LDS, so the whole tree is ceil(L / 9) launches;
//   * layers whose sum-check tables hold at most SC_T entries (the top ones: layers 0..SC_LT) run in ONE single-workgroup kernel
//     with the tables in LDS and the transcript in-kernel (k_gkr_small, head form);
//   * a bigger layer k: the eq table in log-many doubling passes (the first SC_LT in one workgroup), then per round one streaming
//     pass that folds the five tables (p0, p1, q0, q1, eq) with the previous challenge AND evaluates the next round polynomial at
//     0, 2, 3 (two-stage reduction; field addition is exact, so the order does not change the words), and one one-wave kernel that
//     adds the partial sums up, observes them and samples the challenge; once the tables fit SC_T entries the rest of the layer
//     goes to k_gkr_small (tail form), which also samples the next layer's challenges.
// The pass, the one-wave kernel and the rounds of k_gkr_small are the sum-check core's (sumcheck_dev.hpp).
// Nothing goes through the host between the first launch and the final read-back.
#include <algorithm>
#include <vector>

#include "host_challenger.hpp"
#include "sumcheck_dev.hpp"

namespace zk {

constexpr unsigned GKR_TREE_DEPTH = 9;        // layers one tree launch reduces (512 entries per workgroup)
constexpr unsigned GKR_MAXL = ZKHIP_GKR_MAX_LOG_N;

// proof words before layer k's round polynomials: the root, then 12 j + 16 words for every layer j < k
ZK_HD size_t gkr_layer_off(unsigned k) { return 8 + 16 * (size_t)k + 6 * (size_t)k * (k ? k - 1 : 0); }
ZK_HD size_t gkr_proof_words(unsigned L) { return gkr_layer_off(L); }

// the layers of the tree: p[k], q[k] hold 2^k entries (extension; p[L] is the caller's numerator array, base field when base_leaves)
struct GkrLayers {
    uint32_t* p[GKR_MAXL + 1];
    uint32_t* q[GKR_MAXL + 1];
};

// ---- the fraction tree -------------------------------------------------------------------------------------------------------
// input layer `log_in` (2^log_in entries), `depth` layers below it; workgroup b reduces entries [512 b, 512 b + 512)
template <bool BASE>
__global__ __launch_bounds__(256) void k_gkr_tree(const uint32_t* __restrict__ p_in, const uint32_t* __restrict__ q_in, unsigned log_in,
                                                  unsigned depth, GkrLayers lay) {
    __shared__ uint4 sp[256], sq[256];
    const unsigned tid = threadIdx.x;
    unsigned n = (log_in >= 9 ? 512u : (1u << log_in)) >> 1;   // entries of the first output layer in this workgroup
    Ext p, q;
    if (tid < n) {
        const size_t i = (size_t)blockIdx.x * 512 + 2 * tid;
        const Ext q0 = sc_ld(q_in, i), q1 = sc_ld(q_in, i + 1);
        if (BASE) p = ext_add(ext_mul_base(q1, p_in[i]), ext_mul_base(q0, p_in[i + 1]));
        else p = ext_add(ext_mul(sc_ld(p_in, i), q1), ext_mul(sc_ld(p_in, i + 1), q0));
        q = ext_mul(q0, q1);
        sc_st(lay.p[log_in - 1], (size_t)blockIdx.x * n + tid, p);
        sc_st(lay.q[log_in - 1], (size_t)blockIdx.x * n + tid, q);
        sp[tid] = ext_pack(p), sq[tid] = ext_pack(q);
    }
    for (unsigned d = 1; d < depth; d++) {
        zk_syncthreads();
        n >>= 1;
        if (tid < n) {
            const Ext p0 = ext_unpack(sp[2 * tid]), p1 = ext_unpack(sp[2 * tid + 1]), q0 = ext_unpack(sq[2 * tid]), q1 = ext_unpack(sq[2 * tid + 1]);
            p = ext_add(ext_mul(p0, q1), ext_mul(p1, q0));
            q = ext_mul(q0, q1);
            sc_st(lay.p[log_in - 1 - d], (size_t)blockIdx.x * n + tid, p);
            sc_st(lay.q[log_in - 1 - d], (size_t)blockIdx.x * n + tid, q);
        }
        zk_syncthreads();
        if (tid < n) sp[tid] = ext_pack(p), sq[tid] = ext_pack(q);
    }
}

// ---- sum-check tables of one layer ----------------------------------------------------------------------------------------------
// P0[j] = p_{k+1}[2j], P1[j] = p_{k+1}[2j+1], Q0, Q1 alike (read from the tree), or five folded tables; E (eq) is always a table
struct GkrSrc {
    const uint32_t* p;
    const uint32_t* q;
    const uint32_t* tab[5];
    int tree, base;
    __device__ __forceinline__ Ext operator()(unsigned t, size_t j) const {
        if (tree && t < 4) {
            const size_t i = 2 * j + (t & 1);
            if (t < 2) return base ? ext_from_base(p[i]) : sc_ld(p, i);
            return sc_ld(q, i);
        }
        return sc_ld(tab[t], j);
    }
};
// a layer's round: s(x) = sum_y eq (p0 q1 + p1 q0 + lambda q0 q1) at 0, 2, 3
struct GkrRound {
    static constexpr unsigned T = 5, E = 3;
    const uint32_t* lam_p;
    Ext lam;
    __device__ __forceinline__ void load() { lam = sc_ld(lam_p, 0); }
    __device__ __forceinline__ Ext operator()(const Ext* v) const {
        const Ext qq = ext_mul(v[2], v[3]);
        const Ext s = ext_add(ext_add(ext_mul(v[0], v[3]), ext_mul(v[1], v[2])), ext_mul(lam, qq));
        return ext_mul(v[4], s);
    }
};

// eq(rho, x) over the highest nv variables of k (x_{k-nv} .. x_{k-1}), by doubling in LDS: out[i], i < 2^nv, bit b of i = x_{k-nv+b}
__global__ __launch_bounds__(SC_SW) void k_gkr_eq_seed(const uint32_t* __restrict__ rho, unsigned k, unsigned nv, uint32_t* __restrict__ out) {
    __shared__ uint4 e[SC_T];
    const unsigned tid = threadIdx.x;
    if (tid == 0) e[0] = ext_pack(ext_one());
    for (unsigned s = 1, j = k - 1; s < (1u << nv); s <<= 1, j--) {
        zk_syncthreads();
        const Ext rj = sc_ld(rho, j);
        Ext v = ext_zero();
        if (tid < s) v = ext_unpack(e[tid]);
        zk_syncthreads();
        if (tid < s) {
            const Ext hi = ext_mul(v, rj), lo = ext_sub(v, hi);   // v (1 - rho_j), v rho_j
            e[2 * tid] = ext_pack(lo), e[2 * tid + 1] = ext_pack(hi);
        }
    }
    zk_syncthreads();
    for (unsigned i = tid; i < (1u << nv); i += SC_SW) reinterpret_cast<uint4*>(out)[i] = e[i];
}
// one doubling: out[2y + b] = in[y] * (b ? rho_j : 1 - rho_j), y < n
__global__ __launch_bounds__(256) void k_gkr_eq_double(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n,
                                                       const uint32_t* __restrict__ rho_j) {
    const size_t y = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (y >= n) return;
    const Ext v = sc_ld(in, y), hi = ext_mul(v, sc_ld(rho_j, 0));
    sc_st(out, 2 * y, ext_sub(v, hi));
    sc_st(out, 2 * y + 1, hi);
}

// ---- the single-workgroup form --------------------------------------------------------------------------------------------------
// head (tail == 0): observe the root, then layers 0..k_last entirely, tables loaded from the tree;
// tail: layer k_last from round i0 on, tables of m entries = src (2m entries) folded with r[i0 - 1].
// Either way every layer it finishes ends with the four values, mu, the next point, and lambda of the next layer (or the claims).
struct GkrSmall {
    DevTranscript* tr;
    GkrLayers lay;
    unsigned L, k_last, tail, i0, m;
    int base_leaves;
    GkrSrc src;
    uint32_t* rho;   // L ext: the current layer's point (Montgomery)
    uint32_t* r;     // L ext: the current layer's round challenges
    uint32_t* lam;   // 1 ext
    uint32_t* out;   // proof words, then the point (4 L), then the claims (8), canonical
};
__global__ __launch_bounds__(SC_SW) void k_gkr_small(GkrSmall a) {
    extern __shared__ uint32_t X[];   // five tables of SC_T extension elements
    __shared__ uint32_t s_rho[GKR_MAXL][4], s_r[GKR_MAXL][4], s_lam[4];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    TrRegs R{};
    CoopConsts cc{};
    if (wave == 0) R = tr_load(a.tr, lane), cc = coop_load_consts(lane & 15u);
    unsigned k = a.tail ? a.k_last : 0;
    if (!a.tail) {
        if (wave == 0) {   // root (P, Q)
            const Ext P = sc_ld(a.lay.p[0], 0), Q = sc_ld(a.lay.q[0], 0);
            for (int w = 0; w < 8; w++) {
                const uint32_t v = w < 4 ? P.c[w] : Q.c[w - 4];
                if (lane == 0) a.out[w] = from_monty(v);
                tr_observe1(R, lane, v, cc);
            }
            for (int q = 0; q < 4; q++) {
                const uint32_t v = tr_sample1(R, lane, cc);
                if (lane == 0) s_lam[q] = v;
            }
        }
    } else {
        if (tid < 4) s_lam[tid] = a.lam[tid];
        if (tid < 4 * a.i0) s_r[tid >> 2][tid & 3] = a.r[tid];
    }
    zk_syncthreads();
    for (;; k++) {
        unsigned m, i;
        if (a.tail) {
            m = a.m, i = a.i0;
            const Ext rp = sc_ld(a.r, a.i0 - 1);
            for (unsigned y = tid; y < m; y += SC_SW)
#pragma unroll
                for (int t = 0; t < 5; t++) sc_st(X, t * SC_T + y, sc_fold(a.src(t, 2 * y), a.src(t, 2 * y + 1), rp));
        } else {
            m = 1u << k, i = 0;
            GkrSrc s{};
            s.p = a.lay.p[k + 1], s.q = a.lay.q[k + 1], s.tree = 1, s.base = a.base_leaves && k + 1 == a.L;
            for (unsigned y = tid; y < m; y += SC_SW)
#pragma unroll
                for (int t = 0; t < 4; t++) sc_st(X, t * SC_T + y, s(t, y));
            if (tid == 0) sc_st(X, 4 * SC_T, ext_one());
            for (unsigned sz = 1, j = k - 1; sz < m; sz <<= 1, j--) {   // eq(rho_k, .) by doubling, highest variable first
                zk_syncthreads();
                const Ext rj{{s_rho[j][0], s_rho[j][1], s_rho[j][2], s_rho[j][3]}};
                Ext v[SC_T / SC_SW];
                for (unsigned y = tid, c = 0; y < sz; y += SC_SW, c++) v[c] = sc_ld(X, 4 * SC_T + y);
                zk_syncthreads();
                for (unsigned y = tid, c = 0; y < sz; y += SC_SW, c++) {
                    const Ext hi = ext_mul(v[c], rj);
                    sc_st(X, 4 * SC_T + 2 * y, ext_sub(v[c], hi));
                    sc_st(X, 4 * SC_T + 2 * y + 1, hi);
                }
            }
        }
        zk_syncthreads();
        const GkrRound g{nullptr, Ext{{s_lam[0], s_lam[1], s_lam[2], s_lam[3]}}};
        uint32_t* proof_k = a.out + gkr_layer_off(k);
        for (; i < k; i++, m >>= 1) sc_small_round(g, X, SC_T, m, R, cc, proof_k + 12 * i, a.r + 4 * i, s_r[i]);   // m <= 2 SC_SW
        // end of layer k: p_{k+1}(0, r), p_{k+1}(1, r), q_{k+1}(0, r), q_{k+1}(1, r); mu; rho_{k+1} = (mu, r_0 .. r_{k-1})
        if (wave == 0) {
            Ext v[4];
            for (int t = 0; t < 4; t++) v[t] = sc_ld(X, t * SC_T);
            for (int w = 0; w < 16; w++) {
                const uint32_t x = v[w >> 2].c[w & 3];
                if (lane == 0) proof_k[12 * k + w] = from_monty(x);
                tr_observe1(R, lane, x, cc);
            }
            Ext mu;
            for (int q = 0; q < 4; q++) mu.c[q] = tr_sample1(R, lane, cc);
            if (lane == 0) {
                for (int j = (int)k; j >= 1; j--)
                    for (int q = 0; q < 4; q++) s_rho[j][q] = s_r[j - 1][q];
                for (int q = 0; q < 4; q++) s_rho[0][q] = mu.c[q];
            }
            if (k + 1 == a.L) {
                if (lane == 0) {
                    const Ext cp = sc_fold(v[0], v[1], mu), cq = sc_fold(v[2], v[3], mu);
                    uint32_t* pt = a.out + gkr_proof_words(a.L);
                    for (unsigned j = 0; j <= k; j++)
                        for (int q = 0; q < 4; q++) pt[4 * j + q] = from_monty(s_rho[j][q]);
                    for (int q = 0; q < 4; q++) pt[4 * a.L + q] = from_monty(cp.c[q]), pt[4 * a.L + 4 + q] = from_monty(cq.c[q]);
                }
            } else {
                for (int q = 0; q < 4; q++) {
                    const uint32_t x = tr_sample1(R, lane, cc);
                    if (lane == 0) s_lam[q] = x;
                }
            }
        }
        zk_syncthreads();
        if (k == a.k_last) break;
    }
    if (wave == 0) {
        tr_store(a.tr, R, lane);
        if (lane < 4) a.lam[lane] = s_lam[lane];
        for (unsigned j = lane; j < 4 * (k + 1) && k + 1 < a.L; j += 64) a.rho[j] = s_rho[j >> 2][j & 3];
    }
}


// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
}  // namespace

// The tree, the folded tables, the eq tables and the proof staging of one proof, in one grow-only buffer of the context.
int gkr_prove_device(zkhip_ctx* ctx, DevTranscript* d_t, const uint32_t* d_num, bool num_ext, const uint32_t* d_den, unsigned L,
                     const uint32_t** d_result) {
    if (L < 1 || L > GKR_MAXL) return set_error(ctx, ZKHIP_ERR_INVALID, "gkr: log_n out of range");
    const bool big = L - 1 > SC_LT;   // some layer needs the streaming passes
    const size_t capA = big ? (size_t)1 << (L - 2) : 1, capB = big ? (size_t)1 << (L - 3) : 1, capE = big ? (size_t)1 << (L - 1) : 1;
    size_t off = 0;
    std::vector<size_t> o_layer(L);
    for (unsigned k = 0; k < L; k++) o_layer[k] = off, off += 2 * align256(((size_t)16) << k);
    const size_t o_A = off; off += align256(5 * capA * 16);
    const size_t o_B = off; off += align256(5 * capB * 16);
    const size_t o_E0 = off; off += align256(capE * 16);
    const size_t o_E1 = off; off += align256(capE * 16);
    const size_t o_partial = off; off += align256(12 * SC_NB * 4);
    const size_t o_rho = off; off += align256(GKR_MAXL * 16);
    const size_t o_r = off; off += align256(GKR_MAXL * 16);
    const size_t o_lam = off; off += 256;
    const size_t o_out = off; off += align256((gkr_proof_words(L) + 4 * (size_t)L + 8) * 4);
    if (ctx->gkr_ws_bytes < off) {
        if (ctx->gkr_ws) {
            ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            ZK_HIP_CHECK(ctx, hipFree(ctx->gkr_ws));
            ctx->gkr_ws = nullptr, ctx->gkr_ws_bytes = 0;
        }
        if (hipMalloc(&ctx->gkr_ws, off) != hipSuccess) return set_error(ctx, ZKHIP_ERR_NOMEM, "gkr workspace");
        ctx->gkr_ws_bytes = off;
    }
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_gkr_small, hipFuncAttributeMaxDynamicSharedMemorySize, 5 * SC_T * 16));
        attr_set.mark(ctx->device);
    }
    uint8_t* base = (uint8_t*)ctx->gkr_ws;
    GkrLayers lay{};
    for (unsigned k = 0; k < L; k++) {
        lay.p[k] = (uint32_t*)(base + o_layer[k]);
        lay.q[k] = (uint32_t*)(base + o_layer[k] + align256(((size_t)16) << k));
    }
    lay.p[L] = const_cast<uint32_t*>(d_num), lay.q[L] = const_cast<uint32_t*>(d_den);   // read only
    uint32_t *A = (uint32_t*)(base + o_A), *B = (uint32_t*)(base + o_B), *E0 = (uint32_t*)(base + o_E0), *E1 = (uint32_t*)(base + o_E1);
    uint32_t *partial = (uint32_t*)(base + o_partial), *rho = (uint32_t*)(base + o_rho), *r = (uint32_t*)(base + o_r);
    uint32_t *lam = (uint32_t*)(base + o_lam), *out = (uint32_t*)(base + o_out);
    hipStream_t st = ctx->stream;

    {   // the fraction tree, GKR_TREE_DEPTH layers per launch
        for (unsigned k = L; k > 0;) {
            KernelScope ks(ctx, "gkr_tree");
            const unsigned d = std::min(GKR_TREE_DEPTH, k);
            const unsigned blocks = k >= GKR_TREE_DEPTH ? 1u << (k - GKR_TREE_DEPTH) : 1u;
            if (k == L && !num_ext) hipLaunchKernelGGL(k_gkr_tree<true>, dim3(blocks), dim3(256), 0, st, lay.p[k], lay.q[k], k, d, lay);
            else hipLaunchKernelGGL(k_gkr_tree<false>, dim3(blocks), dim3(256), 0, st, lay.p[k], lay.q[k], k, d, lay);
            k -= d;
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    const size_t lds = 5 * SC_T * 16;
    {   // root and layers 0 .. SC_LT: one workgroup
        KernelScope ks(ctx, "gkr_small");
        GkrSmall s{};
        s.tr = d_t, s.lay = lay, s.L = L, s.k_last = std::min(L - 1, SC_LT), s.tail = 0, s.base_leaves = !num_ext;
        s.rho = rho, s.r = r, s.lam = lam, s.out = out;
        hipLaunchKernelGGL(k_gkr_small, dim3(1), dim3(SC_SW), lds, st, s);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    for (unsigned k = SC_LT + 1; k < L; k++) {
        {   // eq(rho_k, .): the highest SC_LT variables in one workgroup, then one doubling per variable; lands in E0
            const unsigned nd = k - SC_LT;
            uint32_t* e = nd % 2 == 0 ? E0 : E1;
            {
                KernelScope ks(ctx, "gkr_eq");
                hipLaunchKernelGGL(k_gkr_eq_seed, dim3(1), dim3(SC_SW), 0, st, (const uint32_t*)rho, k, SC_LT, e);
            }
            size_t n = SC_T;
            for (unsigned j = nd; j-- > 0; n <<= 1) {
                KernelScope ks(ctx, "gkr_eq");
                uint32_t* o = e == E0 ? E1 : E0;
                hipLaunchKernelGGL(k_gkr_eq_double, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)e, o, n,
                                   (const uint32_t*)(rho + 4 * j));
                e = o;
            }
            ZK_HIP_CHECK(ctx, hipGetLastError());
        }
        GkrSrc src{};
        src.p = lay.p[k + 1], src.q = lay.q[k + 1], src.tab[4] = E0, src.tree = 1, src.base = !num_ext && k + 1 == L;
        size_t m = (size_t)1 << k;
        unsigned i = 0;
        for (; m > SC_T; m >>= 1, i++) {   // round i on tables of m entries: fold with r_{i-1}, evaluate s_i
            ScPass<GkrSrc, GkrRound> p{};
            p.src = src, p.g.lam_p = lam, p.n_pairs = m / 2, p.partial = partial;
            p.r = i ? r + 4 * (i - 1) : nullptr;
            if (i)
                for (int t = 0; t < 5; t++) p.dst[t] = (i % 2 ? A : B) + 4 * t * (i % 2 ? capA : capB);
            const unsigned nb = (unsigned)std::min<size_t>(SC_NB, (m / 2 + 255) / 256);
            {
                KernelScope ks(ctx, "gkr_pass");
                hipLaunchKernelGGL(k_sc_pass, dim3(nb), dim3(256), 0, st, p);
            }
            {
                KernelScope ks(ctx, "gkr_round_tr");
                hipLaunchKernelGGL(k_sc_round_tr<12>, dim3(1), dim3(64), 0, st, d_t, (const uint32_t*)partial, nb, out + gkr_layer_off(k) + 12 * i,
                                   r + 4 * i);
            }
            ZK_HIP_CHECK(ctx, hipGetLastError());
            if (i) {
                src.tree = 0;
                for (int t = 0; t < 5; t++) src.tab[t] = p.dst[t];
            }
        }
        {   // the rest of layer k in one workgroup
            KernelScope ks(ctx, "gkr_small");
            GkrSmall s{};
            s.tr = d_t, s.lay = lay, s.L = L, s.k_last = k, s.tail = 1, s.i0 = i, s.m = (unsigned)m, s.base_leaves = !num_ext, s.src = src;
            s.rho = rho, s.r = r, s.lam = lam, s.out = out;
            hipLaunchKernelGGL(k_gkr_small, dim3(1), dim3(SC_SW), lds, st, s);
            ZK_HIP_CHECK(ctx, hipGetLastError());
        }
    }
    *d_result = out;
    return ZKHIP_OK;
}

// ---- the host verifier ---------------------------------------------------------------------------------------------------------
// replays the proof on `ch`; point_out (4 L words) / claims_out (8 words) canonical, root_out = (P, Q) in Montgomery form
int gkr_verify_host(HostChallenger& ch, const uint32_t* proof, size_t words, unsigned L, uint32_t* point_out, uint32_t* claims_out,
                    Ext root_out[2]) {
    if (!proof || L < 1 || L > GKR_MAXL || words != gkr_proof_words(L)) return ZKHIP_ERR_VERIFY;
    for (size_t w = 0; w < words; w++)
        if (proof[w] >= P) return ZKHIP_ERR_VERIFY;
    for (size_t w = 0; w < 8; w++) ch.observe(to_monty(proof[w]));
    Ext cp = ext_from_canon(proof), cq = ext_from_canon(proof + 4);
    root_out[0] = cp, root_out[1] = cq;
    std::vector<Ext> rho, r;
    for (unsigned k = 0; k < L; k++) {
        const Ext lam = ch.sample_ext();
        Ext claim = ext_add(cp, ext_mul(lam, cq));
        const uint32_t* pk = proof + gkr_layer_off(k);
        r.clear();
        for (unsigned i = 0; i < k; i++) {
            const uint32_t* w = pk + 12 * i;
            const Ext s0 = ext_from_canon(w), s[4] = {s0, ext_sub(claim, s0), ext_from_canon(w + 4), ext_from_canon(w + 8)};
            for (int j = 0; j < 12; j++) ch.observe(to_monty(w[j]));
            const Ext ri = ch.sample_ext();
            claim = poly_at(s, 3, ri);
            r.push_back(ri);
        }
        const uint32_t* w = pk + 12 * k;
        const Ext p0 = ext_from_canon(w), p1 = ext_from_canon(w + 4), q0 = ext_from_canon(w + 8), q1 = ext_from_canon(w + 12);
        const Ext eq = eq_eval(rho.data(), r.data(), k);
        const Ext body = ext_add(ext_add(ext_mul(p0, q1), ext_mul(p1, q0)), ext_mul(lam, ext_mul(q0, q1)));
        if (!ext_eq(ext_mul(eq, body), claim)) return ZKHIP_ERR_VERIFY;
        for (int j = 0; j < 16; j++) ch.observe(to_monty(w[j]));
        const Ext mu = ch.sample_ext();
        rho.assign(1, mu);
        rho.insert(rho.end(), r.begin(), r.end());
        cp = ext_add(p0, ext_mul(mu, ext_sub(p1, p0)));
        cq = ext_add(q0, ext_mul(mu, ext_sub(q1, q0)));
    }
    if (point_out)
        for (unsigned j = 0; j < L; j++) ext_to_canon(point_out + 4 * j, rho[j]);
    if (claims_out) ext_to_canon(claims_out, cp), ext_to_canon(claims_out + 4, cq);
    return ZKHIP_OK;
}

}  // namespace zk

using namespace zk;

extern "C" {

size_t zkhip_gkr_proof_words(unsigned log_n) { return log_n >= 1 && log_n <= GKR_MAXL ? gkr_proof_words(log_n) : 0; }

int zkhip_gkr_fraction_prove(zkhip_ctx* ctx, zkhip_transcript* transcript, const uint32_t* d_num, int num_is_ext, const uint32_t* d_den,
                             unsigned log_n, uint32_t* proof_out, size_t cap, uint32_t* point_out, uint32_t* claims_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !transcript || !d_num || !d_den || !proof_out) return ZKHIP_ERR_INVALID;
    if (log_n < 1 || log_n > GKR_MAXL) return set_error(ctx, ZKHIP_ERR_INVALID, "gkr: log_n out of range");
    const size_t words = gkr_proof_words(log_n);
    if (cap < words) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, "gkr: proof buffer too small");
    const uint32_t* d_res = nullptr;
    ZK_TRY(gkr_prove_device(ctx, transcript->d, d_num, num_is_ext != 0, d_den, log_n, &d_res));
    std::vector<uint32_t> h(words + 4 * (size_t)log_n + 8);
    ZK_TRY(zkhip_d2h(ctx, h.data(), d_res, h.size() * 4));
    memcpy(proof_out, h.data(), words * 4);
    if (point_out) memcpy(point_out, h.data() + words, 16 * (size_t)log_n);
    if (claims_out) memcpy(claims_out, h.data() + words + 4 * (size_t)log_n, 32);
    return ZKHIP_OK;
}

int zkhip_gkr_fraction_verify(const uint32_t* prefix, size_t n_prefix, const uint32_t* proof, size_t words, unsigned log_n,
                              uint32_t* point_out, uint32_t* claims_out) {
    if (n_prefix && !prefix) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    Ext root[2];
    return gkr_verify_host(ch, proof, words, log_n, point_out, claims_out, root);
}

int zkhip_bus_gkr_verify(const uint32_t* prefix, size_t n_prefix, const uint32_t* proof, size_t words, unsigned log_leaves,
                         uint32_t* challenges_out, uint32_t* point_out, uint32_t* claims_out) {
    if (n_prefix && !prefix) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    const Ext gamma = ch.sample_ext(), beta = ch.sample_ext();
    if (challenges_out) ext_to_canon(challenges_out, gamma), ext_to_canon(challenges_out + 4, beta);
    Ext root[2];
    ZK_TRY(gkr_verify_host(ch, proof, words, log_leaves, point_out, claims_out, root));
    if (!ext_eq(root[0], ext_zero()) || ext_eq(root[1], ext_zero())) return ZKHIP_ERR_VERIFY;   // balanced: P = 0, Q != 0
    return ZKHIP_OK;
}

}  // extern "C"
