// ntt.hip -- batched BabyBear NTT / coset LDE for gfx950 (K1 of SURVEY.md 2.3).
//
// Replaces, behind include/zkhip.h, what the reference's engine gets from p3-dft 0.4.3
// (`dft_batch`, `coset_lde_batch`; Cargo.lock:5590) when it RS-encodes committed traces
// (SURVEY.md 8(a) a7.1).  Definition: out[i] = sum_j in[j] w^(ij); coset LDE =
// iDFT, scale coefficient i by shift^i, zero-pad, DFT; committed LDEs keep rows bit-reversed.
//
// Design (column-major, one column = 2^n contiguous u32 in HBM):
//  * Transforms are decimation-in-frequency networks, natural order in, bit-reversed out, run
//    as 1-3 passes.  Each pass stages a [R strided rows] x [C contiguous words] tile in LDS
//    (up to 128 KiB of the CU's 160 KiB), runs log2(R) butterfly stages there and writes the
//    tile back, so a size-2^22 transform moves each element through HBM twice.
//  * LDE of blow-up 2^a = one inverse DIF (natural -> bit-reversed coefficients), one
//    tiled bit-reversal pass that also applies shift_j^i / N for each of the 2^a cosets, and
//    2^a forward DIFs whose bit-reversed outputs ARE the committed layout: rows [jN,(j+1)N)
//    hold coset shift * w_{2^(n+a)}^{bitrev_a(j)} * H in bit-reversed order.
//  * Twiddles come from one table per direction (w^e, e < 2^(L-1)) kept resident in HBM /
//    Infinity Cache; exponent arithmetic is shifts only.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "lds_barrier.hpp"
#include "zkhip_internal.hpp"

namespace zk {

// ---------------------------------------------------------------------------------------------
__global__ void k_gen_twiddles(uint32_t* fwd, uint32_t* inv, uint32_t w, uint32_t winv, size_t half) {
    size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= half) return;
    fwd[e] = mpow(w, e);
    inv[e] = mpow(winv, e);
}

int ensure_twiddles(zkhip_ctx* ctx, unsigned log_n) {
    if (log_n < 1) log_n = 1;
    if (log_n > 27) return set_error(ctx, ZKHIP_ERR_INVALID, "transform size exceeds two-adicity 27");
    if (ctx->tw_log >= log_n) return ZKHIP_OK;
    // grow generously so mixed sizes share one table
    unsigned want = std::max(log_n, 16u);
    if (ctx->d_tw_fwd) {
        ZK_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ZK_HIP_CHECK(ctx, hipFree(ctx->d_tw_fwd));
        ZK_HIP_CHECK(ctx, hipFree(ctx->d_tw_inv));
        ctx->d_tw_fwd = ctx->d_tw_inv = nullptr;
        ctx->tw_log = 0;
    }
    size_t half = (size_t)1 << (want - 1);
    ZK_HIP_CHECK(ctx, hipMalloc(&ctx->d_tw_fwd, half * sizeof(uint32_t)));
    ZK_HIP_CHECK(ctx, hipMalloc(&ctx->d_tw_inv, half * sizeof(uint32_t)));
    uint32_t w = two_adic_generator(want), winv = minv(w);
    {
        KernelScope ks(ctx, "gen_twiddles");
        unsigned bs = 256;
        hipLaunchKernelGGL(k_gen_twiddles, dim3((unsigned)((half + bs - 1) / bs)), dim3(bs), 0, ctx->stream,
                           ctx->d_tw_fwd, ctx->d_tw_inv, w, winv, half);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ctx->tw_log = want;
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------------
struct PassArgs {
    const uint32_t* src;
    size_t src_stride;
    uint32_t* dst;
    size_t dst_stride;
    const uint32_t* tw;
    unsigned log_m;     // transform size
    unsigned s0;        // first butterfly stage handled by this pass
    unsigned log_r;     // stages in this pass; tile has 2^log_r rows
    unsigned log_c;     // contiguous words per tile row
    unsigned log_sub;   // each matrix column holds 2^log_sub independent transforms back to back
    unsigned tw_shift;  // log2(table size) - log_m
};

// One DIF pass: stages [s0, s0+log_r) of the size-2^log_m network on a tile staged in LDS.
// View the column as [g_hi : 2^s0][r : 2^log_r][low : S], S = 2^(log_m - s0 - log_r); the tile
// covers all r for 2^log_c consecutive values of the flattened outer index u = g_hi*S + low.
__global__ __launch_bounds__(1024) void k_ntt_dif_pass(PassArgs a) {
    extern __shared__ uint32_t lds[];
    const unsigned tid = threadIdx.x, nt = blockDim.x;
    const unsigned log_S = a.log_m - a.s0 - a.log_r;
    const unsigned S_mask = (1u << log_S) - 1u;
    const unsigned C_mask = (1u << a.log_c) - 1u;
    const unsigned total = 1u << (a.log_r + a.log_c);
    const unsigned col = blockIdx.y;
    const unsigned sub = col & ((1u << a.log_sub) - 1u);
    const size_t mcol = col >> a.log_sub;
    const uint32_t* src = a.src + mcol * a.src_stride + ((size_t)sub << a.log_m);
    uint32_t* dst = a.dst + mcol * a.dst_stride + ((size_t)sub << a.log_m);
    const unsigned u0 = blockIdx.x << a.log_c;
    const bool wide = log_S >= a.log_c;  // tile rows are C contiguous words of one g_hi
    size_t base;
    if (wide) {
        base = ((size_t)(u0 >> log_S) << (a.log_r + log_S)) + (u0 & S_mask);
        for (unsigned e = tid; e < total; e += nt) {
            unsigned r = e >> a.log_c, c = e & C_mask;
            lds[e] = src[base + ((size_t)r << log_S) + c];
        }
    } else {
        // the tile is one contiguous run of `total` words covering C/S consecutive g_hi
        base = (size_t)(u0 >> log_S) << (a.log_r + log_S);
        const unsigned grp_mask = (1u << (a.log_r + log_S)) - 1u;
        for (unsigned e = tid; e < total; e += nt) {
            unsigned g = e >> (a.log_r + log_S), rem = e & grp_mask;
            unsigned r = rem >> log_S, low = rem & S_mask;
            lds[(r << a.log_c) + (g << log_S) + low] = src[base + e];
        }
    }
    zk_syncthreads();
    const unsigned low0 = wide ? (u0 & S_mask) : 0u;
    for (unsigned j = 0; j < a.log_r; j++) {
        const unsigned log_half = a.log_r - 1 - j;  // half_r = 2^log_half
        const unsigned half_mask = (1u << log_half) - 1u;
        const unsigned s = a.s0 + j;
        for (unsigned b = tid; b < (total >> 1); b += nt) {
            unsigned c = b & C_mask, pr = b >> a.log_c;
            unsigned off = pr & half_mask, blk = pr >> log_half;
            unsigned ra = (blk << (log_half + 1)) + off;
            unsigned ia = (ra << a.log_c) + c, ib = ia + (1u << (log_half + a.log_c));
            unsigned low = wide ? (low0 + c) : (c & S_mask);
            size_t e = ((((size_t)off << log_S) + low) << s) << a.tw_shift;
            uint32_t w = a.tw[e];
            uint32_t x = lds[ia], y = lds[ib];
            lds[ia] = madd(x, y);
            lds[ib] = mmul(msub(x, y), w);
        }
        zk_syncthreads();
    }
    if (wide) {
        for (unsigned e = tid; e < total; e += nt) {
            unsigned r = e >> a.log_c, c = e & C_mask;
            dst[base + ((size_t)r << log_S) + c] = lds[e];
        }
    } else {
        const unsigned grp_mask = (1u << (a.log_r + log_S)) - 1u;
        for (unsigned e = tid; e < total; e += nt) {
            unsigned g = e >> (a.log_r + log_S), rem = e & grp_mask;
            unsigned r = rem >> log_S, low = rem & S_mask;
            dst[base + e] = lds[(r << a.log_c) + (g << log_S) + low];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Four-step pass for transforms larger than one LDS tile (log_m >= 12).
//
// A size-M transform, M = R1*R2(*R3), is run as 2 (3) passes.  Pass p performs pure size-R_p DFTs
// along one index digit with twiddles of w_{R_p} only (a 4 KiB table in LDS, shared by the 16
// columns of a tile); the inter-digit twiddles w^(k*idx) are applied while the NEXT pass loads its
// operands, where they form a geometric sequence along the 16 registers of a radix-16 unit (two
// table look-ups + 15 products per 16 elements).  Each pass reads a tile of [R rows, strided] x
// [16 contiguous words] (64-byte segments), keeps it in LDS as [row][17] (pad 1: both the row-wise
// butterfly accesses and the column-wise write-out are bank-conflict free), runs radix-16 / radix-8
// butterflies in registers (6 LDS touches per element instead of 4 per radix-2 stage) and writes
// each of its 16 columns as one contiguous run of R words, in the layout the next pass wants
// (digit-transposed), the last pass producing the standard bit-reversed order.
struct Pass4Args {
    const uint32_t* src;
    uint32_t* dst;
    size_t src_col_stride, dst_col_stride;
    const uint32_t* tw;  // w^e, e < 2^(tw_log-1)
    size_t in_x_stride, in_rs;
    size_t out_x_stride, out_hi_stride, out_lo_stride;
    unsigned log_sub, log_m, log_r, log_f, log_lo, tw_log, log_c;
    // input twiddle: element (row r, column F, outer X) *= w_{2^log_tt}^(bitrev(F, log_prev) * (r*tw_a + X*tw_bx))
    int in_tw;
    unsigned log_prev, log_tt;
    uint32_t tw_a, tw_bx;
    // first pass of an LDE's forward transform: read the coefficients where the inverse transform
    // left them (bit-reversed order) and scale coefficient i by shift_sub^i / N on the way in
    int br_src;
    const uint32_t* scale_col;  // [2^log_sub][2^log_f]   N^-1 * s^F
    const uint32_t* scale_row;  // [2^log_sub][2^(log_r-4)] s^(L*j), L = 2^log_f
    const uint32_t* scale_rho;  // [2^log_sub]            s^(L * 2^(log_r-4))
    // optional per-column base pointers (columns of several matrices transformed as one batch): when set they replace
    // src + col * src_col_stride (first pass of a transform) / dst + col * dst_col_stride (last pass)
    const uint32_t* const* src_cols;
    uint32_t* const* dst_cols;
};

template <int Q>
__device__ __forceinline__ void dif_unit(uint32_t (&v)[16], const uint32_t* twl, unsigned j, unsigned log_rq,
                                         unsigned tshift) {
#pragma unroll
    for (int t = 0; t < Q; t++) {
        constexpr int dummy = 0;
        (void)dummy;
        const int half = 1 << (Q - 1 - t);
#pragma unroll
        for (int kl = 0; kl < half; kl++) {
            const uint32_t w = twl[((j + ((unsigned)kl << log_rq)) << t) << tshift];
#pragma unroll
            for (int blk = 0; blk < (1 << t); blk++) {
                const int ka = blk * 2 * half + kl, kb = ka + half;
                const uint32_t x = v[ka], y = v[kb];
                v[ka] = madd(x, y);
                // x - y lies in (-p, p) as a signed word: the signed Montgomery product takes it as it is (no + p),
                // result in (-p, p), one conditional addition at the end
                v[kb] = canon_signed(smml((int32_t)(x - y), (int32_t)w));
            }
        }
    }
}

template <int Q>
__device__ __forceinline__ void lds_round(uint32_t* lv, const uint32_t* twl, unsigned log_r, unsigned log_rcur,
                                          unsigned log_c, unsigned tid, unsigned nt) {
    const unsigned log_rq = log_rcur - Q;               // rows between the registers of a unit
    const unsigned n_units = 1u << (log_r - Q + log_c);  // (R >> Q) * C columns
    const unsigned cmask = (1u << log_c) - 1u, pitch = (1u << log_c) + 1u;
    for (unsigned u = tid; u < n_units; u += nt) {
        const unsigned c = u & cmask, jj = u >> log_c;
        const unsigned j = jj & ((1u << log_rq) - 1u), blk = jj >> log_rq;
        const unsigned row0 = (blk << log_rcur) + j;
        uint32_t v[16];
#pragma unroll
        for (int k = 0; k < (1 << Q); k++) v[k] = lv[(row0 + ((unsigned)k << log_rq)) * pitch + c];
        dif_unit<Q>(v, twl, j, log_rq, log_r - log_rcur);
#pragma unroll
        for (int k = 0; k < (1 << Q); k++) lv[(row0 + ((unsigned)k << log_rq)) * pitch + c] = v[k];
    }
}

// The run-time-shaped pass: the tile shape comes from the arguments.  It serves the passes that no compile-time shape below covers
// (see pass4_kernel_for: no table entry matches), which are the short ones of the two smallest four-step sizes:
//  * 2^12 points, both passes: [2^6 x 16] tiles, 64 lanes;
//  * 2^13 points, second pass: [2^6 x 16] tiles, 64 lanes;
//  * 2^13 points, first pass at ntt_log_lanes = 10: 2^7 rows want 128 columns and the pass has only 2^6 -- [2^7 x 64] tiles, 512 lanes
//    (at 9 / 8 lanes the [2^7 x 64] / [2^7 x 32] tile is a compile-time shape).
// Every pass of 2^14 points and more has at least 2^7 rows and at least as many columns as its tile wants.
__global__ __launch_bounds__(1024) void k_ntt_pass4(Pass4Args a) {
    extern __shared__ uint32_t sm[];
    const unsigned log_r = a.log_r;
    const unsigned R = 1u << log_r;
    const unsigned log_c = a.log_c, C = 1u << log_c, cmask = C - 1u, pitch = C + 1u;
    uint32_t* lv = sm;
    uint32_t* twl = sm + R * pitch;
    const unsigned tid = threadIdx.x, nt = blockDim.x;
    for (unsigned e = tid; e < (R >> 1); e += nt) twl[e] = a.tw[(size_t)e << (a.tw_log - log_r)];
    const unsigned col = blockIdx.y;
    const unsigned sub = col & ((1u << a.log_sub) - 1u);
    const size_t mcol = col >> a.log_sub;
    const uint32_t* src = (a.src_cols ? a.src_cols[mcol] : a.src + mcol * a.src_col_stride) + ((size_t)sub << a.log_m);
    uint32_t* dst = (a.dst_cols ? a.dst_cols[mcol] : a.dst + mcol * a.dst_col_stride) + ((size_t)sub << a.log_m);
    // tile index; with 8-column tiles the two halves of a 64-byte segment group are given to
    // workgroups b and b+8, which the dispatcher places on the same XCD (shared L2) -- speed only
    unsigned tile = blockIdx.x;
    if (log_c == 3 && (gridDim.x & 15u) == 0) {
        const unsigned within = tile & 15u;
        tile = ((((tile >> 4) << 3) + (within & 7u)) << 1) | (within >> 3);
    }
    const unsigned cg_bits = a.log_f - log_c;
    const unsigned X = tile >> cg_bits, F0 = (tile & ((1u << cg_bits) - 1u)) << log_c;
    const size_t in_base = (size_t)X * a.in_x_stride + F0;
    zk_syncthreads();
    // ---- round 1: radix-16 straight from HBM ----
    {
        const unsigned log_rq = log_r - 4;
        for (unsigned u = tid; u < (R >> 4) * C; u += nt) {
            const unsigned c = u & cmask, j = u >> log_c;
            uint32_t v[16];
            if (a.br_src) {
                // rows j + k*2^log_rq of tile column c sit in ONE 64-byte chunk of the bit-reversed
                // coefficient array: run br(F) (2^log_r words), chunk br(j), word br4(k)
                const uint32_t* run = a.src + mcol * a.src_col_stride + ((size_t)bitrev32(F0 + c, a.log_f) << log_r);
                const uint4* ch = reinterpret_cast<const uint4*>(run + ((size_t)bitrev32(j, log_rq) << 4));
                const uint4 q0 = ch[0], q1 = ch[1], q2 = ch[2], q3 = ch[3];
                const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                        q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
                for (int k = 0; k < 16; k++) v[k] = w[((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3)];
                uint32_t t = mmul(a.scale_col[((size_t)sub << a.log_f) + F0 + c], a.scale_row[((size_t)sub << log_rq) + j]);
                const uint32_t rho = a.scale_rho[sub];
                v[0] = mmul(v[0], t);
#pragma unroll
                for (int k = 1; k < 16; k++) {
                    t = mmul(t, rho);
                    v[k] = mmul(v[k], t);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; k++) v[k] = src[in_base + (size_t)(j + ((unsigned)k << log_rq)) * a.in_rs + c];
            }
            if (a.in_tw) {
                const uint32_t mask = (a.log_tt >= 32) ? 0xffffffffu : ((1u << a.log_tt) - 1u);
                const uint32_t kc = bitrev32(F0 + c, a.log_prev);
                const uint32_t e0 = (kc * (j * a.tw_a + X * a.tw_bx)) & mask;
                const uint32_t de = (kc * ((1u << log_rq) * a.tw_a)) & mask;
                const unsigned sh = a.tw_log - a.log_tt;
                const uint32_t half = 1u << (a.log_tt - 1);
                uint32_t t = e0 < half ? a.tw[(size_t)e0 << sh] : mneg(a.tw[(size_t)(e0 - half) << sh]);
                const uint32_t rho = de < half ? a.tw[(size_t)de << sh] : mneg(a.tw[(size_t)(de - half) << sh]);
                v[0] = mmul(v[0], t);
#pragma unroll
                for (int k = 1; k < 16; k++) {
                    t = mmul(t, rho);
                    v[k] = mmul(v[k], t);
                }
            }
            dif_unit<4>(v, twl, j, log_rq, 0);
#pragma unroll
            for (int k = 0; k < 16; k++) lv[(j + ((unsigned)k << log_rq)) * pitch + c] = v[k];
        }
    }
    zk_syncthreads();
    // ---- remaining stages out of LDS ----
    unsigned log_rcur = log_r - 4;
    while (log_rcur > 0) {
        const unsigned q = log_rcur >= 4 ? 4 : log_rcur;
        switch (q) {
            case 4: lds_round<4>(lv, twl, log_r, log_rcur, log_c, tid, nt); break;
            case 3: lds_round<3>(lv, twl, log_r, log_rcur, log_c, tid, nt); break;
            case 2: lds_round<2>(lv, twl, log_r, log_rcur, log_c, tid, nt); break;
            default: lds_round<1>(lv, twl, log_r, log_rcur, log_c, tid, nt); break;
        }
        log_rcur -= q;
        zk_syncthreads();
    }
    // ---- write-out: each tile column is one contiguous run of R words ----
    const unsigned lo_mask = (1u << a.log_lo) - 1u;
    for (unsigned e = tid; e < (R << log_c); e += nt) {
        const unsigned c = e >> log_r, p = e & (R - 1u);
        const unsigned F = F0 + c;
        const size_t o = (size_t)X * a.out_x_stride + (size_t)(F >> a.log_lo) * a.out_hi_stride +
                         (size_t)(F & lo_mask) * a.out_lo_stride + p;
        dst[o] = lv[p * pitch + c];
    }
}

// ---------------------------------------------------------------------------------------------
// Compile-time shaped variant of the pass kernel (first written for the two tile shapes every transform >= 2^20
// uses, [2^11 x 8] and [2^10 x 16] at 1024 lanes; P4_SHAPES lists its instantiations).  Same data flow as k_ntt_pass4 above; what changes
// is the instruction count (1678 VALU instructions per wave before, 1106 now -- profiles/round01_pmc_valu.json --, of
// which only ~900 are butterflies):
//  * every LDS address is one per-lane base plus an immediate, every HBM address is a uniform
//    (scalar) base plus one 32-bit per-lane offset -- no per-element 64-bit multiplies;
//  * the 2^Q - 1 twiddles of a register unit are read from the LDS table before the butterflies
//    start instead of one dependent read per stage;
//  * the write-out is unrolled so that the tile column of each store is a compile-time constant.
// LAST: the unit ends the tile's transform (rows 1 apart, first row 0): the twiddle of its last stage and the first
// twiddle of the stage before are w^0 = 1 -- no product
template <int Q, bool LAST = false>
__device__ __forceinline__ void dif_unit_w(uint32_t (&v)[1 << Q], const uint32_t (&w)[(1 << Q) - 1]) {
#pragma unroll
    for (int t = 0; t < Q; t++) {
        const int half = 1 << (Q - 1 - t);
        const int woff = (1 << Q) - (1 << (Q - t));
#pragma unroll
        for (int kl = 0; kl < half; kl++) {
#pragma unroll
            for (int blk = 0; blk < (1 << t); blk++) {
                const int ka = blk * 2 * half + kl, kb = ka + half;
                const uint32_t x = v[ka], y = v[kb];
                v[ka] = madd(x, y);
                if (LAST && kl == 0)
                    v[kb] = msub(x, y);
                else
                    v[kb] = canon_signed(smml((int32_t)(x - y), (int32_t)w[woff + kl]));
            }
        }
    }
}
// twiddles of the unit whose first row is j (rows j + k * 2^LOG_RQ), table exponent scaled by 2^TSHIFT
template <int Q, int LOG_RQ, int TSHIFT>
__device__ __forceinline__ void load_unit_twiddles(const uint32_t* twl, unsigned j, uint32_t (&w)[(1 << Q) - 1]) {
#pragma unroll
    for (int t = 0; t < Q; t++) {
        const int half = 1 << (Q - 1 - t);
        const int woff = (1 << Q) - (1 << (Q - t));
        const uint32_t* tb = twl + (j << (t + TSHIFT));
#pragma unroll
        for (int kl = 0; kl < half; kl++) w[woff + kl] = tb[kl << (LOG_RQ + t + TSHIFT)];
    }
}
template <int LOG_R, int LOG_C, int LOG_RCUR, unsigned NT = 1024u>
__device__ __forceinline__ void lds_rounds_ct(uint32_t* lv, const uint32_t* twl, unsigned tid) {
    if constexpr (LOG_RCUR > 0) {
        constexpr int Q = LOG_RCUR >= 4 ? 4 : LOG_RCUR;
        constexpr int LOG_RQ = LOG_RCUR - Q;
        constexpr unsigned n_units = 1u << (LOG_R - Q + LOG_C);
        constexpr unsigned pitch = (1u << LOG_C) + 1u;
#pragma unroll
        for (unsigned u0 = 0; u0 < n_units; u0 += NT) {
            const unsigned u = u0 + tid;
            const unsigned c = u & ((1u << LOG_C) - 1u), jj = u >> LOG_C;
            const unsigned j = jj & ((1u << LOG_RQ) - 1u), blk = jj >> LOG_RQ;
            uint32_t* base = lv + ((blk << LOG_RCUR) + j) * pitch + c;
            uint32_t v[1 << Q], w[(1 << Q) - 1];
#pragma unroll
            for (int k = 0; k < (1 << Q); k++) v[k] = base[(k << LOG_RQ) * pitch];
            load_unit_twiddles<Q, LOG_RQ, LOG_R - LOG_RCUR>(twl, j, w);
            dif_unit_w<Q, LOG_RQ == 0>(v, w);
#pragma unroll
            for (int k = 0; k < (1 << Q); k++) base[(k << LOG_RQ) * pitch] = v[k];
        }
        zk_syncthreads();
        lds_rounds_ct<LOG_R, LOG_C, LOG_RCUR - Q, NT>(lv, twl, tid);
    }
}

// LOG_T: log2 of the workgroup's lanes (10; 9 / 8 for the short transforms of proofs with many small chips: a 1024-lane, 70 KiB workgroup waits
// for a quarter of a CU to fall free at once, and beside the other kernels of a guest flow's streams it mostly waits -- docs/round5_b.md)
template <int LOG_R, int LOG_C, int LOG_T = 10>
__global__ __launch_bounds__(1 << LOG_T) void k_ntt_pass4_ct(Pass4Args a) {
    static_assert(LOG_R >= 7 && LOG_R - 4 + LOG_C == LOG_T, "one radix-16 unit per lane in the first round");
    constexpr unsigned NT = 1u << LOG_T;
    extern __shared__ uint32_t sm[];
    constexpr unsigned R = 1u << LOG_R, C = 1u << LOG_C, pitch = C + 1u;
    constexpr int LOG_RQ = LOG_R - 4;
    uint32_t* lv = sm;
    uint32_t* twl = sm + R * pitch;
    const unsigned tid = threadIdx.x;
    for (unsigned e = tid; e < (R >> 1); e += NT) twl[e] = a.tw[(size_t)e << (a.tw_log - LOG_R)];
    const unsigned col = blockIdx.y;
    const unsigned sub = col & ((1u << a.log_sub) - 1u);
    const size_t mcol = col >> a.log_sub;
    unsigned tile = blockIdx.x;
    // XCD-aware tile order: consecutive workgroup ids go round-robin over the 8 XCDs, so workgroups b, b+8, ...,
    // b+8(k-1) share an L2.  They are given k ADJACENT tiles, whose 32-byte row segments are neighbours in the
    // same 128-byte lines and DRAM pages (2^22 x 300 LDE: k = 1 23.7 ms, 2 20.4, 4 19.3, 8 18.6, 16 and 32 18.1).
    if (LOG_C == 3) {
        unsigned k = gridDim.x >> 3;
        if (k > 16u) k = 16u;
        if (k >= 2u && (k & (k - 1u)) == 0 && (gridDim.x & (8u * k - 1u)) == 0) {
            const unsigned within = tile & (8u * k - 1u);
            tile = (tile & ~(8u * k - 1u)) | ((within & 7u) * k) | (within >> 3);
        }
    }
    const unsigned cg_bits = a.log_f - LOG_C;
    const unsigned X = tile >> cg_bits, F0 = (tile & ((1u << cg_bits) - 1u)) << LOG_C;
    zk_syncthreads();
    // ---- round 1: one radix-16 unit per lane straight from HBM ----
    {
        // Which unit a lane takes is free in this round (a unit's rows sit 2^LOG_RQ apart, HBM sees the same
        // 32-byte segments either way), so the rows of one half-wave are placed 8 apart (16 for 16-column tiles):
        // with the odd pitch their LDS stores then hit 32 distinct banks instead of colliding two-way on
        // consecutive rows (profiles/round01_ntt_ablation.txt).
        const unsigned c = tid & (C - 1u), jj = tid >> LOG_C;
        unsigned j = jj;
        if constexpr (LOG_C <= 4 && LOG_C >= 3 && LOG_R - 4 >= (5 - LOG_C) + (LOG_C == 3 ? 3 : 4)) {
            constexpr unsigned HB = 5 - LOG_C;           // unit-index bits inside a half-wave (2 or 1)
            constexpr unsigned SP = LOG_C == 3 ? 3 : 4;  // log2 of the row spacing wanted
            j = ((jj & ((1u << HB) - 1u)) << SP) | ((jj >> HB) & ((1u << SP) - 1u)) | (jj & ~((1u << (HB + SP)) - 1u));
        }
        uint32_t v[16];
        if (a.br_src) {
            const uint32_t* run = a.src + mcol * a.src_col_stride + ((size_t)bitrev32(F0 + c, a.log_f) << LOG_R);
            const uint4* ch = reinterpret_cast<const uint4*>(run + ((size_t)bitrev32(j, LOG_RQ) << 4));
            const uint4 q0 = ch[0], q1 = ch[1], q2 = ch[2], q3 = ch[3];
            const uint32_t wv[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                     q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = wv[((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3)];
            uint32_t t = mmul(a.scale_col[((size_t)sub << a.log_f) + F0 + c], a.scale_row[((size_t)sub << LOG_RQ) + j]);
            const uint32_t rho = a.scale_rho[sub];
            // the running power stays a signed word (|t| < p needs no conditional step between products)
            int32_t ts = (int32_t)t;
            v[0] = mmul(v[0], t);
#pragma unroll
            for (int k = 1; k < 16; k++) {
                ts = smml(ts, (int32_t)rho);
                v[k] = canon_signed(smml((int32_t)v[k], ts));
            }
        } else {
            // uniform base of the tile + one 32-bit lane offset; register k is 2^(LOG_RQ + log_f) words further
            const uint32_t* tile_src = (a.src_cols ? a.src_cols[mcol] : a.src + mcol * a.src_col_stride) + ((size_t)sub << a.log_m) +
                                       (size_t)X * a.in_x_stride + F0;
            const uint32_t lane_off = (j << a.log_f) + c;
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = (tile_src + ((size_t)k << (LOG_RQ + a.log_f)))[lane_off];
        }
        if (a.in_tw) {
            const uint32_t mask = (a.log_tt >= 32) ? 0xffffffffu : ((1u << a.log_tt) - 1u);
            const uint32_t kc = bitrev32(F0 + c, a.log_prev);
            const uint32_t e0 = (kc * (j * a.tw_a + X * a.tw_bx)) & mask;
            const uint32_t de = (kc * ((1u << LOG_RQ) * a.tw_a)) & mask;
            const unsigned sh = a.tw_log - a.log_tt;
            const uint32_t half = 1u << (a.log_tt - 1);
            uint32_t t = e0 < half ? a.tw[(size_t)e0 << sh] : mneg(a.tw[(size_t)(e0 - half) << sh]);
            const uint32_t rho = de < half ? a.tw[(size_t)de << sh] : mneg(a.tw[(size_t)(de - half) << sh]);
            // the running power stays a signed word (|t| < p needs no conditional step between products)
            int32_t ts = (int32_t)t;
            v[0] = mmul(v[0], t);
#pragma unroll
            for (int k = 1; k < 16; k++) {
                ts = smml(ts, (int32_t)rho);
                v[k] = canon_signed(smml((int32_t)v[k], ts));
            }
        }
        uint32_t w[15];
        load_unit_twiddles<4, LOG_RQ, 0>(twl, j, w);
        dif_unit_w<4>(v, w);
        uint32_t* base = lv + j * pitch + c;
#pragma unroll
        for (int k = 0; k < 16; k++) base[(k << LOG_RQ) * pitch] = v[k];
    }
    zk_syncthreads();
    lds_rounds_ct<LOG_R, LOG_C, LOG_RQ, NT>(lv, twl, tid);
    // ---- write-out: each tile column is one contiguous run of R words; the column of every store is
    // a compile-time constant, so its HBM base is scalar and the LDS address an immediate ----
    const unsigned lo_mask = (1u << a.log_lo) - 1u;
    uint32_t* dst = (a.dst_cols ? a.dst_cols[mcol] : a.dst + mcol * a.dst_col_stride) + ((size_t)sub << a.log_m) + (size_t)X * a.out_x_stride;
    if constexpr (LOG_R >= LOG_T) {
        const uint32_t* lrow = lv + tid * pitch;
#pragma unroll
        for (unsigned i = 0; i < (R * C) / NT; i++) {
            const unsigned c = (NT * i) >> LOG_R, p0 = (NT * i) & (R - 1u);
            const unsigned F = F0 + c;
            uint32_t* dcol = dst + (size_t)(F >> a.log_lo) * a.out_hi_stride + (size_t)(F & lo_mask) * a.out_lo_stride + p0;
            dcol[tid] = lrow[p0 * pitch + c];
        }
    } else {
        // short runs: one store instruction covers 1024 / R tile columns, the column is per lane
        const unsigned p = tid & (R - 1u), c_lane = tid >> LOG_R;
        const uint32_t* lrow = lv + p * pitch + c_lane;
#pragma unroll
        for (unsigned i = 0; i < (R * C) / NT; i++) {
            const unsigned F = F0 + c_lane + i * (NT >> LOG_R);
            uint32_t* dcol = dst + (size_t)(F >> a.log_lo) * a.out_hi_stride + (size_t)(F & lo_mask) * a.out_lo_stride + p;
            *dcol = lrow[i * (NT >> LOG_R)];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Shape-specialised pass (round 7; zkhip_config.ntt_pass_form = 0): the passes of a TWO-pass transform whose digits both have SH::LOG_R
// bits -- 2^22 points as [2^11 x 8] tiles, the four passes of the flagship's LDEs.  Same butterflies, same LDS rounds and the same words
// out as k_ntt_pass4_ct; what changes is what a tile's waves wait for and what they issue around the butterflies:
//  * k_ntt_pass4_ct reads HBM in up to five dependent steps -- the twiddle table (wait, LDS store, barrier), the sixteen operands (wait),
//    the input twiddle t behind a divergent branch (wait), its ratio rho behind another (wait) -- and with two workgroups on a CU nothing
//    hides those round trips.  Here every read of the round is issued before the first wait: table entry, t / rho (or the coset scales),
//    then the operands; the barrier that publishes the table comes after the scaling products, where only the butterflies need it.
//    (In this shape the exponents kc * (j + k 2^LOG_RQ) stay below 2^(2 LOG_R - 1): the table's second half, and with it the branch on
//    e0 < half and the negation, is never reached.)
//  * the pass's mode (plain / input twiddle / bit-reversed scaled source) is a template parameter, and log_f, log_lo, log_m, the tile
//    grid, the strides and the twiddle parameters are constants: tile and column bases are scalar shifts, and the write-out's sixteen
//    column bases cost one scalar addition each instead of two 64-bit scalar products.
struct ShapeSq11 {
    static constexpr int LOG_R = 11, LOG_C = 3, LOG_T = 10;
};
enum : int { P4_PLAIN = 0, P4_IN_TW = 1, P4_BR_SRC = 2 };

// v[k] <- v[k] t rho^k, canonical.  t, rho in [0, p); v[k] in [0, p).  Every product is a signed Montgomery product of two words in
// (-p, p): |d| <= p^2 / 2^32 + p / 2 < 0.97 p, so the running power stays in (-p, p) with no conditional step between products; one
// conditional addition brings each scaled operand back to [0, p), which the additions of the first butterfly stage need.
// (The powers as a tree -- rho^2, rho^4, rho^8, dependent depth 4 instead of 15, three products more -- were measured and moved nothing:
// 16.09 against 16.05 ms for the 2^22 x 302 LDE, docs/kernels_2.md round 7.  With eight waves on a SIMD the chain's latency is covered.)
__device__ __forceinline__ void scale_geometric(uint32_t (&v)[16], uint32_t t, uint32_t rho) {
    int32_t ts = (int32_t)t;
    v[0] = canon_signed(smml((int32_t)v[0], ts));
#pragma unroll
    for (int k = 1; k < 16; k++) {
        ts = smml(ts, (int32_t)rho);
        v[k] = canon_signed(smml((int32_t)v[k], ts));
    }
}

// A column base is the same for every lane of the workgroup and points to device memory, whether it is computed from the arguments or
// read from a table of column pointers (which the compiler must take for a generic address: flat loads with a 64-bit address per lane).
// Said so here: the base lives in scalar registers and every access is a global one with a 32-bit lane offset.
typedef __attribute__((address_space(1))) uint32_t* global_words;
__device__ __forceinline__ global_words uniform_global(const uint32_t* p) {
    const uint64_t x = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return (global_words)(((uint64_t)hi << 32) | lo);
}
// (a base per access, each held in scalar registers: without this the compiler folds the sixteen bases of a round into one 64-bit
// vector address and pays two vector additions per access)
__device__ __forceinline__ global_words uniform_global(global_words p) {
    const uint64_t x = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return (global_words)(((uint64_t)hi << 32) | lo);
}

template <class SH, int MODE>
__global__ __launch_bounds__(1 << SH::LOG_T, 8) void k_ntt_pass4_ct_sq(Pass4Args a) {
    constexpr int LOG_R = SH::LOG_R, LOG_C = SH::LOG_C, LOG_T = SH::LOG_T;
    constexpr int LOG_F = LOG_R, LOG_M = 2 * LOG_R, LOG_RQ = LOG_R - 4;
    constexpr unsigned NT = 1u << LOG_T, R = 1u << LOG_R, C = 1u << LOG_C, pitch = C + 1u;
    static_assert(LOG_C == 3 && LOG_RQ + LOG_C == LOG_T && LOG_R >= LOG_T && (R >> 1) % NT == 0 && LOG_F - LOG_C >= 7, "[2^11 x 8] tiles of 1024 lanes");
    extern __shared__ uint32_t sm[];
    uint32_t* lv = sm;
    uint32_t* twl = sm + R * pitch;
    const unsigned tid = threadIdx.x;
    const unsigned col = blockIdx.y;
    const unsigned sub = col & ((1u << a.log_sub) - 1u);
    const size_t mcol = col >> a.log_sub;
    // XCD-aware tile order of k_ntt_pass4_ct for a grid of 2^(LOG_F - LOG_C) >= 128 tiles: groups of 128, 16 adjacent tiles per XCD
    unsigned tile = blockIdx.x;
    tile = (tile & ~127u) | ((tile & 7u) << 4) | ((tile & 127u) >> 3);
    const unsigned F0 = tile << LOG_C;
    const unsigned c = tid & (C - 1u), jj = tid >> LOG_C;
    // (bank-friendly unit order: as k_ntt_pass4_ct)
    const unsigned j = ((jj & 3u) << 3) | ((jj >> 2) & 7u) | (jj & ~31u);
    // ---- every HBM read of the first round, before the first wait ----
    uint32_t twe[(R >> 1) / NT];
#pragma unroll
    for (unsigned i = 0; i < (R >> 1) / NT; i++) twe[i] = a.tw[(size_t)(tid + i * NT) << (a.tw_log - LOG_R)];
    uint32_t t = 0, rho = 0, v[16];
    if constexpr (MODE == P4_BR_SRC) {
        // rows j + k 2^LOG_RQ of tile column c sit in ONE 64-byte chunk of the bit-reversed coefficient array (as k_ntt_pass4_ct)
        const uint32_t sc = a.scale_col[((size_t)sub << LOG_F) + F0 + c], sr = a.scale_row[((size_t)sub << LOG_RQ) + j];
        rho = a.scale_rho[sub];
        const uint32_t* run = a.src + mcol * a.src_col_stride + ((size_t)bitrev32(F0 + c, LOG_F) << LOG_R);
        const uint4* ch = reinterpret_cast<const uint4*>(run + ((size_t)bitrev32(j, LOG_RQ) << 4));
        const uint4 q0 = ch[0], q1 = ch[1], q2 = ch[2], q3 = ch[3];
        const uint32_t wv[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = wv[((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3)];
        t = mmul(sc, sr);
    } else {
        if constexpr (MODE == P4_IN_TW) {
            // element (row r, column F) *= w_M^(bitrev(F) r), r = j + k 2^LOG_RQ: exponents kc j + k (kc 2^LOG_RQ) < 2^(LOG_M - 1)
            const uint32_t kc = bitrev32(F0 + c, LOG_F);
            const unsigned sh = a.tw_log - LOG_M;
            t = a.tw[(size_t)(kc * j) << sh];
            rho = a.tw[(size_t)(kc << LOG_RQ) << sh];
        }
        const global_words tile_src = uniform_global((a.src_cols ? a.src_cols[mcol] : a.src + mcol * a.src_col_stride) + ((size_t)sub << LOG_M) + F0);
        const uint32_t lane_off = (j << LOG_F) + c;
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = uniform_global(tile_src + ((size_t)k << (LOG_RQ + LOG_F)))[lane_off];
    }
#pragma unroll
    for (unsigned i = 0; i < (R >> 1) / NT; i++) twl[tid + i * NT] = twe[i];
    if constexpr (MODE != P4_PLAIN) scale_geometric(v, t, rho);
    zk_syncthreads();   // (the twiddle table)
    {
        uint32_t w[15];
        load_unit_twiddles<4, LOG_RQ, 0>(twl, j, w);
        dif_unit_w<4>(v, w);
        uint32_t* base = lv + j * pitch + c;
#pragma unroll
        for (int k = 0; k < 16; k++) base[(k << LOG_RQ) * pitch] = v[k];
    }
    zk_syncthreads();
    lds_rounds_ct<LOG_R, LOG_C, LOG_RQ, NT>(lv, twl, tid);
    // ---- write-out: tile column cc is one contiguous run of R words at [F0 + cc][p] ----
    const global_words dst = uniform_global((a.dst_cols ? a.dst_cols[mcol] : a.dst + mcol * a.dst_col_stride) + ((size_t)sub << LOG_M) + ((size_t)F0 << LOG_R));
    const uint32_t* lrow = lv + tid * pitch;
#pragma unroll
    for (unsigned i = 0; i < (R * C) / NT; i++) {
        const unsigned cc = (NT * i) >> LOG_R, p0 = (NT * i) & (R - 1u);
        uniform_global(dst + ((size_t)cc << LOG_R) + p0)[tid] = lrow[p0 * pitch + cc];
    }
}

// ---------------------------------------------------------------------------------------------
// The LDE's middle, fused (round 6). A coset LDE of 2^(2 LOG_R) points was four passes over HBM: inverse pass 1, inverse pass 2
// (coefficients, bit-reversed, written to scratch), then per coset forward pass 1 (which read those coefficients back, once per coset)
// and forward pass 2 -- 12 N words moved for N read and 2 N written.  The inverse's last pass leaves in its LDS tile, per tile column
// p1, ALL coefficients whose bit-reversed index begins with p1 -- exactly one column F = bitrev(p1) of the forward transform's first pass
// (which transforms along the other digit, column by column).  So the tile stays where it is: every lane takes its radix-16 unit's sixteen
// coefficients out of the tile into registers (they sit in one 16-row chunk, bit-reversed -- the layout forward pass 1 reads from HBM
// today), and for each coset scales them by s_c^i / N, runs the forward pass's rounds over the same LDS and writes the column out in the
// layout forward pass 2 expects.  The coefficient array is never written or read: 9 N words instead of 12 N, one launch fewer.
// Only for transforms whose two passes have the same number of stages (LOG_R = 11: 2^22 points).
// MEASURED (round 6, profiles/round06_lde_fused.txt; 2^22 x 302 columns, blow-up 2, one stream): the four-pass form takes 6.81 ms (inverse) +
// 12.93 ms (forward) = 19.74 ms; this form 3.00 (inverse pass 1) + 9.93 (fused) + 6.98 (forward pass 2) = 19.91 ms with two workgroups per
// CU, 20.9 ms with one (ZKHIP_LDE_FUSED_WAVES=4).  A quarter of the HBM traffic is gone and the time is the same: the fused kernel costs
// what the two passes it replaces cost together (3.4 + 6.0 ms), although it drops a tile load per coset and a tile store -- the passes are
// not waiting for HBM.  They are bound by what a tile's sixteen waves execute between barriers (1.1 k VALU instructions per wave at 3.0
// cycles each on the kernel's own mix, ~500 SALU, 77 LDS instructions: ~14 k of the ~25 k cycles a CU spends per tile are VALU issue), so
// neither this nor an LDS-DMA double buffer -- which could only hide the same loads -- moves them.  OFF by default (no gain, one more code
// path); ZKHIP_LDE_FUSED=1 selects it, tests/test_gpu_config_forms.py keeps it bit-exact.
struct LdeFusedArgs {
    const uint32_t* src;        // inverse pass 1's output, [d2][p1] per column
    size_t src_col_stride;
    uint32_t* dst;              // forward pass 1's output, per column 2^log_cosets blocks of [F][p]
    size_t dst_col_stride;
    const uint32_t *tw_inv, *tw_fwd;
    unsigned tw_log, log_m, log_cosets;
    const uint32_t *scale_col, *scale_row, *scale_rho;   // lde_scale_tables
};
// MIN_WAVES: waves per SIMD the register allocation must leave room for (8 = two workgroups per CU, 64 VGPRs, the sixteen kept coefficients
// partly in scratch; 4 = one workgroup per CU, no spill) -- ZKHIP_LDE_FUSED_WAVES picks the instantiation for measurements
template <int LOG_R, int LOG_C, int MIN_WAVES>
__global__ __launch_bounds__(1024, MIN_WAVES) void k_ntt_lde_fused(LdeFusedArgs a) {
    constexpr int LOG_T = 10;
    static_assert(LOG_R - 4 + LOG_C == LOG_T, "one radix-16 unit per lane");
    constexpr unsigned NT = 1u << LOG_T;
    extern __shared__ uint32_t sm[];
    constexpr unsigned R = 1u << LOG_R, C = 1u << LOG_C, pitch = C + 1u;
    constexpr int LOG_RQ = LOG_R - 4;
    constexpr unsigned log_f = LOG_R;   // both digits have LOG_R bits
    uint32_t* lv = sm;
    uint32_t* twl = sm + R * pitch;
    const unsigned tid = threadIdx.x;
    for (unsigned e = tid; e < (R >> 1); e += NT) twl[e] = a.tw_inv[(size_t)e << (a.tw_log - LOG_R)];
    const size_t mcol = blockIdx.y;
    unsigned tile = blockIdx.x;
    if (LOG_C == 3) {   // (XCD-aware tile order: as k_ntt_pass4_ct)
        unsigned k = gridDim.x >> 3;
        if (k > 16u) k = 16u;
        if (k >= 2u && (k & (k - 1u)) == 0 && (gridDim.x & (8u * k - 1u)) == 0) {
            const unsigned within = tile & (8u * k - 1u);
            tile = (tile & ~(8u * k - 1u)) | ((within & 7u) * k) | (within >> 3);
        }
    }
    const unsigned F0 = tile << LOG_C;   // (two passes: the tile index is the column group)
    const unsigned c = tid & (C - 1u), jj = tid >> LOG_C;
    unsigned j = jj;
    if constexpr (LOG_C <= 4 && LOG_C >= 3 && LOG_R - 4 >= (5 - LOG_C) + (LOG_C == 3 ? 3 : 4)) {   // (bank-friendly unit order: as k_ntt_pass4_ct)
        constexpr unsigned HB = 5 - LOG_C;
        constexpr unsigned SP = LOG_C == 3 ? 3 : 4;
        j = ((jj & ((1u << HB) - 1u)) << SP) | ((jj >> HB) & ((1u << SP) - 1u)) | (jj & ~((1u << (HB + SP)) - 1u));
    }
    zk_syncthreads();
    // ---- the inverse transform's second pass: rows d2, columns p1 = F0 + c, twiddle w_M^-(bitrev(p1) d2) on the way in ----
    {
        uint32_t v[16];
        const uint32_t* tile_src = a.src + mcol * a.src_col_stride + F0;
        const uint32_t lane_off = (j << log_f) + c;
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = (tile_src + ((size_t)k << (LOG_RQ + log_f)))[lane_off];
        {
            const unsigned log_tt = 2 * LOG_R;
            const uint32_t mask = (1u << log_tt) - 1u;
            const uint32_t kc = bitrev32(F0 + c, LOG_R);
            const uint32_t e0 = (kc * j) & mask;
            const uint32_t de = (kc * (1u << LOG_RQ)) & mask;
            const unsigned sh = a.tw_log - log_tt;
            const uint32_t half = 1u << (log_tt - 1);
            uint32_t t = e0 < half ? a.tw_inv[(size_t)e0 << sh] : mneg(a.tw_inv[(size_t)(e0 - half) << sh]);
            const uint32_t rho = de < half ? a.tw_inv[(size_t)de << sh] : mneg(a.tw_inv[(size_t)(de - half) << sh]);
            int32_t ts = (int32_t)t;
            v[0] = mmul(v[0], t);
#pragma unroll
            for (int k = 1; k < 16; k++) {
                ts = smml(ts, (int32_t)rho);
                v[k] = canon_signed(smml((int32_t)v[k], ts));
            }
        }
        uint32_t w[15];
        load_unit_twiddles<4, LOG_RQ, 0>(twl, j, w);
        dif_unit_w<4>(v, w);
        uint32_t* base = lv + j * pitch + c;
#pragma unroll
        for (int k = 0; k < 16; k++) base[(k << LOG_RQ) * pitch] = v[k];
    }
    zk_syncthreads();
    lds_rounds_ct<LOG_R, LOG_C, LOG_RQ, NT>(lv, twl, tid);
    // (the tile now holds, in row p2 of column c, the coefficient with bit-reversed index (F0 + c) 2^LOG_R + p2, not yet divided by N)
    // ---- the forward transform's first pass, per coset, out of the same tile ----
    for (unsigned e = tid; e < (R >> 1); e += NT) twl[e] = a.tw_fwd[(size_t)e << (a.tw_log - LOG_R)];
    uint32_t raw[16];
    {
        // the unit of forward column F = bitrev(F0 + c) with first row j takes coefficients d1 = j + k 2^LOG_RQ: tile rows bitrev(d1) =
        // 16 bitrev(j) + bitrev4(k)
        const uint32_t* chunk = lv + ((size_t)bitrev32(j, LOG_RQ) << 4) * pitch + c;
#pragma unroll
        for (int k = 0; k < 16; k++) raw[k] = chunk[(((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | ((k & 8) >> 3)) * pitch];
    }
    zk_syncthreads();
    const unsigned Ff = bitrev32(F0 + c, log_f);
    for (unsigned sub = 0; sub < (1u << a.log_cosets); sub++) {
        {
            uint32_t v[16];
            const uint32_t t = mmul(a.scale_col[((size_t)sub << log_f) + Ff], a.scale_row[((size_t)sub << LOG_RQ) + j]);
            const uint32_t rho = a.scale_rho[sub];
            int32_t ts = (int32_t)t;
            v[0] = mmul(raw[0], t);
#pragma unroll
            for (int k = 1; k < 16; k++) {
                ts = smml(ts, (int32_t)rho);
                v[k] = canon_signed(smml((int32_t)raw[k], ts));
            }
            uint32_t w[15];
            load_unit_twiddles<4, LOG_RQ, 0>(twl, j, w);
            dif_unit_w<4>(v, w);
            uint32_t* base = lv + j * pitch + c;
#pragma unroll
            for (int k = 0; k < 16; k++) base[(k << LOG_RQ) * pitch] = v[k];
        }
        zk_syncthreads();
        lds_rounds_ct<LOG_R, LOG_C, LOG_RQ, NT>(lv, twl, tid);
        // write-out: tile column cc is forward column bitrev(F0 + cc): one contiguous run of R words at [F][p] of this coset's block
        uint32_t* dst = a.dst + mcol * a.dst_col_stride + ((size_t)sub << a.log_m);
        if constexpr (LOG_R >= LOG_T) {
            const uint32_t* lrow = lv + tid * pitch;
#pragma unroll
            for (unsigned i = 0; i < (R * C) / NT; i++) {
                const unsigned cc = (NT * i) >> LOG_R, p0 = (NT * i) & (R - 1u);
                const unsigned F = bitrev32(F0 + cc, log_f);
                uint32_t* dcol = dst + ((size_t)F << LOG_R) + p0;
                dcol[tid] = lrow[p0 * pitch + cc];
            }
        }
        zk_syncthreads();   // (the next coset's units overwrite the tile)
    }
}

// Stages per pass: 11 = two passes up to 2^22 points ([2^11 x 8] tiles of 70 KiB, two workgroups per CU).  At most three passes exist
// (fourstep_split writes a[0..2]) and 3 x 11 covers the field's two-adicity of 27, so a smaller limit must never be set: one below 9 once
// made 2^22-point transforms silently wrong (docs/kernels_2.md; a limit of 9 or 10 was measured there too and is slower).
static constexpr unsigned MAX_LOG_R = 11;
static constexpr unsigned P4_MIN_LOG_M = 12;

// the coset scale tables of an LDE's forward transform (lde_scale_tables), for a first pass that reads bit-reversed coefficients
struct BrSrc {
    const uint32_t *scale_col, *scale_row, *scale_rho;
};
// stage split of the four-step passes
static unsigned fourstep_split(unsigned log_n, unsigned a[3]) {
    const unsigned n_pass = std::max(2u, (log_n + MAX_LOG_R - 1) / MAX_LOG_R);
    a[0] = a[1] = a[2] = 0;
    for (unsigned p = 0; p < n_pass; p++) a[p] = log_n / n_pass + (p < log_n % n_pass ? 1 : 0);
    return n_pass;
}
// The passes' scratch (slot 4): `words` words for the passes to write their intermediate to, and as many again behind them for the
// three-pass sizes (log_n > 2 * MAX_LOG_R), whose middle pass cannot write where it reads.
static int pass_scratch(zkhip_ctx* ctx, unsigned log_n, size_t words, uint32_t** t1, uint32_t** t2) {
    const bool three = log_n > 2 * MAX_LOG_R;
    void* tmp;
    ZK_TRY(get_scratch(ctx, 4, words * 4 * (three ? 2 : 1), &tmp));
    *t1 = (uint32_t*)tmp;
    *t2 = three ? *t1 + words : nullptr;
    return ZKHIP_OK;
}

// Every compile-time tile shape of k_ntt_pass4_ct: 2^log_r rows x 2^log_c columns for a workgroup of 2^log_t lanes, one radix-16 unit per
// lane (log_r - 4 + log_c == log_t).  The dispatcher launches from this table and sets the kernels' LDS attribute from it.
typedef void (*Pass4Kernel)(Pass4Args);
struct Pass4Shape {
    unsigned log_r, log_c, log_t;
    Pass4Kernel kernel;
};
#define ZK_P4_CT(R_, C_, T_) {R_, C_, T_, k_ntt_pass4_ct<R_, C_, T_>}
static const Pass4Shape P4_SHAPES[] = {
    ZK_P4_CT(11, 3, 10), ZK_P4_CT(10, 4, 10), ZK_P4_CT(9, 5, 10), ZK_P4_CT(8, 6, 10), ZK_P4_CT(7, 7, 10),  // 2^14 words, 70 KiB
    ZK_P4_CT(10, 3, 9),  ZK_P4_CT(9, 4, 9),   ZK_P4_CT(8, 5, 9),  ZK_P4_CT(7, 6, 9),                       // 2^13 words, 37 KiB
    ZK_P4_CT(10, 2, 8),  ZK_P4_CT(9, 3, 8),   ZK_P4_CT(8, 4, 8),  ZK_P4_CT(7, 5, 8),                       // 2^12 words, 18 KiB
};
#undef ZK_P4_CT
// the shape-specialised form by pass mode (P4_PLAIN, P4_IN_TW, P4_BR_SRC)
static const Pass4Kernel P4_SQ11[3] = {k_ntt_pass4_ct_sq<ShapeSq11, P4_PLAIN>, k_ntt_pass4_ct_sq<ShapeSq11, P4_IN_TW>,
                                       k_ntt_pass4_ct_sq<ShapeSq11, P4_BR_SRC>};
// The passes of the two-pass 2^22-point transform may run in their shape-specialised form (zkhip_config.ntt_pass_form = 0): everything
// k_ntt_pass4_ct_sq<ShapeSq11, MODE> holds as a constant is checked here.
static bool pass4_is_sq11(const Pass4Args& pa, unsigned n_pass, unsigned n_x, unsigned log_n) {
    return n_pass == 2 && n_x == 1 && log_n == 22 && pa.log_r == 11 && pa.log_f == 11 && pa.log_c == 3 && pa.log_lo == 0 && pa.in_x_stride == 0 &&
           pa.out_x_stride == 0 && pa.out_hi_stride == ((size_t)1 << 11) && !(pa.br_src && pa.in_tw) &&
           (!pa.in_tw || (pa.log_prev == 11 && pa.log_tt == 22 && pa.tw_a == 1 && pa.tw_bx == 0));
}
// The kernel of a pass whose tile shape (pa.log_r, pa.log_c, log_t) is settled: the specialised form, else the table, else the
// run-time-shaped kernel (k_ntt_pass4's header lists what reaches it).
static Pass4Kernel pass4_kernel_for(const Pass4Args& pa, unsigned log_t, int pass_form, unsigned n_pass, unsigned n_x, unsigned log_n) {
    if (pass_form == 0 && pass4_is_sq11(pa, n_pass, n_x, log_n)) return P4_SQ11[pa.br_src ? P4_BR_SRC : pa.in_tw ? P4_IN_TW : P4_PLAIN];
    for (const Pass4Shape& sh : P4_SHAPES)
        if (sh.log_r == pa.log_r && sh.log_c == pa.log_c && sh.log_t == log_t) return sh.kernel;
    return k_ntt_pass4;
}

// src -> dst through tmp (and tmp2 for 3-pass sizes); dst may alias src.  Buffers hold `width`
// columns of 2^log_sub transforms each, with the given column strides.
static int ntt_dif_fourstep(zkhip_ctx* ctx, const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride,
                            uint32_t* tmp, uint32_t* tmp2, size_t tmp_stride, unsigned log_n, size_t width,
                            unsigned log_sub, bool inverse, const BrSrc* brsrc = nullptr,
                            const uint32_t* const* src_cols = nullptr, uint32_t* const* dst_cols = nullptr) {
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        const int lds_max = ((17u << MAX_LOG_R) + (1u << (MAX_LOG_R - 1))) * 4;
        for (const Pass4Shape& sh : P4_SHAPES) ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)sh.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        for (Pass4Kernel k : P4_SQ11) ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_ntt_pass4, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
        attr_set.mark(ctx->device);
    }
    unsigned a[3];
    const unsigned n_pass = fourstep_split(log_n, a);
    const uint32_t* tw = inverse ? ctx->d_tw_inv : ctx->d_tw_fwd;
    auto launch = [&](Pass4Args& pa, const uint32_t* s, size_t ss, uint32_t* d, size_t ds, unsigned n_x) -> int {
        pa.src = s;
        pa.src_col_stride = ss;
        pa.dst = d;
        pa.dst_col_stride = ds;
        pa.tw = tw;
        pa.tw_log = ctx->tw_log;
        pa.log_sub = log_sub;
        pa.log_m = log_n;
        const unsigned R = 1u << pa.log_r;
        // tiles of 2^14 words (one radix-16 unit per lane): [2^11 x 8] (70 KiB of LDS, two workgroups per CU so one loads while the other
        // computes: measured 20 % faster than one 139 KiB / 16-column workgroup per CU), [2^10 x 16], and for the short passes of
        // three-pass sizes [2^9 x 32], [2^8 x 64], [2^7 x 128]; below 2^7 rows 16 columns (64-byte segments)
        pa.log_c = pa.log_r >= 11 ? 3u : (pa.log_r >= 7 ? 14u - pa.log_r : 4u);
        // workgroups of 2^log_t lanes for the passes of at most 2^10 rows (zkhip_config.ntt_log_lanes: 10 = the 1024-lane tiles above; 9 / 8 =
        // tiles of 2^13 / 2^12 words, 37 / 18 KiB of LDS, four / eight workgroups per CU)
        unsigned log_t = 10;
        if (pa.log_r >= 7 && pa.log_r <= 10 && ctx->cfg.ntt_log_lanes >= 8 && ctx->cfg.ntt_log_lanes <= 9) {
            const unsigned lc = ctx->cfg.ntt_log_lanes + 4 - pa.log_r;
            if (lc >= 2 && lc <= pa.log_f) log_t = ctx->cfg.ntt_log_lanes, pa.log_c = lc;
        }
        if (pa.log_c > pa.log_f) pa.log_c = pa.log_f;
        const unsigned C = 1u << pa.log_c;
        // one lane per radix-16 unit: 2^log_t for a table shape; the run-time-shaped kernel takes any count
        const unsigned threads = std::min(1024u, std::max(64u, (R >> 4) * C));
        const size_t lds = ((size_t)R * (C + 1) + (R >> 1)) * 4;
        dim3 grid(n_x << (pa.log_f - pa.log_c), (unsigned)(width << log_sub));
        KernelScope ks(ctx, inverse ? "ntt_pass_inv" : "ntt_pass_fwd");
        hipLaunchKernelGGL(pass4_kernel_for(pa, log_t, ctx->cfg.ntt_pass_form, n_pass, n_x, log_n), grid, dim3(threads), lds, ctx->stream, pa);
        ZK_HIP_CHECK(ctx, hipGetLastError());
        return ZKHIP_OK;
    };
    Pass4Args pa;
    memset(&pa, 0, sizeof pa);
    auto first_pass_src = [&]() {
        if (brsrc) {
            pa.br_src = 1;
            pa.scale_col = brsrc->scale_col, pa.scale_row = brsrc->scale_row, pa.scale_rho = brsrc->scale_rho;
        }
    };
    if (n_pass == 2) {
        const unsigned a1 = a[0], a2 = a[1];
        // pass 1: digit d1 (rows), F = d2
        pa.log_r = a1, pa.log_f = a2, pa.in_x_stride = 0, pa.in_rs = (size_t)1 << a2;
        pa.out_x_stride = 0, pa.out_hi_stride = (size_t)1 << a1, pa.out_lo_stride = 0, pa.log_lo = 0, pa.in_tw = 0;
        first_pass_src();
        pa.src_cols = src_cols;
        ZK_TRY(launch(pa, src, src_stride, tmp, tmp_stride, 1));
        pa.src_cols = nullptr, pa.dst_cols = nullptr;
        pa.br_src = 0;
        // pass 2: digit d2 (rows), F = p1; twiddle w_M^(k1 * d2)
        pa.log_r = a2, pa.log_f = a1, pa.in_rs = (size_t)1 << a1, pa.out_hi_stride = (size_t)1 << a2;
        pa.in_tw = 1, pa.log_prev = a1, pa.log_tt = log_n, pa.tw_a = 1, pa.tw_bx = 0;
        pa.dst_cols = dst_cols;
        ZK_TRY(launch(pa, tmp, tmp_stride, dst, dst_stride, 1));
        pa.src_cols = nullptr, pa.dst_cols = nullptr;
    } else {
        const unsigned a1 = a[0], a2 = a[1], a3 = a[2];
        // pass 1: rows d1, F = (d2,d3) flat; out (d3, d2, p1)
        pa.log_r = a1, pa.log_f = a2 + a3, pa.in_x_stride = 0, pa.in_rs = (size_t)1 << (a2 + a3);
        pa.out_x_stride = 0, pa.log_lo = a3, pa.out_lo_stride = (size_t)1 << (a1 + a2), pa.out_hi_stride = (size_t)1 << a1;
        pa.in_tw = 0;
        first_pass_src();
        pa.src_cols = src_cols;
        ZK_TRY(launch(pa, src, src_stride, tmp, tmp_stride, 1));
        pa.src_cols = nullptr, pa.dst_cols = nullptr;
        pa.br_src = 0;
        // pass 2: X = d3, rows d2, F = p1; twiddle w_M^(k1 * (d2*R3 + d3)); out (p1, d3, p2)
        pa.log_r = a2, pa.log_f = a1, pa.in_x_stride = (size_t)1 << (a1 + a2), pa.in_rs = (size_t)1 << a1;
        pa.out_x_stride = (size_t)1 << a2, pa.log_lo = 0, pa.out_lo_stride = 0, pa.out_hi_stride = (size_t)1 << (a2 + a3);
        pa.in_tw = 1, pa.log_prev = a1, pa.log_tt = log_n, pa.tw_a = 1u << a3, pa.tw_bx = 1;
        ZK_TRY(launch(pa, tmp, tmp_stride, tmp2, tmp_stride, 1u << a3));
        // pass 3: X = p1, rows d3, F = p2; twiddle w_{R2R3}^(k2 * d3); out (p1, p2, q3)
        pa.log_r = a3, pa.log_f = a2, pa.in_x_stride = (size_t)1 << (a2 + a3), pa.in_rs = (size_t)1 << a2;
        pa.out_x_stride = (size_t)1 << (a2 + a3), pa.out_hi_stride = (size_t)1 << a3;
        pa.in_tw = 1, pa.log_prev = a2, pa.log_tt = a2 + a3, pa.tw_a = 1, pa.tw_bx = 0;
        pa.dst_cols = dst_cols;
        ZK_TRY(launch(pa, tmp2, tmp_stride, dst, dst_stride, 1u << a1));
        pa.src_cols = nullptr, pa.dst_cols = nullptr;
    }
    return ZKHIP_OK;
}

static constexpr unsigned MAX_LOG_TILE = 15;   // 2^15 words = 128 KiB of LDS
static constexpr unsigned MAX_LOG_C = 7;

int ntt_dif_inplace(zkhip_ctx* ctx, const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride,
                    unsigned log_n, size_t width, unsigned log_sub, bool inverse) {
    if (width == 0) return ZKHIP_OK;
    ZK_TRY(ensure_twiddles(ctx, log_n));
    if (log_n >= P4_MIN_LOG_M && ctx->cfg.ntt_pass_form != 2) {
        const size_t per_col = (size_t)1 << (log_n + log_sub);
        uint32_t *t1, *t2;
        ZK_TRY(pass_scratch(ctx, log_n, per_col * width, &t1, &t2));
        return ntt_dif_fourstep(ctx, src, src_stride, dst, dst_stride, t1, t2, per_col, log_n, width, log_sub, inverse);
    }
    if (log_n == 0) {
        if (src != dst) {
            // height-1 columns: plain strided copy
            ZK_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dst_stride * 4, src, src_stride * 4, 4u << log_sub, width,
                                               hipMemcpyDeviceToDevice, ctx->stream));
        }
        return ZKHIP_OK;
    }
    static DeviceOnce attr_set;
    if (attr_set.need(ctx->device)) {
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_ntt_dif_pass,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 4 << MAX_LOG_TILE));
        attr_set.mark(ctx->device);
    }
    unsigned n_pass = (log_n + MAX_LOG_R - 1) / MAX_LOG_R;
    unsigned base = log_n / n_pass, rem = log_n % n_pass;
    unsigned s0 = 0;
    for (unsigned p = 0; p < n_pass; p++) {
        PassArgs a;
        a.src = (p == 0) ? src : dst;
        a.src_stride = (p == 0) ? src_stride : dst_stride;
        a.dst = dst;
        a.dst_stride = dst_stride;
        a.tw = inverse ? ctx->d_tw_inv : ctx->d_tw_fwd;
        a.log_m = log_n;
        a.s0 = s0;
        a.log_r = base + (p < rem ? 1 : 0);
        unsigned log_outer = log_n - a.log_r;  // log2 of the number of flattened outer indices
        a.log_c = std::min({MAX_LOG_TILE - a.log_r, MAX_LOG_C, log_outer});
        a.log_sub = log_sub;
        a.tw_shift = ctx->tw_log - log_n;
        unsigned total = 1u << (a.log_r + a.log_c);
        unsigned threads = std::max(64u, std::min(1024u, total >> 1));
        dim3 grid(1u << (log_outer - a.log_c), (unsigned)(width << log_sub));
        {
            KernelScope ks(ctx, inverse ? "ntt_dif_pass_inv" : "ntt_dif_pass_fwd");
            hipLaunchKernelGGL(k_ntt_dif_pass, grid, dim3(threads), total * sizeof(uint32_t), ctx->stream, a);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
        s0 += a.log_r;
    }
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// Bit-reversal permutation through 32x32 LDS tiles (128-byte segments on both sides), fused
// with the per-coset coefficient scaling of the LDE.  src holds n-point data with
// src[p] = v[bitrev(p)]; dst coset j receives v[i] * hi_j[i >> lb] * lo_j[i & (2^lb - 1)].
struct BitrevArgs {
    const uint32_t* src;
    size_t src_stride;
    uint32_t* dst;
    size_t dst_stride;
    const uint32_t* pw;  // per coset: lo[2^lb] then hi[2^(log_n-lb)]; nullptr -> multiply by `uniform`
    uint32_t uniform;    // Montgomery scalar used when pw == nullptr (MONTY_ONE = plain permutation)
    unsigned log_n;
    unsigned log_cosets;
    unsigned lb;
};

__device__ __forceinline__ uint32_t scale_for(const BitrevArgs& a, unsigned coset, unsigned i) {
    if (a.pw == nullptr) return a.uniform;
    const uint32_t* t = a.pw + (size_t)coset * ((1u << a.lb) + (1u << (a.log_n - a.lb)));
    return mmul(t[i & ((1u << a.lb) - 1u)], t[(1u << a.lb) + (i >> a.lb)]);
}

__global__ __launch_bounds__(256) void k_bitrev_scale_tiled(BitrevArgs a) {
    __shared__ uint32_t tile[32][33];
    const unsigned tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;  // 32 x 8
    const unsigned mid = blockIdx.x, log_mid = a.log_n - 10;
    const uint32_t* src = a.src + (size_t)blockIdx.y * a.src_stride;
#pragma unroll
    for (unsigned rr = 0; rr < 4; rr++) {
        unsigned hi5 = ty + 8 * rr;
        tile[hi5][tx] = src[((size_t)hi5 << (a.log_n - 5)) + ((size_t)mid << 5) + tx];
    }
    zk_syncthreads();
    const unsigned brmid = bitrev32(mid, log_mid);
#pragma unroll
    for (unsigned rr = 0; rr < 4; rr++) {
        unsigned B = ty + 8 * rr, A = tx;  // output index i = B*2^(n-5) + brmid*32 + A
        uint32_t v = tile[bitrev32(A, 5)][bitrev32(B, 5)];
        unsigned i = (B << (a.log_n - 5)) + (brmid << 5) + A;
        for (unsigned j = 0; j < (1u << a.log_cosets); j++) {
            uint32_t* dst = a.dst + (size_t)blockIdx.y * a.dst_stride + ((size_t)j << a.log_n);
            dst[i] = mmul(v, scale_for(a, j, i));
        }
    }
}

__global__ void k_bitrev_scale_small(BitrevArgs a) {
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << a.log_n)) return;
    const uint32_t* src = a.src + (size_t)blockIdx.y * a.src_stride;
    uint32_t v = src[bitrev32(i, a.log_n)];
    for (unsigned j = 0; j < (1u << a.log_cosets); j++) {
        uint32_t* dst = a.dst + (size_t)blockIdx.y * a.dst_stride + ((size_t)j << a.log_n);
        dst[i] = mmul(v, scale_for(a, j, i));
    }
}

static int launch_bitrev(zkhip_ctx* ctx, const BitrevArgs& a, size_t width) {
    if (width == 0) return ZKHIP_OK;
    KernelScope ks(ctx, "bitrev_scale");
    if (a.log_n >= 10) {
        hipLaunchKernelGGL(k_bitrev_scale_tiled, dim3(1u << (a.log_n - 10), (unsigned)width), dim3(256), 0,
                           ctx->stream, a);
    } else {
        unsigned n = 1u << a.log_n, bs = std::min(256u, std::max(64u, n));
        hipLaunchKernelGGL(k_bitrev_scale_small, dim3((n + bs - 1) / bs, (unsigned)width), dim3(bs), 0,
                           ctx->stream, a);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return ZKHIP_OK;
}

// pw tables for the LDE: coset j has shift s_j = shift * w_{n+a}^{bitrev_a(j)};
// lo[k] = s_j^k, hi[k] = s_j^(k << lb) / N
__global__ void k_gen_coset_powers(uint32_t* pw, uint32_t shift, uint32_t w_big, uint32_t n_inv, unsigned log_n,
                                   unsigned log_cosets, unsigned lb) {
    unsigned per = (1u << lb) + (1u << (log_n - lb));
    unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (per << log_cosets)) return;
    unsigned j = idx / per, k = idx % per;
    uint32_t s = mmul(shift, mpow(w_big, bitrev32(j, log_cosets)));
    if (k < (1u << lb))
        pw[idx] = mpow(s, k);
    else
        pw[idx] = mmul(n_inv, mpow(s, (uint64_t)(k - (1u << lb)) << lb));
}

// The same plain permutation for MANY small matrices in one launch per kernel form (the quotient chunks of every chip of a
// proof): segment = `width` columns of 2^log_n words; the flattened grid is searched like the LogUp kernels' (prover.hip).
__device__ __forceinline__ uint32_t bitrev_seg_of(const BitrevSeg* segs, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].first_block <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_bitrev_copy_tiled_multi(const BitrevSeg* __restrict__ segs, uint32_t n_seg) {
    __shared__ uint32_t tile[32][33];
    const BitrevSeg sg = segs[bitrev_seg_of(segs, n_seg, blockIdx.x)];
    const uint32_t lb = blockIdx.x - sg.first_block, log_mid = sg.log_n - 10;
    const unsigned mid = lb & ((1u << log_mid) - 1u), colx = lb >> log_mid;
    const unsigned tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint32_t* src = sg.src + (size_t)colx * sg.src_stride;
    uint32_t* dst = sg.dst + (size_t)colx * sg.dst_stride;
#pragma unroll
    for (unsigned rr = 0; rr < 4; rr++) {
        unsigned hi5 = ty + 8 * rr;
        tile[hi5][tx] = src[((size_t)hi5 << (sg.log_n - 5)) + ((size_t)mid << 5) + tx];
    }
    zk_syncthreads();
    const unsigned brmid = bitrev32(mid, log_mid);
#pragma unroll
    for (unsigned rr = 0; rr < 4; rr++) {
        unsigned B = ty + 8 * rr, A = tx;
        dst[(B << (sg.log_n - 5)) + (brmid << 5) + A] = tile[bitrev32(A, 5)][bitrev32(B, 5)];
    }
}
__global__ __launch_bounds__(256) void k_bitrev_copy_small_multi(const BitrevSeg* __restrict__ segs, uint32_t n_seg) {
    const BitrevSeg sg = segs[bitrev_seg_of(segs, n_seg, blockIdx.x)];
    const uint32_t lb = blockIdx.x - sg.first_block;
    const uint32_t n = 1u << sg.log_n, bpc = (n + 255u) / 256u;  // blocks per column
    const uint32_t colx = lb / bpc, i = (lb % bpc) * 256u + threadIdx.x;
    if (i >= n) return;
    sg.dst[(size_t)colx * sg.dst_stride + i] = sg.src[(size_t)colx * sg.src_stride + bitrev32(i, sg.log_n)];
}
uint32_t ntt_bitrev_copy_blocks(unsigned log_n, uint32_t width) {
    return log_n >= 10 ? (width << (log_n - 10)) : width * (((1u << log_n) + 255u) / 256u);
}
// d_tiled: segments with log_n >= 10, d_small: the others (first_block counted separately in each table)
int ntt_bitrev_copy_multi(zkhip_ctx* ctx, const BitrevSeg* d_tiled, uint32_t n_tiled, uint32_t blocks_tiled,
                          const BitrevSeg* d_small, uint32_t n_small, uint32_t blocks_small) {
    KernelScope ks(ctx, "bitrev_scale");
    if (n_tiled && blocks_tiled)
        hipLaunchKernelGGL(k_bitrev_copy_tiled_multi, dim3(blocks_tiled), dim3(256), 0, ctx->stream, d_tiled, n_tiled);
    if (n_small && blocks_small)
        hipLaunchKernelGGL(k_bitrev_copy_small_multi, dim3(blocks_small), dim3(256), 0, ctx->stream, d_small, n_small);
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return ZKHIP_OK;
}

// plain bit-reversal permutation of `width` columns (no scaling), out of place
int ntt_bitrev_copy(zkhip_ctx* ctx, const uint32_t* src, size_t src_stride, uint32_t* dst, size_t dst_stride,
                    unsigned log_n, size_t width) {
    BitrevArgs a{src, src_stride, dst, dst_stride, nullptr, MONTY_ONE, log_n, 0, 0};
    return launch_bitrev(ctx, a, width);
}

// tables for the fused LDE path: coset c has shift s_c = shift * w_{n+a}^{bitrev_a(c)};
//   col[c][F] = s_c^F / N (F < 2^log_f), row[c][j] = s_c^(j << log_f) (j < 2^log_rq), rho[c] = s_c^(1 << (log_f+log_rq))
__global__ void k_gen_lde_scales(uint32_t* col, uint32_t* row, uint32_t* rho, uint32_t shift, uint32_t w_big,
                                 uint32_t n_inv, unsigned log_cosets, unsigned log_f, unsigned log_rq) {
    const size_t n_col = (size_t)1 << log_f, n_row = (size_t)1 << log_rq, n_co = (size_t)1 << log_cosets;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n_co * n_col) {
        const unsigned c = (unsigned)(idx >> log_f);
        const uint32_t s = mmul(shift, mpow(w_big, bitrev32(c, log_cosets)));
        col[idx] = mmul(n_inv, mpow(s, idx & (n_col - 1)));
        return;
    }
    idx -= n_co * n_col;
    if (idx < n_co * n_row) {
        const unsigned c = (unsigned)(idx >> log_rq);
        const uint32_t s = mmul(shift, mpow(w_big, bitrev32(c, log_cosets)));
        row[idx] = mpow(s, (uint64_t)(idx & (n_row - 1)) << log_f);
        return;
    }
    idx -= n_co * n_row;
    if (idx < n_co) {
        const uint32_t s = mmul(shift, mpow(w_big, bitrev32((unsigned)idx, log_cosets)));
        rho[idx] = mpow(s, (uint64_t)1 << (log_f + log_rq));
    }
}

int ntt_batch(zkhip_ctx* ctx, uint32_t* d_mat, unsigned log_n, size_t width, size_t stride, bool inverse,
              bool bitrev_out) {
    if (width == 0) return ZKHIP_OK;
    if (stride < ((size_t)1 << log_n)) return set_error(ctx, ZKHIP_ERR_INVALID, "stride < height");
    uint32_t n_inv = minv(to_monty((uint32_t)(((uint64_t)1 << log_n) % P)));
    if (!bitrev_out) {
        // natural order in and out: the transform writes its bit-reversed result into scratch and the bit-reversal pass
        // brings it home (round 1 transformed in place, permuted into scratch and copied back: one pass over memory more)
        const size_t n = (size_t)1 << log_n;
        void* tmp;
        ZK_TRY(get_scratch(ctx, 0, n * width * 4, &tmp));
        ZK_TRY(ntt_dif_inplace(ctx, d_mat, stride, (uint32_t*)tmp, n, log_n, width, 0, inverse));
        BitrevArgs a{(uint32_t*)tmp, n, d_mat, stride, nullptr, inverse ? n_inv : MONTY_ONE, log_n, 0, 0};
        return launch_bitrev(ctx, a, width);
    }
    ZK_TRY(ntt_dif_inplace(ctx, d_mat, stride, d_mat, stride, log_n, width, 0, inverse));
    if (bitrev_out) {
        if (inverse) {
            // scale in place by 1/n
            size_t n = (size_t)1 << log_n;
            void* tmp;
            ZK_TRY(get_scratch(ctx, 0, n * width * 4, &tmp));
            BitrevArgs a{d_mat, stride, (uint32_t*)tmp, n, nullptr, n_inv, log_n, 0, 0};
            // permute to natural (scaled) then back to bit-reversed keeps the code path single; the
            // cheap way is a dedicated scale, done by two permutations only for this rarely used mode
            ZK_TRY(launch_bitrev(ctx, a, width));
            BitrevArgs b{(uint32_t*)tmp, n, d_mat, stride, nullptr, MONTY_ONE, log_n, 0, 0};
            ZK_TRY(launch_bitrev(ctx, b, width));
        }
        return ZKHIP_OK;
    }
    return ZKHIP_OK;
}

// The scale tables of a four-step LDE (d_col | d_row | d_rho, see k_gen_lde_scales) depend on (log_n, added_bits, shift) only: generated once
// per context (and waited for: later users may sit on another stream of the context), read-only afterwards.
static int lde_scale_tables(zkhip_ctx* ctx, unsigned log_n, unsigned added_bits, uint32_t shift_monty, unsigned log_f, unsigned log_rq, uint32_t** out) {
    const uint64_t key = ((uint64_t)log_n << 56) | ((uint64_t)added_bits << 48) | ((uint64_t)log_f << 40) | ((uint64_t)log_rq << 32) | shift_monty;
    auto it = ctx->lde_tables.find(key);
    if (it != ctx->lde_tables.end()) {
        *out = it->second;
        return ZKHIP_OK;
    }
    const unsigned n_co = 1u << added_bits;
    const size_t n = (size_t)1 << log_n, n_col = (size_t)1 << log_f, n_row = (size_t)1 << log_rq, cnt = n_co * (n_col + n_row + 1);
    uint32_t* tabs = nullptr;
    if (hipMalloc(&tabs, cnt * 4) != hipSuccess) return set_error(ctx, ZKHIP_ERR_NOMEM, "lde scale tables");
    {
        KernelScope ks(ctx, "gen_coset_powers");
        const uint32_t n_inv = minv(to_monty((uint32_t)(n % P)));
        hipLaunchKernelGGL(k_gen_lde_scales, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, tabs, tabs + n_co * n_col, tabs + n_co * (n_col + n_row), shift_monty,
                           two_adic_generator(log_n + added_bits), n_inv, added_bits, log_f, log_rq);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(tabs);
        return set_error(ctx, ZKHIP_ERR_HIP, "lde scale tables");
    }
    ctx->lde_tables[key] = tabs;
    *out = tabs;
    return ZKHIP_OK;
}

// The fused middle of a coset LDE (k_ntt_lde_fused): inverse pass 1 -> [fused: inverse pass 2 + every coset's forward pass 1] -> forward
// pass 2.  `applies`: transforms of 2^22 points (two passes of eleven stages), and only when ZKHIP_LDE_FUSED=1 asks for it (see the kernel's
// header: measured, no faster than the four-pass form).  Read per call: the parity test switches it inside one process.
static bool lde_fused_applies(unsigned log_n) {
    const char* e = getenv("ZKHIP_LDE_FUSED");
    unsigned a[3];
    return e && e[0] == '1' && fourstep_split(log_n, a) == 2 && a[0] == a[1] && a[0] == 11;
}
static int lde_fused(zkhip_ctx* ctx, const uint32_t* d_in, size_t in_stride, const uint32_t* const* d_src_cols, uint32_t* d_out, size_t out_stride,
                     uint32_t* const* d_dst_cols, unsigned log_n, unsigned added_bits, size_t width, uint32_t shift_monty) {
    const size_t n = (size_t)1 << log_n, per_col = n << added_bits;
    unsigned a[3];
    fourstep_split(log_n, a);
    const unsigned a1 = a[0], a2 = a[1];
    const unsigned log_f = log_n - a1, log_rq = a1 - 4, n_co = 1u << added_bits;
    uint32_t* d_col = nullptr;
    ZK_TRY(lde_scale_tables(ctx, log_n, added_bits, shift_monty, log_f, log_rq, &d_col));
    uint32_t* d_row = d_col + n_co * ((size_t)1 << log_f);
    uint32_t* d_rho = d_row + n_co * ((size_t)1 << log_rq);
    void *t1v, *t2v;
    ZK_TRY(get_scratch(ctx, 0, n * width * 4, &t1v));
    ZK_TRY(get_scratch(ctx, 4, per_col * width * 4, &t2v));
    uint32_t *t1 = (uint32_t*)t1v, *t2 = (uint32_t*)t2v;
    static DeviceOnce attr_set;
    const int lds = (int)(((((size_t)1 << a2) * 9u) + ((size_t)1 << (a2 - 1))) * 4);   // [2^11][8 + 1] + the twiddle table
    if (attr_set.need(ctx->device)) {
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_ntt_lde_fused<11, 3, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_ntt_lde_fused<11, 3, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        ZK_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)k_ntt_pass4_ct<11, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_set.mark(ctx->device);
    }
    // inverse pass 1 alone: the first launch of ntt_dif_fourstep's two-pass form (digit d1 in rows, F = d2; out [d2][p1])
    {
        Pass4Args pa;
        memset(&pa, 0, sizeof pa);
        pa.log_r = a1, pa.log_f = a2, pa.in_x_stride = 0, pa.in_rs = (size_t)1 << a2;
        pa.out_x_stride = 0, pa.out_hi_stride = (size_t)1 << a1, pa.out_lo_stride = 0, pa.log_lo = 0, pa.in_tw = 0;
        pa.src = d_in, pa.src_col_stride = in_stride, pa.src_cols = d_src_cols;
        pa.dst = t1, pa.dst_col_stride = n;
        pa.tw = ctx->d_tw_inv, pa.tw_log = ctx->tw_log, pa.log_sub = 0, pa.log_m = log_n, pa.log_c = 3;
        KernelScope ks(ctx, "ntt_pass_inv");
        const dim3 grid(1u << (pa.log_f - pa.log_c), (unsigned)width);
        const size_t lds1 = ((((size_t)1 << a1) * 9u) + ((size_t)1 << (a1 - 1))) * 4;
        hipLaunchKernelGGL((k_ntt_pass4_ct<11, 3>), grid, dim3(1024), lds1, ctx->stream, pa);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    {
        LdeFusedArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.src = t1, fa.src_col_stride = n, fa.dst = t2, fa.dst_col_stride = per_col;
        fa.tw_inv = ctx->d_tw_inv, fa.tw_fwd = ctx->d_tw_fwd, fa.tw_log = ctx->tw_log, fa.log_m = log_n, fa.log_cosets = added_bits;
        fa.scale_col = d_col, fa.scale_row = d_row, fa.scale_rho = d_rho;
        KernelScope ks(ctx, "ntt_lde_fused");
        const dim3 grid(1u << (a1 - 3), (unsigned)width);
        const bool one_wg = getenv("ZKHIP_LDE_FUSED_WAVES") && atoi(getenv("ZKHIP_LDE_FUSED_WAVES")) == 4;
        if (one_wg) hipLaunchKernelGGL((k_ntt_lde_fused<11, 3, 4>), grid, dim3(1024), (size_t)lds, ctx->stream, fa);
        else hipLaunchKernelGGL((k_ntt_lde_fused<11, 3, 8>), grid, dim3(1024), (size_t)lds, ctx->stream, fa);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    // forward pass 2 alone: the second launch of the two-pass form (digit d2 in rows, F = p1; twiddle w_M^(k1 d2)), every coset
    {
        Pass4Args pa;
        memset(&pa, 0, sizeof pa);
        pa.log_r = a2, pa.log_f = a1, pa.in_x_stride = 0, pa.in_rs = (size_t)1 << a1;
        pa.out_x_stride = 0, pa.out_hi_stride = (size_t)1 << a2, pa.out_lo_stride = 0, pa.log_lo = 0;
        pa.in_tw = 1, pa.log_prev = a1, pa.log_tt = log_n, pa.tw_a = 1, pa.tw_bx = 0;
        pa.src = t2, pa.src_col_stride = per_col;
        pa.dst = d_out, pa.dst_col_stride = out_stride, pa.dst_cols = d_dst_cols;
        pa.tw = ctx->d_tw_fwd, pa.tw_log = ctx->tw_log, pa.log_sub = added_bits, pa.log_m = log_n, pa.log_c = 3;
        KernelScope ks(ctx, "ntt_pass_fwd");
        const dim3 grid(1u << (pa.log_f - pa.log_c), (unsigned)(width << added_bits));
        const size_t lds2 = ((((size_t)1 << a2) * 9u) + ((size_t)1 << (a2 - 1))) * 4;
        hipLaunchKernelGGL((k_ntt_pass4_ct<11, 3>), grid, dim3(1024), lds2, ctx->stream, pa);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    return ZKHIP_OK;
}

// The tail both LDE entry points share: the forward four-step of every coset straight from the bit-reversed coefficients (`width` columns
// of n words, contiguous).  The first pass reads each lane's 16 operands as one 64-byte chunk and applies shift_j^i / N as a geometric
// sequence (the coset scale tables); the last writes to d_out, or to the columns of d_dst_cols when that is set.
static int lde_forward_from_coeffs(zkhip_ctx* ctx, const uint32_t* coeffs, uint32_t* d_out, size_t out_stride, uint32_t* const* d_dst_cols,
                                   unsigned log_n, unsigned added_bits, size_t width, uint32_t shift_monty) {
    const size_t n = (size_t)1 << log_n, per_col = n << added_bits;
    unsigned a[3];
    fourstep_split(log_n, a);
    const unsigned log_f = log_n - a[0], log_rq = a[0] - 4, n_co = 1u << added_bits;
    uint32_t* d_col = nullptr;
    ZK_TRY(lde_scale_tables(ctx, log_n, added_bits, shift_monty, log_f, log_rq, &d_col));
    uint32_t* d_row = d_col + n_co * ((size_t)1 << log_f);
    uint32_t* d_rho = d_row + n_co * ((size_t)1 << log_rq);
    const BrSrc bs{d_col, d_row, d_rho};
    uint32_t *t1, *t2;
    ZK_TRY(pass_scratch(ctx, log_n, per_col * width, &t1, &t2));
    return ntt_dif_fourstep(ctx, coeffs, n, d_out, out_stride, t1, t2, per_col, log_n, width, added_bits, false, &bs, nullptr, d_dst_cols);
}

int lde_batch(zkhip_ctx* ctx, const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride,
              unsigned log_n, unsigned added_bits, size_t width, uint32_t shift_monty) {
    if (width == 0) return ZKHIP_OK;
    const size_t n = (size_t)1 << log_n;
    if (in_stride < n || out_stride < (n << added_bits)) return set_error(ctx, ZKHIP_ERR_INVALID, "stride < height");
    if (log_n + added_bits > 27) return set_error(ctx, ZKHIP_ERR_INVALID, "LDE size exceeds two-adicity");
    ZK_TRY(ensure_twiddles(ctx, log_n + added_bits));
    if (lde_fused_applies(log_n) && ctx->cfg.ntt_pass_form != 2) return lde_fused(ctx, d_in, in_stride, nullptr, d_out, out_stride, nullptr, log_n, added_bits, width, shift_monty);
    // 1. inverse DIF into scratch: coefficients (unnormalised) in bit-reversed order
    void* coeffs;
    ZK_TRY(get_scratch(ctx, 0, n * width * 4, &coeffs));
    ZK_TRY(ntt_dif_inplace(ctx, d_in, in_stride, (uint32_t*)coeffs, n, log_n, width, 0, true));
    if (log_n >= P4_MIN_LOG_M && ctx->cfg.ntt_pass_form != 2) {
        // 2'. forward four-step straight from the bit-reversed coefficients
        return lde_forward_from_coeffs(ctx, (const uint32_t*)coeffs, d_out, out_stride, nullptr, log_n, added_bits, width, shift_monty);
    }
    // 2. per-coset power tables
    unsigned lb = (log_n + 1) / 2;
    unsigned per = (1u << lb) + (1u << (log_n - lb));
    // (the power tables depend on (log_n, added_bits, shift) only: once per context, like the four-step form's scale tables)
    uint32_t* pw = nullptr;
    {
        const uint64_t key = ((uint64_t)1 << 63) | ((uint64_t)log_n << 56) | ((uint64_t)added_bits << 48) | shift_monty;
        auto it = ctx->lde_tables.find(key);
        if (it == ctx->lde_tables.end()) {
            const unsigned cnt = per << added_bits, bs = 256;
            if (hipMalloc(&pw, (size_t)cnt * 4) != hipSuccess) return set_error(ctx, ZKHIP_ERR_NOMEM, "lde power tables");
            {
                KernelScope ks(ctx, "gen_coset_powers");
                const uint32_t n_inv = minv(to_monty((uint32_t)(n % P)));
                hipLaunchKernelGGL(k_gen_coset_powers, dim3((cnt + bs - 1) / bs), dim3(bs), 0, ctx->stream, pw, shift_monty, two_adic_generator(log_n + added_bits), n_inv, log_n,
                                   added_bits, lb);
            }
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
                (void)hipFree(pw);
                return set_error(ctx, ZKHIP_ERR_HIP, "lde power tables");
            }
            ctx->lde_tables[key] = pw;
        } else {
            pw = it->second;
        }
    }
    // 3. bit-reverse to natural order, scaling into every coset block of the output
    BitrevArgs a{(const uint32_t*)coeffs, n, d_out, out_stride, (const uint32_t*)pw, MONTY_ONE, log_n, added_bits, lb};
    ZK_TRY(launch_bitrev(ctx, a, width));
    // 4. forward DIF of every coset block in place -> bit-reversed evaluations
    ZK_TRY(ntt_dif_inplace(ctx, d_out, out_stride, d_out, out_stride, log_n, width, added_bits, false));
    return ZKHIP_OK;
}

// LDE of `n_cols` columns that live in different matrices (per-column device pointer tables) as ONE batch: the
// chips of a proof that share a height are extended by the same launches.  Four-step sizes only (log_n >= 12).
int lde_batch_cols(zkhip_ctx* ctx, const uint32_t* const* d_src_cols, uint32_t* const* d_dst_cols, size_t n_cols,
                   unsigned log_n, unsigned added_bits, uint32_t shift_monty) {
    if (n_cols == 0) return ZKHIP_OK;
    if (log_n < P4_MIN_LOG_M) return set_error(ctx, ZKHIP_ERR_INVALID, "lde_batch_cols: transform too small");
    if (log_n + added_bits > 27) return set_error(ctx, ZKHIP_ERR_INVALID, "LDE size exceeds two-adicity");
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(ensure_twiddles(ctx, log_n + added_bits));
    if (lde_fused_applies(log_n)) return lde_fused(ctx, nullptr, 0, d_src_cols, nullptr, 0, d_dst_cols, log_n, added_bits, n_cols, shift_monty);
    void* coeffs;
    ZK_TRY(get_scratch(ctx, 0, n * n_cols * 4, &coeffs));
    {
        // inverse transform: columns come from the table, coefficients go to contiguous scratch (asked for at the size the forward
        // transform will ask for, so that the scratch is not allocated twice)
        uint32_t *t1, *t2;
        ZK_TRY(pass_scratch(ctx, log_n, (n << added_bits) * n_cols, &t1, &t2));
        ZK_TRY(ntt_dif_fourstep(ctx, nullptr, 0, (uint32_t*)coeffs, n, t1, t2, n, log_n, n_cols, 0, true, nullptr, d_src_cols, nullptr));
    }
    return lde_forward_from_coeffs(ctx, (const uint32_t*)coeffs, nullptr, 0, d_dst_cols, log_n, added_bits, n_cols, shift_monty);
}

// ---------------------------------------------------------------------------------------------
__global__ void k_convert(uint32_t* d, size_t n, int to_m) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t step = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += step) d[i] = to_m ? to_monty(d[i]) : from_monty(d[i]);
}

int convert_repr(zkhip_ctx* ctx, uint32_t* d, size_t n, bool to_m) {
    if (n == 0) return ZKHIP_OK;
    KernelScope ks(ctx, "convert_repr");
    unsigned bs = 256;
    size_t blocks = std::min<size_t>((n + bs - 1) / bs, 256 * 16);
    hipLaunchKernelGGL(k_convert, dim3((unsigned)blocks), dim3(bs), 0, ctx->stream, d, n, to_m ? 1 : 0);
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return ZKHIP_OK;
}

}  // namespace zk
