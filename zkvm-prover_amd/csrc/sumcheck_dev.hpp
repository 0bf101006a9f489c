// sumcheck_dev.hpp -- the device core of the library's sum-checks: extension loads and stores, the fold, the wave and workgroup
// sums, the streaming round pass, the one-wave transcript step and the round of the single-workgroup form.  Its users are the
// LogUp-GKR layers (csrc/logup_gkr.hip), the WHIR opening (csrc/whir.hip), the stacking reduction (csrc/stacking.hip) and the
// stage kernels of csrc/sumcheck.hip.
//
// A round description G names the round's tables and its summand: G::T tables, the round polynomial s(x) = sum_y G(f_y(x)) evaluated
// at the E points 0, 2, 3, .., E (s(1) follows from the claim), G(v) the summand on one value of every table, and G::load(), which
// fetches what G reads from device memory before a pass uses it.
#pragma once
#include "lds_barrier.hpp"
#include "transcript_dev.hpp"
#include "zkhip_internal.hpp"

namespace zk {

constexpr unsigned SC_NB = 1024;   // most workgroups of a streaming pass (partial sums: word w of workgroup b at w * SC_NB + b)
constexpr unsigned SC_SW = 512;    // threads of the single-workgroup kernels (one pair each)
constexpr unsigned SC_LT = 10;     // tables of <= 2^SC_LT entries: the single-workgroup form, tables in LDS
constexpr unsigned SC_T = 1u << SC_LT;

// ---- extension elements: 16 bytes each, in global memory or LDS ----------------------------------------------------------------
__device__ __forceinline__ uint4 ext_pack(const Ext& e) { return make_uint4(e.c[0], e.c[1], e.c[2], e.c[3]); }
__device__ __forceinline__ Ext ext_unpack(const uint4& v) { return Ext{{v.x, v.y, v.z, v.w}}; }
__device__ __forceinline__ Ext sc_ld(const uint32_t* p, size_t i) { return ext_unpack(reinterpret_cast<const uint4*>(p)[i]); }
__device__ __forceinline__ void sc_st(uint32_t* p, size_t i, const Ext& e) { reinterpret_cast<uint4*>(p)[i] = ext_pack(e); }

// the pair (a, b) of a table bound to r: a + r (b - a)
__device__ __forceinline__ Ext sc_fold(const Ext& a, const Ext& b, const Ext& r) { return ext_add(a, ext_mul(r, ext_sub(b, a))); }

__device__ __forceinline__ uint32_t sc_wave_sum(uint32_t x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = madd(x, __shfl_xor(x, off, 64));
    return x;
}

// a 256-thread workgroup's sum of NE extension values per thread: word w = 4 e + q (w < n) to out[w * stride].  No barrier behind
// it: a caller that runs it again first syncs.
template <unsigned NE>
__device__ __forceinline__ void sc_block_sum(const Ext (&acc)[NE], uint32_t* out, size_t stride = SC_NB, unsigned n = 4 * NE) {
    __shared__ uint32_t red[4][4 * NE];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (unsigned e = 0; e < NE; e++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = sc_wave_sum(acc[e].c[q]);
            if (lane == 0) red[wave][4 * e + q] = x;
        }
    zk_syncthreads();
    if (tid < n) out[(size_t)tid * stride] = madd(madd(red[0][tid], red[1][tid]), madd(red[2][tid], red[3][tid]));
}

// acc[e] += G at point e of the pair (f0, f1) of every table, the points 0, 2, 3, ..: f0, then f1 + d, then + d again
template <class G>
__device__ __forceinline__ void sc_eval(const G& g, const Ext* f0, const Ext* f1, Ext* acc) {
    Ext v[G::T], d[G::T];
#pragma unroll
    for (unsigned t = 0; t < G::T; t++) v[t] = f0[t], d[t] = ext_sub(f1[t], f0[t]);
    acc[0] = ext_add(acc[0], g(v));
#pragma unroll
    for (unsigned e = 1; e < G::E; e++) {
#pragma unroll
        for (unsigned t = 0; t < G::T; t++) v[t] = ext_add(e == 1 ? f1[t] : v[t], d[t]);
        acc[e] = ext_add(acc[e], g(v));
    }
}

// ---- the streaming round -------------------------------------------------------------------------------------------------------
// T plain tables: entry j of table t at tab[t] + 4 j
template <unsigned T>
struct ScTables {
    const uint32_t* tab[T];
    __device__ __forceinline__ Ext operator()(unsigned t, size_t j) const { return sc_ld(tab[t], j); }
};

// one round over the pairs y < n_pairs of the G::T tables `src` reads (src(t, j): entry j of table t): with r, the tables (4 n_pairs
// entries) are folded with r first and stored into dst[t] (2 n_pairs entries); without r (null) they are read as they are.  partial
// (null: fold only) gets this workgroup's sums of s at the G::E points, word w of the round polynomial at w * SC_NB + blockIdx.x.
template <class Src, class G>
struct ScPass {
    Src src;
    G g;
    uint32_t* dst[G::T];
    const uint32_t* r;
    size_t n_pairs;
    uint32_t* partial;
};
template <class Src, class G>
__global__ __launch_bounds__(256) void k_sc_pass(ScPass<Src, G> a) {
    constexpr unsigned T = G::T, E = G::E;
    G g = a.g;
    g.load();
    const Ext r = a.r ? sc_ld(a.r, 0) : ext_zero();
    Ext acc[E];
#pragma unroll
    for (unsigned e = 0; e < E; e++) acc[e] = ext_zero();
    for (size_t y = (size_t)blockIdx.x * 256 + threadIdx.x; y < a.n_pairs; y += (size_t)gridDim.x * 256) {
        Ext f0[T], f1[T];
        if (a.r) {
#pragma unroll
            for (unsigned t = 0; t < T; t++) {
                f0[t] = sc_fold(a.src(t, 4 * y), a.src(t, 4 * y + 1), r), f1[t] = sc_fold(a.src(t, 4 * y + 2), a.src(t, 4 * y + 3), r);
                sc_st(a.dst[t], 2 * y, f0[t]), sc_st(a.dst[t], 2 * y + 1, f1[t]);
            }
        } else {
#pragma unroll
            for (unsigned t = 0; t < T; t++) f0[t] = a.src(t, 2 * y), f1[t] = a.src(t, 2 * y + 1);
        }
        if (a.partial) sc_eval(g, f0, f1, acc);
    }
    if (!a.partial) return;   // uniform across the grid
    sc_block_sum(acc, a.partial + blockIdx.x);
}

// the product of two tables (the WHIR opening's and the stacking reduction's sum-check): s(x) = sum_y f w at 0, 2
struct WhirRound {
    static constexpr unsigned T = 2, E = 2;
    __device__ __forceinline__ void load() {}
    __device__ __forceinline__ Ext operator()(const Ext* v) const { return ext_mul(v[0], v[1]); }
};

// ---- the transcript step -------------------------------------------------------------------------------------------------------
// one wave: the round polynomial's NW words (Montgomery) into the proof (canonical) and observed, the round challenge sampled into
// r_out and, if given, r_lds (lane 0 writes)
template <unsigned NW>
__device__ __forceinline__ void sc_tr_round(TrRegs& R, unsigned lane, const CoopConsts& cc, const uint32_t (&s)[NW], uint32_t* proof,
                                            uint32_t* r_out, uint32_t* r_lds = nullptr) {
#pragma unroll
    for (unsigned k = 0; k < NW; k++) {
        if (lane == 0) proof[k] = from_monty(s[k]);
        tr_observe1(R, lane, s[k], cc);
    }
    for (int q = 0; q < 4; q++) {
        const uint32_t v = tr_sample1(R, lane, cc);
        if (lane == 0) {
            r_out[q] = v;
            if (r_lds) r_lds[q] = v;
        }
    }
}

// the partials of a pass (nb workgroups) -> the round polynomial: written into the proof, observed, and the challenge sampled
template <unsigned NW>
__global__ __launch_bounds__(64) void k_sc_round_tr(DevTranscript* tr, const uint32_t* __restrict__ partial, unsigned nb,
                                                     uint32_t* __restrict__ proof_out, uint32_t* __restrict__ r_out) {
    const unsigned lane = threadIdx.x;
    const CoopConsts cc = coop_load_consts(lane & 15u);
    uint32_t s[NW] = {};
    for (unsigned b = lane; b < nb; b += 64)   // NW independent loads per step
#pragma unroll
        for (unsigned k = 0; k < NW; k++) s[k] = madd(s[k], partial[(size_t)k * SC_NB + b]);
#pragma unroll
    for (unsigned k = 0; k < NW; k++) s[k] = sc_wave_sum(s[k]);
    TrRegs R = tr_load(tr, lane);
    sc_tr_round(R, lane, cc, s, proof_out, r_out);
    tr_store(tr, R, lane);
}

// ---- a round of the single-workgroup form --------------------------------------------------------------------------------------
// G::T tables of m <= 2 SC_SW entries in LDS, entry j of table t at X + 4 (t stride + j), in an SC_SW-thread workgroup: every thread
// evaluates one pair, the waves' sums are added, wave 0 (which holds the transcript R) writes the round polynomial into `proof`,
// observes it and samples r into r_out (global) and r_lds (4 words of LDS), and every table is folded with r in place.  Starts
// after, and ends on, a barrier.
template <class G>
__device__ __forceinline__ void sc_small_round(const G& g, uint32_t* X, unsigned stride, unsigned m, TrRegs& R, const CoopConsts& cc,
                                               uint32_t* proof, uint32_t* r_out, uint32_t* r_lds) {
    constexpr unsigned T = G::T, E = G::E;
    __shared__ uint32_t red[SC_SW / 64][4 * E];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    Ext acc[E];
#pragma unroll
    for (unsigned e = 0; e < E; e++) acc[e] = ext_zero();
    if (tid < m / 2) {
        Ext f0[T], f1[T];
#pragma unroll
        for (unsigned t = 0; t < T; t++) f0[t] = sc_ld(X, t * stride + 2 * tid), f1[t] = sc_ld(X, t * stride + 2 * tid + 1);
        sc_eval(g, f0, f1, acc);
    }
#pragma unroll
    for (unsigned e = 0; e < E; e++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = sc_wave_sum(acc[e].c[q]);
            if (lane == 0) red[wave][4 * e + q] = x;
        }
    zk_syncthreads();
    if (wave == 0) {
        uint32_t s[4 * E];
#pragma unroll
        for (unsigned w = 0; w < 4 * E; w++) {
            uint32_t x = 0;
            for (unsigned v = 0; v < SC_SW / 64; v++) x = madd(x, red[v][w]);
            s[w] = x;
        }
        sc_tr_round(R, lane, cc, s, proof, r_out, r_lds);
    }
    zk_syncthreads();
    const Ext r{{r_lds[0], r_lds[1], r_lds[2], r_lds[3]}};
    Ext nv[T];
    if (tid < m / 2)
#pragma unroll
        for (unsigned t = 0; t < T; t++) nv[t] = sc_fold(sc_ld(X, t * stride + 2 * tid), sc_ld(X, t * stride + 2 * tid + 1), r);
    zk_syncthreads();
    if (tid < m / 2)
#pragma unroll
        for (unsigned t = 0; t < T; t++) sc_st(X, t * stride + tid, nv[t]);
    zk_syncthreads();
}

}  // namespace zk
