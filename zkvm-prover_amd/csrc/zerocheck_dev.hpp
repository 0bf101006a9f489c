// zerocheck_dev.hpp -- the per-AIR part of the AIR zero-check (docs/zerocheck.md) and the AIR-set proof (docs/airset.md), included
// by airset.hip alone, which holds the host side of both: the plan of one AIR, the sum-check kernels over the lowered constraint
// program, the rotation reduction, one AIR's device prover (zc_prove_air) and the host evaluation of a plan's nodes.
//
// The constraint kernels have a compile-time BUS form for the AIR-set proof: a second eq table (eq(rho_a, .)) and a second
// coefficient set; an ASSERT whose number is at or above n_cons adds to a second combination, which the second eq factor multiplies.
// With BUS = false they are the zero-check's kernels as they were.
//
// The keyed proofs (zkhip_airkey_*) run a second compile-time form, PREP: kernels of their own (k_zc_round0_p, k_zc_pass_p,
// k_zc_combine_p) over the same bodies, which also read the key's resident preprocessed columns (ZcPrep).  With PREP = false the
// bodies are the unkeyed kernels' code: every preprocessed read sits behind the compile-time flag.
#pragma once
#include <algorithm>
#include <vector>

#include "air_compile.hpp"
#include "host_challenger.hpp"
#include "sumcheck_dev.hpp"

namespace zk {

constexpr unsigned ZC_W = 64;            // threads of a constraint-pass workgroup: one wave, its sums need no barrier
constexpr unsigned ZC_MAX_SLOTS = 64;    // live intermediates: 1 KiB of LDS each in the extension passes (16 B x 64 lanes)
constexpr unsigned ZC_LT = 9;            // the rotation reduction's single-workgroup tail: 4 tables of <= 2^9 entries in LDS
constexpr unsigned ZC_T = 1u << ZC_LT;

// the lowered program of one AIR (device): its proven constraints only, ASSERT k carrying the constraint's number among them
struct ZcProg {
    const uint32_t* code;     // 3 words per instruction (air_compile.hpp); the extension passes' copy names tables in its VAR operands
    unsigned n_ins;
    const uint32_t* consts;   // Montgomery
    const uint32_t* pvs;      // Montgomery
    const uint32_t* apow;     // alpha^k, extension
    const uint32_t* bcoef;    // BUS: the coefficient of root n_cons + k, extension
    unsigned n_cons;          // BUS: an ASSERT numbered n_cons or above goes to the second combination
};

// PREP: the preprocessed columns of one AIR as the key holds them (device)
struct ZcPrep {
    const uint32_t* cols;   // wp columns of 2^m Montgomery words
    const uint32_t* rot;    // the columns read with rotation 1, increasing
    unsigned wp, n_rot;
};

// x^k for k < n
static __global__ __launch_bounds__(256) void k_zc_pows(const uint32_t* __restrict__ x, unsigned n, uint32_t* __restrict__ out) {
    const Ext a = sc_ld(x, 0);
    for (unsigned k = threadIdx.x; k < n; k += 256) sc_st(out, k, ext_pow(a, k));
}

// one wave's sums of the round polynomial: word 4 e + q at partial[(4 e + q) SC_NB + wg]
template <unsigned D>
__device__ __forceinline__ void zc_wave_out(const Ext (&acc)[D], uint32_t* partial, unsigned wg) {
#pragma unroll
    for (unsigned e = 0; e < D; e++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = sc_wave_sum(acc[e].c[q]);
            if (threadIdx.x == 0) partial[(size_t)(4 * e + q) * SC_NB + wg] = x;
        }
}

// the integer t as a field element
__device__ __forceinline__ uint32_t zc_small(unsigned t) { return mmul(t, MONTY_R2); }

// ---- round 0: the base-field trace in place ------------------------------------------------------------------------------------
// Pair y holds rows 2y and 2y + 1; a next-row cell is the same column one row on (mod n).  At the integer point t a cell's value is
// the base element f0 + t (f1 - f0), so the program runs in the base field; the alpha-combination and the eq factor are extension.
// The workgroup is number wg of the n_wg that share the pairs (the single-AIR kernels: the grid; the batched ones: its job's range).
template <unsigned D, bool BUS, bool PREP>
__device__ __forceinline__ void zc_round0_body(const ZcProg& pg, const uint32_t* __restrict__ trace, const uint32_t* __restrict__ prep, unsigned m,
                                               const uint32_t* __restrict__ E, const uint32_t* __restrict__ E2, uint32_t* __restrict__ partial,
                                               unsigned wg, unsigned n_wg) {
    extern __shared__ uint32_t zc_slots[];   // [slot][lane]
    const unsigned lane = threadIdx.x;
    const size_t n = (size_t)1 << m, n_pairs = n >> 1;
    Ext acc[D];
#pragma unroll
    for (unsigned e = 0; e < D; e++) acc[e] = ext_zero();
    for (size_t y = (size_t)wg * ZC_W + lane; y < n_pairs; y += (size_t)n_wg * ZC_W) {
        const size_t x0 = 2 * y, x1 = x0 + 1, x2 = (x0 + 2) & (n - 1);
        const Ext e0 = sc_ld(E, x0), e1 = sc_ld(E, x1), de = ext_sub(e1, e0);
        Ext et = e0;
        Ext b0, b1, db, bt;   // BUS: the second eq factor
        if (BUS) b0 = sc_ld(E2, x0), b1 = sc_ld(E2, x1), db = ext_sub(b1, b0), bt = b0;
#pragma unroll
        for (unsigned p = 0; p < D; p++) {
            const uint32_t tm = zc_small(p ? p + 1 : 0);
            auto operand = [&](uint32_t w) -> uint32_t {
                const uint32_t pay = w & 0x0fffffffu;
                if (PREP && (w >> 28) == K_PREP) {   // a cell of the key's columns: K_VAR's pair and next-row addressing
                    const size_t base = (size_t)(pay & 0x07ffffffu) * n;
                    const bool rot = (pay >> 27) & 1u;
                    const uint32_t f0 = prep[base + (rot ? x1 : x0)], f1 = prep[base + (rot ? x2 : x1)];
                    return madd(f0, mmul(tm, msub(f1, f0)));
                }
                switch (w >> 28) {
                    case K_SLOT:
                        return zc_slots[pay * ZC_W + lane];
                    case K_VAR: {
                        const size_t base = (size_t)(pay & 0x07ffffffu) * n;
                        const bool rot = (pay >> 27) & 1u;
                        const uint32_t f0 = trace[base + (rot ? x1 : x0)], f1 = trace[base + (rot ? x2 : x1)];
                        return madd(f0, mmul(tm, msub(f1, f0)));
                    }
                    case K_PUB:
                        return pg.pvs[pay];
                    case K_CONST:
                        return pg.consts[pay];
                    default: {   // K_SEL: first = 1 - t on pair 0, last = t on the last pair, transition = 1 - last
                        const uint32_t first = x0 == 0 ? msub(MONTY_ONE, tm) : 0u, last = x1 == n - 1 ? tm : 0u;
                        return pay == 0 ? first : pay == 1 ? last : msub(MONTY_ONE, last);
                    }
                }
            };
            Ext comb = ext_zero(), comb2 = ext_zero();
            for (unsigned i = 0; i < pg.n_ins; i++) {
                const uint32_t w0 = pg.code[3 * i], op = w0 & 0xffu, dst = w0 >> 8;
                const uint32_t a = operand(pg.code[3 * i + 1]);
                if (op == Q_ASSERT) {
                    if (BUS && dst >= pg.n_cons) comb2 = ext_add(comb2, ext_mul_base(sc_ld(pg.bcoef, dst - pg.n_cons), a));
                    else comb = ext_add(comb, ext_mul_base(sc_ld(pg.apow, dst), a));
                    continue;
                }
                const uint32_t b = op == Q_NEG ? 0u : operand(pg.code[3 * i + 2]);
                zc_slots[dst * ZC_W + lane] = op == Q_ADD ? madd(a, b) : op == Q_SUB ? msub(a, b) : op == Q_MUL ? mmul(a, b) : mneg(a);
            }
            if (p) et = ext_add(p == 1 ? e1 : et, de);
            acc[p] = ext_add(acc[p], ext_mul(comb, et));
            if (BUS) {
                if (p) bt = ext_add(p == 1 ? b1 : bt, db);
                acc[p] = ext_add(acc[p], ext_mul(comb2, bt));
            }
        }
    }
    zc_wave_out(acc, partial, wg);
}
template <unsigned D, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zc_round0(ZcProg pg, const uint32_t* __restrict__ trace, unsigned m, const uint32_t* __restrict__ E,
                                                    const uint32_t* __restrict__ E2, uint32_t* __restrict__ partial) {
    zc_round0_body<D, BUS, false>(pg, trace, nullptr, m, E, E2, partial, blockIdx.x, gridDim.x);
}
template <unsigned D, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zc_round0_p(ZcProg pg, const uint32_t* __restrict__ trace, const uint32_t* __restrict__ prep, unsigned m,
                                                      const uint32_t* __restrict__ E, const uint32_t* __restrict__ E2, uint32_t* __restrict__ partial) {
    zc_round0_body<D, BUS, true>(pg, trace, prep, m, E, E2, partial, blockIdx.x, gridDim.x);
}

// ---- rounds >= 1: fold with the previous challenge and evaluate, one pass --------------------------------------------------------
// The tables of a pass: [w columns | n_rot next-row tables (| PREP: w_p preprocessed columns | their n_rot_p next-row tables) | first |
// last | eq (| BUS: the second eq)], table t's entry j at tab + 4 (t stride + j).  From the base trace (the first fold) the next-row
// tables are the rotated columns; after it they are tables of their own.
struct ZcTabs {
    const uint32_t* trace;   // FROM_BASE: the trace (2^m rows), eq(tau, .) and the rotated columns' numbers
    const uint32_t* E;
    const uint32_t* E2;      // BUS: eq(rho_a, .)
    const uint32_t* rot;
    unsigned m, w, n_rot;
    const uint32_t* src;     // otherwise: tables of 2 nd entries
    size_t src_stride;
    uint32_t* dst;           // tables of nd entries
    size_t dst_stride;
    size_t nd;
};

template <bool FROM_BASE, bool PREP>
__device__ __forceinline__ Ext zc_fold_entry(const ZcTabs& tb, const ZcPrep& pp, unsigned t, size_t e, const Ext& r) {
    if (FROM_BASE) {
        const size_t n = (size_t)1 << tb.m, i0 = 2 * e, i1 = i0 + 1;
        if (t < tb.w + tb.n_rot) {
            const bool rot = t >= tb.w;
            const size_t base = (size_t)(rot ? tb.rot[t - tb.w] : t) * n;
            const uint32_t a = tb.trace[base + (rot ? i1 : i0)], b = tb.trace[base + (rot ? ((i1 + 1) & (n - 1)) : i1)];
            Ext v = ext_mul_base(r, msub(b, a));
            v.c[0] = madd(v.c[0], a);
            return v;
        }
        unsigned s = t - tb.w - tb.n_rot;
        if (PREP) {
            if (s < pp.wp + pp.n_rot) {   // the key's columns, addressed as the trace's
                const bool rot = s >= pp.wp;
                const size_t base = (size_t)(rot ? pp.rot[s - pp.wp] : s) * n;
                const uint32_t a = pp.cols[base + (rot ? i1 : i0)], b = pp.cols[base + (rot ? ((i1 + 1) & (n - 1)) : i1)];
                Ext v = ext_mul_base(r, msub(b, a));
                v.c[0] = madd(v.c[0], a);
                return v;
            }
            s -= pp.wp + pp.n_rot;
        }
        if (s == 2) return sc_fold(sc_ld(tb.E, i0), sc_ld(tb.E, i1), r);
        if (s == 3) return sc_fold(sc_ld(tb.E2, i0), sc_ld(tb.E2, i1), r);
        const Ext one = ext_one();
        if (s == 0) return i0 == 0 ? ext_sub(one, r) : ext_zero();   // first: (1, 0) on pair 0
        return i1 == n - 1 ? r : ext_zero();                          // last: (0, 1) on the last pair
    }
    return sc_fold(sc_ld(tb.src, t * tb.src_stride + 2 * e), sc_ld(tb.src, t * tb.src_stride + 2 * e + 1), r);
}

// partial null: fold only (the last fold, nd = 1).  Every thread evaluates the pair whose two entries it has just written.
template <unsigned D, bool FROM_BASE, bool BUS, bool PREP>
__device__ __forceinline__ void zc_pass_body(const ZcProg& pg, const ZcTabs& tb, const ZcPrep& pp, const uint32_t* __restrict__ r_ptr,
                                             uint32_t* __restrict__ partial, unsigned wg, unsigned n_wg) {
    extern __shared__ uint4 zc_xslots[];   // [slot][lane]
    const unsigned lane = threadIdx.x, t_first = tb.w + tb.n_rot + (PREP ? pp.wp + pp.n_rot : 0u), nt = t_first + (BUS ? 4 : 3);
    const Ext r = sc_ld(r_ptr, 0), one = ext_one();
    const size_t n_pairs = tb.nd > 1 ? tb.nd >> 1 : 1;
    Ext acc[D];
#pragma unroll
    for (unsigned e = 0; e < D; e++) acc[e] = ext_zero();
    for (size_t y = (size_t)wg * ZC_W + lane; y < n_pairs; y += (size_t)n_wg * ZC_W) {
        for (unsigned t = 0; t < nt; t++) {
            sc_st(tb.dst, t * tb.dst_stride + 2 * y, zc_fold_entry<FROM_BASE, PREP>(tb, pp, t, 2 * y, r));
            if (2 * y + 1 < tb.nd) sc_st(tb.dst, t * tb.dst_stride + 2 * y + 1, zc_fold_entry<FROM_BASE, PREP>(tb, pp, t, 2 * y + 1, r));
        }
        if (!partial) continue;
        const Ext e0 = sc_ld(tb.dst, (t_first + 2) * tb.dst_stride + 2 * y), e1 = sc_ld(tb.dst, (t_first + 2) * tb.dst_stride + 2 * y + 1);
        const Ext de = ext_sub(e1, e0);
        Ext et = e0;
        Ext b0, b1, db, bt;   // BUS: the second eq factor
        if (BUS) {
            b0 = sc_ld(tb.dst, (t_first + 3) * tb.dst_stride + 2 * y), b1 = sc_ld(tb.dst, (t_first + 3) * tb.dst_stride + 2 * y + 1);
            db = ext_sub(b1, b0), bt = b0;
        }
#pragma unroll
        for (unsigned p = 0; p < D; p++) {
            const uint32_t tm = zc_small(p ? p + 1 : 0);
            auto table_at = [&](unsigned t) -> Ext {
                const Ext f0 = sc_ld(tb.dst, t * tb.dst_stride + 2 * y), f1 = sc_ld(tb.dst, t * tb.dst_stride + 2 * y + 1);
                return ext_add(f0, ext_mul_base(ext_sub(f1, f0), tm));
            };
            auto operand = [&](uint32_t w) -> Ext {
                const uint32_t pay = w & 0x0fffffffu;
                switch (w >> 28) {
                    case K_SLOT:
                        return ext_unpack(zc_xslots[pay * ZC_W + lane]);
                    case K_VAR:
                        return table_at(pay);
                    case K_PUB:
                        return ext_from_base(pg.pvs[pay]);
                    case K_CONST:
                        return ext_from_base(pg.consts[pay]);
                    default:
                        return pay == 0 ? table_at(t_first) : pay == 1 ? table_at(t_first + 1) : ext_sub(one, table_at(t_first + 1));
                }
            };
            Ext comb = ext_zero(), comb2 = ext_zero();
            for (unsigned i = 0; i < pg.n_ins; i++) {
                const uint32_t w0 = pg.code[3 * i], op = w0 & 0xffu, dst = w0 >> 8;
                const Ext a = operand(pg.code[3 * i + 1]);
                if (op == Q_ASSERT) {
                    if (BUS && dst >= pg.n_cons) comb2 = ext_add(comb2, ext_mul(sc_ld(pg.bcoef, dst - pg.n_cons), a));
                    else comb = ext_add(comb, ext_mul(sc_ld(pg.apow, dst), a));
                    continue;
                }
                const Ext b = op == Q_NEG ? ext_zero() : operand(pg.code[3 * i + 2]);
                zc_xslots[dst * ZC_W + lane] = ext_pack(op == Q_ADD ? ext_add(a, b) : op == Q_SUB ? ext_sub(a, b) : op == Q_MUL ? ext_mul(a, b) : ext_neg(a));
            }
            if (p) et = ext_add(p == 1 ? e1 : et, de);
            acc[p] = ext_add(acc[p], ext_mul(comb, et));
            if (BUS) {
                if (p) bt = ext_add(p == 1 ? b1 : bt, db);
                acc[p] = ext_add(acc[p], ext_mul(comb2, bt));
            }
        }
    }
    if (!partial) return;   // uniform across the workgroup's share
    zc_wave_out(acc, partial, wg);
}
template <unsigned D, bool FROM_BASE, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zc_pass(ZcProg pg, ZcTabs tb, const uint32_t* __restrict__ r_ptr, uint32_t* __restrict__ partial) {
    zc_pass_body<D, FROM_BASE, BUS, false>(pg, tb, ZcPrep{}, r_ptr, partial, blockIdx.x, gridDim.x);
}
// PREP: the extension passes' code names the preprocessed tables in K_VAR operands (zc_prove_air's remap), so only the table count differs
template <unsigned D, bool FROM_BASE, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zc_pass_p(ZcProg pg, ZcTabs tb, ZcPrep pp, const uint32_t* __restrict__ r_ptr, uint32_t* __restrict__ partial) {
    zc_pass_body<D, FROM_BASE, BUS, true>(pg, tb, pp, r_ptr, partial, blockIdx.x, gridDim.x);
}

// entry 0 of the first `cnt` tables, canonical, to out[4 t ..]
static __global__ __launch_bounds__(256) void k_zc_emit(const uint32_t* __restrict__ tab, size_t stride, unsigned cnt, uint32_t* __restrict__ out) {
    for (unsigned i = threadIdx.x; i < 4 * cnt; i += 256) out[i] = from_monty(tab[4 * (size_t)(i >> 2) * stride + (i & 3u)]);
}

// ---- the rotation reduction ------------------------------------------------------------------------------------------------------
// F_a = sum_j lambda^j col_j and F_b = sum_t lambda^(w + t) col_{j_t} (k_whir_combine's pattern, the powers from a table); PREP: the
// powers run on over [v_p | v_p'], F_a gains the preprocessed columns and F_b the rotated ones
template <bool PREP>
__device__ __forceinline__ void zc_combine_body(const uint32_t* __restrict__ trace, size_t n, unsigned w, const uint32_t* __restrict__ rot, unsigned n_rot,
                                                const ZcPrep& pp, const uint32_t* __restrict__ lpow, uint32_t* __restrict__ fa,
                                                uint32_t* __restrict__ fb) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        Ext a = ext_zero(), b = ext_zero();
        for (unsigned j = 0; j < w; j++) a = ext_add(a, ext_mul_base(sc_ld(lpow, j), trace[(size_t)j * n + i]));
        for (unsigned t = 0; t < n_rot; t++) b = ext_add(b, ext_mul_base(sc_ld(lpow, w + t), trace[(size_t)rot[t] * n + i]));
        if (PREP) {
            const unsigned o = w + n_rot;
            for (unsigned j = 0; j < pp.wp; j++) a = ext_add(a, ext_mul_base(sc_ld(lpow, o + j), pp.cols[(size_t)j * n + i]));
            for (unsigned t = 0; t < pp.n_rot; t++) b = ext_add(b, ext_mul_base(sc_ld(lpow, o + pp.wp + t), pp.cols[(size_t)pp.rot[t] * n + i]));
        }
        sc_st(fa, i, a), sc_st(fb, i, b);
    }
}
static __global__ __launch_bounds__(256) void k_zc_combine(const uint32_t* __restrict__ trace, size_t n, unsigned w, const uint32_t* __restrict__ rot,
                                                    unsigned n_rot, const uint32_t* __restrict__ lpow, uint32_t* __restrict__ fa,
                                                    uint32_t* __restrict__ fb) {
    zc_combine_body<false>(trace, n, w, rot, n_rot, ZcPrep{}, lpow, fa, fb);
}
static __global__ __launch_bounds__(256) void k_zc_combine_p(const uint32_t* __restrict__ trace, size_t n, unsigned w, const uint32_t* __restrict__ rot,
                                                      unsigned n_rot, ZcPrep pp, const uint32_t* __restrict__ lpow, uint32_t* __restrict__ fa,
                                                      uint32_t* __restrict__ fb) {
    zc_combine_body<true>(trace, n, w, rot, n_rot, pp, lpow, fa, fb);
}

// its four tables before the second round's fold writes them out: F_a, eq(r, .), F_b, rot(r, .)[x] = eq(r, .)[(x - 1) mod n]
struct ZcRotSrc {
    const uint32_t *fa, *fb, *E;
    size_t mask;
    __device__ __forceinline__ Ext operator()(unsigned t, size_t j) const {
        return t == 0 ? sc_ld(fa, j) : t == 1 ? sc_ld(E, j) : t == 2 ? sc_ld(fb, j) : sc_ld(E, (j - 1) & mask);
    }
};
// s(x) = sum_y F_a eq + F_b rot at 0, 2
struct ZcRotRound {
    static constexpr unsigned T = 4, E = 2;
    __device__ __forceinline__ void load() {}
    __device__ __forceinline__ Ext operator()(const Ext* v) const { return ext_add(ext_mul(v[0], v[1]), ext_mul(v[2], v[3])); }
};

// the last `rounds` rounds in ONE workgroup: the four tables, n <= ZC_T entries after folding with r_prev (if given), in LDS
template <class Src>
__global__ __launch_bounds__(SC_SW) void k_zc_rot_small(DevTranscript* tr, Src src, const uint32_t* __restrict__ r_prev, unsigned n, unsigned rounds,
                                                        uint32_t* __restrict__ proof_out, uint32_t* __restrict__ r_out) {
    __shared__ uint4 X4[4 * ZC_T];
    __shared__ uint32_t s_r[4];
    uint32_t* X = reinterpret_cast<uint32_t*>(X4);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Ext r = r_prev ? sc_ld(r_prev, 0) : ext_zero();
    for (unsigned i = tid; i < n; i += SC_SW)
#pragma unroll
        for (unsigned t = 0; t < 4; t++) sc_st(X, t * ZC_T + i, r_prev ? sc_fold(src(t, 2 * (size_t)i), src(t, 2 * (size_t)i + 1), r) : src(t, i));
    CoopConsts cc;
    TrRegs R{};
    if (wave == 0) cc = coop_load_consts(lane & 15u), R = tr_load(tr, lane);
    zk_syncthreads();
    for (unsigned t = 0; t < rounds; t++, n >>= 1) sc_small_round(ZcRotRound{}, X, ZC_T, n, R, cc, proof_out + 8 * t, r_out + 4 * t, s_r);
    if (wave == 0) tr_store(tr, R, lane);
}

// workgroup j: u_j = sum_i col_j[i] E[i], canonical, to out[4 j ..]
static __global__ __launch_bounds__(256) void k_zc_dot(const uint32_t* __restrict__ trace, size_t n, const uint32_t* __restrict__ E, uint32_t* __restrict__ out) {
    __shared__ uint32_t s[4];
    const uint32_t* col = trace + (size_t)blockIdx.x * n;
    Ext acc[1] = {ext_zero()};
    for (size_t i = threadIdx.x; i < n; i += 256) acc[0] = ext_add(acc[0], ext_mul_base(sc_ld(E, i), col[i]));
    sc_block_sum(acc, s, 1);
    zk_syncthreads();
    if (threadIdx.x < 4) out[4 * (size_t)blockIdx.x + threadIdx.x] = from_monty(s[threadIdx.x]);
}

// ---- host side: what prover and verifier derive from a program ---------------------------------------------------------------------
namespace {
unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(SC_NB, (n + 255) / 256)); }
unsigned grid_w(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(SC_NB, (n + ZC_W - 1) / ZC_W)); }

struct ZcPlan {
    AirProgram prog;
    unsigned m = 0, D = 0;
    size_t w = 0;
    std::vector<uint32_t> proven;   // node of every proven constraint, program order
    std::vector<uint32_t> rot;      // the columns the proven constraints read with rotation 1, increasing
    std::vector<int> rot_of;        // column -> its place in rot, or -1
    std::vector<char> reach;        // nodes the proven constraints reach
    // the keyed proofs only (zc_plan keyed): the preprocessed width, the preprocessed columns read with rotation 1, increasing
    size_t wp = 0;
    std::vector<uint32_t> rot_p;
    std::vector<int> rot_p_of;
    // the AIR-set proof only (zc_plan with_bus): the roots of the bus part, per interaction its count node, then its field nodes
    std::vector<uint32_t> bus_roots;
    std::vector<char> bus_reach;    // nodes the bus roots reach
    bool active() const { return D > 0; }
    bool reduces() const { return !rot.empty() || !rot_p.empty(); }
    size_t words() const { return 4 * (size_t)D * m + 4 * (w + rot.size() + wp + rot_p.size()) + (reduces() ? 8 * (size_t)m + 4 * (w + wp) : 0); }
};

// with_bus: D = max(d_cons, d_bus) + 1 over the parts that exist, d_bus the largest degree of a count or field node.
// keyed: a PREP section is taken, its cells are proven like main cells (degree 1); without it PREP is refused
bool zc_plan(const zkhip_air& a, ZcPlan* p, bool with_bus, bool keyed = false) {
    if (!a.program || a.width < 1 || a.log_height < 1 || a.log_height > ZKHIP_WHIR_MAX_LOG_N) return false;
    if (parse_air(a.program, a.program_len, a.width, &p->prog, nullptr) != 0) return false;
    const AirProgram& g = p->prog;
    if ((g.prep_width && !keyed) || g.n_pvs != a.n_pvs) return false;
    p->m = a.log_height, p->w = a.width, p->wp = g.prep_width;
    // multilinear degrees in the row index (is_transition = 1 - is_last counts 1); a node that reaches a LogUp-phase leaf is not proven
    std::vector<unsigned> deg(g.n_nodes, 0);
    std::vector<char> later(g.n_nodes, 0);
    for (uint32_t i = 0; i < g.n_nodes; i++) {
        const uint32_t op = g.nodes[3 * i], x = g.nodes[3 * i + 1], y = g.nodes[3 * i + 2];
        switch (op) {
            case A_VAR:
            case A_PREP:
            case A_FIRST:
            case A_LAST:
            case A_TRANS:
                deg[i] = 1;
                break;
            case A_PUB:
            case A_CONST:
                break;
            case A_ADD:
            case A_SUB:
                deg[i] = std::max(deg[x], deg[y]), later[i] = later[x] | later[y];
                break;
            case A_MUL:
                deg[i] = deg[x] + deg[y], later[i] = later[x] | later[y];
                break;
            case A_NEG:
                deg[i] = deg[x], later[i] = later[x];
                break;
            default:   // PERM, CHAL, EXPOSED
                later[i] = 1;
        }
    }
    unsigned d = 0;
    p->reach.assign(g.n_nodes, 0);
    for (uint32_t k = 0; k < g.n_cons; k++)
        if (!later[g.cons[k]]) p->proven.push_back(g.cons[k]), p->reach[g.cons[k]] = 1, d = std::max(d, deg[g.cons[k]]);
    p->rot_of.assign(p->w, -1), p->rot_p_of.assign(p->wp, -1);
    for (uint32_t i = g.n_nodes; i-- > 0;) {
        if (!p->reach[i]) continue;
        const uint32_t op = g.nodes[3 * i], x = g.nodes[3 * i + 1], y = g.nodes[3 * i + 2];
        if (op == A_VAR && y == 1) p->rot_of[x] = 0;
        if (op == A_PREP && y == 1) p->rot_p_of[x] = 0;
        if (op >= A_ADD && op <= A_NEG) {
            p->reach[x] = 1;
            if (op != A_NEG) p->reach[y] = 1;
        }
    }
    for (size_t c = 0; c < p->w; c++)
        if (p->rot_of[c] == 0) p->rot_of[c] = (int)p->rot.size(), p->rot.push_back((uint32_t)c);
    for (size_t c = 0; c < p->wp; c++)
        if (p->rot_p_of[c] == 0) p->rot_p_of[c] = (int)p->rot_p.size(), p->rot_p.push_back((uint32_t)c);
    p->D = p->proven.empty() ? 0 : d + 1;
    if (with_bus && !g.ints.empty()) {
        unsigned d_bus = 0;
        for (const Interaction& it : g.ints) {
            p->bus_roots.push_back(it.count), d_bus = std::max(d_bus, deg[it.count]);
            for (uint32_t i = 0; i < it.n_fields; i++) p->bus_roots.push_back(it.fields[i]), d_bus = std::max(d_bus, deg[it.fields[i]]);
        }
        p->D = std::max(p->D, d_bus + 1);
        p->bus_reach.assign(g.n_nodes, 0);
        for (uint32_t r : p->bus_roots) p->bus_reach[r] = 1;
        for (uint32_t i = g.n_nodes; i-- > 0;) {
            const uint32_t op = g.nodes[3 * i];
            if (!p->bus_reach[i] || op < A_ADD || op > A_NEG) continue;
            p->bus_reach[g.nodes[3 * i + 1]] = 1;
            if (op != A_NEG) p->bus_reach[g.nodes[3 * i + 2]] = 1;
        }
    }
    return p->D <= ZKHIP_ZEROCHECK_MAX_DEGREE;
}

// ---- the device prover ---------------------------------------------------------------------------------------------------------
template <unsigned D, bool BUS, bool PREP>
void zc_launch_d(hipStream_t st, int which, unsigned grid, size_t lds, const ZcProg& pg, const ZcTabs& tb, const ZcPrep& pp, const uint32_t* r,
                 uint32_t* partial, DevTranscript* d_t, uint32_t* proof, uint32_t* r_out) {
    if (which == 3) {
        hipLaunchKernelGGL(k_sc_round_tr<4 * D>, dim3(1), dim3(64), 0, st, d_t, (const uint32_t*)partial, grid, proof, r_out);
    } else if (PREP) {
        if (which == 0) hipLaunchKernelGGL((k_zc_round0_p<D, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb.trace, pp.cols, tb.m, tb.E, tb.E2, partial);
        else if (which == 1) hipLaunchKernelGGL((k_zc_pass_p<D, true, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb, pp, r, partial);
        else hipLaunchKernelGGL((k_zc_pass_p<D, false, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb, pp, r, partial);
    } else {
        if (which == 0) hipLaunchKernelGGL((k_zc_round0<D, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb.trace, tb.m, tb.E, tb.E2, partial);
        else if (which == 1) hipLaunchKernelGGL((k_zc_pass<D, true, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb, r, partial);
        else hipLaunchKernelGGL((k_zc_pass<D, false, BUS>), dim3(grid), dim3(ZC_W), lds, st, pg, tb, r, partial);
    }
}
// which: 0 = round 0, 1 = pass from the base trace, 2 = pass on tables, 3 = the transcript step (grid = the pass's workgroups)
template <bool BUS, bool PREP>
void zc_launch(unsigned D, hipStream_t st, int which, unsigned grid, size_t lds, const ZcProg& pg, const ZcTabs& tb, const ZcPrep& pp, const uint32_t* r,
               uint32_t* partial, DevTranscript* d_t = nullptr, uint32_t* proof = nullptr, uint32_t* r_out = nullptr) {
    switch (D) {
#define ZC_CASE(d) \
    case d:        \
        return zc_launch_d<d, BUS, PREP>(st, which, grid, lds, pg, tb, pp, r, partial, d_t, proof, r_out);
        ZC_CASE(1) ZC_CASE(2) ZC_CASE(3) ZC_CASE(4) ZC_CASE(5) ZC_CASE(6) ZC_CASE(7) ZC_CASE(8)
#undef ZC_CASE
    }
}

// the bus part of the AIR-set proof's joint sum-check (device): eq(rho_a, .) (2^m entries) and the coefficients of pl.bus_roots
struct ZcBus {
    const uint32_t* E2;
    const uint32_t* coef;
};

// one AIR's part: the words at dP (device, canonical), its point r' at d_rp (4 m Montgomery words).  BUS: the joint sum-check of
// docs/airset.md on the proven constraints and pl.bus_roots (tau and alpha are sampled only if there are proven constraints).
// PREP (the keyed proofs): `prep` holds the key's pl.wp preprocessed columns of this AIR, Montgomery, stride 2^m; their values follow
// v and v', and u_p follows u
template <bool BUS, bool PREP = false>
int zc_prove_air(zkhip_ctx* ctx, DevTranscript* d_t, const ZcPlan& pl, const uint32_t* trace, const uint32_t* pvs, uint32_t* dP, uint32_t* d_rp,
                 const ZcBus& bus = ZcBus{}, const uint32_t* prep = nullptr) {
    hipStream_t st = ctx->stream;
    const unsigned m = pl.m, D = pl.D, w = (unsigned)pl.w, n_rot = (unsigned)pl.rot.size(), n_cons = (unsigned)pl.proven.size();
    const unsigned wp = PREP ? (unsigned)pl.wp : 0, n_rot_p = PREP ? (unsigned)pl.rot_p.size() : 0, n_val = w + n_rot + wp + n_rot_p;
    const unsigned nt = n_val + (BUS ? 4 : 3);
    const size_t n = (size_t)1 << m;
    if (!pl.active()) return transcript_sample(ctx, d_t, d_rp, nullptr, 4 * m);
    std::vector<uint32_t> roots = pl.proven;
    if (BUS) roots.insert(roots.end(), pl.bus_roots.begin(), pl.bus_roots.end());
    // the lowered program, once for the base round and once with tables in place of cells
    CompiledAir ca;
    std::string err;
    if (compile_air(pl.prog, &ca, &err, &roots) != 0 || ca.n_slots > ZC_MAX_SLOTS)
        return set_error(ctx, ZKHIP_ERR_INVALID, "zerocheck: " + (err.empty() ? "the AIR needs more than 64 live intermediates" : err));
    const size_t n_code = ca.code.size(), n_ins = n_code / 3;
    std::vector<uint32_t> up(2 * n_code + ca.consts.size() + pl.prog.n_pvs + n_rot + n_rot_p);
    std::copy(ca.code.begin(), ca.code.end(), up.begin());
    for (size_t i = 0; i < n_ins; i++) {
        uint32_t* x = up.data() + n_code + 3 * i;
        x[0] = ca.code[3 * i];
        for (int k = 1; k < 3; k++) {
            const uint32_t o = ca.code[3 * i + k];
            x[k] = (o >> 28) != K_VAR ? o : (K_VAR << 28) | (((o >> 27) & 1u) ? w + (uint32_t)pl.rot_of[o & 0x07ffffffu] : (o & 0x07ffffffu));
            if (PREP && (o >> 28) == K_PREP)   // the preprocessed tables follow the main ones
                x[k] = (K_VAR << 28) | (w + n_rot + (((o >> 27) & 1u) ? wp + (uint32_t)pl.rot_p_of[o & 0x07ffffffu] : (o & 0x07ffffffu)));
        }
    }
    uint32_t* hp = up.data() + 2 * n_code;
    std::copy(ca.consts.begin(), ca.consts.end(), hp), hp += ca.consts.size();
    for (uint32_t i = 0; i < pl.prog.n_pvs; i++) *hp++ = to_monty(pvs[i]);
    hp = std::copy(pl.rot.begin(), pl.rot.end(), hp);
    if (PREP) std::copy(pl.rot_p.begin(), pl.rot_p.end(), hp);
    DevBufs B(ctx);
    // challenges: [tau (4 m) | alpha (4) | r (4 m) | lambda (4)]
    uint32_t *d_up = B.get(up.size()), *ch = B.get(8 * (size_t)m + 8), *apow = B.get(4 * (size_t)std::max(n_cons, n_val));
    uint32_t *E = B.get(4 * n), *partial = B.get(4 * (size_t)ZKHIP_ZEROCHECK_MAX_DEGREE * SC_NB);
    uint32_t *tA = B.get(4 * (size_t)nt * (n / 2)), *tB = B.get(4 * (size_t)nt * std::max<size_t>(n / 4, 1));
    if (!d_up || !ch || !apow || !E || !partial || !tA || !tB) return set_error(ctx, ZKHIP_ERR_NOMEM, "zerocheck: the folded tables do not fit");
    uint32_t *tau = ch, *alpha = ch + 4 * m, *rs = alpha + 4, *lambda = rs + 4 * m;
    ZK_TRY(zkhip_h2d(ctx, d_up, up.data(), up.size() * 4));
    if (n_cons) {
        ZK_TRY(transcript_sample(ctx, d_t, tau, nullptr, 4 * m + 4));
        KernelScope ks(ctx, "zc_eq");
        whir_eq_launch(st, E, m, tau);
    }
    if (n_cons) {
        KernelScope ks(ctx, "zc_pows");
        hipLaunchKernelGGL(k_zc_pows, dim3(1), dim3(256), 0, st, (const uint32_t*)alpha, n_cons, apow);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ZcProg pg{d_up, (unsigned)n_ins, d_up + 2 * n_code, d_up + 2 * n_code + ca.consts.size(), apow, bus.coef, n_cons};
    ZcProg pgx = pg;
    pgx.code = d_up + n_code;
    ZcTabs tb{};
    tb.trace = trace, tb.E = n_cons ? E : bus.E2, tb.E2 = bus.E2, tb.rot = d_up + up.size() - n_rot - n_rot_p, tb.m = m, tb.w = w, tb.n_rot = n_rot;
    const ZcPrep pp{prep, d_up + up.size() - n_rot_p, wp, n_rot_p};
    const size_t sA = n / 2, sB = std::max<size_t>(n / 4, 1);
    uint32_t* cur = nullptr;   // the tables the last pass wrote
    size_t cur_stride = 0;
    for (unsigned i = 0; i <= m; i++) {   // round i; i = m: the last fold only
        const bool fold_only = i == m;
        unsigned grid;
        if (i == 0) {
            grid = grid_w(n / 2);
            KernelScope ks(ctx, "zc_round0");
            zc_launch<BUS, PREP>(D, st, 0, grid, (size_t)ca.n_slots * ZC_W * 4, pg, tb, pp, nullptr, partial);
        } else {
            tb.nd = n >> i;
            tb.src = cur, tb.src_stride = cur_stride;
            tb.dst = cur == tA ? tB : tA, tb.dst_stride = tb.dst == tA ? sA : sB;
            grid = grid_w(tb.nd > 1 ? tb.nd / 2 : 1);
            KernelScope ks(ctx, "zc_pass");
            zc_launch<BUS, PREP>(D, st, i == 1 ? 1 : 2, grid, (size_t)ca.n_slots * ZC_W * 16, pgx, tb, pp, rs + 4 * (i - 1), fold_only ? nullptr : partial);
            cur = tb.dst, cur_stride = tb.dst_stride;
        }
        if (!fold_only) {
            KernelScope ks(ctx, "zc_round_tr");
            zc_launch<BUS, PREP>(D, st, 3, grid, 0, pg, tb, pp, nullptr, partial, d_t, dP + 4 * (size_t)D * i, rs + 4 * i);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    uint32_t* dV = dP + 4 * (size_t)D * m;   // v, v' (PREP: v_p, v_p')
    {
        KernelScope ks(ctx, "zc_emit");
        hipLaunchKernelGGL(k_zc_emit, dim3(1), dim3(256), 0, st, (const uint32_t*)cur, cur_stride, n_val, dV);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ZK_TRY(transcript_observe(ctx, d_t, dV, 4 * n_val, true));
    if (n_rot + n_rot_p == 0) {
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(d_rp, rs, 16 * (size_t)m, hipMemcpyDeviceToDevice, st));
        return ZKHIP_OK;
    }
    // the rotation reduction: a degree-2 sum-check on F_a eq(r, .) + F_b rot(r, .), the folded tables in tA (4 x n/2) and tB (4 x n/4)
    uint32_t *fa = B.get(4 * n), *fb = B.get(4 * n);
    if (!fa || !fb) return set_error(ctx, ZKHIP_ERR_NOMEM, "zerocheck: the reduction's tables do not fit");
    uint32_t* dR = dV + 4 * n_val;   // the reduction's rounds, then u (PREP: u_p)
    ZK_TRY(transcript_sample(ctx, d_t, lambda, nullptr, 4));
    {
        KernelScope ks(ctx, "zc_pows");
        hipLaunchKernelGGL(k_zc_pows, dim3(1), dim3(256), 0, st, (const uint32_t*)lambda, n_val, apow);
    }
    {
        KernelScope ks(ctx, "zc_eq");
        whir_eq_launch(st, E, m, rs);
    }
    {
        KernelScope ks(ctx, "zc_combine");
        if (PREP) hipLaunchKernelGGL(k_zc_combine_p, dim3(grid_of(n)), dim3(256), 0, st, trace, n, w, tb.rot, n_rot, pp, (const uint32_t*)apow, fa, fb);
        else hipLaunchKernelGGL(k_zc_combine, dim3(grid_of(n)), dim3(256), 0, st, trace, n, w, tb.rot, n_rot, (const uint32_t*)apow, fa, fb);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    const ZcRotSrc src{fa, fb, E, n - 1};
    uint32_t* tabs[2][4];
    for (unsigned t = 0; t < 4; t++) tabs[0][t] = tA + 4 * (size_t)t * sA, tabs[1][t] = tB + 4 * (size_t)t * sB;
    int at = -1;   // which of tabs holds the folded tables
    const uint32_t* pending = nullptr;
    size_t sz = n;   // entries after the pending fold
    unsigned t = 0;
    for (; t < m && sz > ZC_T; t++, sz >>= 1) {
        {
            KernelScope ks(ctx, "zc_rot_pass");
            if (t < 2) {
                ScPass<ZcRotSrc, ZcRotRound> p{};
                p.src = src, p.r = pending, p.n_pairs = sz / 2, p.partial = partial;
                for (unsigned q = 0; q < 4; q++) p.dst[q] = tabs[0][q];
                hipLaunchKernelGGL(k_sc_pass, dim3(grid_of(sz / 2)), dim3(256), 0, st, p);
            } else {
                ScPass<ScTables<4>, ZcRotRound> p{};
                p.r = pending, p.n_pairs = sz / 2, p.partial = partial;
                for (unsigned q = 0; q < 4; q++) p.src.tab[q] = tabs[at][q], p.dst[q] = tabs[at ^ 1][q];
                hipLaunchKernelGGL(k_sc_pass, dim3(grid_of(sz / 2)), dim3(256), 0, st, p);
            }
        }
        {
            KernelScope ks(ctx, "zc_round_tr");
            hipLaunchKernelGGL(k_sc_round_tr<8>, dim3(1), dim3(64), 0, st, d_t, (const uint32_t*)partial, grid_of(sz / 2), dR + 8 * t, d_rp + 4 * t);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
        if (pending) at = at < 0 ? 0 : at ^ 1;
        pending = d_rp + 4 * t;
    }
    if (t < m) {
        KernelScope ks(ctx, "zc_rot_small");
        if (t < 2) {
            hipLaunchKernelGGL(k_zc_rot_small<ZcRotSrc>, dim3(1), dim3(SC_SW), 0, st, d_t, src, pending, (unsigned)sz, m - t, dR + 8 * t, d_rp + 4 * t);
        } else {
            ScTables<4> s4{};
            for (unsigned q = 0; q < 4; q++) s4.tab[q] = tabs[at][q];
            hipLaunchKernelGGL(k_zc_rot_small<ScTables<4>>, dim3(1), dim3(SC_SW), 0, st, d_t, s4, pending, (unsigned)sz, m - t, dR + 8 * t, d_rp + 4 * t);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    uint32_t* dU = dR + 8 * (size_t)m;
    {
        KernelScope ks(ctx, "zc_eq");
        whir_eq_launch(st, E, m, d_rp);
    }
    {
        KernelScope ks(ctx, "zc_dot");
        hipLaunchKernelGGL(k_zc_dot, dim3(w), dim3(256), 0, st, trace, n, (const uint32_t*)E, dU);
        if (wp) hipLaunchKernelGGL(k_zc_dot, dim3(wp), dim3(256), 0, st, prep, n, (const uint32_t*)E, dU + 4 * w);   // u_p: the key's columns
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return transcript_observe(ctx, d_t, dU, 4 * (w + wp), true);
}

// ---- the host verifier ---------------------------------------------------------------------------------------------------------
// rot(a, b): the multilinear extension of the successor relation b = a + 1 mod 2^m
Ext zc_rot_eval(const Ext* a, const Ext* b, unsigned m) {
    const Ext one = ext_one();
    std::vector<Ext> lo(m + 1), hi(m + 1);   // lo[k] = prod_{j<k} a_j (1 - b_j), hi[k] = prod_{j>=k} eq(a_j, b_j)
    lo[0] = one, hi[m] = one;
    for (unsigned j = 0; j < m; j++) lo[j + 1] = ext_mul(lo[j], ext_mul(a[j], ext_sub(one, b[j])));
    for (unsigned j = m; j-- > 0;) hi[j] = ext_mul(hi[j + 1], eq_eval(a + j, b + j, 1));
    Ext acc = lo[m];
    for (unsigned k = 0; k < m; k++) acc = ext_add(acc, ext_mul(ext_mul(lo[k], ext_mul(ext_sub(one, a[k]), b[k])), hi[k + 1]));
    return acc;
}

// the nodes marked in `reach` (pl.reach or pl.bus_reach) on (v, v', first, last, pvs); the others stay 0.  A keyed plan's PREP leaves
// read vp and vpn (v_p, v_p')
std::vector<Ext> zc_eval_host(const ZcPlan& pl, const std::vector<char>& reach, const Ext* v, const Ext* vn, const Ext& first, const Ext& last,
                              const uint32_t* pvs, const Ext* vp = nullptr, const Ext* vpn = nullptr) {
    const AirProgram& g = pl.prog;
    std::vector<Ext> val(g.n_nodes, ext_zero());
    for (uint32_t i = 0; i < g.n_nodes; i++) {
        if (!reach[i]) continue;
        const uint32_t op = g.nodes[3 * i], x = g.nodes[3 * i + 1], y = g.nodes[3 * i + 2];
        switch (op) {
            case A_VAR:
                val[i] = y ? vn[pl.rot_of[x]] : v[x];
                break;
            case A_PREP:
                val[i] = y ? vpn[pl.rot_p_of[x]] : vp[x];
                break;
            case A_PUB:
                val[i] = ext_from_base(to_monty(pvs[x]));
                break;
            case A_CONST:
                val[i] = ext_from_base(to_monty(x));
                break;
            case A_FIRST:
                val[i] = first;
                break;
            case A_LAST:
                val[i] = last;
                break;
            case A_TRANS:
                val[i] = ext_sub(ext_one(), last);
                break;
            case A_ADD:
                val[i] = ext_add(val[x], val[y]);
                break;
            case A_SUB:
                val[i] = ext_sub(val[x], val[y]);
                break;
            case A_MUL:
                val[i] = ext_mul(val[x], val[y]);
                break;
            default:
                val[i] = ext_neg(val[x]);
        }
    }
    return val;
}

}  // namespace

}  // namespace zk
