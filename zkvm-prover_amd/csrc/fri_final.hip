// fri_final.hip -- the FRI final-polynomial chip on the device (air.py fri_final_air, include/zkhip_chips.hpp; docs/fri_final.md): a query's
// last check, Horner over the L = 2^log_final_poly_len coefficients of the proof's final polynomial at the query's point, a row per
// coefficient from the highest down.  Every call has the same length L and L divides 256, so the launch is ONE kernel with one lane per
// trace row in workgroups of 256 lanes, and a call never straddles a workgroup: row r is row t = r & (L - 1) of call r >> lfp.  The
// accumulator column is a segmented inclusive scan under y -> y x + coef; x is uniform within a call, so step d of a Hillis-Steele scan is
// v_i = v_(i-d) x^d + v_i for t >= d -- one ext_mul_base a step, x^d squared between steps: six __shfl_up steps inside a wave for L <= 64,
// and for L = 128 / 256 the waves' carries go through LDS behind one barrier.  Consecutive lanes hold consecutive rows of every column, so
// the 19 column stores run along rows with no staging; the rows behind the last call (and a refused call's rows) are written as zeros by
// the kernel itself, so the trace needs no memset.  No workgroup waits on another.
#include "../../include/zkhip.h"
#include "babybear.hpp"
#include "fri_final_host.hpp"
#include "lds_barrier.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {

constexpr unsigned FF_COLS = ZKHIP_FRI_FINAL_WIDTH;
static_assert(FF_COLS == 19, "coef[4] | acc[4] | x | x_inv | xi2 | k | lvl | j | poly | is_first | is_last | is_real | call");
constexpr unsigned FF_MAX_LVL = 26;   // the bits of a pair index domain_point_air holds

// W_j and W_j^-1 in Montgomery form, W_j the generator of the subgroup of order 2^(j + 2) (air.domain_point_inverse_roots): bit j of k
// contributes W_j to g_(lvl+1)^bitrev(k, lvl) whatever lvl is.  x_inv is the product of the W_j^-1 over the set bits of k -- what
// domain_point_air holds for k -- and the point of index k in the domain of 2^lvl points is the square of the matching product of the W_j.
// (A second copy of the constants csrc/fri_query.hip holds: that file and its compiled kernels stay as they are.)
struct FfRoots {
    uint32_t w[FF_MAX_LVL], winv[FF_MAX_LVL];
};
constexpr uint64_t ff_cpow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    for (a %= P; e; e >>= 1, a = a * a % P)
        if (e & 1) r = r * a % P;
    return r;
}
constexpr FfRoots ff_roots() {
    FfRoots t{};
    for (unsigned j = 0; j < FF_MAX_LVL; j++) {
        const uint64_t w = ff_cpow(GEN_2_27_CANON, (uint64_t)1 << (27 - (j + 2)));
        t.w[j] = (uint32_t)(w * MONTY_ONE % P);
        t.winv[j] = (uint32_t)(ff_cpow(w, P - 2) * MONTY_ONE % P);
    }
    return t;
}
static __constant__ const FfRoots FF_W = ff_roots();

struct FfIn {
    const uint32_t *k, *lvl, *poly;   // per call
    const uint32_t* coef;             // [n_polys][L][4], ascending
    size_t n_polys, n_calls;
};

__device__ __forceinline__ Ext ff_shfl_up(const Ext& v, unsigned d) { return Ext{{__shfl_up(v.c[0], d), __shfl_up(v.c[1], d), __shfl_up(v.c[2], d), __shfl_up(v.c[3], d)}}; }

__global__ __launch_bounds__(256) void k_fri_final(FfIn in, unsigned lfp, size_t N, uint32_t* __restrict__ trace, uint32_t* __restrict__ value, uint32_t* __restrict__ bad) {
    __shared__ uint32_t carry[4][4];   // a wave's last accumulator, for the waves behind it in the same call (L = 128 / 256)
    const unsigned L = 1u << lfp, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x, c = r >> lfp;
    const unsigned t = (unsigned)r & (L - 1u), j = L - 1u - t;
    // the call's records: the call index is compared with n_calls before any use, d_poly[c] with n_polys, and no shift count exceeds 26.
    // Every lane stays to the end (the shuffles and the barrier take whole waves); a lane without a row of a good call holds zeros.
    bool real = false;
    uint32_t k = 0, lvl = 0, poly = 0;
    if (r < N && c < in.n_calls) {
        k = in.k[c], lvl = in.lvl[c], poly = in.poly[c];
        real = lvl - 1u < FF_MAX_LVL && (k >> lvl) == 0u && (size_t)poly < in.n_polys;
        if (!real && t == 0) atomicAdd(bad, 1u);
    }
    Ext co = ext_zero();
    uint32_t x = MONTY_ONE, xinv = MONTY_ONE;
    if (real) {
        const uint32_t* p = in.coef + (((size_t)poly << lfp) + j) * 4;
        co = Ext{{field_word(p[0], bad), field_word(p[1], bad), field_word(p[2], bad), field_word(p[3], bad)}};
#pragma unroll 1
        for (unsigned b = 0; b < FF_MAX_LVL && (k >> b); b++) {
            const bool set = (k >> b) & 1u;
            x = mmul(x, set ? FF_W.w[b] : MONTY_ONE), xinv = mmul(xinv, set ? FF_W.winv[b] : MONTY_ONE);
        }
        x = mmul(x, x);
    }
    // inside the wave: after the step of distance d, v_t = sum over the last min(t + 1, 2 d) rows i <= t of the call of coef_i x^(t - i)
    Ext v = co;
    uint32_t xp = x;                                      // x^d
    const unsigned span = L < 64u ? L : 64u;
#pragma unroll 1
    for (unsigned d = 1; d < span; d <<= 1) {
        const Ext u = ff_shfl_up(v, d);
        if ((lane & (span - 1u)) >= d) v = ext_add(ext_mul_base(u, xp), v);
        xp = mmul(xp, xp);
    }
    if (lfp > 6u) {                                       // (uniform: the whole launch has one L)
        // xp = x^64.  Wave wi of a call adds x^(lane + 1) times the accumulator behind the waves in front of it
        if (lane == 63u) carry[wave][0] = v.c[0], carry[wave][1] = v.c[1], carry[wave][2] = v.c[2], carry[wave][3] = v.c[3];
        zk_syncthreads();
        const unsigned wi = wave & ((L >> 6) - 1u);
        if (wi) {
            Ext cr = ext_zero();
            for (unsigned u = wave - wi; u < wave; u++) cr = ext_add(ext_mul_base(cr, xp), Ext{{carry[u][0], carry[u][1], carry[u][2], carry[u][3]}});
            v = ext_add(v, ext_mul_base(cr, mpow(x, lane + 1u)));
        }
    }
    if (r >= N) return;
    if (real) {
        const uint32_t xi2 = mmul(xinv, xinv);
#pragma unroll
        for (int i = 0; i < 4; i++) trace[(size_t)i * N + r] = co.c[i], trace[(size_t)(4 + i) * N + r] = v.c[i];
        trace[(size_t)8 * N + r] = x;
        trace[(size_t)9 * N + r] = xinv;
        trace[(size_t)10 * N + r] = xi2;
        trace[(size_t)11 * N + r] = to_monty(k);
        trace[(size_t)12 * N + r] = to_monty(lvl);
        trace[(size_t)13 * N + r] = to_monty(j);
        trace[(size_t)14 * N + r] = to_monty(poly);
        trace[(size_t)15 * N + r] = t == 0 ? MONTY_ONE : 0u;
        trace[(size_t)16 * N + r] = j == 0 ? MONTY_ONE : 0u;
        trace[(size_t)17 * N + r] = MONTY_ONE;
        trace[(size_t)18 * N + r] = to_monty((uint32_t)c);
        if (value && j == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) value[4 * c + i] = from_monty(v.c[i]);
        }
    } else {
#pragma unroll 1
        for (unsigned q = 0; q < FF_COLS; q++) trace[(size_t)q * N + r] = 0u;
        if (value && c < in.n_calls && j == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) value[4 * c + i] = 0u;
        }
    }
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_fri_final_host(unsigned log_final_poly_len, unsigned lvl, uint64_t k, const uint32_t* coef, uint32_t x_out[1], uint32_t value_out[4]) {
    return fri_final_canonical(log_final_poly_len, lvl, k, coef, x_out, value_out);
}

int zkhip_fri_final_tracegen(zkhip_ctx* ctx, unsigned log_final_poly_len, const uint32_t* d_k, const uint32_t* d_lvl, const uint32_t* d_poly, const uint32_t* d_coef,
                             size_t n_polys, size_t n_calls, unsigned log_height, uint32_t* d_trace, uint32_t* d_value) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || log_height > 27 || log_final_poly_len > ZKHIP_MAX_LOG_FINAL_POLY || (n_calls && (!d_k || !d_lvl || !d_poly || !d_coef))) return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    // (n_calls L > N, without the product: a trace shorter than one call holds none)
    if (n_calls > (N >> log_final_poly_len)) return set_error(ctx, ZKHIP_ERR_INVALID, "fri_final_tracegen: more calls than the trace has rows for");
    const FfIn in{d_k, d_lvl, d_poly, d_coef, n_polys, n_calls};
    return tracegen_frame(
        ctx, "fri_final_tracegen", {},
        [&](uint32_t* bad) { hipLaunchKernelGGL(k_fri_final, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, in, log_final_poly_len, N, d_trace, d_value, bad); },
        "fri_final_tracegen (lvl = 0 or > 26, k outside 2^lvl, a polynomial the table does not have, or a coefficient word that is not a field element)");
}

}  // extern "C"
