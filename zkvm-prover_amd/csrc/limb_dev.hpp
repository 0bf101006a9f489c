// limb_dev.hpp -- the device core of the limb chips' trace generators (csrc/modular.hip, fp2.hip, ecc.hip, int256.hip; docs/limb_core.md):
// byte limbs of word operands, the row writer, the emission of operand limbs, carries and "below the modulus" marks with their lookups,
// binary long division by the modulus, the signed accumulators of the identities with products of two operands, and the VM chips'
// timestamp column.  One lane per row throughout.  What a chip IS -- its record, its identities and their limb sums, its flags -- stays
// in the chip's own kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "babybear.hpp"
#include "hist.hpp"
#include "zkhip_internal.hpp"

namespace zk {

// byte i of a little-endian word array
__device__ __forceinline__ uint32_t limb_byte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// the cells of one row of a column-major trace of N rows (Montgomery form, as every cell)
struct RowWriter {
    uint32_t* trace;
    size_t N, row;
    __device__ __forceinline__ void put(size_t col, uint32_t v) const { trace[col * N + row] = to_monty(v); }
    __device__ __forceinline__ void zero(size_t width) const {   // a padding row
        for (size_t c = 0; c < width; c++) trace[c * N + row] = 0u;
    }
};

// LIMBS byte limbs of x at columns col .., and their byte pairs in the range column of the 8-bit table (an odd last byte pairs with 0)
template <int LIMBS>
__device__ __forceinline__ void emit_limbs(const RowWriter& w, size_t col, const uint32_t* x, uint32_t* bitwise_range) {
    for (int i = 0; i < LIMBS; i++) {
        w.put(col + i, limb_byte(x, i));
        if (!(i & 1)) hist_add(bitwise_range, limb_byte(x, i) * 256 + (i + 1 < LIMBS ? limb_byte(x, i + 1) : 0u));
    }
}

// The carries of one limb identity: position k of the chip's limb sum `sum(k)`, plus the carry in, is 256 times the carry out.  The
// first n_carry carries, shifted by the chip's offset, go to the columns cx .. / cy .. and into the tuple table (x < 256, y < tuple_y);
// one outside that range is written as 0 and refused.  An identity that does not hold (a sum that is no multiple of 256, a carry out of
// a position past n_carry) is refused too unless the row was refused already (`holds` false: the quotient did not fit).
template <class Sum>
__device__ __forceinline__ void emit_carries(const RowWriter& w, int n_pos, int n_carry, int64_t offset, uint32_t tuple_y, size_t cx, size_t cy, bool holds,
                                             uint32_t* tuple, uint32_t* bad, Sum&& sum) {
    int64_t c = 0;
    for (int k = 0; k < n_pos; k++) {
        const int64_t s = c + sum(k);
        if ((s & 255) != 0 && holds) atomicAdd(bad, 1u);
        c = s >> 8;
        if (k < n_carry) {
            const int64_t shifted = c + offset;
            const uint32_t v = shifted < 0 || shifted >= (int64_t)256 * tuple_y ? 0u : (uint32_t)shifted;
            if ((int64_t)v != shifted) atomicAdd(bad, 1u);
            w.put(cx + k, v & 255u), w.put(cy + k, v >> 8);
            hist_add(tuple, (v & 255u) * tuple_y + (v >> 8));
        } else if (c != 0 && holds) {
            atomicAdd(bad, 1u);
        }
    }
}

// x < p by its most significant limb that differs from p's: the L mark cells, the diff cell and the lookup of diff - 1 (with diff = 0 where
// there is no mark).  CHECKED is for values a record hands in (a division's quotient) or that may not be reduced: a value that is not
// below p gets no mark and is refused; with `on` false the cells are zero and there is no lookup.  The unchecked form is for remainders,
// which are below p by construction.
template <int L, bool CHECKED>
__device__ __forceinline__ void emit_below(const RowWriter& w, const uint32_t* x, const uint32_t* p, bool on, size_t mark_col, size_t diff_col,
                                           uint32_t* bitwise_range, uint32_t* bad) {
    int mark = -1;
    if (on)
        for (int i = L - 1; i >= 0; i--)
            if (limb_byte(x, i) != limb_byte(p, i)) {
                mark = !CHECKED || limb_byte(x, i) < limb_byte(p, i) ? i : -2;
                break;
            }
    if (CHECKED && on && mark < 0) atomicAdd(bad, 1u);
    for (int i = 0; i < L; i++) w.put(mark_col + i, i == mark ? 1u : 0u);
    const uint32_t diff = mark >= 0 ? limb_byte(p, mark) - limb_byte(x, mark) : 0u;
    w.put(diff_col, diff);
    if (on) hist_add(bitwise_range, ((diff - 1u) & 255u) * 256);
}

// v = quo p + rem, 0 <= rem < p, by 32 VW shift-compare-subtract steps (v of VW words, p of NW words, rem on NW + 1 words)
template <int NW, int VW, int QW = VW>
__device__ __forceinline__ bool divmod_bits(const uint32_t* v, const uint32_t* p, uint32_t* quo /*QW*/, uint32_t* rem /*NW + 1*/) {
    bool high = false;
#pragma unroll
    for (int i = 0; i <= NW; i++) rem[i] = 0;
#pragma unroll
    for (int i = 0; i < QW; i++) quo[i] = 0;
    for (int bit = 32 * VW - 1; bit >= 0; bit--) {
        for (int k = NW; k > 0; k--) rem[k] = (rem[k] << 1) | (rem[k - 1] >> 31);
        rem[0] = (rem[0] << 1) | ((v[bit >> 5] >> (bit & 31)) & 1u);
        bool ge = rem[NW] != 0;
        if (!ge) {
            ge = true;
            for (int k = NW - 1; k >= 0; k--)
                if (rem[k] != p[k]) {
                    ge = rem[k] > p[k];
                    break;
                }
        }
        if (ge) {
            uint32_t br = 0;
            for (int k = 0; k <= NW; k++) {
                const uint64_t d = (uint64_t)rem[k] - (k < NW ? p[k] : 0u) - br;
                rem[k] = (uint32_t)d, br = (uint32_t)(d >> 32) & 1u;
            }
            if (bit >= 32 * QW) high = true;
            else quo[bit >> 5] |= 1u << (bit & 31);
        }
    }
    return high;
}

// Signed accumulators (csrc/ecc.hip, csrc/fp2.hip): sums of products of two NW-word operands with signs (2 NW + 2 words, two's
// complement: 576 bits for 256-bit operands, 832 for 384-bit ones), and their division by an NW-word modulus into a signed quotient and
// the canonical residue.
template <int NW>
struct Signed {
    static constexpr int SW = 2 * NW + 2;   // words of a signed accumulator

    // v += sign * scale * x * y  (x, y NW words; scale small)
    __device__ static __forceinline__ void acc_product(uint32_t* v, const uint32_t* x, const uint32_t* y, int sign, uint32_t scale) {
        uint32_t prod[SW];
        for (int i = 0; i < SW; i++) prod[i] = 0;
        for (int i = 0; i < NW; i++) {
            uint64_t c = 0;
            for (int j = 0; j < NW; j++) {
                c += (uint64_t)x[i] * y[j] + prod[i + j];
                prod[i + j] = (uint32_t)c, c >>= 32;
            }
            prod[i + NW] = (uint32_t)c;
        }
        if (scale != 1) {
            uint64_t c = 0;
            for (int i = 0; i < SW; i++) c += (uint64_t)prod[i] * scale, prod[i] = (uint32_t)c, c >>= 32;
        }
        if (sign > 0) {
            uint64_t c = 0;
            for (int i = 0; i < SW; i++) c += (uint64_t)v[i] + prod[i], v[i] = (uint32_t)c, c >>= 32;
        } else {
            uint32_t br = 0;
            for (int i = 0; i < SW; i++) {
                const uint64_t d = (uint64_t)v[i] - prod[i] - br;
                v[i] = (uint32_t)d, br = (uint32_t)(d >> 32) & 1u;
            }
        }
    }
    // v += sign * x  (x NW words)
    __device__ static __forceinline__ void acc_word(uint32_t* v, const uint32_t* x, int sign) {
        if (sign > 0) {
            uint64_t c = 0;
            for (int i = 0; i < SW; i++) c += (uint64_t)v[i] + (i < NW ? x[i] : 0u), v[i] = (uint32_t)c, c >>= 32;
        } else {
            uint32_t br = 0;
            for (int i = 0; i < SW; i++) {
                const uint64_t d = (uint64_t)v[i] - (i < NW ? x[i] : 0u) - br;
                v[i] = (uint32_t)d, br = (uint32_t)(d >> 32) & 1u;
            }
        }
    }
    // v (signed) = sgn * (quo * p + rem) with 0 <= rem < p as a magnitude split; then the canonical residue of v and the signed quotient
    // with v - res = (neg ? -1 : 1) * q * p.  Returns false if q does not fit 4 NW + 1 bytes.
    __device__ static __forceinline__ bool signed_divmod(uint32_t* v, const uint32_t* p, uint32_t* q /*NW + 1*/, uint32_t* res /*NW*/, bool* neg) {
        *neg = (v[SW - 1] >> 31) != 0;
        if (*neg) {   // magnitude
            uint64_t c = 1;
            for (int i = 0; i < SW; i++) c += (uint64_t)(~v[i]), v[i] = (uint32_t)c, c >>= 32;
        }
        uint32_t rem[NW + 1], quo[SW];
        divmod_bits<NW, SW>(v, p, quo, rem);
        bool rem_zero = true;
        for (int k = 0; k < NW; k++) rem_zero = rem_zero && rem[k] == 0;
        if (*neg && !rem_zero) {   // -(quo p + rem) = -(quo + 1) p + (p - rem)
            uint32_t br = 0;
            for (int k = 0; k < NW; k++) {
                const uint64_t d = (uint64_t)p[k] - rem[k] - br;
                rem[k] = (uint32_t)d, br = (uint32_t)(d >> 32) & 1u;
            }
            uint64_t c = 1;
            for (int i = 0; i < SW; i++) c += quo[i], quo[i] = (uint32_t)c, c >>= 32;
        }
        bool fits = quo[NW] < 256u, q_zero = true;
        for (int i = NW + 1; i < SW; i++) fits = fits && quo[i] == 0;
        for (int i = 0; i <= NW; i++) q[i] = quo[i], q_zero = q_zero && quo[i] == 0;
        for (int k = 0; k < NW; k++) res[k] = rem[k];
        if (q_zero) *neg = false;   // one representation of zero
        return fits;
    }
};

// the VM chips' timestamp column: row i carries the timestamp of call i
static __global__ __launch_bounds__(256) void k_call_ts(const uint32_t* __restrict__ ts, size_t n, size_t N, uint32_t* __restrict__ col) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row < N) col[row] = row < n ? to_monty(ts[row] % P) : 0u;
}
inline int call_timestamps(zkhip_ctx* ctx, const char* scope, const uint32_t* d_ts, size_t n, unsigned log_height, uint32_t* d_col) {
    const size_t N = (size_t)1 << log_height;
    KernelScope ks(ctx, scope);
    hipLaunchKernelGGL(k_call_ts, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, d_ts, n, N, d_col);
    ZK_HIP_CHECK(ctx, hipGetLastError());
    return ZKHIP_OK;
}

}  // namespace zk
