// fp2.hip -- the Fp2 chip on the device (include/zkhip_fp2.hpp: multiplication, division, addition, subtraction in Fp[u] / (u^2 + 1) on byte
// limbs, one operation per row, 648 columns).  Record = op | a0[8] a1[8] | b0[8] b1[8] (little-endian 32-bit words; a division's record
// holds the quotient x / y in the a slot -- the executor owns the inversion -- and its row is the product (x / y) y = x).  One lane per
// row: the two component identities' left sides as 576-bit signed integers, binary long division by the modulus for the signed quotients
// and the canonical r0, r1, then the carries of the 2 x 64 limb equations; the row's lookups (130 byte pairs, 126 carry tuples, 2 - 4
// comparisons) are counted into the bitwise and range-tuple tables in the same pass.  Replaces the trace generation of OpenVM's
// Fp2AddSub / Fp2MulDiv chips (openvm-algebra-circuit, un-vendored).
#include <string.h>

#include <utility>

#include "../../include/zkhip.h"
#include "../../include/zkhip_fp2.hpp"
#include "babybear.hpp"
#include "limb_dev.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {
namespace f2 = zkhip::fp2;

struct Fp2Words {
    uint32_t p[12];
};

// NW = words of the modulus: 8 (32 limbs) or 12 (48 limbs: BLS12-381's Fp2, crates/circuits/batch-circuit/openvm.toml)
template <int NW>
__global__ __launch_bounds__(64) void k_fp2_trace(const uint32_t* __restrict__ recs, size_t n, size_t N, Fp2Words cw, uint32_t* __restrict__ trace,
                                                  uint32_t* __restrict__ bitwise_range, uint32_t* __restrict__ tuple, uint32_t tuple_y, uint32_t* __restrict__ bad) {
    constexpr f2::Cols C(4 * NW);
    constexpr int L = 4 * NW, SW = Signed<NW>::SW;
    const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= N) return;
    const RowWriter w{trace, N, row};
    if (row >= n) return w.zero(C.WIDTH);
    const uint32_t* rec = recs + C.RECORD_WORDS * row;
    const uint32_t op_in = rec[0];
    if (op_in >= f2::N_OPS) atomicAdd(bad, 1u);
    const bool is_div = op_in == f2::OP_DIV;
    const uint32_t op = is_div ? (uint32_t)f2::OP_MUL : op_in;
    uint32_t a[2][NW], b[2][NW], r[2][NW], q[2][NW + 1], v[SW];
    bool neg[2];
    for (int i = 0; i < NW; i++) a[0][i] = rec[1 + i], a[1][i] = rec[1 + NW + i], b[0][i] = rec[1 + 2 * NW + i], b[1][i] = rec[1 + 3 * NW + i];
    bool fits = true;
    for (int e = 0; e < 2; e++) {
        for (int i = 0; i < SW; i++) v[i] = 0;
        if (op == f2::OP_MUL) {
            if (e == 0) Signed<NW>::acc_product(v, a[0], b[0], +1, 1), Signed<NW>::acc_product(v, a[1], b[1], -1, 1);
            else Signed<NW>::acc_product(v, a[0], b[1], +1, 1), Signed<NW>::acc_product(v, a[1], b[0], +1, 1);
        } else {
            Signed<NW>::acc_word(v, a[e], +1), Signed<NW>::acc_word(v, b[e], op == f2::OP_ADD ? +1 : -1);
        }
        fits = Signed<NW>::signed_divmod(v, cw.p, q[e], r[e], &neg[e]) && fits;
    }
    if (!fits) atomicAdd(bad, 1u);
    const uint32_t* vars[6] = {a[0], a[1], b[0], b[1], r[0], r[1]};
    for (int o = 0; o < 6; o++) emit_limbs<L>(w, L * o, vars[o], bitwise_range);
    for (int e = 0; e < 2; e++) {
        emit_limbs<(int)C.Q_LIMBS>(w, C.Q + e * C.Q_LIMBS, q[e], bitwise_range);
        w.put(C.QS + e, neg[e] ? 1u : 0u);
    }
    for (int e = 0; e < 2; e++) {
        const int64_t q_sign = neg[e] ? -1 : 1;
        emit_carries(w, (int)C.N_POS, (int)C.N_CARRY, f2::CARRY_OFFSET, tuple_y, C.CX + e * C.N_CARRY, C.CY + e * C.N_CARRY, fits, tuple, bad, [&](int k) {
            int64_t s = 0;
            for (int i = 0; i < (int)C.Q_LIMBS; i++) {
                const int j = k - i;
                if (j < 0 || j >= L) continue;
                s -= q_sign * (int64_t)limb_byte(q[e], i) * limb_byte(cw.p, j);
                if (i >= L || op != f2::OP_MUL) continue;
                if (e == 0) s += (int64_t)limb_byte(a[0], i) * limb_byte(b[0], j) - (int64_t)limb_byte(a[1], i) * limb_byte(b[1], j);
                else s += (int64_t)limb_byte(a[0], i) * limb_byte(b[1], j) + (int64_t)limb_byte(a[1], i) * limb_byte(b[0], j);
            }
            if (k < L) {
                if (op == f2::OP_ADD) s += (int64_t)limb_byte(a[e], k) + limb_byte(b[e], k);
                if (op == f2::OP_SUB) s += (int64_t)limb_byte(a[e], k) - limb_byte(b[e], k);
                s -= limb_byte(r[e], k);
            }
            return s;
        });
    }
    // r0, r1 < P; on a division row also a0, a1 < P (the quotient).  Both are checked: a result or a quotient that is not below the modulus is refused
    for (int e = 0; e < 2; e++) emit_below<L, true>(w, r[e], cw.p, true, C.MARK + L * e, C.DIFF + e, bitwise_range, bad);
    for (int e = 0; e < 2; e++) emit_below<L, true>(w, a[e], cw.p, is_div, C.MARK2 + L * e, C.DIFF2 + e, bitwise_range, bad);
    w.put(C.REAL, 1u), w.put(C.IS_ADD, op_in == f2::OP_ADD ? 1u : 0u), w.put(C.IS_SUB, op_in == f2::OP_SUB ? 1u : 0u), w.put(C.IS_DIV, is_div ? 1u : 0u);
}

AirCache<std::pair<f2::Modulus, std::pair<uint32_t, uint32_t>>> g_programs;   // (modulus, buses) -> program

// an odd modulus that fills its top two words (room for the (L + 1)-byte quotients)
bool modulus_ok(const uint32_t* m, uint32_t nw) { return (nw == 8 || nw == 12) && (m[0] & 1u) && m[nw - 1] != 0 && m[nw - 2] != 0; }

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_fp2_air_x(const uint8_t* modulus, uint32_t n_limbs, uint32_t bitwise_bus, uint32_t tuple_bus, zkhip_air* out) {
    if (!modulus || !out || (n_limbs != 32 && n_limbs != 48) || !(modulus[0] & 1u) || !modulus[n_limbs - 1]) return ZKHIP_ERR_INVALID;
    f2::Modulus m;
    m.limbs = n_limbs;
    memcpy(m.data(), modulus, n_limbs);
    const f2::Cols C(n_limbs);
    return g_programs.get(std::make_pair(m, std::make_pair(bitwise_bus, tuple_bus)), C.WIDTH, [&](zkhip::air::AirBuilder& b) { f2::fp2_air(b, m, bitwise_bus, tuple_bus); }, out);
}
int zkhip_fp2_air(const uint8_t modulus[32], uint32_t bitwise_bus, uint32_t tuple_bus, zkhip_air* out) { return zkhip_fp2_air_x(modulus, 32, bitwise_bus, tuple_bus, out); }

int zkhip_fp2_host_x(uint32_t op, uint32_t n_words, const uint32_t* modulus, const uint32_t* a, const uint32_t* b, uint32_t* r) {
    if (!modulus || !a || !b || !r || !modulus_ok(modulus, n_words)) return ZKHIP_ERR_INVALID;
    const f2::U256 p = zkhip::modular::load_words(modulus, n_words);
    f2::Elem A{zkhip::modular::load_words(a, n_words), zkhip::modular::load_words(a + n_words, n_words)},
        B{zkhip::modular::load_words(b, n_words), zkhip::modular::load_words(b + n_words, n_words)}, R;
    if (!f2::fp2_op(op, p, A, B, &R)) return ZKHIP_ERR_INVALID;
    memcpy(r, R.c0.w, 4 * n_words), memcpy(r + n_words, R.c1.w, 4 * n_words);
    return ZKHIP_OK;
}
int zkhip_fp2_host(uint32_t op, const uint32_t modulus[8], const uint32_t a[16], const uint32_t b[16], uint32_t r[16]) { return zkhip_fp2_host_x(op, 8, modulus, a, b, r); }

int zkhip_fp2_tracegen_x(zkhip_ctx* ctx, uint32_t n_words, const uint32_t* modulus, const uint32_t* d_records, size_t n, unsigned log_height, uint32_t* d_trace,
                         uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !modulus || !d_trace || !d_bitwise_trace || !d_tuple_counts || log_height > 22 || (n && !d_records)) return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    ZK_TRY(tracegen_shape(ctx, "fp2_tracegen", n, N, size_x, size_y, 2048));
    if (!modulus_ok(modulus, n_words)) return set_error(ctx, ZKHIP_ERR_INVALID, "fp2_tracegen: the modulus must be odd, of 8 or 12 words, and fill its top words");
    Fp2Words cw{};
    memcpy(cw.p, modulus, 4 * n_words);
    const auto kernel = n_words == 8 ? k_fp2_trace<8> : k_fp2_trace<12>;
    return tracegen_frame(
        ctx, "fp2_tracegen", {{d_tuple_counts, (size_t)size_x * size_y}, {d_bitwise_trace, BITWISE_WORDS}},
        [&](uint32_t* bad) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, ctx->stream, d_records, n, N, cw, d_trace, d_bitwise_trace, d_tuple_counts, size_y, bad);
        },
        "fp2 tracegen (a quotient beyond L + 1 bytes, a division record whose quotient is not reduced, or an unknown operation)");
}
int zkhip_fp2_tracegen(zkhip_ctx* ctx, const uint32_t modulus[8], const uint32_t* d_records, size_t n, unsigned log_height, uint32_t* d_trace,
                       uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    return zkhip_fp2_tracegen_x(ctx, 8, modulus, d_records, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y);
}

int zkhip_vm_fp2_tracegen_x(zkhip_ctx* ctx, uint32_t n_words, const uint32_t* modulus, const uint32_t* d_records, const uint32_t* d_ts, size_t n, unsigned log_height,
                            uint32_t* d_trace, uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || (n && !d_ts) || (n_words != 8 && n_words != 12)) return ZKHIP_ERR_INVALID;
    ZK_TRY(zkhip_fp2_tracegen_x(ctx, n_words, modulus, d_records, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y));
    return call_timestamps(ctx, "vm_fp2_timestamps", d_ts, n, log_height, d_trace + ((size_t)f2::Cols(4 * n_words).TS << log_height));
}
int zkhip_vm_fp2_tracegen(zkhip_ctx* ctx, const uint32_t modulus[8], const uint32_t* d_records, const uint32_t* d_ts, size_t n, unsigned log_height,
                          uint32_t* d_trace, uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    return zkhip_vm_fp2_tracegen_x(ctx, 8, modulus, d_records, d_ts, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y);
}

}  // extern "C"
