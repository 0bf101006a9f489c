// ecc.hip -- the elliptic-curve chip on the device (include/zkhip_ecc.hpp: chord addition / tangent doubling on byte limbs, one point
// operation per row, 772 columns).  Record = op | x1[8] y1[8] x2[8] y2[8] | slope[8] (little-endian 32-bit words; the executor owns the
// one modular inversion of a call and hands the slope over).  One lane per row: the three identities' left sides as 576-bit signed
// integers (schoolbook products), binary long division by the modulus for the signed quotients and the canonical x3, y3, then the
// carries of the 3 x 64 limb equations; the row's lookups (163 byte pairs, 189 carry tuples, 2 comparisons) are counted into the bitwise
// and range-tuple tables in the same pass (wave-merged atomics, csrc/hist.hpp).  Replaces the trace generation of OpenVM's EcAddNe /
// EcDouble chips (openvm-ecc-circuit, un-vendored).
#include <string.h>

#include "../../include/zkhip.h"
#include "../../include/zkhip_ecc.hpp"
#include "babybear.hpp"
#include "limb_dev.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {
namespace ec = zkhip::ecc;

struct EcWords {
    uint32_t p[12], a[12];
};

// NW = words of the modulus: 8 (32 limbs) or 12 (48 limbs: BLS12-381 G1, crates/circuits/batch-circuit/openvm.toml)
template <int NW>
__global__ __launch_bounds__(64) void k_ec_trace(const uint32_t* __restrict__ recs, size_t n, size_t N, EcWords cw, uint32_t* __restrict__ trace,
                                                 uint32_t* __restrict__ bitwise_range, uint32_t* __restrict__ tuple, uint32_t tuple_y, uint32_t* __restrict__ bad) {
    constexpr ec::Cols C(4 * NW);
    constexpr int L = 4 * NW, SW = Signed<NW>::SW;
    using S = Signed<NW>;
    const size_t row = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= N) return;
    const RowWriter w{trace, N, row};
    if (row >= n) return w.zero(C.WIDTH);
    const uint32_t* rec = recs + C.RECORD_WORDS * row;
    const uint32_t op = rec[0];
    if (op >= ec::N_OPS) atomicAdd(bad, 1u);
    const bool dbl = op == ec::OP_DOUBLE;
    uint32_t x1[NW], y1[NW], x2[NW], y2[NW], l[NW], x3[NW], y3[NW], q[3][NW + 1], v[SW];
    bool neg[3];
    for (int i = 0; i < NW; i++) x1[i] = rec[1 + i], y1[i] = rec[1 + NW + i], x2[i] = rec[1 + 2 * NW + i], y2[i] = rec[1 + 3 * NW + i], l[i] = rec[1 + 4 * NW + i];
    // identity 1: the slope
    for (int i = 0; i < SW; i++) v[i] = 0;
    if (dbl) {
        S::acc_product(v, l, y1, +1, 2), S::acc_product(v, x1, x1, -1, 3), S::acc_word(v, cw.a, -1);
    } else {
        S::acc_product(v, l, x2, +1, 1), S::acc_product(v, l, x1, -1, 1), S::acc_word(v, y2, -1), S::acc_word(v, y1, +1);
    }
    uint32_t res[NW];
    bool fits = S::signed_divmod(v, cw.p, q[0], res, &neg[0]);
    for (int i = 0; i < NW; i++) fits = fits && res[i] == 0;   // the slope the record carries must solve the first identity
    // identity 2: x3
    for (int i = 0; i < SW; i++) v[i] = 0;
    S::acc_product(v, l, l, +1, 1), S::acc_word(v, x1, -1), S::acc_word(v, dbl ? x1 : x2, -1);
    fits = S::signed_divmod(v, cw.p, q[1], x3, &neg[1]) && fits;
    // identity 3: y3
    for (int i = 0; i < SW; i++) v[i] = 0;
    S::acc_product(v, l, x1, +1, 1), S::acc_product(v, l, x3, -1, 1), S::acc_word(v, y1, -1);
    fits = S::signed_divmod(v, cw.p, q[2], y3, &neg[2]) && fits;
    if (!fits) atomicAdd(bad, 1u);

    const uint32_t* vars[7] = {x1, y1, x2, y2, l, x3, y3};
    for (int o = 0; o < 7; o++) emit_limbs<L>(w, L * o, vars[o], bitwise_range);
    for (int e = 0; e < 3; e++) {
        emit_limbs<(int)C.Q_LIMBS>(w, C.Q + e * C.Q_LIMBS, q[e], bitwise_range);
        w.put(C.QS + e, neg[e] ? 1u : 0u);
    }
    // carries of the three identities' limb sums
    for (int e = 0; e < 3; e++) {
        const int64_t q_sign = neg[e] ? -1 : 1;
        emit_carries(w, (int)C.N_POS, (int)C.N_CARRY, ec::CARRY_OFFSET, tuple_y, C.CX + e * C.N_CARRY, C.CY + e * C.N_CARRY, fits, tuple, bad, [&](int k) {
            int64_t s = 0;
            for (int i = 0; i < (int)C.Q_LIMBS; i++) {
                const int j = k - i;
                if (j < 0 || j >= L) continue;
                s -= q_sign * (int64_t)limb_byte(q[e], i) * limb_byte(cw.p, j);
                if (i >= L) continue;
                const int64_t li = limb_byte(l, i);
                if (e == 0) s += dbl ? 2 * li * limb_byte(y1, j) - 3 * (int64_t)limb_byte(x1, i) * limb_byte(x1, j) : li * ((int64_t)limb_byte(x2, j) - limb_byte(x1, j));
                else if (e == 1) s += li * limb_byte(l, j);
                else s += li * ((int64_t)limb_byte(x1, j) - limb_byte(x3, j));
            }
            if (k < L) {
                if (e == 0) s -= dbl ? (int64_t)limb_byte(cw.a, k) : (int64_t)limb_byte(y2, k) - limb_byte(y1, k);
                else if (e == 1) s -= (int64_t)limb_byte(x1, k) + limb_byte(dbl ? x1 : x2, k) + limb_byte(x3, k);
                else s -= (int64_t)limb_byte(y1, k) + limb_byte(y3, k);
            }
            return s;
        });
    }
    emit_below<L, false>(w, x3, cw.p, true, C.MARK, C.DIFF, bitwise_range, bad);           // x3 < P
    emit_below<L, false>(w, y3, cw.p, true, C.MARK + L, C.DIFF + 1, bitwise_range, bad);   // y3 < P
    w.put(C.REAL, 1u), w.put(C.IS_DOUBLE, dbl ? 1u : 0u);
}

struct AirKey {
    ec::Modulus p, a;
    uint32_t bitwise_bus, tuple_bus;
    bool operator<(const AirKey& o) const {
        if (p != o.p) return p < o.p;
        if (a != o.a) return a < o.a;
        if (bitwise_bus != o.bitwise_bus) return bitwise_bus < o.bitwise_bus;
        return tuple_bus < o.tuple_bus;
    }
};
AirCache<AirKey> g_programs;

bool curve_of(uint32_t nw, const uint32_t* modulus, const uint32_t* a, ec::Curve* c) {
    if (nw != 8 && nw != 12) return false;
    c->p = zkhip::modular::load_words(modulus, nw), c->a = zkhip::modular::load_words(a, nw);
    // an odd modulus that fills its top two words (room for the (L + 1)-byte quotients), and a reduced coefficient
    return (c->p.w[0] & 1u) && c->p.w[nw - 1] != 0 && c->p.w[nw - 2] != 0 && ec::less(c->a, c->p);
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_ec_air_x(const uint8_t* modulus, const uint8_t* a, uint32_t n_limbs, uint32_t bitwise_bus, uint32_t tuple_bus, zkhip_air* out) {
    if (!modulus || !a || !out || (n_limbs != 32 && n_limbs != 48)) return ZKHIP_ERR_INVALID;
    AirKey key;
    key.p.limbs = key.a.limbs = n_limbs;
    memcpy(key.p.data(), modulus, n_limbs), memcpy(key.a.data(), a, n_limbs);
    key.bitwise_bus = bitwise_bus, key.tuple_bus = tuple_bus;
    if (!(key.p[0] & 1u) || !key.p[n_limbs - 1]) return ZKHIP_ERR_INVALID;
    const ec::Cols C(n_limbs);
    return g_programs.get(key, C.WIDTH, [&](zkhip::air::AirBuilder& b) { ec::ec_air(b, key.p, key.a, bitwise_bus, tuple_bus); }, out);
}
int zkhip_ec_air(const uint8_t modulus[32], const uint8_t a[32], uint32_t bitwise_bus, uint32_t tuple_bus, zkhip_air* out) {
    return zkhip_ec_air_x(modulus, a, 32, bitwise_bus, tuple_bus, out);
}

int zkhip_ec_host_x(uint32_t op, uint32_t n_words, const uint32_t* modulus, const uint32_t* a, const uint32_t* x1, const uint32_t* y1, const uint32_t* x2, const uint32_t* y2,
                    uint32_t* slope, uint32_t* x3, uint32_t* y3) {
    if (!modulus || !a || !x1 || !y1 || !x2 || !y2 || !slope || !x3 || !y3) return ZKHIP_ERR_INVALID;
    ec::Curve c;
    if (!curve_of(n_words, modulus, a, &c)) return ZKHIP_ERR_INVALID;
    using zkhip::modular::load_words;
    ec::U256 L, X3, Y3;
    if (!ec::ec_op(op, c, load_words(x1, n_words), load_words(y1, n_words), load_words(x2, n_words), load_words(y2, n_words), &L, &X3, &Y3)) return ZKHIP_ERR_INVALID;
    memcpy(slope, L.w, 4 * n_words), memcpy(x3, X3.w, 4 * n_words), memcpy(y3, Y3.w, 4 * n_words);
    return ZKHIP_OK;
}
int zkhip_ec_host(uint32_t op, const uint32_t modulus[8], const uint32_t a[8], const uint32_t x1[8], const uint32_t y1[8], const uint32_t x2[8],
                  const uint32_t y2[8], uint32_t slope[8], uint32_t x3[8], uint32_t y3[8]) {
    return zkhip_ec_host_x(op, 8, modulus, a, x1, y1, x2, y2, slope, x3, y3);
}

int zkhip_ec_tracegen_x(zkhip_ctx* ctx, uint32_t n_words, const uint32_t* modulus, const uint32_t* a, const uint32_t* d_records, size_t n, unsigned log_height,
                        uint32_t* d_trace, uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !modulus || !a || !d_trace || !d_bitwise_trace || !d_tuple_counts || log_height > 22 || (n && !d_records)) return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    ZK_TRY(tracegen_shape(ctx, "ec_tracegen", n, N, size_x, size_y, 2048));
    ec::Curve c;
    if (!curve_of(n_words, modulus, a, &c)) return set_error(ctx, ZKHIP_ERR_INVALID, "ec_tracegen: the modulus must be odd, of 8 or 12 words, and fill its top words, the coefficient reduced");
    EcWords cw{};
    memcpy(cw.p, modulus, 4 * n_words), memcpy(cw.a, a, 4 * n_words);
    const auto kernel = n_words == 8 ? k_ec_trace<8> : k_ec_trace<12>;
    return tracegen_frame(
        ctx, "ec_tracegen", {{d_tuple_counts, (size_t)size_x * size_y}, {d_bitwise_trace, BITWISE_WORDS}},   // (the range column of the 8-bit table)
        [&](uint32_t* bad) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, ctx->stream, d_records, n, N, cw, d_trace, d_bitwise_trace, d_tuple_counts, size_y, bad);
        },
        "ec tracegen (a slope that does not solve the chord / tangent identity, a quotient beyond L + 1 bytes, or an unknown operation)");
}
int zkhip_ec_tracegen(zkhip_ctx* ctx, const uint32_t modulus[8], const uint32_t a[8], const uint32_t* d_records, size_t n, unsigned log_height, uint32_t* d_trace,
                      uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    return zkhip_ec_tracegen_x(ctx, 8, modulus, a, d_records, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y);
}

int zkhip_vm_ec_tracegen_x(zkhip_ctx* ctx, uint32_t n_words, const uint32_t* modulus, const uint32_t* a, const uint32_t* d_records, const uint32_t* d_ts, size_t n,
                           unsigned log_height, uint32_t* d_trace, uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || (n && !d_ts) || (n_words != 8 && n_words != 12)) return ZKHIP_ERR_INVALID;
    ZK_TRY(zkhip_ec_tracegen_x(ctx, n_words, modulus, a, d_records, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y));
    return call_timestamps(ctx, "vm_ec_timestamps", d_ts, n, log_height, d_trace + ((size_t)ec::Cols(4 * n_words).TS << log_height));
}
int zkhip_vm_ec_tracegen(zkhip_ctx* ctx, const uint32_t modulus[8], const uint32_t a[8], const uint32_t* d_records, const uint32_t* d_ts, size_t n,
                         unsigned log_height, uint32_t* d_trace, uint32_t* d_bitwise_trace, uint32_t* d_tuple_counts, uint32_t size_x, uint32_t size_y) {
    return zkhip_vm_ec_tracegen_x(ctx, 8, modulus, a, d_records, d_ts, n, log_height, d_trace, d_bitwise_trace, d_tuple_counts, size_x, size_y);
}

}  // extern "C"
