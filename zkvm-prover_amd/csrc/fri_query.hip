// fri_query.hip -- the FRI query chip on the device (air.py fri_query_air, include/zkhip_chips.hpp; docs/fri_query.md): one query's fold
// loop, a row per commit-phase layer.  A call is a strictly serial chain of at most 26 cheap extension steps (the value folded on a layer is
// opened on the next); every row then needs one full Poseidon2 permutation of its own pair, and those are independent across rows and are
// where the work is.  So the two are separate launches on the context's stream, none of which waits on another workgroup:
//   k_ro_len_sums, k_ro_offsets   roff[c] = the first row of call c (call_offsets.hpp, shared: shift 0, the total must be n_rows)
//   k_fri_query_chain             one lane per CALL: walks the chain, leaves every row's pair (e0, e1) in d_hash_inputs, the last eval in d_final
//   k_fri_query_rows              one lane per ROW: finds its call in roff, redoes the row's own fold from the pair (everything else in a row
//                                 is a function of the row's records), permutes e0 | e1 | 0^8 and stores the 61 cells
// One lane per row keeps the stores along rows with no staging: consecutive lanes hold consecutive rows of every column.  The padding rows
// are written as zeros by k_fri_query_rows itself, so the trace needs no memset.  A second form of the row kernel (16 lanes per row on
// coop_permute_regs, staged through LDS) was measured against it, lost at both workloads and was removed (docs/fri_query.md "Measured").
#include <algorithm>

#include "../../include/zkhip.h"
#include "babybear.hpp"
#include "call_offsets.hpp"
#include "fri_query_host.hpp"
#include "poseidon2_coop.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {

constexpr unsigned FQ_COLS = ZKHIP_FRI_QUERY_WIDTH;
static_assert(FQ_COLS == 61, "e0 e1 beta bsq [4] | x_inv | folded ro eval [4] | st_out[16] | root[8] | bit has_ro k lvl is_first is_last is_real call");
constexpr unsigned FQ_MAX_LAYERS = 26;   // rows of a call: lvl = log_max - 1 - t >= 1 with log_max <= 27

// W_j^-1 in Montgomery form, W_j the generator of the subgroup of order 2^(j + 2) (air.domain_point_inverse_roots): bit j of a pair index k
// contributes W_j to x = g^bitrev(k) whatever the layer's size is, so x^-1 is the product over the set bits of k.
struct FqRoots {
    uint32_t v[FQ_MAX_LAYERS];
};
constexpr uint64_t fq_cpow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    for (a %= P; e; e >>= 1, a = a * a % P)
        if (e & 1) r = r * a % P;
    return r;
}
constexpr FqRoots fq_roots() {
    FqRoots t{};
    for (unsigned j = 0; j < FQ_MAX_LAYERS; j++) t.v[j] = (uint32_t)(fq_cpow(fq_cpow(GEN_2_27_CANON, (uint64_t)1 << (27 - (j + 2))), P - 2) * MONTY_ONE % P);
    return t;
}
static __constant__ const FqRoots FQ_WINV = fq_roots();

__device__ __forceinline__ uint32_t fq_x_inv(uint32_t k) {
    uint32_t acc = MONTY_ONE;
#pragma unroll 1
    for (unsigned j = 0; j < FQ_MAX_LAYERS && (k >> j); j++) acc = mmul(acc, (k >> j) & 1u ? FQ_WINV.v[j] : MONTY_ONE);
    return acc;
}
__device__ __forceinline__ Ext fq_ext(const uint32_t* p, uint32_t* bad) { return Ext{{field_word(p[0], bad), field_word(p[1], bad), field_word(p[2], bad), field_word(p[3], bad)}}; }
// folded = ((e0 + e1) + x_inv (beta (e0 - e1))) / 2: the line of air.fri_fold_air
__device__ __forceinline__ Ext fq_fold(const Ext& e0, const Ext& e1, const Ext& beta, uint32_t xinv) {
    return ext_mul_base(ext_add(ext_add(e0, e1), ext_mul_base(ext_mul(beta, ext_sub(e0, e1)), xinv)), to_monty((P + 1) / 2));
}

struct FqIn {
    const uint32_t *log_max, *index, *ro_top;            // per call
    const uint32_t *beta, *root, *sibling, *has_ro, *ro;   // per row
    const uint32_t* roff;                                  // n_calls + 1 words (k_ro_offsets), clamped to n_rows + 1
    uint32_t n_calls, n_rows;
};
// what both kernels take a call's shape from: its length from the offsets, never from d_n_layers; false for a refused call, whose rows
// stay zero
__device__ __forceinline__ bool fq_call(const FqIn& in, uint32_t c, uint32_t* r0, uint32_t* len, uint32_t* lm, uint32_t* idx) {
    *r0 = in.roff[c], *len = in.roff[c + 1] - *r0, *lm = in.log_max[c], *idx = in.index[c];
    return *lm <= 27 && *len >= 1 && *len + 1 <= *lm && (*idx >> *lm) == 0;
}

// the chain's own x_inv: W_j = W_(j+1)^2, so x_inv(k >> 1) = (x_inv(k) W_0^(k & 1))^2 -- one squaring a layer instead of a product over the set bits
constexpr uint32_t FQ_W0 = (uint32_t)(fq_cpow(GEN_2_27_CANON, (uint64_t)1 << 25) * MONTY_ONE % P);

__global__ __launch_bounds__(256) void k_fri_query_chain(FqIn in, size_t N, uint32_t* __restrict__ hash_inputs, uint32_t* __restrict__ fin, uint32_t* __restrict__ bad) {
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c == 0 && ((size_t)in.n_rows > N || (in.n_calls == 0 && in.n_rows != 0))) atomicAdd(bad, 1u);   // more rows than the trace has; rows of no call
    if (c >= in.n_calls) return;
    uint32_t r0, len, lm, idx;
    const bool ok = fq_call(in, (uint32_t)c, &r0, &len, &lm, &idx);
    if (!ok) atomicAdd(bad, 1u);
    Ext ev = fq_ext(in.ro_top + 4 * c, bad);
    if (!ok) ev = ext_zero(), len = 0;
    uint32_t xinv = ok ? fq_x_inv(idx >> 1) : MONTY_ONE;
#pragma unroll 1
    for (uint32_t t = 0; t < len; t++) {
        const size_t r = (size_t)r0 + t;
        if (r >= in.n_rows || r >= N) break;               // (offsets that were clamped: refused there)
        const Ext beta = fq_ext(in.beta + 4 * r, bad), sib = fq_ext(in.sibling + 4 * r, bad);
        Ext ro = fq_ext(in.ro + 4 * r, bad);
        const uint32_t has = in.has_ro[r];
        if (has > 1u || (has == 0u && (ro.c[0] | ro.c[1] | ro.c[2] | ro.c[3]))) atomicAdd(bad, 1u), ro = ext_zero();
        const bool bit = (idx >> t) & 1u;
        const Ext e0 = bit ? sib : ev, e1 = bit ? ev : sib;
#pragma unroll
        for (int i = 0; i < 4; i++) hash_inputs[16 * r + i] = e0.c[i], hash_inputs[16 * r + 4 + i] = e1.c[i];
        ev = fq_fold(e0, e1, beta, xinv);
        if (has == 1u) ev = ext_add(ev, ext_mul(ext_mul(beta, beta), ro));
        xinv = mmul(xinv, (idx >> (t + 1)) & 1u ? FQ_W0 : MONTY_ONE);
        xinv = mmul(xinv, xinv);
    }
    if (fin) {
#pragma unroll
        for (int i = 0; i < 4; i++) fin[4 * c + i] = from_monty(ev.c[i]);
    }
}

// ---- the rows: a row's call comes from the offsets, its cells from the row's own records and the pair the chain left ----
// the last call whose first row is not behind r (roff is non-decreasing), and whether r is a row of it
__device__ __forceinline__ bool fq_find(const FqIn& in, size_t r, uint32_t* c, uint32_t* t, uint32_t* len, uint32_t* lm, uint32_t* idx) {
    uint32_t lo = 0, hi = in.n_calls, r0;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (in.roff[mid] <= r) lo = mid;
        else hi = mid;
    }
    *c = lo;
    if (!fq_call(in, lo, &r0, len, lm, idx) || r < r0 || r - r0 >= *len) return false;
    *t = (uint32_t)r - r0;
    return true;
}
// (the chain kernel has counted the words of beta and ro that are no field elements: here they are only read as 0)
__device__ __forceinline__ Ext fq_ext_quiet(const uint32_t* p) {
    Ext e;
#pragma unroll
    for (int i = 0; i < 4; i++) e.c[i] = to_monty(p[i] < P ? p[i] : 0u);
    return e;
}
// the 37 cells of row r that are neither the state nor the root, each handed to put(column, word)
template <class Put>
__device__ __forceinline__ void fq_cells(const FqIn& in, size_t r, uint32_t c, uint32_t t, uint32_t len, uint32_t lm, uint32_t idx, const uint32_t* __restrict__ hash_inputs, Put put) {
    const uint32_t k = idx >> (t + 1);
    const bool has = in.has_ro[r] == 1u, bit = (idx >> t) & 1u;
    Ext e0, e1;
#pragma unroll
    for (int i = 0; i < 4; i++) e0.c[i] = hash_inputs[16 * r + i], e1.c[i] = hash_inputs[16 * r + 4 + i];
    const Ext beta = fq_ext_quiet(in.beta + 4 * r);
    const Ext ro = has ? fq_ext_quiet(in.ro + 4 * r) : ext_zero();
    const Ext bsq = ext_mul(beta, beta);
    const uint32_t xinv = fq_x_inv(k);
    const Ext folded = fq_fold(e0, e1, beta, xinv);
    const Ext ev = ext_add(folded, ext_mul(bsq, ro));
#pragma unroll
    for (int i = 0; i < 4; i++) {
        put(i, e0.c[i]), put(4 + i, e1.c[i]), put(8 + i, beta.c[i]), put(12 + i, bsq.c[i]);
        put(17 + i, folded.c[i]), put(21 + i, ro.c[i]), put(25 + i, ev.c[i]);
    }
    put(16, xinv);
    put(53, bit ? MONTY_ONE : 0u);
    put(54, has ? MONTY_ONE : 0u);
    put(55, to_monty(k));
    put(56, to_monty(lm - 1u - t));
    put(57, t == 0 ? MONTY_ONE : 0u);
    put(58, t + 1 == len ? MONTY_ONE : 0u);
    put(59, MONTY_ONE);
    put(60, to_monty(c));
}

// One lane per ROW on the batch permutation's device function: consecutive lanes hold consecutive rows of every column, so the stores run
// along rows with no staging.
__global__ __launch_bounds__(256) void k_fri_query_rows(FqIn in, size_t N, uint32_t* __restrict__ trace, const uint32_t* __restrict__ hash_inputs,
                                                        uint32_t* __restrict__ leaf, uint32_t* __restrict__ bad) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    uint32_t c = 0, t = 0, len = 0, lm = 0, idx = 0;
    const bool real = r < in.n_rows && in.n_calls != 0 && fq_find(in, r, &c, &t, &len, &lm, &idx);
    if (real) {
        fq_cells(in, r, c, t, len, lm, idx, hash_inputs, [&](unsigned q, uint32_t v) { trace[(size_t)q * N + r] = v; });
        uint32_t st[16];
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = hash_inputs[16 * r + i], st[8 + i] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) trace[(size_t)(45 + i) * N + r] = field_word(in.root[8 * r + i], bad);
        poseidon2_permute_rolled(st);                      // (only the state is live across it: the other cells are out)
#pragma unroll
        for (int i = 0; i < 16; i++) trace[(size_t)(29 + i) * N + r] = st[i];
        if (leaf) {
#pragma unroll
            for (int i = 0; i < 8; i++) leaf[8 * r + i] = from_monty(st[i]);
        }
    } else {
#pragma unroll 1
        for (unsigned q = 0; q < FQ_COLS; q++) trace[(size_t)q * N + r] = 0u;
        if (leaf && r < in.n_rows) {
#pragma unroll
            for (int i = 0; i < 8; i++) leaf[8 * r + i] = 0u;
        }
    }
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_fri_query_host(uint64_t index, unsigned log_max, unsigned n_layers, const uint32_t* beta, const uint32_t* sibling, const uint32_t* has_ro, const uint32_t* ro,
                         const uint32_t ro_top[4], uint32_t* e0, uint32_t* e1, uint32_t* eval) {
    return fri_query_canonical(index, log_max, n_layers, beta, sibling, has_ro, ro, ro_top, e0, e1, eval);
}

int zkhip_fri_query_tracegen(zkhip_ctx* ctx, const uint32_t* d_n_layers, const uint32_t* d_log_max, const uint32_t* d_index, const uint32_t* d_ro_top,
                             const uint32_t* d_beta, const uint32_t* d_root, const uint32_t* d_sibling, const uint32_t* d_has_ro, const uint32_t* d_ro, size_t n_calls,
                             size_t n_rows, unsigned log_height, uint32_t* d_trace, uint32_t* d_hash_inputs, uint32_t* d_leaf_digest, uint32_t* d_final) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || !d_hash_inputs || log_height > 27 || (n_calls && (!d_n_layers || !d_log_max || !d_index || !d_ro_top)) ||
        (n_rows && (!d_beta || !d_root || !d_sibling || !d_has_ro || !d_ro)))
        return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    if (n_calls > n_rows) return set_error(ctx, ZKHIP_ERR_INVALID, "fri_query_tracegen: more calls than rows (a call has at least one)");
    // (what keeps the offsets inside 32 bits; a call has at most 26 rows, so the device's checks would refuse it as well)
    if (n_rows > ((size_t)1 << 31)) return set_error(ctx, ZKHIP_ERR_INVALID, "fri_query_tracegen: more rows than any trace has");
    // scratch: roff[n_calls + 1] | sums
    CallScratch s;
    ZK_TRY(call_scratch(ctx, n_calls, 1, 0, &s));
    uint32_t* roff = s.off[0];
    const FqIn in{d_log_max, d_index, d_ro_top, d_beta, d_root, d_sibling, d_has_ro, d_ro, roff, (uint32_t)n_calls, (uint32_t)n_rows};
    return tracegen_frame(
        ctx, "fri_query_tracegen", {},
        [&](uint32_t* bad) -> int {
            ZK_HIP_CHECK(ctx, hipMemsetAsync(d_hash_inputs, 0, 16 * N * 4, ctx->stream));
            if (n_calls) launch_call_offsets(ctx, d_n_layers, n_calls, n_rows, 0, true, s.sums, roff, bad);
            // (with no call the chain kernel still runs its one check: rows without calls are refused there)
            hipLaunchKernelGGL(k_fri_query_chain, dim3((unsigned)((std::max<size_t>(n_calls, 1) + 255) / 256)), dim3(256), 0, ctx->stream, in, N, d_hash_inputs, d_final, bad);
            hipLaunchKernelGGL(k_fri_query_rows, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, in, N, d_trace, (const uint32_t*)d_hash_inputs, d_leaf_digest, bad);
            return ZKHIP_OK;
        },
        "fri_query_tracegen (a call of 0 or more than log_max - 1 layers, log_max > 27, an index outside 2^log_max, lengths that do not sum to n_rows, "
        "more rows than the trace has, has_ro outside {0, 1}, a non-zero ro under has_ro = 0, or a word that is not a field element)");
}

}  // extern "C"
