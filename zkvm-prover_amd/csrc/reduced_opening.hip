// reduced_opening.hip -- the reduced-opening chip on the device (air.py reduced_opening_air, include/zkhip_chips.hpp; docs/reduced_opening.md):
// ro = sum_i alpha^i (b_i - a_i) of one query at one height class, one element per row, walked by Horner from the call's last element to
// its first.  Calls are as long as the opened matrices are wide (1 to more than a thousand rows) and every row of a call depends on the
// rows before it, so the generator is not one lane per record: the accumulator column is a SCAN over the rows under the monoid of affine
// maps x -> x m + v of the extension field.  A row's map is (alpha, b - a); the first row of a call has m = 0, which forgets whatever came
// before it -- the segments need no flags.  Five launches on the context's stream, none of which waits on another workgroup:
//   k_ro_len_sums   the sum of the lengths of each slice of calls                                                    (call_offsets.hpp, shared
//   k_ro_offsets    off[c] = the first row of call c (exclusive scan of the lengths; each workgroup adds the slices      with mmcs_rows.hip)
//                   before its own), the checks on the lengths
//   k_ro_pass<0>    the composed map of each workgroup's rows
//   k_ro_carries    one wave scans those: the accumulator in front of each workgroup's first row
//   k_ro_pass<1>    the rows: call and element from the offsets, operands, the scan again from the carry, the 18 columns
// A lane owns one row of a ZKHIP_REDUCED_OPENING_BLOCK_ROWS-row pass, so operand loads and column stores run along rows.  Nothing is read
// back: lengths that are refused (0, or not summing to n_elems) still give offsets that are clamped to n_elems + 1 and non-decreasing,
// and every index made from them is checked against n_elems before it is used.
#include <algorithm>

#include "../../include/zkhip.h"
#include "babybear.hpp"
#include "call_offsets.hpp"
#include "lds_barrier.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {

// x -> x m + v
struct Affine {
    Ext m, v;
};
__device__ __forceinline__ Affine affine_identity() { return Affine{ext_one(), ext_zero()}; }
// f, then g
__device__ __forceinline__ Affine affine_then(const Affine& f, const Affine& g) { return Affine{ext_mul(f.m, g.m), ext_add(ext_mul(f.v, g.m), g.v)}; }
__device__ __forceinline__ Ext affine_at(const Ext& x, const Affine& f) { return ext_add(ext_mul(x, f.m), f.v); }

__device__ __forceinline__ Ext ext_shfl_up(const Ext& x, unsigned off) {
    return Ext{{(uint32_t)__shfl_up((int)x.c[0], off, 64), (uint32_t)__shfl_up((int)x.c[1], off, 64), (uint32_t)__shfl_up((int)x.c[2], off, 64),
                (uint32_t)__shfl_up((int)x.c[3], off, 64)}};
}
// lane l: the composition of lanes 0 .. l, in that order
__device__ __forceinline__ Affine affine_wave_scan(Affine f, unsigned lane) {
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const Affine o{ext_shfl_up(f.m, off), ext_shfl_up(f.v, off)};
        if (lane >= off) f = affine_then(o, f);
    }
    return f;
}
__device__ __forceinline__ Affine affine_ld(const uint32_t* p) { return Affine{Ext{{p[0], p[1], p[2], p[3]}}, Ext{{p[4], p[5], p[6], p[7]}}}; }
__device__ __forceinline__ void affine_st(uint32_t* p, const Affine& f) {
#pragma unroll
    for (int q = 0; q < 4; q++) p[q] = f.m.c[q], p[4 + q] = f.v.c[q];
}

// ---- the rows --------------------------------------------------------------------------------------------------------------------------
struct RoIn {
    const uint32_t *alpha, *a, *b, *off;   // off: n_calls + 1 words of k_ro_offsets
    uint32_t n_calls, n_elems;
};
// the cells of one row, Montgomery
struct RoRow {
    Ext alpha, b;
    uint32_t a, idx, call;
    bool real, first, last;
};

// Row r: its call is the last c with off[c] <= r, searched in [c_lo, c_hi] (off[c_lo] <= r on entry; the bounds are then set for row
// r + RO_W: a call has at least one row, so that row's call is at most RO_W calls on).  Row t = r - off[c] of the call holds element
// off[c + 1] - 1 - t.  With CHECK the operands are compared with p (alpha on the call's first row, so once per call).
template <bool CHECK>
__device__ __forceinline__ RoRow ro_row(const RoIn& in, uint32_t r, uint32_t& c_lo, uint32_t& c_hi, uint32_t* bad) {
    RoRow row{};
    if (r >= in.n_elems) return row;
    uint32_t lo = c_lo, hi = c_hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (in.off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    c_lo = lo, c_hi = std::min(lo + RO_W, in.n_calls - 1);
    const uint32_t o0 = in.off[lo], o1 = in.off[lo + 1];
    if (r >= o1) return row;   // (only behind the last call of lengths that fall short of n_elems: refused by k_ro_offsets)
    const uint32_t t = r - o0, e = o1 - 1 - t;
    if (e >= in.n_elems) return row;   // (only with lengths beyond n_elems: refused as well)
    const uint4 al = ((const uint4*)in.alpha)[lo], bw = ((const uint4*)in.b)[e];
    const uint32_t aw = in.a[e];
    row.real = true, row.first = t == 0, row.last = r + 1 == o1, row.idx = to_monty(t), row.call = to_monty(lo);
    if (CHECK) {
        bool ok = aw < P && bw.x < P && bw.y < P && bw.z < P && bw.w < P;
        if (row.first) ok = ok && al.x < P && al.y < P && al.z < P && al.w < P;
        if (!ok) atomicAdd(bad, 1u);
    }
    row.alpha = Ext{{to_monty(al.x), to_monty(al.y), to_monty(al.z), to_monty(al.w)}};
    row.b = Ext{{to_monty(bw.x), to_monty(bw.y), to_monty(bw.z), to_monty(bw.w)}};
    row.a = to_monty(aw);
    return row;
}

// One workgroup walks rows [blockIdx.x rows_per_block, + rows_per_block) of the N trace rows, RO_W at a time.  APPLY = false: the composed
// map of those rows to io[8 blockIdx.x ..].  APPLY = true: io[4 blockIdx.x ..] is the accumulator in front of the first of them
// (k_ro_carries) and the rows are written.  Per pass: a scan inside each wave, the waves' maps through LDS (two buffers in turn, so one
// barrier a pass: a wave writes a buffer again only behind the next pass's barrier, which every wave reaches after its reads of this one),
// and every lane walks the four waves' maps in order.
template <bool APPLY>
__global__ __launch_bounds__(RO_W) void k_ro_pass(RoIn in, size_t N, size_t rows_per_block, uint32_t* __restrict__ io, uint32_t* __restrict__ trace,
                                                  uint32_t* __restrict__ bad) {
    __shared__ uint32_t wave_map[2][RO_WAVES][8];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * rows_per_block, row1 = std::min(row0 + rows_per_block, N);
    uint32_t c_lo = 0, c_hi = in.n_calls - 1;
    Ext x = ext_zero();               // APPLY: acc of the row in front of the pass
    Affine chunk = affine_identity();   // !APPLY: the rows so far
    if (APPLY) x = Ext{{io[4 * blockIdx.x], io[4 * blockIdx.x + 1], io[4 * blockIdx.x + 2], io[4 * blockIdx.x + 3]}};
    unsigned buf = 0;
    for (size_t base = row0; base < row1; base += RO_W) {
        const size_t r = base + tid;
        if (base >= in.n_elems) {   // padding only: the same for the whole workgroup
            if (APPLY && r < row1) {
#pragma unroll
                for (int q = 0; q < ZKHIP_REDUCED_OPENING_WIDTH; q++) trace[(size_t)q * N + r] = 0u;
            }
            continue;
        }
        const RoRow row = ro_row<APPLY>(in, (uint32_t)std::min(r, (size_t)in.n_elems), c_lo, c_hi, bad);
        Affine f{ext_zero(), ext_zero()};   // (a row behind the last call: nothing follows it)
        if (row.real) {
            f.v = row.b, f.v.c[0] = msub(row.b.c[0], row.a);
            if (!row.first) f.m = row.alpha;
        }
        const Affine incl = affine_wave_scan(f, lane);
        if (lane == 63) affine_st(wave_map[buf][wave], incl);
        zk_syncthreads();
        if (APPLY) {
            Ext y = x, mine = x;
            for (unsigned w = 0; w < RO_WAVES; w++) {
                if (w == wave) mine = y;
                y = affine_at(y, affine_ld(wave_map[buf][w]));
            }
            x = y;
            const Ext acc = affine_at(mine, incl);
            if (r < row1) {
                uint32_t col[ZKHIP_REDUCED_OPENING_WIDTH] = {};
                if (row.real) {
#pragma unroll
                    for (int q = 0; q < 4; q++) col[q] = row.alpha.c[q], col[5 + q] = row.b.c[q], col[9 + q] = acc.c[q];
                    col[4] = row.a, col[13] = row.idx, col[14] = row.first ? MONTY_ONE : 0u, col[15] = row.last ? MONTY_ONE : 0u, col[16] = MONTY_ONE;
                    col[17] = row.call;
                }
#pragma unroll
                for (int q = 0; q < ZKHIP_REDUCED_OPENING_WIDTH; q++) trace[(size_t)q * N + r] = col[q];
            }
        } else if (wave == 0) {   // (one wave keeps the composed map; the others only feed it)
            for (unsigned w = 0; w < RO_WAVES; w++) chunk = affine_then(chunk, affine_ld(wave_map[buf][w]));
        }
        buf ^= 1u;
    }
    if (!APPLY && tid == 0) affine_st(io + 8 * (size_t)blockIdx.x, chunk);
}

// one wave: carry[4 i ..] = the accumulator in front of workgroup i's rows, from the workgroups' maps (the first real row of the trace has
// m = 0, so the 0 this starts from never shows)
__global__ __launch_bounds__(64) void k_ro_carries(const uint32_t* __restrict__ maps, unsigned n_blocks, uint32_t* __restrict__ carry) {
    const unsigned lane = threadIdx.x;
    Ext x = ext_zero();
    for (unsigned start = 0; start < n_blocks; start += 64) {
        const unsigned i = start + lane;
        const Affine incl = affine_wave_scan(i < n_blocks ? affine_ld(maps + 8 * (size_t)i) : affine_identity(), lane);
        const Affine before{ext_shfl_up(incl.m, 1), ext_shfl_up(incl.v, 1)};
        const Ext c = lane == 0 ? x : affine_at(x, before);
        if (i < n_blocks) {
#pragma unroll
            for (int q = 0; q < 4; q++) carry[4 * (size_t)i + q] = c.c[q];
        }
        const Ext end = affine_at(x, incl);
#pragma unroll
        for (int q = 0; q < 4; q++) x.c[q] = (uint32_t)__shfl((int)end.c[q], 63, 64);
    }
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_reduced_opening_host(const uint32_t alpha[4], const uint32_t* a, const uint32_t* b, size_t len, uint32_t out[4]) {
    if (!alpha || !a || !b || !out || len == 0) return ZKHIP_ERR_INVALID;
    for (int q = 0; q < 4; q++)
        if (alpha[q] >= P) return ZKHIP_ERR_INVALID;
    const Ext al{{to_monty(alpha[0]), to_monty(alpha[1]), to_monty(alpha[2]), to_monty(alpha[3])}};
    Ext power = ext_one(), ro = ext_zero();
    for (size_t i = 0; i < len; i++) {
        if (a[i] >= P || b[4 * i] >= P || b[4 * i + 1] >= P || b[4 * i + 2] >= P || b[4 * i + 3] >= P) return ZKHIP_ERR_INVALID;
        const Ext d{{msub(to_monty(b[4 * i]), to_monty(a[i])), to_monty(b[4 * i + 1]), to_monty(b[4 * i + 2]), to_monty(b[4 * i + 3])}};
        ro = ext_add(ro, ext_mul(power, d));
        power = ext_mul(power, al);
    }
    for (int q = 0; q < 4; q++) out[q] = from_monty(ro.c[q]);
    return ZKHIP_OK;
}

int zkhip_reduced_opening_tracegen(zkhip_ctx* ctx, const uint32_t* d_alpha, const uint32_t* d_len, const uint32_t* d_a, const uint32_t* d_b, size_t n_calls,
                                   size_t n_elems, unsigned log_height, uint32_t* d_trace) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || log_height > 27 || (n_calls && (!d_alpha || !d_len)) || (n_elems && (!d_a || !d_b))) return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    ZK_TRY(tracegen_shape(ctx, "reduced_opening_tracegen", n_elems, N, 0, 0, 0));
    if (n_calls > n_elems) return set_error(ctx, ZKHIP_ERR_INVALID, "reduced_opening_tracegen: more calls than elements (a call has at least one)");
    if ((((uintptr_t)d_alpha) | ((uintptr_t)d_b)) & 15u)
        return set_error(ctx, ZKHIP_ERR_INVALID, "reduced_opening_tracegen: d_alpha and d_b must be 16-byte aligned");
    if (n_calls == 0 && n_elems != 0) return set_error(ctx, ZKHIP_ERR_INVALID, "reduced_opening_tracegen: elements but no call (the lengths must sum to n_elems)");
    if (n_calls == 0) {   // no call, no element: padding only
        KernelScope ks(ctx, "reduced_opening_tracegen");
        ZK_HIP_CHECK(ctx, hipMemsetAsync(d_trace, 0, (size_t)ZKHIP_REDUCED_OPENING_WIDTH * N * 4, ctx->stream));
        return ZKHIP_OK;
    }
    // rows per workgroup of the passes: whole passes, at most RO_MAX_BLOCKS workgroups.  A workgroup of the passes takes at least two of
    // them where the trace has two: half the maps for k_ro_carries at the price of one carried word
    const auto whole = [](size_t x) { return (x + RO_W - 1) / RO_W * RO_W; };
    const size_t rows_per_block = std::max<size_t>(whole((N + RO_MAX_BLOCKS - 1) / RO_MAX_BLOCKS), 2 * RO_W);
    const unsigned row_blocks = (unsigned)((N + rows_per_block - 1) / rows_per_block);
    // scratch: off[n_calls + 1] | sums | maps[row_blocks][8] | carry[row_blocks][4]
    CallScratch s;
    ZK_TRY(call_scratch(ctx, n_calls, 1, 12 * (size_t)RO_MAX_BLOCKS, &s));
    uint32_t *off = s.off[0], *maps = s.extra, *carry = maps + 8 * RO_MAX_BLOCKS;
    uint64_t* sums = s.sums;
    const RoIn in{d_alpha, d_a, d_b, off, (uint32_t)n_calls, (uint32_t)n_elems};
    return tracegen_frame(
        ctx, "reduced_opening_tracegen", {},
        [&](uint32_t* bad) {
            launch_call_offsets(ctx, d_len, n_calls, n_elems, 0, true, sums, off, bad);   // k_ro_len_sums, k_ro_offsets
            hipLaunchKernelGGL(k_ro_pass<false>, dim3(row_blocks), dim3(RO_W), 0, ctx->stream, in, N, rows_per_block, maps, (uint32_t*)nullptr, bad);
            hipLaunchKernelGGL(k_ro_carries, dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)maps, row_blocks, carry);
            hipLaunchKernelGGL(k_ro_pass<true>, dim3(row_blocks), dim3(RO_W), 0, ctx->stream, in, N, rows_per_block, carry, d_trace, bad);
        },
        "reduced_opening_tracegen (a length of 0, lengths that do not sum to n_elems, or an operand that is not a field element)");
}

}  // extern "C"
