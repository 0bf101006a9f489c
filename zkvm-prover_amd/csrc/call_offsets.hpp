// call_offsets.hpp -- the first row of every call from the calls' lengths, on the device: what the generators of the chips whose calls take a
// variable number of consecutive rows share (reduced_opening.hip: one row per element; mmcs_rows.hip: one row per 8 words, and the words'
// own offsets).  An exclusive scan in 64 bits (2^27 lengths of 32 bits cannot overflow it) of ceil(len / 2^shift), two launches, no
// workgroup waits on another and nothing is read back:
//   k_ro_len_sums   the sum of each slice of calls
//   k_ro_offsets    off[c] (each workgroup adds the slices before its own, then scans its slice), the checks on the lengths
// Lengths that are refused still give offsets that are clamped to n_elems + 1 and non-decreasing.
#pragma once
#include <algorithm>

#include "../../include/zkhip.h"
#include "lds_barrier.hpp"
#include "zkhip_internal.hpp"

namespace zk {
namespace {

constexpr unsigned RO_W = ZKHIP_REDUCED_OPENING_BLOCK_ROWS;   // lanes of a workgroup of the offset kernels (and rows of one pass of the reduced-opening generator)
constexpr unsigned RO_WAVES = RO_W / 64;
constexpr unsigned RO_MAX_BLOCKS = 1024;                      // workgroups per launch (4 per CU)
static_assert(RO_W % 64 == 0 && RO_W <= 1024, "a workgroup pass is a whole number of waves");

__device__ __forceinline__ uint64_t u64_shfl_up(uint64_t v, unsigned off) {
    return ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
}
// the inclusive scan of one value per lane over the workgroup and the workgroup's sum; `tot` (LDS, a word per wave) is free again on return
__device__ __forceinline__ uint64_t block_scan_u64(uint64_t v, uint64_t* tot, uint64_t* total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const uint64_t o = u64_shfl_up(v, off);
        if (lane >= off) v += o;
    }
    zk_syncthreads();   // (every wave has read what the call before left in `tot`)
    if (lane == 63) tot[wave] = v;
    zk_syncthreads();
    uint64_t before = 0, all = 0;
    for (unsigned w = 0; w < RO_WAVES; w++) {
        const uint64_t t = tot[w];
        before += w < wave ? t : 0;
        all += t;
    }
    *total = all;
    return v + before;
}
// what a call of length l adds to the scan: ceil(l / 2^shift)
__device__ __forceinline__ uint64_t call_units(uint32_t l, unsigned shift) { return ((uint64_t)l + ((1u << shift) - 1u)) >> shift; }

// per_block: calls per workgroup, a multiple of RO_W
__global__ __launch_bounds__(RO_W) void k_ro_len_sums(const uint32_t* __restrict__ len, size_t n_calls, size_t per_block, unsigned shift, uint64_t* __restrict__ sums) {
    __shared__ uint64_t tot[RO_WAVES];
    const size_t begin = (size_t)blockIdx.x * per_block, end = std::min(begin + per_block, n_calls);
    uint64_t s = 0;
    for (size_t i = begin + threadIdx.x; i < end; i += RO_W) s += call_units(len[i], shift);
    uint64_t all;
    block_scan_u64(s, tot, &all);
    if (threadIdx.x == 0) sums[blockIdx.x] = all;
}

// off[c] = min(u[0] + .. + u[c - 1], n_elems + 1) for c <= n_calls with u = ceil(len / 2^shift); refuses a length of 0 and a total other
// than n_elems (exact) or beyond n_elems (!exact)
__global__ __launch_bounds__(RO_W) void k_ro_offsets(const uint32_t* __restrict__ len, size_t n_calls, size_t n_elems, size_t per_block, unsigned shift, int exact,
                                                     const uint64_t* __restrict__ sums, uint32_t* __restrict__ off, uint32_t* __restrict__ bad) {
    __shared__ uint64_t tot[RO_WAVES];
    const size_t begin = (size_t)blockIdx.x * per_block, end = std::min(begin + per_block, n_calls);
    const uint64_t cap = (uint64_t)n_elems + 1;
    uint64_t pre = 0, base;
    for (unsigned j = threadIdx.x; j < blockIdx.x; j += RO_W) pre += sums[j];
    block_scan_u64(pre, tot, &base);
    for (size_t start = begin; start < end; start += RO_W) {
        const size_t i = start + threadIdx.x;
        const uint32_t l = i < end ? len[i] : 0u;
        if (i < end && l == 0) atomicAdd(bad, 1u);
        const uint64_t u = call_units(l, shift);
        uint64_t all;
        const uint64_t incl = block_scan_u64(u, tot, &all);
        if (i < end) off[i] = (uint32_t)std::min(base + incl - u, cap);
        base += all;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        off[n_calls] = (uint32_t)std::min(base, cap);
        if (exact ? base != (uint64_t)n_elems : base > (uint64_t)n_elems) atomicAdd(bad, 1u);
    }
}

// both launches on the context's stream for n_calls >= 1 calls: off[0 .. n_calls] from len; `sums` holds RO_MAX_BLOCKS 64-bit words
inline void launch_call_offsets(zkhip_ctx* ctx, const uint32_t* d_len, size_t n_calls, size_t n_elems, unsigned shift, bool exact, uint64_t* sums, uint32_t* off,
                                uint32_t* bad) {
    const size_t per_block = ((n_calls + RO_MAX_BLOCKS - 1) / RO_MAX_BLOCKS + RO_W - 1) / RO_W * RO_W;   // whole rounds of a workgroup's scan
    const unsigned blocks = (unsigned)((n_calls + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_ro_len_sums, dim3(blocks), dim3(RO_W), 0, ctx->stream, d_len, n_calls, per_block, shift, sums);
    hipLaunchKernelGGL(k_ro_offsets, dim3(blocks), dim3(RO_W), 0, ctx->stream, d_len, n_calls, n_elems, per_block, shift, exact ? 1 : 0, (const uint64_t*)sums, off, bad);
}

// The scratch of such a generator (slot 3): n_off arrays of n_calls + 1 offsets, each rounded up to four words | sums[RO_MAX_BLOCKS] (64
// bits) | `extra_words` words of the generator's own
struct CallScratch {
    uint32_t* off[2];
    uint64_t* sums;
    uint32_t* extra;
};
inline int call_scratch(zkhip_ctx* ctx, size_t n_calls, unsigned n_off, size_t extra_words, CallScratch* s) {
    const size_t off_words = (n_calls + 1 + 3) / 4 * 4;
    void* buf = nullptr;
    ZK_TRY(get_scratch(ctx, 3, (n_off * off_words + 2 * (size_t)RO_MAX_BLOCKS + extra_words) * 4, &buf));
    uint32_t* p = (uint32_t*)buf;
    s->off[0] = p, s->off[1] = n_off > 1 ? p + off_words : nullptr;
    p += n_off * off_words;
    s->sums = (uint64_t*)p, s->extra = p + 2 * RO_MAX_BLOCKS;
    return ZKHIP_OK;
}

}  // namespace
}  // namespace zk
