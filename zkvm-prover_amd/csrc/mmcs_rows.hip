// mmcs_rows.hip -- the row-digest chip on the device (air.py mmcs_rows_air, include/zkhip_chips.hpp; docs/mmcs_rows.md): the sponge between
// the opened words of one query at one height class and the row digest the MMCS path chip claims for them.  A call of L words is
// ceil(L / 8) permutations, each on the output of the one before: many independent, strictly serial chains of very different lengths (1 to
// 55 permutations on the reference's stored openings).  So a call belongs to 16 lanes, not to one: lane i of the group holds state word i
// and the permutation is poseidon2_coop.hpp's -- four calls per wave.  Launches on the context's stream, none of which waits on another
// workgroup:
//   k_ro_len_sums, k_ro_offsets   woff[c] = the first word of call c (call_offsets.hpp, shared with reduced_opening.hip), the checks on
//                                 the lengths
//   k_ro_len_sums, k_ro_offsets   roff[c] = its first row: the same scan over ceil(len / 8), refused beyond the trace's rows
//   k_mmcs_rows                   the rows
// k_mmcs_rows is ONE flat loop per wave: every iteration is one permutation for each of the wave's four groups (DPP needs the 16 lanes of
// a row active, so a group with nothing left permutes along and stores nothing); a group whose call has ended takes the next one at the
// top of the iteration, from a counter in device memory (a vector atomic by the group's first lane).  Which group walks which call does
// not show in the trace.  The 56 cells of a row lie in 56 columns; a group keeps MR_SLOTS rows in LDS and stores them column by column,
// lane k the k-th of them: the consecutive rows of a call leave as runs of up to 64 bytes.
#include <algorithm>

#include "../../include/zkhip.h"
#include "babybear.hpp"
#include "call_offsets.hpp"
#include "hash_slice_host.hpp"
#include "lds_barrier.hpp"
#include "poseidon2_coop.hpp"
#include "tracegen_common.hpp"

namespace zk {
namespace {

constexpr unsigned MR_COLS = ZKHIP_MMCS_ROWS_WIDTH;
constexpr unsigned MR_SLOTS = 16;                         // rows a group stages = its lanes
constexpr unsigned MR_SLOT_STRIDE = MR_SLOTS + 1;         // (odd: the 16 lanes of a group write 16 columns of one slot to 16 banks)
constexpr unsigned MR_GROUP_WORDS = MR_COLS * MR_SLOT_STRIDE + 24;   // (= 16 mod 64: the four groups read disjoint banks)
static_assert(MR_COLS == 56, "st_in[16] | st_out[16] | f[8] | 16 cells a lane each");
static_assert(MR_GROUP_WORDS % 64 == 16, "bank offset between the groups");

struct MrIn {
    const uint32_t *len, *root, *lvl, *idx, *mult, *values;
    const uint32_t *woff, *roff;   // n_calls + 1 words each (k_ro_offsets)
    uint32_t n_calls, n_words;
};

// One wave per workgroup, four groups of 16 lanes.  Columns: lane i of a group owns st_in[i] (column i), st_out[i] (16 + i), f[i] (32 + i,
// i < 8) and cell 40 + i of is_first | is_last | is_real | root[8] | lvl | idx | mult | call | blk.  Every index made from the offsets is
// checked before it is used: refused lengths give clamped offsets, and a call's length is taken from them, never from len[].
__global__ __launch_bounds__(64) void k_mmcs_rows(MrIn in, size_t N, uint32_t* __restrict__ next_call, uint32_t* __restrict__ trace, uint32_t* __restrict__ hash_inputs,
                                                  uint32_t* __restrict__ digest, uint32_t* __restrict__ bad) {
    __shared__ uint32_t stage[4][MR_GROUP_WORDS];
    __shared__ uint32_t stage_row[4][MR_SLOTS];
    const unsigned lane = threadIdx.x & 15u, g = threadIdx.x >> 4;
    const CoopConsts cc = coop_load_consts(lane);
    uint32_t* const sg = stage[g];
    uint32_t x = 0;                                  // state word `lane` of the group's call
    uint32_t c = 0, t = 0, nblk = 0, L = 0, w0 = 0, r0 = 0, cell = 0;
    bool done = false;
    unsigned filled = 0;
    for (;;) {
        if (!done && t == nblk) {                    // (the same for the 16 lanes of a group) the call has ended: the next one
            uint32_t nc = 0;
            if (lane == 0) nc = atomicAdd(next_call, 1u);
            c = (uint32_t)__shfl((int)nc, 0, 16);
            t = 0, nblk = 0, x = 0;
            if (c >= in.n_calls) {
                done = true;
            } else {
                w0 = in.woff[c], L = in.woff[c + 1] - w0, r0 = in.roff[c];
                nblk = (L + 7u) >> 3;                // (0 for a call the offsets were clamped in front of: refused there)
                uint32_t v = 0;                      // the call's cell of column 40 + lane; the per-row ones are set below
                if (lane >= 3 && lane <= 10) v = in.root[8 * (size_t)c + (lane - 3)];
                else if (lane == 11) v = in.lvl[c];
                else if (lane == 12) v = in.idx[c];
                else if (lane == 13) v = in.mult[c];
                else if (lane == 14) v = c;
                cell = field_word(v, bad);
            }
        }
        const bool all_done = __all(done);
        if (!all_done) {
            const bool act = !done && t < nblk;
            const uint32_t k = act ? std::min(8u, L - 8u * t) : 0u;   // words of this block
            if (lane < k) {
                const uint32_t e = w0 + 8u * t + lane;
                x = field_word(e < in.n_words ? in.values[e] : 0u, bad);
            }
            const uint32_t st_in = x;
            x = coop_permute_regs(x, lane, cc);
            const bool last = t + 1 == nblk;
            const size_t r = (size_t)r0 + t;
            const bool put = act && r < N;
            uint32_t m = cell;
            if (lane == 0) m = t == 0 ? MONTY_ONE : 0u;
            else if (lane == 1) m = last ? MONTY_ONE : 0u;
            else if (lane == 2) m = MONTY_ONE;
            else if (lane == 13) m = last ? cell : 0u;
            else if (lane == 15) m = to_monty(t);
            if (lane == 0) stage_row[g][filled] = put ? (uint32_t)r : ~0u;
            sg[lane * MR_SLOT_STRIDE + filled] = st_in;
            sg[(16 + lane) * MR_SLOT_STRIDE + filled] = x;
            if (lane < 8) sg[(32 + lane) * MR_SLOT_STRIDE + filled] = lane < k ? MONTY_ONE : 0u;
            sg[(40 + lane) * MR_SLOT_STRIDE + filled] = m;
            if (put) hash_inputs[16 * r + lane] = st_in;
            if (act && last && digest && lane < 8) digest[8 * (size_t)c + lane] = from_monty(x);
            if (act) t++;
            filled++;
        }
        if (filled == MR_SLOTS || (all_done && filled)) {   // (the same for the whole wave) the staged rows out, along rows
            zk_syncthreads();
            const uint32_t r = lane < filled ? stage_row[g][lane] : ~0u;
            if (r != ~0u) {
#pragma unroll
                for (unsigned q = 0; q < MR_COLS; q++) trace[(size_t)q * N + r] = sg[q * MR_SLOT_STRIDE + lane];
            }
            zk_syncthreads();
            filled = 0;
        }
        if (all_done) break;
    }
}

}  // namespace
}  // namespace zk

using namespace zk;

extern "C" {

int zkhip_hash_slice_host(const uint32_t* in, size_t len, uint32_t out[8]) {
    try {
        return hash_slice_canonical(in, len, out);
    } catch (const std::exception&) {
        return ZKHIP_ERR_NOMEM;
    }
}

int zkhip_mmcs_rows_tracegen(zkhip_ctx* ctx, const uint32_t* d_len, const uint32_t* d_root, const uint32_t* d_lvl, const uint32_t* d_idx, const uint32_t* d_mult,
                             const uint32_t* d_values, size_t n_calls, size_t n_words, unsigned log_height, uint32_t* d_trace, uint32_t* d_hash_inputs,
                             uint32_t* d_digest) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !d_trace || !d_hash_inputs || log_height > 27 || (n_calls && (!d_len || !d_root || !d_lvl || !d_idx || !d_mult)) || (n_words && !d_values))
        return ZKHIP_ERR_INVALID;
    const size_t N = (size_t)1 << log_height;
    // (what keeps the offsets inside 32 bits; both would be refused by the device's checks as well)
    if (n_words > 8 * N) return set_error(ctx, ZKHIP_ERR_INVALID, "mmcs_rows_tracegen: more rows than the trace has");
    if (n_calls > n_words) return set_error(ctx, ZKHIP_ERR_INVALID, "mmcs_rows_tracegen: more calls than words (a call has at least one)");
    if (n_calls == 0 && n_words != 0) return set_error(ctx, ZKHIP_ERR_INVALID, "mmcs_rows_tracegen: words but no call (the lengths must sum to n_words)");
    // scratch: woff[n_calls + 1] | roff[n_calls + 1] | sums | the call counter
    CallScratch s;
    ZK_TRY(call_scratch(ctx, n_calls, 2, 4, &s));
    uint32_t *woff = s.off[0], *roff = s.off[1], *next_call = s.extra;
    uint64_t* sums = s.sums;
    const MrIn in{d_len, d_root, d_lvl, d_idx, d_mult, d_values, woff, roff, (uint32_t)n_calls, (uint32_t)n_words};
    // as many groups as calls, up to the 10 one-wave workgroups whose staging fits a CU's LDS: the counter balances the rest
    const size_t waves = std::min<size_t>((n_calls + 3) / 4, (size_t)std::max(ctx->cu_count, 1) * 10);
    return tracegen_frame(
        ctx, "mmcs_rows_tracegen", {},
        [&](uint32_t* bad) -> int {
            ZK_HIP_CHECK(ctx, hipMemsetAsync(d_trace, 0, (size_t)ZKHIP_MMCS_ROWS_WIDTH * N * 4, ctx->stream));
            ZK_HIP_CHECK(ctx, hipMemsetAsync(d_hash_inputs, 0, 16 * N * 4, ctx->stream));
            if (!n_calls) return ZKHIP_OK;
            ZK_HIP_CHECK(ctx, hipMemsetAsync(next_call, 0, 4, ctx->stream));
            launch_call_offsets(ctx, d_len, n_calls, n_words, 0, true, sums, woff, bad);
            launch_call_offsets(ctx, d_len, n_calls, N, 3, false, sums, roff, bad);
            hipLaunchKernelGGL(k_mmcs_rows, dim3((unsigned)waves), dim3(64), 0, ctx->stream, in, N, next_call, d_trace, d_hash_inputs, d_digest, bad);
            return ZKHIP_OK;
        },
        "mmcs_rows_tracegen (a length of 0, lengths that do not sum to n_words, more rows than the trace has, or a word that is not a field element)");
}

}  // extern "C"
