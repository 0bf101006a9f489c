// transcript_dev.hpp -- the device transcript's register form: one wave holds the duplex sponge (lanes 0..15 a state word each,
// poseidon2_coop.hpp); kernels that run a protocol step in-kernel (csrc/transcript.hip, csrc/logup_gkr.hip) load it, observe and
// sample on it, and store it back.
#pragma once
#include "poseidon2_coop.hpp"
#include "transcript.hpp"

namespace zk {

// All transcript kernels run one wave; lanes 0..15 hold the sponge state (poseidon2_coop.hpp).
struct TrRegs {
    uint32_t s;  // state word of this lane (lane < 16)
    uint32_t n_in, n_out;
};
__device__ __forceinline__ TrRegs tr_load(const DevTranscript* t, unsigned lane) {
    TrRegs r;
    r.s = t->state[lane & 15u];
    r.n_in = t->n_in;
    r.n_out = t->n_out;
    return r;
}
__device__ __forceinline__ void tr_store(DevTranscript* t, const TrRegs& r, unsigned lane) {
    if (lane < 16) t->state[lane] = r.s;
    if (lane == 0) {
        t->n_in = r.n_in;
        t->n_out = r.n_out;
    }
}
__device__ __forceinline__ void tr_duplex(TrRegs& r, unsigned lane) {
    r.s = coop_permute(r.s, lane & 15u);
    r.n_in = 0;
    r.n_out = 8;
}
__device__ __forceinline__ void tr_observe1(TrRegs& r, unsigned lane, uint32_t v) {
    r.n_out = 0;
    if ((lane & 15u) == r.n_in) r.s = v;
    r.n_in++;
    if (r.n_in == 8) tr_duplex(r, lane);
}
__device__ __forceinline__ uint32_t tr_sample1(TrRegs& r, unsigned lane) {
    if (r.n_in != 0 || r.n_out == 0) tr_duplex(r, lane);
    r.n_out--;
    return __shfl(r.s, (int)r.n_out, 64);
}
// the same three steps with this lane's round constants in registers (coop_load_consts): for kernels that run many transcript steps
__device__ __forceinline__ void tr_duplex(TrRegs& r, unsigned lane, const CoopConsts& cc) {
    r.s = coop_permute_regs(r.s, lane & 15u, cc);
    r.n_in = 0;
    r.n_out = 8;
}
__device__ __forceinline__ void tr_observe1(TrRegs& r, unsigned lane, uint32_t v, const CoopConsts& cc) {
    r.n_out = 0;
    if ((lane & 15u) == r.n_in) r.s = v;
    r.n_in++;
    if (r.n_in == 8) tr_duplex(r, lane, cc);
}
__device__ __forceinline__ uint32_t tr_sample1(TrRegs& r, unsigned lane, const CoopConsts& cc) {
    if (r.n_in != 0 || r.n_out == 0) tr_duplex(r, lane, cc);
    r.n_out--;
    return __shfl(r.s, (int)r.n_out, 64);
}

}  // namespace zk
