// airbatch_pass.hip -- the per-class constraint kernels of the batched AIR-set proof (docs/airbatch.md): the zero-check's bodies
// (zerocheck_dev.hpp) per job.  A workgroup, still one wave, finds its job by a binary search over the jobs' first workgroups; D_a, BUS
// and (the keyed form) PREP stay compile-time, so a round is one launch per (D_a, BUS, PREP) class over that class's run of the job
// table.  The host side (the job table, the rounds' order) is prove_batch in airset.hip.
#include "airbatch_job.hpp"

namespace zk {

// round 0 of every job of one class
template <unsigned D, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zb_round0(const ZbJob* __restrict__ jobs, uint32_t n) {
    const ZbJob jb = jobs[zb_job_of(jobs, n, blockIdx.x)];
    zc_round0_body<D, BUS, false>(jb.pg, jb.trace, nullptr, jb.m, jb.E, jb.E2, jb.partial, blockIdx.x - jb.first_wg, jb.n_wg);
}

// round i >= 1 of every job of one class that is still alive: fold with r_{i-1} and evaluate; a job with m = i runs its last fold only
template <unsigned D, bool FROM_BASE, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zb_pass(const ZbJob* __restrict__ jobs, uint32_t n, uint32_t i, const uint32_t* __restrict__ r_ptr) {
    const ZbJob jb = jobs[zb_job_of(jobs, n, blockIdx.x)];
    if (jb.m < i) return;
    const size_t sA = (size_t)1 << (jb.m - 1), sB = jb.m >= 2 ? (size_t)1 << (jb.m - 2) : 1;
    ZcTabs tb{};
    tb.trace = jb.trace, tb.E = jb.E, tb.E2 = jb.E2, tb.rot = jb.rot, tb.m = jb.m, tb.w = jb.w, tb.n_rot = jb.n_rot;
    tb.nd = (size_t)1 << (jb.m - i);
    if (i & 1u) tb.src = jb.tB, tb.src_stride = sB, tb.dst = jb.tA, tb.dst_stride = sA;
    else tb.src = jb.tA, tb.src_stride = sA, tb.dst = jb.tB, tb.dst_stride = sB;
    ZcProg pg = jb.pg;
    pg.code = jb.xcode;
    zc_pass_body<D, FROM_BASE, BUS, false>(pg, tb, ZcPrep{}, r_ptr, jb.m == i ? nullptr : jb.partial, blockIdx.x - jb.first_wg, jb.n_wg);
}

// the keyed form's classes with preprocessed columns: the same bodies in their PREP form, on the job's ZcPrep; the extension passes'
// code names the preprocessed tables in K_VAR operands (prove_batch's remap), so only the table count differs
template <unsigned D, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zb_round0_p(const ZbJob* __restrict__ jobs, uint32_t n) {
    const ZbJob jb = jobs[zb_job_of(jobs, n, blockIdx.x)];
    zc_round0_body<D, BUS, true>(jb.pg, jb.trace, jb.pp.cols, jb.m, jb.E, jb.E2, jb.partial, blockIdx.x - jb.first_wg, jb.n_wg);
}
template <unsigned D, bool FROM_BASE, bool BUS>
__global__ __launch_bounds__(ZC_W) void k_zb_pass_p(const ZbJob* __restrict__ jobs, uint32_t n, uint32_t i, const uint32_t* __restrict__ r_ptr) {
    const ZbJob jb = jobs[zb_job_of(jobs, n, blockIdx.x)];
    if (jb.m < i) return;
    const size_t sA = (size_t)1 << (jb.m - 1), sB = jb.m >= 2 ? (size_t)1 << (jb.m - 2) : 1;
    ZcTabs tb{};
    tb.trace = jb.trace, tb.E = jb.E, tb.E2 = jb.E2, tb.rot = jb.rot, tb.m = jb.m, tb.w = jb.w, tb.n_rot = jb.n_rot;
    tb.nd = (size_t)1 << (jb.m - i);
    if (i & 1u) tb.src = jb.tB, tb.src_stride = sB, tb.dst = jb.tA, tb.dst_stride = sA;
    else tb.src = jb.tA, tb.src_stride = sA, tb.dst = jb.tB, tb.dst_stride = sB;
    ZcProg pg = jb.pg;
    pg.code = jb.xcode;
    zc_pass_body<D, FROM_BASE, BUS, true>(pg, tb, jb.pp, r_ptr, jb.m == i ? nullptr : jb.partial, blockIdx.x - jb.first_wg, jb.n_wg);
}

namespace {
template <unsigned D, bool BUS>
void zb_launch_d(hipStream_t st, unsigned grid, size_t lds, const ZbJob* jobs, uint32_t n, unsigned i, const uint32_t* r) {
    if (i == 0) hipLaunchKernelGGL((k_zb_round0<D, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n);
    else if (i == 1) hipLaunchKernelGGL((k_zb_pass<D, true, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n, i, r);
    else hipLaunchKernelGGL((k_zb_pass<D, false, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n, i, r);
}
template <unsigned D, bool BUS>
void zb_launch_dp(hipStream_t st, unsigned grid, size_t lds, const ZbJob* jobs, uint32_t n, unsigned i, const uint32_t* r) {
    if (i == 0) hipLaunchKernelGGL((k_zb_round0_p<D, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n);
    else if (i == 1) hipLaunchKernelGGL((k_zb_pass_p<D, true, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n, i, r);
    else hipLaunchKernelGGL((k_zb_pass_p<D, false, BUS>), dim3(grid), dim3(ZC_W), lds, st, jobs, n, i, r);
}
}  // namespace

// round i of the class (D, bus, prep) over its n jobs
void zb_launch(unsigned D, bool bus, bool prep, hipStream_t st, unsigned grid, size_t lds, const ZbJob* jobs, uint32_t n, unsigned i,
               const uint32_t* r) {
    switch (D) {
#define ZB_CASE(d)                                                                                                                              \
    case d:                                                                                                                                     \
        if (prep) return bus ? zb_launch_dp<d, true>(st, grid, lds, jobs, n, i, r) : zb_launch_dp<d, false>(st, grid, lds, jobs, n, i, r); \
        return bus ? zb_launch_d<d, true>(st, grid, lds, jobs, n, i, r) : zb_launch_d<d, false>(st, grid, lds, jobs, n, i, r);
        ZB_CASE(1) ZB_CASE(2) ZB_CASE(3) ZB_CASE(4) ZB_CASE(5) ZB_CASE(6) ZB_CASE(7) ZB_CASE(8)
#undef ZB_CASE
    }
}

}  // namespace zk
