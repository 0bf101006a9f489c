// airbatch_job.hpp -- the job entry of the batched AIR-set proof (docs/airbatch.md) and the launch of its per-class constraint
// kernels: what airset.hip (host side, through airbatch_dev.hpp) and airbatch_pass.hip (the kernels) share.
#pragma once
#include "zerocheck_dev.hpp"

namespace zk {

// one active AIR in the batched constraint sum-check.  The jobs of a (D, BUS, PREP) class are consecutive, tallest first; first_wg
// counts from the class's first job.
struct ZbJob {
    ZcProg pg;               // the base round's program; apow is the set's alpha powers
    const uint32_t* xcode;   // the extension passes' copy (tables in place of cells)
    const uint32_t* trace;
    const uint32_t* E;       // eq(tau[0..m), .); an AIR without proven constraints: E2
    const uint32_t* E2;      // BUS: eq(rho[0..m), .)
    const uint32_t* rot;
    uint32_t* tA;            // ping-pong tables: nt tables of 2^(m-1) entries, and of max(2^(m-2), 1)
    uint32_t* tB;
    uint32_t* partial;       // 4 D SC_NB words
    uint32_t m, w, n_rot, D;
    uint32_t j;              // its number among the active AIRs, caller order: the weight is mu^j 2^(M - m)
    uint32_t first_wg, n_wg;
    uint32_t val_at;         // its v, v' in the proof's value section (words)
    uint32_t cst_at, cst_n;  // BUS: its interactions in the constant table
    uint32_t b_at;           // BUS: its leaf claim's number
    ZcPrep pp;               // PREP (the keyed form): the key's columns of this AIR, rot_p in the upload; wp = 0: none
};

// the job of a workgroup: the last one whose first_wg is <= wg
__device__ __forceinline__ uint32_t zb_job_of(const ZbJob* __restrict__ jobs, uint32_t n, uint32_t wg) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_wg <= wg) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// round i of the class (D, bus, prep) over its n jobs: k_zb_round0 / k_zb_pass, with prep their PREP forms (airbatch_pass.hip)
void zb_launch(unsigned D, bool bus, bool prep, hipStream_t st, unsigned grid, size_t lds, const ZbJob* jobs, uint32_t n, unsigned i,
               const uint32_t* r);

}  // namespace zk
