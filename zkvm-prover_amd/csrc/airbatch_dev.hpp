// airbatch_dev.hpp -- the device side of the batched AIR-set proof (docs/airbatch.md), included by airset.hip alone: ONE constraint
// sum-check and ONE rotation reduction for a whole set of AIRs.  Every launch takes a job table that was uploaded once, so neither
// the launches nor the host round trips grow with the number of AIRs.
//
// The constraint rounds run the zero-check's bodies (zerocheck_dev.hpp) per job: a workgroup, still one wave, finds its job by a
// binary search over the jobs' first workgroups (as_block_of's pattern); D_a, BUS and (the keyed form) PREP stay compile-time, so a
// round is one launch per (D_a, BUS, PREP) class over that class's run of the job table.  One workgroup per round (k_zb_round_tr) adds the jobs' partial sums
// up, extends every s_a from 0..D_a to 0..D, weights, writes the round, runs the transcript step and keeps every AIR's running claim.
// The job entry (ZbJob) is in airbatch_job.hpp; the per-class constraint kernels (k_zb_round0, k_zb_pass and their PREP forms) are a
// translation unit of their own, airbatch_pass.hip, reached through zb_launch: they are most of this proof's device code, and the
// build compiles the two units side by side.
#pragma once
#include "airbatch_job.hpp"

namespace zk {

constexpr unsigned ZB_TR = 1024;                               // threads of the round kernels: a wave per job at a time
constexpr unsigned ZB_MAX_JOBS = ZKHIP_STACK_MAX_POINTS;       // one job per active AIR
constexpr unsigned ZB_PTS = ZKHIP_ZEROCHECK_MAX_DEGREE + 1;    // points 0..D of a round polynomial

// workgroups of a job that hold pairs in round i (i < m): the single-AIR grid_w, within the job's range
__device__ __forceinline__ uint32_t zb_wgs(uint32_t m, uint32_t i, uint32_t n_wg) {
    const uint64_t pairs = (uint64_t)1 << (m - i - 1), need = (pairs + ZC_W - 1) / ZC_W;
    return (uint32_t)(need < n_wg ? need : n_wg);
}

// one interaction of a BUS job: its denominators' constant part leaves through the claim
struct ZbCst {
    uint32_t coef_at;   // its count root among the job's bus coefficients: the coefficient there is +-e
    uint32_t bus1;      // bus + 1, Montgomery
    uint32_t sign;
};

// what the round kernel reads besides the jobs
struct ZbTr {
    const uint32_t* mu;
    const uint32_t* lagx;    // [d][t][j]: the weight of s(j), j <= d, in s(t), t > d (base field)
    const uint32_t* lagw;    // [t]: 1 / prod_{i != t} (t - i) over 0..D
    const ZbCst* cst;
    const uint32_t* chal;    // BUS: gamma | beta | kappa
    const uint32_t* dB;      // BUS: the leaf claims, canonical
    uint32_t* wgt;           // per job mu^j 2^(M - m)
    uint32_t* claim;         // per job: s_a's running claim; once it ran out, its constant's current value g_a(r_a) / 2^k
    uint32_t* proof;         // the rounds: 4 D words each
    uint32_t* r;             // the challenges: 4 words each
};

__device__ __forceinline__ Ext zb_lds(const uint32_t* p, unsigned i) { return Ext{{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]}}; }
__device__ __forceinline__ void zb_lds_st(uint32_t* p, unsigned i, const Ext& e) {
    for (int q = 0; q < 4; q++) p[4 * i + q] = e.c[q];
}

// wave `wave` of nw: the sums of word k < n_words of every job it owns over that job's nb workgroups, to raw[job * stride + k]
template <class NB, class NW>
__device__ __forceinline__ void zb_sum_partials(unsigned n_jobs, unsigned wave, unsigned nw, unsigned lane, uint32_t* raw, unsigned stride, NB nb_of,
                                                NW words_of, const uint32_t* const* partial_of) {
    for (unsigned job = wave; job < n_jobs; job += nw) {
        const unsigned nb = nb_of(job), n_words = words_of(job);
        const uint32_t* part = partial_of[job];
        for (unsigned k = 0; k < n_words; k++) {
            uint32_t x = 0;
            for (unsigned b = lane; b < nb; b += 64) x = madd(x, part[(size_t)k * SC_NB + b]);
            x = sc_wave_sum(x);
            if (lane == 0) raw[job * stride + k] = x;
        }
    }
}

// wave 0: word k of the round = the sum over the jobs of wt[job * stride + k]; written (canonical), observed; then r is sampled
__device__ __forceinline__ void zb_tr_step(DevTranscript* tr, unsigned lane, unsigned n_jobs, const uint32_t* wt, unsigned stride, unsigned n_words,
                                           uint32_t* proof, uint32_t* r_out, uint32_t* r_lds) {
    const CoopConsts cc = coop_load_consts(lane & 15u);
    TrRegs R = tr_load(tr, lane);
    for (unsigned k = 0; k < n_words; k++) {
        const uint32_t x = sc_wave_sum(lane < n_jobs ? wt[lane * stride + k] : 0u);
        if (lane == 0) proof[k] = from_monty(x);
        tr_observe1(R, lane, x, cc);
    }
    for (int q = 0; q < 4; q++) {
        const uint32_t v = tr_sample1(R, lane, cc);
        if (lane == 0) r_out[q] = v, r_lds[q] = v;
    }
    tr_store(tr, R, lane);
}

// Round `round` of the batched constraint sum-check, one workgroup.  s = sum_a wgt_a s_a + the used-up AIRs' constants at 0, 2, .., D.
__global__ __launch_bounds__(ZB_TR) void k_zb_round_tr(DevTranscript* tr, const ZbJob* __restrict__ jobs, unsigned n_jobs, unsigned round, unsigned M,
                                                        unsigned D, ZbTr a) {
    __shared__ uint32_t S[ZB_MAX_JOBS * ZB_PTS * 4];    // per job: the raw sums (point e of 0, 2, .., D_a at word 4 e), then s_a(0..D)
    __shared__ uint32_t Wt[ZB_MAX_JOBS * ZB_PTS * 4];   // per job: its weighted contribution at 0, 2, .., D (4 D words)
    __shared__ uint32_t s_claim[ZB_MAX_JOBS * 4], s_wgt[ZB_MAX_JOBS * 4], s_basis[ZB_PTS * 4], s_r[4];
    __shared__ const uint32_t* s_part[ZB_MAX_JOBS];
    __shared__ uint32_t s_m[ZB_MAX_JOBS], s_d[ZB_MAX_JOBS], s_nwg[ZB_MAX_JOBS];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    constexpr unsigned STR = ZB_PTS * 4;
    if (tid < n_jobs) {
        const ZbJob& jb = jobs[tid];
        s_part[tid] = jb.partial, s_m[tid] = jb.m, s_d[tid] = jb.D, s_nwg[tid] = jb.n_wg;
        Ext w, c;
        if (round == 0) {   // the weight, and the claim c_a = B_a - kappa sum_j e_j (gamma + bus_j + 1) (0 without a bus part)
            w = ext_mul_base(ext_pow(sc_ld(a.mu, 0), jb.j), mpow(to_monty(2), M - jb.m));
            c = ext_zero();
            if (jb.cst_n) {
                const Ext gamma = sc_ld(a.chal, 0), kappa = sc_ld(a.chal, 2);
                Ext acc = ext_zero();
                for (unsigned k = 0; k < jb.cst_n; k++) {
                    const ZbCst cs = a.cst[jb.cst_at + k];
                    const Ext e = sc_ld(jb.pg.bcoef, cs.coef_at);
                    Ext g1 = gamma;
                    g1.c[0] = madd(g1.c[0], cs.bus1);
                    acc = ext_add(acc, ext_mul(cs.sign ? ext_neg(e) : e, g1));
                }
                for (int q = 0; q < 4; q++) c.c[q] = to_monty(a.dB[4 * jb.b_at + q]);
                c = ext_sub(c, ext_mul(kappa, acc));
            }
            sc_st(a.wgt, tid, w);
        } else {
            w = sc_ld(a.wgt, tid), c = sc_ld(a.claim, tid);
        }
        zb_lds_st(s_wgt, tid, w), zb_lds_st(s_claim, tid, c);
    }
    zk_syncthreads();
    zb_sum_partials(
        n_jobs, wave, ZB_TR / 64, lane, S, STR, [&](unsigned job) { return s_m[job] > round ? zb_wgs(s_m[job], round, s_nwg[job]) : 0u; },
        [&](unsigned job) { return s_m[job] > round ? 4 * s_d[job] : 0u; }, s_part);
    zk_syncthreads();
    if (tid < n_jobs) {
        uint32_t* Sj = S + tid * STR;
        uint32_t* Wj = Wt + tid * STR;
        const Ext w = zb_lds(s_wgt, tid);
        Ext c = zb_lds(s_claim, tid);
        const unsigned d = s_d[tid];
        if (s_m[tid] > round) {
            // the raw sums are s_a at 0, 2, .., d: move them to their points, s_a(1) from the claim, then d + 1 .. D
            for (unsigned e = d; e-- > 1;) zb_lds_st(Sj, e + 1, zb_lds(Sj, e));
            zb_lds_st(Sj, 1, ext_sub(c, zb_lds(Sj, 0)));
            for (unsigned t = d + 1; t <= D; t++) {
                Ext x = ext_zero();
                for (unsigned j = 0; j <= d; j++) x = ext_add(x, ext_mul_base(zb_lds(Sj, j), a.lagx[(d * ZB_PTS + t) * ZB_PTS + j]));
                zb_lds_st(Sj, t, x);
            }
            zb_lds_st(Wj, 0, ext_mul(w, zb_lds(Sj, 0)));
            for (unsigned t = 2; t <= D; t++) zb_lds_st(Wj, t - 1, ext_mul(w, zb_lds(Sj, t)));
        } else {   // used up: the constant, halved every round
            c = ext_mul_base(c, to_monty((P + 1) / 2));
            zb_lds_st(s_claim, tid, c);
            const Ext k = ext_mul(w, c);
            for (unsigned e = 0; e < D; e++) zb_lds_st(Wj, e, k);
        }
    }
    zk_syncthreads();
    if (wave == 0) zb_tr_step(tr, lane, n_jobs, Wt, STR, 4 * D, a.proof + 4 * (size_t)D * round, a.r + 4 * round, s_r);
    zk_syncthreads();
    // the Lagrange basis on 0..D at r, then every live job's claim s_a(r)
    const Ext r = zb_lds(s_r, 0);
    if (tid <= D) {
        Ext b = ext_from_base(a.lagw[tid]);
        for (unsigned i = 0; i <= D; i++)
            if (i != tid) b = ext_mul(b, ext_sub(r, ext_from_base(zc_small(i))));
        zb_lds_st(s_basis, tid, b);
    }
    zk_syncthreads();
    if (tid < n_jobs) {
        Ext c = zb_lds(s_claim, tid);
        if (s_m[tid] > round) {
            c = ext_zero();
            for (unsigned t = 0; t <= D; t++) c = ext_add(c, ext_mul(zb_lds(s_basis, t), zb_lds(S + tid * STR, t)));
        }
        sc_st(a.claim, tid, c);
    }
}

// v, v' (v_p, v_p') of every job: entry 0 of the tables its last fold wrote, canonical, to out + val_at
__global__ __launch_bounds__(64) void k_zb_emit(const ZbJob* __restrict__ jobs, uint32_t* __restrict__ out) {
    const ZbJob& jb = jobs[blockIdx.x];
    const uint32_t* tab = (jb.m & 1u) ? jb.tA : jb.tB;
    const size_t stride = (jb.m & 1u) ? (size_t)1 << (jb.m - 1) : (jb.m >= 2 ? (size_t)1 << (jb.m - 2) : 1);
    for (unsigned i = threadIdx.x; i < 4 * (jb.w + jb.n_rot + jb.pp.wp + jb.pp.n_rot); i += 64) out[jb.val_at + i] = from_monty(tab[4 * (size_t)(i >> 2) * stride + (i & 3u)]);
}

// ---- the batched rotation reduction ----------------------------------------------------------------------------------------------
// one reducing AIR: F_a, F_b (2^m entries each), eq(r[0..m), .), its folded tables (4 of 2^(m-1) and of max(2^(m-2), 1) entries)
struct ZbRot {
    const uint32_t* trace;
    const uint32_t* rot;
    const uint32_t* lpow;    // lambda^(o_a + k)
    const uint32_t* E;
    uint32_t* fa;
    uint32_t* fb;
    uint32_t* tA;
    uint32_t* tB;
    uint32_t* partial;       // 8 SC_NB words
    uint32_t m, w, n_rot;
    uint32_t wgt;            // 2^(M' - m), Montgomery
    uint32_t u_at;           // its u in the proof's u section (words)
    ZcPrep pp;               // the keyed form: the job's
};

// F_a and F_b of every reducing AIR: blockIdx.y is the AIR
__global__ __launch_bounds__(256) void k_zb_combine(const ZbRot* __restrict__ jobs) {
    const ZbRot jb = jobs[blockIdx.y];
    zc_combine_body<false>(jb.trace, (size_t)1 << jb.m, jb.w, jb.rot, jb.n_rot, ZcPrep{}, jb.lpow, jb.fa, jb.fb);
}

// the keyed form: lambda's powers run on over [v_p | v_p'], F_a gains the key's columns and F_b the rotated ones
__global__ __launch_bounds__(256) void k_zb_combine_p(const ZbRot* __restrict__ jobs) {
    const ZbRot jb = jobs[blockIdx.y];
    zc_combine_body<true>(jb.trace, (size_t)1 << jb.m, jb.w, jb.rot, jb.n_rot, jb.pp, jb.lpow, jb.fa, jb.fb);
}

// Round t of the reduction for every AIR with m >= t (blockIdx.y): from round 1 on the four tables are folded with r'_{t-1} first (from
// F_a, F_b and eq in round 1, from the other buffer later) and written out; an AIR with m = t folds only.
__global__ __launch_bounds__(256) void k_zb_rot_pass(const ZbRot* __restrict__ jobs, uint32_t t, const uint32_t* __restrict__ r_ptr) {
    const ZbRot jb = jobs[blockIdx.y];
    if (jb.m < t) return;   // uniform across the workgroup
    const size_t n = (size_t)1 << jb.m, sA = n >> 1, sB = jb.m >= 2 ? n >> 2 : 1;
    const ZcRotSrc base{jb.fa, jb.fb, jb.E, n - 1};
    const bool alive = jb.m > t;
    const size_t nd = n >> t, n_items = alive ? nd >> 1 : 1;
    const uint32_t* src = (t & 1u) ? jb.tB : jb.tA;
    uint32_t* dst = (t & 1u) ? jb.tA : jb.tB;
    const size_t ss = (t & 1u) ? sB : sA, ds = (t & 1u) ? sA : sB;
    const Ext r = t ? sc_ld(r_ptr, 0) : ext_zero();
    Ext acc[2] = {ext_zero(), ext_zero()};
    for (size_t y = (size_t)blockIdx.x * 256 + threadIdx.x; y < n_items; y += (size_t)gridDim.x * 256) {
        Ext f0[4], f1[4];
#pragma unroll
        for (unsigned q = 0; q < 4; q++) {
            if (t == 0) {
                f0[q] = base(q, 2 * y), f1[q] = base(q, 2 * y + 1);
            } else {
                auto entry = [&](size_t e) {   // entry e of this round's table q
                    return t == 1 ? sc_fold(base(q, 2 * e), base(q, 2 * e + 1), r) : sc_fold(sc_ld(src, q * ss + 2 * e), sc_ld(src, q * ss + 2 * e + 1), r);
                };
                f0[q] = entry(2 * y);
                sc_st(dst, q * ds + 2 * y, f0[q]);
                if (alive) f1[q] = entry(2 * y + 1), sc_st(dst, q * ds + 2 * y + 1, f1[q]);
            }
        }
        if (alive) sc_eval(ZcRotRound{}, f0, f1, acc);
    }
    if (!alive) return;
    sc_block_sum(acc, jb.partial + blockIdx.x);
}

struct ZbRotTr {
    uint32_t* state;   // per used-up AIR: its constant's current value
    uint32_t* proof;   // 8 words a round
    uint32_t* r;
};

// Round t of the reduction, one workgroup: s(0), s(2) = sum_a 2^(M' - m_a) s_a + the used-up AIRs' constants
__global__ __launch_bounds__(ZB_TR) void k_zb_rot_tr(DevTranscript* tr, const ZbRot* __restrict__ jobs, unsigned n_jobs, unsigned t, ZbRotTr a) {
    __shared__ uint32_t S[ZB_MAX_JOBS * 8], s_r[4];
    __shared__ const uint32_t* s_part[ZB_MAX_JOBS];
    __shared__ uint32_t s_m[ZB_MAX_JOBS];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid < n_jobs) s_part[tid] = jobs[tid].partial, s_m[tid] = jobs[tid].m;
    zk_syncthreads();
    zb_sum_partials(
        n_jobs, wave, ZB_TR / 64, lane, S, 8,
        [&](unsigned job) {   // k_zb_rot_pass's grid over its pairs
            if (s_m[job] <= t) return 0u;
            const uint64_t need = ((((uint64_t)1 << (s_m[job] - t)) >> 1) + 255) / 256;
            return (uint32_t)(need < 1 ? 1 : need > SC_NB ? SC_NB : need);
        },
        [&](unsigned job) { return s_m[job] > t ? 8u : 0u; }, s_part);
    zk_syncthreads();
    if (tid < n_jobs) {
        const ZbRot& jb = jobs[tid];
        if (jb.m > t) {
            zb_lds_st(S, 2 * tid, ext_mul_base(zb_lds(S, 2 * tid), jb.wgt));
            zb_lds_st(S, 2 * tid + 1, ext_mul_base(zb_lds(S, 2 * tid + 1), jb.wgt));
        } else {
            Ext c;
            if (jb.m == t) {   // it has just run out: F_a eq + F_b rot at its point, from the entries its last fold wrote
                const uint32_t* tab = (t & 1u) ? jb.tA : jb.tB;
                const size_t ds = (t & 1u) ? (size_t)1 << (jb.m - 1) : (jb.m >= 2 ? (size_t)1 << (jb.m - 2) : 1);
                c = ext_add(ext_mul(sc_ld(tab, 0), sc_ld(tab, ds)), ext_mul(sc_ld(tab, 2 * ds), sc_ld(tab, 3 * ds)));
                c = ext_mul_base(c, jb.wgt);
            } else {
                c = sc_ld(a.state, tid);
            }
            c = ext_mul_base(c, to_monty((P + 1) / 2));
            sc_st(a.state, tid, c);
            zb_lds_st(S, 2 * tid, c), zb_lds_st(S, 2 * tid + 1, c);
        }
    }
    zk_syncthreads();
    if (wave == 0) zb_tr_step(tr, lane, n_jobs, S, 8, 8, a.proof + 8 * (size_t)t, a.r + 4 * t, s_r);
}

// one column of a reducing AIR: u = sum_i col[i] E[i], canonical, to out[out_at ..]
struct ZbCol {
    const uint32_t* col;
    const uint32_t* E;
    uint32_t m, out_at;
};
__global__ __launch_bounds__(256) void k_zb_dot(const ZbCol* __restrict__ cols, uint32_t* __restrict__ out) {
    __shared__ uint32_t s[4];
    const ZbCol c = cols[blockIdx.x];
    const size_t n = (size_t)1 << c.m;
    Ext acc[1] = {ext_zero()};
    for (size_t i = threadIdx.x; i < n; i += 256) acc[0] = ext_add(acc[0], ext_mul_base(sc_ld(c.E, i), c.col[i]));
    sc_block_sum(acc, s, 1);
    zk_syncthreads();
    if (threadIdx.x < 4) out[c.out_at + threadIdx.x] = from_monty(s[threadIdx.x]);
}

}  // namespace zk
