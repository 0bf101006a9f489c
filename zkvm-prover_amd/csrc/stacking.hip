// stacking.hip -- the stacked WHIR commitment: base-field columns of mixed heights laid end to end in one matrix of height 2^l,
// committed once with WHIR, and every column's claim at a point of its own dimension reduced to one WHIR opening by a sum-check of
// l rounds.  Protocol, limits and measurements: docs/stacking.md.  The independent model is tests/stacking_model.py.
//
// Device side: a gather of the caller's columns into the long vector S (the commitment owns it); per opening, the eq tables of the
// points (k_whir_weight), every column's value in one segmented pass over S plus one reduce launch, and the sum-check on S W, whose
// weight table W(off_j + i) = alpha^j eq(z_p(j), i) is read on the fly (column of an entry found through the height classes) until the
// second round's fold writes it as an ordinary extension table.  The rounds are the sum-check core's (sumcheck_dev.hpp).
#include <algorithm>
#include <vector>

#include "host_challenger.hpp"
#include "sumcheck_dev.hpp"

namespace zk {

constexpr unsigned STACK_MAX_RUNS = 33;                // heights 2^0 .. 2^32
constexpr unsigned STACK_MAX_LOG_H = 32;
constexpr unsigned STACK_VLT = 4;                      // entries per thread of the values pass: 2^4
constexpr unsigned STACK_VLCH = STACK_VLT + 8;         // one values workgroup covers 2^12 entries of the long vector
constexpr size_t STACK_VCH = (size_t)1 << STACK_VLCH;

// the height classes of the sorted layout: run q holds the sorted columns first[q] .. of 2^logh[q] entries each, from long-vector entry
// start[q]; start[n] = T, the end of the columns
struct StackRuns {
    uint64_t start[STACK_MAX_RUNS + 1];
    uint32_t logh[STACK_MAX_RUNS];
    uint32_t first[STACK_MAX_RUNS];
    uint32_t n;
};

struct StackPos {
    unsigned s, lh;   // sorted column, its log height
    size_t i;         // entry within the column
};
// the column of long-vector entry e < T: a binary search over the runs
__device__ __forceinline__ StackPos stack_find(const StackRuns& R, size_t e) {
    unsigned lo = 0, hi = R.n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (R.start[mid] <= e) lo = mid;
        else hi = mid;
    }
    const size_t local = e - R.start[lo];
    const unsigned lh = R.logh[lo];
    return StackPos{R.first[lo] + (unsigned)(local >> lh), lh, local & (((size_t)1 << lh) - 1)};
}

// per caller column j (device): its offset in the long vector, its sorted position and log height
struct StackCol {
    uint64_t off;
    uint32_t s, lh;
};

// the two tables of the first rounds: 0 = S as extension elements, 1 = W(e) = coef[s] E[eoff[s] + i] (0 from T on)
struct StackSrc {
    StackRuns runs;
    const uint32_t* S;      // n_stack 2^l Montgomery words
    const uint32_t* E;      // the eq tables, end to end
    const uint64_t* eoff;   // sorted column -> first entry of its point's eq table
    const uint32_t* coef;   // sorted column -> alpha^j (extension)
    __device__ __forceinline__ Ext operator()(unsigned t, size_t e) const {
        if (t == 0) return ext_from_base(S[e]);
        if (e >= runs.start[runs.n]) return ext_zero();
        const StackPos p = stack_find(runs, e);
        return ext_mul(sc_ld(coef, p.s), sc_ld(E, eoff[p.s] + p.i));
    }
};

// the caller's columns (src: sorted column -> device pointer) into the long vector out (N words), zero from T on
__global__ __launch_bounds__(256) void k_stack_gather(StackRuns runs, const uint32_t* const* __restrict__ src, size_t N, uint32_t* __restrict__ out) {
    const size_t T = runs.start[runs.n];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (size_t)gridDim.x * 256) {
        uint32_t v = 0;
        if (e < T) {
            const StackPos p = stack_find(runs, e);
            v = src[p.s][p.i];
        }
        out[e] = v;
    }
}

// sum_i col_s[i] E_s[i] for every column, segmented: workgroup b takes entries [b 2^12, (b + 1) 2^12), 16 consecutive per thread.
// Columns are aligned to their own height, so a thread's 16 entries are one column of >= 16 entries, or whole columns of < 16, which
// the thread sums and stores itself (slot n_chunks + s).  The longer columns add up over aligned power-of-two runs of threads in LDS;
// a column of >= 2^12 entries leaves one partial per workgroup (slot b), a shorter one its sum (slot n_chunks + s).
__global__ __launch_bounds__(256) void k_stack_values(StackRuns runs, const uint32_t* __restrict__ S, const uint32_t* __restrict__ E,
                                                      const uint64_t* __restrict__ eoff, size_t n_chunks, uint32_t* __restrict__ partial) {
    __shared__ uint4 red[256];
    const unsigned tid = threadIdx.x;
    const size_t T = runs.start[runs.n], e0 = (size_t)blockIdx.x * STACK_VCH + ((size_t)tid << STACK_VLT);
    Ext acc = ext_zero();
    unsigned seg = 1, s = 0, lh = 0;   // threads of this thread's column (1: nothing for the tree)
    for (unsigned k = 0; k < (1u << STACK_VLT) && e0 + k < T; k++) {
        const StackPos p = stack_find(runs, e0 + k);
        acc = ext_add(acc, ext_mul_base(sc_ld(E, eoff[p.s] + p.i), S[e0 + k]));
        s = p.s, lh = p.lh;
        if (lh < STACK_VLT) {
            if (p.i + 1 == ((size_t)1 << lh)) sc_st(partial, n_chunks + s, acc), acc = ext_zero();
        } else {
            seg = 1u << ((lh < STACK_VLCH ? lh : STACK_VLCH) - STACK_VLT);
        }
    }
    red[tid] = ext_pack(acc);
    for (unsigned d = 1; d < 256; d <<= 1) {
        zk_syncthreads();
        if ((tid & (2 * d - 1)) == 0 && seg >= 2 * d) red[tid] = ext_pack(ext_add(ext_unpack(red[tid]), ext_unpack(red[tid + d])));
    }
    zk_syncthreads();
    if (seg > 1 || lh >= STACK_VLT)
        if ((tid & (seg - 1)) == 0) sc_st(partial, lh >= STACK_VLCH ? (size_t)blockIdx.x : n_chunks + s, ext_unpack(red[tid]));
}

// workgroup j: column j's value (caller order) from its partials, canonical, to out[4 j ..]
__global__ __launch_bounds__(256) void k_stack_reduce(const StackCol* __restrict__ cols, const uint32_t* __restrict__ partial, size_t n_chunks,
                                                      uint32_t* __restrict__ out) {
    __shared__ uint32_t red[4][4];
    const unsigned j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const StackCol c = cols[j];
    Ext acc = ext_zero();
    if (c.lh >= STACK_VLCH) {
        const size_t b0 = c.off >> STACK_VLCH, nb = (size_t)1 << (c.lh - STACK_VLCH);
        for (size_t b = tid; b < nb; b += 256) acc = ext_add(acc, sc_ld(partial, b0 + b));
    } else if (tid == 0) {
        acc = sc_ld(partial, n_chunks + c.s);
    }
    for (int q = 0; q < 4; q++) {
        const uint32_t x = sc_wave_sum(acc.c[q]);
        if (lane == 0) red[wave][q] = x;
    }
    zk_syncthreads();
    if (tid < 4) out[4 * (size_t)j + tid] = from_monty(madd(madd(red[0][tid], red[1][tid]), madd(red[2][tid], red[3][tid])));
}

// coef[s(j)] = alpha^j
__global__ __launch_bounds__(256) void k_stack_coef(const StackCol* __restrict__ cols, unsigned n_cols, const uint32_t* __restrict__ alpha,
                                                    uint32_t* __restrict__ coef) {
    const Ext a = sc_ld(alpha, 0);
    for (unsigned j = threadIdx.x; j < n_cols; j += 256) sc_st(coef, cols[j].s, ext_pow(a, j));
}

// the last `rounds` rounds in ONE workgroup: the two tables src reads, n <= SC_T entries after folding with r_prev (if given), in LDS
template <class Src>
__global__ __launch_bounds__(SC_SW) void k_stack_small(DevTranscript* tr, Src src, const uint32_t* __restrict__ r_prev, unsigned n,
                                                       unsigned rounds, uint32_t* __restrict__ proof_out, uint32_t* __restrict__ r_out) {
    __shared__ uint4 X4[2 * SC_T];   // S, then W
    __shared__ uint32_t s_r[4];
    uint32_t* X = reinterpret_cast<uint32_t*>(X4);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Ext r = r_prev ? sc_ld(r_prev, 0) : ext_zero();
    for (unsigned i = tid; i < n; i += SC_SW)
#pragma unroll
        for (unsigned t = 0; t < 2; t++) sc_st(X, t * SC_T + i, r_prev ? sc_fold(src(t, 2 * i), src(t, 2 * i + 1), r) : src(t, i));
    CoopConsts cc;
    TrRegs R{};
    if (wave == 0) cc = coop_load_consts(lane & 15u), R = tr_load(tr, lane);
    zk_syncthreads();
    for (unsigned t = 0; t < rounds; t++, n >>= 1) sc_small_round(WhirRound{}, X, SC_T, n, R, cc, proof_out + 8 * t, r_out + 4 * t, s_r);
    if (wave == 0) tr_store(tr, R, lane);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
namespace {
unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(SC_NB, (n + 255) / 256)); }

// the public layout of a shape
struct StackLayout {
    bool ok = false;
    size_t n_stack = 0;
    uint64_t T = 0;
    std::vector<unsigned> order;   // sorted position -> caller index
    std::vector<unsigned> pos;     // caller index -> sorted position
    std::vector<uint64_t> off;     // caller index -> offset in the long vector
    StackRuns runs{};
};
StackLayout stack_layout(const zkhip_whir_params* prm, const unsigned* lh, size_t n_cols, unsigned l) {
    StackLayout L;
    if (!prm || !lh || n_cols < 1 || n_cols > ZKHIP_STACK_MAX_COLS || l < prm->fold_log || l > ZKHIP_WHIR_MAX_LOG_N) return L;
    for (size_t j = 0; j < n_cols; j++)
        if (lh[j] > STACK_MAX_LOG_H) return L;
    L.order.resize(n_cols);
    for (size_t j = 0; j < n_cols; j++) L.order[j] = (unsigned)j;
    std::stable_sort(L.order.begin(), L.order.end(), [&](unsigned a, unsigned b) { return lh[a] > lh[b]; });
    L.pos.resize(n_cols), L.off.resize(n_cols);
    uint64_t o = 0;
    for (size_t s = 0; s < n_cols; s++) {
        const unsigned j = L.order[s];
        L.pos[j] = (unsigned)s, L.off[j] = o;
        if (s == 0 || lh[j] != L.runs.logh[L.runs.n - 1]) {
            L.runs.start[L.runs.n] = o, L.runs.logh[L.runs.n] = lh[j], L.runs.first[L.runs.n] = (unsigned)s;
            L.runs.n++;
        }
        o += (uint64_t)1 << lh[j];
    }
    L.T = o, L.runs.start[L.runs.n] = o;
    L.n_stack = (size_t)((o + ((uint64_t)1 << l) - 1) >> l);
    if (L.n_stack > ZKHIP_WHIR_MAX_COLS || !zkhip_whir_proof_words(prm, l, L.n_stack)) return L;
    L.ok = true;
    return L;
}

// the points and the columns' claims of an opening: checks every shape rule; eofs[p] = first entry of point p's eq table (used points)
struct StackClaims {
    bool ok = false;
    std::vector<size_t> pofs;       // point p's first word in `points`
    std::vector<uint64_t> eofs;     // point p's eq table (entries), ~0 when no column names it
    uint64_t e_total = 0;
};
StackClaims stack_claims(const std::vector<unsigned>& heights, const uint32_t* points, const unsigned* dims, size_t n_points,
                         const unsigned* col_point) {
    StackClaims C;
    if (!points || !dims || !col_point || n_points < 1 || n_points > ZKHIP_STACK_MAX_POINTS) return C;
    C.pofs.resize(n_points), C.eofs.assign(n_points, ~(uint64_t)0);
    size_t w = 0;
    for (size_t p = 0; p < n_points; p++) {
        if (dims[p] > STACK_MAX_LOG_H) return C;
        C.pofs[p] = w, w += 4 * (size_t)dims[p];
    }
    for (size_t i = 0; i < w; i++)
        if (points[i] >= P) return C;
    for (size_t j = 0; j < heights.size(); j++) {
        const unsigned p = col_point[j];
        if (p >= n_points || dims[p] != heights[j]) return C;
        if (C.eofs[p] == ~(uint64_t)0) C.eofs[p] = C.e_total, C.e_total += (uint64_t)1 << dims[p];
    }
    C.ok = true;
    return C;
}
}  // namespace

}  // namespace zk

struct zkhip_stack_commitment {
    zkhip_whir_params params{};
    unsigned l = 0;
    std::vector<unsigned> heights;   // caller order
    zk::StackLayout lay;
    uint32_t* d_mat = nullptr;       // the long vector: n_stack stacked columns of 2^l Montgomery words
    zkhip_whir_commitment* whir = nullptr;
    uint32_t root[8] = {};
};

namespace zk {

void stack_destroy(zkhip_ctx* ctx, zkhip_stack_commitment* sc) {
    if (!sc) return;
    whir_destroy(ctx, sc->whir);   // synchronises
    if (sc->d_mat) (void)hipFree(sc->d_mat);
    delete sc;
}

int stack_commit(zkhip_ctx* ctx, const zkhip_whir_params* prm, const uint32_t* const* d_cols, const unsigned* lh, size_t n_cols, unsigned l,
                 zkhip_stack_commitment** out, uint32_t* root_out) {
    StackLayout lay = stack_layout(prm, lh, n_cols, l);
    if (!lay.ok) return set_error(ctx, ZKHIP_ERR_INVALID, "stack: the shape does not fit the limits");
    for (size_t j = 0; j < n_cols; j++)
        if (!d_cols[j]) return set_error(ctx, ZKHIP_ERR_INVALID, "stack: null column");
    zkhip_stack_commitment* sc = new zkhip_stack_commitment();
    sc->params = *prm, sc->l = l, sc->heights.assign(lh, lh + n_cols), sc->lay = lay;
    const size_t N = lay.n_stack << l;
    int rc = ZKHIP_OK;
    {
        DevBufs B(ctx);
        uint32_t* d_src = B.get(2 * n_cols);
        if (!d_src || hipMalloc(&sc->d_mat, N * 4) != hipSuccess) rc = set_error(ctx, ZKHIP_ERR_NOMEM, "stack: commitment buffers");
        std::vector<const uint32_t*> src(n_cols);
        for (size_t s = 0; s < n_cols; s++) src[s] = d_cols[lay.order[s]];
        if (rc == ZKHIP_OK) rc = zkhip_h2d(ctx, d_src, src.data(), n_cols * sizeof(void*));
        if (rc == ZKHIP_OK) {
            KernelScope ks(ctx, "stack_gather");
            hipLaunchKernelGGL(k_stack_gather, dim3(grid_of(N)), dim3(256), 0, ctx->stream, lay.runs, (const uint32_t* const*)d_src, N, sc->d_mat);
            if (hipGetLastError() != hipSuccess) rc = set_error(ctx, ZKHIP_ERR_HIP, "stack: gather launch");
        }
        if (rc == ZKHIP_OK) {
            WhirCols cols{};
            for (size_t c = 0; c < lay.n_stack; c++) cols.p[c] = sc->d_mat + (c << l), cols.es[c] = 1;
            rc = whir_commit_cols(ctx, prm, cols, lay.n_stack, l, &sc->whir, sc->root);   // synchronises
        }
    }
    if (rc != ZKHIP_OK) {
        stack_destroy(ctx, sc);
        return rc;
    }
    if (root_out) memcpy(root_out, sc->root, 32);
    *out = sc;
    return ZKHIP_OK;
}

int stack_open(zkhip_ctx* ctx, zkhip_stack_commitment* sc, DevTranscript* d_t, const uint32_t* points, const unsigned* dims, size_t n_points,
               const unsigned* col_point, uint32_t* values_out, uint32_t* proof_out, size_t cap) {
    const StackLayout& lay = sc->lay;
    const size_t n_cols = sc->heights.size(), n_stack = lay.n_stack;
    const unsigned l = sc->l;
    const StackClaims C = stack_claims(sc->heights, points, dims, n_points, col_point);
    if (!C.ok) return set_error(ctx, ZKHIP_ERR_INVALID, "stack: points do not fit the columns");
    const size_t head = 4 * n_cols + 8 * (size_t)l, total = head + zkhip_whir_proof_words(&sc->params, l, n_stack);
    if (cap < total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, "stack: proof buffer too small");
    const size_t N = n_stack << l, n_chunks = (size_t)((lay.T + STACK_VCH - 1) >> STACK_VLCH);
    // one upload: [points (Montgomery) | StackCol per caller column | eoff per sorted column]
    const size_t pw = C.pofs.back() + 4 * (size_t)dims[n_points - 1], pw4 = (pw + 3) & ~(size_t)3;
    std::vector<uint32_t> up(pw4 + 4 * n_cols + 2 * n_cols);
    for (size_t i = 0; i < pw; i++) up[i] = to_monty(points[i]);
    StackCol* hc = reinterpret_cast<StackCol*>(up.data() + pw4);
    uint64_t* he = reinterpret_cast<uint64_t*>(up.data() + pw4 + 4 * n_cols);
    for (size_t j = 0; j < n_cols; j++) {
        hc[j] = StackCol{lay.off[j], lay.pos[j], sc->heights[j]};
        he[lay.pos[j]] = C.eofs[col_point[j]];
    }
    DevBufs B(ctx);
    uint32_t *d_up = B.get(up.size()), *E = B.get(4 * C.e_total), *vpart = B.get(4 * (n_chunks + n_cols)), *partial = B.get(8 * (size_t)SC_NB);
    uint32_t *coef = B.get(4 * n_cols), *dP = B.get(head + 4 * (size_t)l + 4), *fA = B.get(2 * N), *wA = B.get(2 * N), *fB = B.get(N), *wB = B.get(N);
    if (!d_up || !E || !vpart || !partial || !coef || !dP || !fA || !wA || !fB || !wB) return set_error(ctx, ZKHIP_ERR_NOMEM, "stack: opening buffers");
    uint32_t *rs = dP + head, *alpha = rs + 4 * (size_t)l;   // the challenges follow the proof words
    const StackCol* d_cols = reinterpret_cast<const StackCol*>(d_up + pw4);
    const uint64_t* d_eoff = reinterpret_cast<const uint64_t*>(d_up + pw4 + 4 * n_cols);
    hipStream_t st = ctx->stream;
    ZK_TRY(zkhip_h2d(ctx, d_up, up.data(), up.size() * 4));
    for (size_t p = 0; p < n_points; p++)
        if (C.eofs[p] != ~(uint64_t)0) {
            KernelScope ks(ctx, "stack_eq");
            whir_eq_launch(st, E + 4 * C.eofs[p], dims[p], d_up + C.pofs[p]);
        }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    {
        KernelScope ks(ctx, "stack_values");
        hipLaunchKernelGGL(k_stack_values, dim3((unsigned)n_chunks), dim3(256), 0, st, lay.runs, (const uint32_t*)sc->d_mat, (const uint32_t*)E,
                           d_eoff, n_chunks, vpart);
    }
    {
        KernelScope ks(ctx, "stack_values");
        hipLaunchKernelGGL(k_stack_reduce, dim3((unsigned)n_cols), dim3(256), 0, st, d_cols, (const uint32_t*)vpart, n_chunks, dP);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    ZK_TRY(transcript_observe(ctx, d_t, dP, (uint32_t)(4 * n_cols), true));
    ZK_TRY(transcript_sample(ctx, d_t, alpha, nullptr, 4));
    {
        KernelScope ks(ctx, "stack_coef");
        hipLaunchKernelGGL(k_stack_coef, dim3(1), dim3(256), 0, st, d_cols, (unsigned)n_cols, (const uint32_t*)alpha, coef);
    }
    ZK_HIP_CHECK(ctx, hipGetLastError());
    // the sum-check: rounds 0 and 1 read S and W through StackSrc, round 1's fold writes them as extension tables (fA, wA)
    const StackSrc ss{lay.runs, sc->d_mat, E, d_eoff, coef};
    uint32_t *f = nullptr, *w = nullptr;
    const uint32_t* pending = nullptr;
    size_t sz = N;   // entries after the pending fold
    unsigned t = 0;
    for (; t < l && sz > SC_T; t++, sz >>= 1) {
        uint32_t *fo = f == fA ? fB : fA, *wo = w == wA ? wB : wA;
        {
            KernelScope ks(ctx, "stack_pass");
            if (t < 2) {
                ScPass<StackSrc, WhirRound> p{};
                p.src = ss, p.dst[0] = fA, p.dst[1] = wA, p.r = pending, p.n_pairs = sz / 2, p.partial = partial;
                hipLaunchKernelGGL(k_sc_pass, dim3(grid_of(sz / 2)), dim3(256), 0, st, p);
            } else {
                ScPass<ScTables<2>, WhirRound> p{};
                p.src.tab[0] = f, p.src.tab[1] = w, p.dst[0] = fo, p.dst[1] = wo, p.r = pending, p.n_pairs = sz / 2, p.partial = partial;
                hipLaunchKernelGGL(k_sc_pass, dim3(grid_of(sz / 2)), dim3(256), 0, st, p);
            }
        }
        {
            KernelScope ks(ctx, "stack_round_tr");
            hipLaunchKernelGGL(k_sc_round_tr<8>, dim3(1), dim3(64), 0, st, d_t, (const uint32_t*)partial, grid_of(sz / 2), dP + 4 * n_cols + 8 * t,
                               rs + 4 * t);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
        if (pending) f = fo, w = wo;
        pending = rs + 4 * t;
    }
    if (t < l) {   // the rest in one workgroup
        KernelScope ks(ctx, "stack_small");
        if (t < 2)
            hipLaunchKernelGGL(k_stack_small<StackSrc>, dim3(1), dim3(SC_SW), 0, st, d_t, ss, pending, (unsigned)sz, l - t, dP + 4 * n_cols + 8 * t,
                               rs + 4 * t);
        else
            hipLaunchKernelGGL(k_stack_small<ScTables<2>>, dim3(1), dim3(SC_SW), 0, st, d_t, ScTables<2>{{f, w}}, pending, (unsigned)sz, l - t,
                               dP + 4 * n_cols + 8 * t, rs + 4 * t);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    // the one read-back before the opening: the words so far and r
    std::vector<uint32_t> h(head + 4 * (size_t)l);
    ZK_TRY(zkhip_d2h(ctx, h.data(), dP, h.size() * 4));
    std::vector<uint32_t> r(4 * (size_t)l);
    for (size_t i = 0; i < r.size(); i++) r[i] = from_monty(h[head + i]);
    ZK_TRY(whir_open_device(ctx, sc->whir, d_t, r.data(), nullptr, proof_out + head, cap - head));
    memcpy(proof_out, h.data(), head * 4);
    if (values_out) memcpy(values_out, h.data(), 16 * n_cols);
    return ZKHIP_OK;
}

int stack_verify_host(HostChallenger& ch, const zkhip_whir_params* prm, const uint32_t* root, const unsigned* lh, size_t n_cols, unsigned l,
                      const uint32_t* points, const unsigned* dims, size_t n_points, const unsigned* col_point, const uint32_t* proof, size_t words) {
    const StackLayout lay = stack_layout(prm, lh, n_cols, l);
    if (!lay.ok) return ZKHIP_ERR_VERIFY;
    const std::vector<unsigned> heights(lh, lh + n_cols);
    const StackClaims C = stack_claims(heights, points, dims, n_points, col_point);
    if (!C.ok) return ZKHIP_ERR_VERIFY;
    const size_t head = 4 * n_cols + 8 * (size_t)l;
    if (words != head + zkhip_whir_proof_words(prm, l, lay.n_stack)) return ZKHIP_ERR_VERIFY;
    for (size_t i = 0; i < head; i++)
        if (proof[i] >= P) return ZKHIP_ERR_VERIFY;
    ch.observe_canon(proof, 4 * n_cols);
    const Ext alpha = ch.sample_ext();
    std::vector<Ext> apow(n_cols);
    Ext claim = ext_zero(), a = ext_one();
    for (size_t j = 0; j < n_cols; j++) apow[j] = a, claim = ext_add(claim, ext_mul(a, ext_from_canon(proof + 4 * j))), a = ext_mul(a, alpha);
    std::vector<Ext> r(l);
    std::vector<uint32_t> rc(4 * (size_t)l);
    for (unsigned t = 0; t < l; t++) {
        const uint32_t* sw = proof + 4 * n_cols + 8 * t;
        const Ext s0 = ext_from_canon(sw), s2 = ext_from_canon(sw + 4);
        ch.observe_canon(sw, 8);
        r[t] = ch.sample_ext();
        const Ext sv[3] = {s0, ext_sub(claim, s0), s2};
        claim = poly_at(sv, 2, r[t]);
        ext_to_canon(rc.data() + 4 * t, r[t]);
    }
    std::vector<uint32_t> u(4 * lay.n_stack);
    ZK_TRY(whir_verify_host(ch, prm, root, l, lay.n_stack, rc.data(), proof + head, words - head, u.data()));
    // W_c~(r) from the public layout: the pieces of every column on stacked column c
    std::vector<Ext> W(lay.n_stack, ext_zero());
    const Ext one = ext_one();
    for (size_t j = 0; j < n_cols; j++) {
        const unsigned m = lh[j];
        std::vector<Ext> z(m);
        for (unsigned i = 0; i < m; i++) z[i] = ext_from_canon(points + C.pofs[col_point[j]] + 4 * i);
        const size_t c0 = (size_t)(lay.off[j] >> l);
        if (m <= l) {
            Ext e = eq_eval(z.data(), r.data(), m);
            const uint64_t hb = (lay.off[j] & (((uint64_t)1 << l) - 1)) >> m;
            for (unsigned k = 0; k < l - m; k++) e = ext_mul(e, (hb >> k) & 1 ? r[m + k] : ext_sub(one, r[m + k]));
            W[c0] = ext_add(W[c0], ext_mul(apow[j], e));
        } else {
            const Ext e = ext_mul(apow[j], eq_eval(z.data(), r.data(), l));
            for (uint64_t hs = 0; hs < ((uint64_t)1 << (m - l)); hs++) {
                Ext c = e;
                for (unsigned k = 0; k < m - l; k++) c = ext_mul(c, (hs >> k) & 1 ? z[l + k] : ext_sub(one, z[l + k]));
                W[c0 + hs] = ext_add(W[c0 + hs], c);
            }
        }
    }
    Ext total = ext_zero();
    for (size_t c = 0; c < lay.n_stack; c++) total = ext_add(total, ext_mul(ext_from_canon(u.data() + 4 * c), W[c]));
    return ext_eq(total, claim) ? ZKHIP_OK : ZKHIP_ERR_VERIFY;
}

}  // namespace zk

using namespace zk;

extern "C" {

size_t zkhip_stack_width(const zkhip_whir_params* params, const unsigned* log_heights, size_t n_cols, unsigned log_stack) {
    const StackLayout lay = stack_layout(params, log_heights, n_cols, log_stack);
    return lay.ok ? lay.n_stack : 0;
}

size_t zkhip_stack_proof_words(const zkhip_whir_params* params, const unsigned* log_heights, size_t n_cols, unsigned log_stack) {
    const StackLayout lay = stack_layout(params, log_heights, n_cols, log_stack);
    return lay.ok ? 4 * n_cols + 8 * (size_t)log_stack + zkhip_whir_proof_words(params, log_stack, lay.n_stack) : 0;
}

int zkhip_stack_commit(zkhip_ctx* ctx, const zkhip_whir_params* params, const uint32_t* const* d_cols, const unsigned* log_heights, size_t n_cols,
                       unsigned log_stack, zkhip_stack_commitment** out, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !d_cols || !log_heights || !out) return ZKHIP_ERR_INVALID;
    return stack_commit(ctx, params, d_cols, log_heights, n_cols, log_stack, out, root_out);
}

int zkhip_stack_open(zkhip_ctx* ctx, zkhip_stack_commitment* scom, zkhip_transcript* transcript, const uint32_t* points, const unsigned* point_dims,
                     size_t n_points, const unsigned* col_point, uint32_t* values_out, uint32_t* proof_out, size_t cap) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !scom || !transcript || !points || !point_dims || !col_point || !proof_out) return ZKHIP_ERR_INVALID;
    return stack_open(ctx, scom, transcript->d, points, point_dims, n_points, col_point, values_out, proof_out, cap);
}

void zkhip_stack_commitment_destroy(zkhip_ctx* ctx, zkhip_stack_commitment* scom) {
    ZK_BIND_DEVICE(ctx);
    stack_destroy(ctx, scom);
}

int zkhip_stack_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const uint32_t* root, const unsigned* log_heights,
                       size_t n_cols, unsigned log_stack, const uint32_t* points, const unsigned* point_dims, size_t n_points,
                       const unsigned* col_point, const uint32_t* values, const uint32_t* proof, size_t words) {
    if ((n_prefix && !prefix) || !values || !root || !log_heights || !points || !point_dims || !col_point || !proof) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    ZK_TRY(stack_verify_host(ch, params, root, log_heights, n_cols, log_stack, points, point_dims, n_points, col_point, proof, words));
    return memcmp(values, proof, 16 * n_cols) == 0 ? ZKHIP_OK : ZKHIP_ERR_VERIFY;
}

}  // extern "C"
