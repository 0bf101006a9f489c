// whir.hip -- WHIR, a multilinear polynomial commitment (Arnon, Chiesa, Fenzi, Yogev, "WHIR: Reed-Solomon Proximity Testing with
// Super-Fast Verification", 2024), in this library's own transcript, and the committed fractional-sum proof built on it.  Protocol,
// proof layout and measurements: docs/whir.md.  The independent model is tests/whir_model.py.
//
// Device side:
//   * commit: the zeta transform (hypercube evaluations -> monomial coefficients) through LDS, several variables per pass; the
//     existing NTT (natural in, bit-reversed out, no coset shift); a regroup into rows of one 2^k coset per column; the existing
//     Merkle commitment;
//   * open: eq(z, .) and the opened values; per sum-check round one streaming pass that folds f and w with the previous challenge and
//     evaluates s(0), s(2) (two-stage reduction), then a one-wave kernel that adds the partials, observes them and samples the
//     challenge; once a table holds <= 2^10 entries ONE workgroup runs the round's remaining sum-check rounds with the transcript
//     in-kernel; the coefficients fold by 2^k in one pass; the out-of-domain answer is a reduction; the weight update adds all of a
//     round's new eq terms in one pass.  The query indices go to the host once per round (Merkle openings take host indices).
//     The pass, the one-wave kernel and the rounds of k_whir_small are the sum-check core's (sumcheck_dev.hpp).
#include <algorithm>
#include <vector>

#include "host_challenger.hpp"
#include "sumcheck_dev.hpp"

namespace zk {

constexpr unsigned WHIR_ZT = 12;           // a zeta-transform tile holds 2^12 words of LDS

// ---- shape -----------------------------------------------------------------------------------------------------------------
struct WhirShape {
    unsigned R = 0, mf = 0;
    bool ok = false;
};
WhirShape whir_shape(const zkhip_whir_params* p, unsigned m, size_t n_cols) {
    WhirShape s;
    if (!p || m < 1 || m > ZKHIP_WHIR_MAX_LOG_N || n_cols < 1 || n_cols > ZKHIP_WHIR_MAX_COLS) return s;
    if (p->log_blowup < 1 || p->log_blowup > 3 || p->fold_log < 1 || p->fold_log > 4 || p->fold_log > m) return s;
    const unsigned R = m > p->final_log ? std::max(1u, (m - p->final_log) / p->fold_log) : 1u;
    if (R > ZKHIP_WHIR_MAX_ROUNDS) return s;
    for (unsigned i = 0; i < R; i++)
        if (p->pow_bits[i] > 30 || p->num_queries[i] < 1 || p->num_queries[i] > ZKHIP_WHIR_MAX_QUERIES) return s;
    s.R = R, s.mf = m - p->fold_log * R, s.ok = true;
    return s;
}
// offsets of an opening proof: values, then per round [sum-check (8 k) | root (8) + OOD (4), or final (4 2^mf) | pow (1) | queries]
struct WhirLayout {
    size_t sc[ZKHIP_WHIR_MAX_ROUNDS], mid[ZKHIP_WHIR_MAX_ROUNDS], pow[ZKHIP_WHIR_MAX_ROUNDS], q[ZKHIP_WHIR_MAX_ROUNDS];
    size_t qw[ZKHIP_WHIR_MAX_ROUNDS];   // words of one opening in round i
    size_t total = 0;
};
WhirLayout whir_layout(const zkhip_whir_params* p, unsigned m, size_t n_cols, const WhirShape& s) {
    WhirLayout L{};
    const unsigned k = p->fold_log;
    size_t off = 4 * n_cols;
    unsigned n = m + p->log_blowup;
    for (unsigned i = 0; i < s.R; i++) {
        const bool last = i + 1 == s.R;
        L.sc[i] = off, off += 8 * k;
        L.mid[i] = off, off += last ? (size_t)4 << s.mf : 12;
        L.pow[i] = off, off += 1;
        L.qw[i] = ((i == 0 ? n_cols : 4) << k) + 8 * (size_t)(n - k);
        L.q[i] = off, off += p->num_queries[i] * L.qw[i];
        n--;
    }
    L.total = off;
    return L;
}

// ---- commit ------------------------------------------------------------------------------------------------------------------
// zeta transform of variables s .. s+v-1 of every column (grid.y = column), through LDS: a tile holds 2^v values of those variables
// times 2^lw consecutive low indices (lw <= s).  src (first pass only, s = 0): the caller's columns; else in place on dst.
__global__ __launch_bounds__(256) void k_whir_zeta(WhirCols src, int from_src, uint32_t* __restrict__ dst, size_t dst_stride, unsigned m,
                                                   unsigned s, unsigned v, unsigned lw) {
    __shared__ uint32_t t[1u << WHIR_ZT];
    const unsigned c = blockIdx.y, tid = threadIdx.x, T = 1u << (v + lw);
    const size_t tile = blockIdx.x, lo_blocks = (size_t)1 << (s - lw);
    const size_t hi = tile / lo_blocks, lob = tile % lo_blocks;
    uint32_t* col = dst + c * dst_stride;
    auto gidx = [&](unsigned e) {   // LDS entry e = tv << lw | lo
        const size_t tv = e >> lw, lo = e & ((1u << lw) - 1u);
        return (hi << (s + v)) + (tv << s) + (lob << lw) + lo;
    };
    for (unsigned e = tid; e < T; e += 256) {
        const size_t g = gidx(e);
        t[e] = from_src ? src.p[c][g * src.es[c]] : col[g];
    }
    zk_syncthreads();
    for (unsigned j = 0; j < v; j++) {
        const unsigned bit = 1u << (lw + j);
        for (unsigned e = tid; e < T / 2; e += 256) {   // pair e: insert a 0 at bit (lw + j)
            const unsigned e0 = ((e >> (lw + j)) << (lw + j + 1)) | (e & (bit - 1u));
            t[e0 | bit] = msub(t[e0 | bit], t[e0]);
        }
        zk_syncthreads();
    }
    for (unsigned e = tid; e < T; e += 256) col[gidx(e)] = t[e];
}

// codeword rows (bit-reversed, n_src columns of 2^log_n, cw_stride apart) -> the committed matrix (column-major, 2^(log_n - k) rows):
// base: column c * 2^k + t; ext (n_src = 4 coordinates): column t * 4 + c; row r holds codeword position r 2^k + t
__global__ __launch_bounds__(256) void k_whir_regroup(const uint32_t* __restrict__ cw, size_t cw_stride, unsigned n_src, unsigned log_n,
                                                      unsigned k, int ext, uint32_t* __restrict__ out) {
    const size_t n = (size_t)1 << log_n, H = n >> k, total = n * n_src;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t c = e >> log_n, pos = e & (n - 1), r = pos >> k, t = pos & ((1u << k) - 1u);
        const size_t oc = ext ? t * 4 + c : (c << k) + t;
        out[oc * H + r] = cw[c * cw_stride + pos];
    }
}

// ---- open --------------------------------------------------------------------------------------------------------------------
// w[b] (+)= sum_t coef_t eq(p_t, b) over 2^mv entries; coef_t = gamma^(t+1) (1 when gamma is null); p_t = pts[t * mv ..] (extension).
// A workgroup's 256 entries share their high bits: the high factor of every point is made once per workgroup, in LDS.
__global__ __launch_bounds__(256) void k_whir_weight(uint32_t* __restrict__ w, unsigned mv, const uint32_t* __restrict__ pts, unsigned np,
                                                     const uint32_t* __restrict__ gamma, int assign) {
    __shared__ uint4 hic[256];
    const unsigned tid = threadIdx.x, lb = mv < 8 ? mv : 8;
    const size_t b = (size_t)blockIdx.x * 256 + tid, n = (size_t)1 << mv;
    const size_t bhi = ((size_t)blockIdx.x * 256) >> 8;   // entries >> 8 (the same for the whole workgroup when mv >= 8)
    Ext acc = ext_zero();
    const Ext one = ext_one();
    for (unsigned t0 = 0; t0 < np; t0 += 256) {
        const unsigned t = t0 + tid;
        if (t < np) {
            Ext c = gamma ? ext_pow(sc_ld(gamma, 0), (uint64_t)t + 1) : one;
            for (unsigned j = lb; j < mv; j++) {
                const Ext pj = sc_ld(pts, (size_t)t * mv + j);
                c = ext_mul(c, ((bhi >> (j - 8)) & 1) ? pj : ext_sub(one, pj));
            }
            hic[tid] = ext_pack(c);
        }
        zk_syncthreads();
        const unsigned nt = np - t0 < 256 ? np - t0 : 256;
        for (unsigned u = 0; u < nt; u++) {
            Ext e = ext_unpack(hic[u]);
            for (unsigned j = 0; j < lb; j++) {
                const Ext pj = sc_ld(pts, (size_t)(t0 + u) * mv + j);
                e = ext_mul(e, ((b >> j) & 1) ? pj : ext_sub(one, pj));
            }
            acc = ext_add(acc, e);
        }
        zk_syncthreads();
    }
    if (b < n) sc_st(w, b, assign ? acc : ext_add(sc_ld(w, b), acc));
}

// partial sums of sum_i col_c[i] w[i] for every column (slot c * 4 + q of the partials)
__global__ __launch_bounds__(256) void k_whir_dot(WhirCols src, unsigned n_cols, const uint32_t* __restrict__ w, size_t n,
                                                  uint32_t* __restrict__ partial) {
    for (unsigned c = 0; c < n_cols; c++) {
        Ext acc[1] = {ext_zero()};
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
            acc[0] = ext_add(acc[0], ext_mul_base(sc_ld(w, i), src.p[c][i * src.es[c]]));
        sc_block_sum(acc, partial + (size_t)c * 4 * SC_NB + blockIdx.x);
        zk_syncthreads();
    }
}

// the partials of `nvals` extension values (nb workgroups each) -> nvals canonical extension values in the proof (one workgroup)
__global__ __launch_bounds__(256) void k_whir_reduce(const uint32_t* __restrict__ partial, unsigned nb, unsigned nvals,
                                                     uint32_t* __restrict__ out) {
    for (unsigned j = threadIdx.x; j < 4 * nvals; j += 256) {
        uint32_t s = 0;
        for (unsigned b = 0; b < nb; b++) s = madd(s, partial[(size_t)j * SC_NB + b]);
        out[j] = from_monty(s);
    }
}

// out[i] = sum_c alpha^c col_c[i] (extension)
__global__ __launch_bounds__(256) void k_whir_combine(WhirCols src, unsigned n_cols, size_t n, const uint32_t* __restrict__ alpha,
                                                      uint32_t* __restrict__ out) {
    const Ext a = sc_ld(alpha, 0);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        Ext acc = ext_zero(), ap = ext_one();
        for (unsigned c = 0; c < n_cols; c++) {
            acc = ext_add(acc, ext_mul_base(ap, src.p[c][i * src.es[c]]));
            ap = ext_mul(ap, a);
        }
        sc_st(out, i, acc);
    }
}

using WhirPass = ScPass<ScTables<2>, WhirRound>;

// The rest of a round's sum-check in ONE workgroup, tables of n <= SC_T entries (after folding with r_prev, if given) in LDS:
// `rounds` rounds, each a reduction, the transcript step on wave 0 and a fold.  fo / wo (may be null): the folded tables at the end.
__global__ __launch_bounds__(SC_SW) void k_whir_small(DevTranscript* tr, const uint32_t* __restrict__ f, const uint32_t* __restrict__ w,
                                                       const uint32_t* __restrict__ r_prev, unsigned n, unsigned rounds,
                                                       uint32_t* __restrict__ proof_out, uint32_t* __restrict__ r_out,
                                                       uint32_t* __restrict__ fo, uint32_t* __restrict__ wo) {
    __shared__ uint4 X4[2 * SC_T];   // f, then w
    __shared__ uint32_t s_r[4];
    uint32_t* X = reinterpret_cast<uint32_t*>(X4);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    {
        const Ext r = r_prev ? sc_ld(r_prev, 0) : ext_zero();
        for (unsigned i = tid; i < n; i += SC_SW) {
            if (r_prev) {
                sc_st(X, i, sc_fold(sc_ld(f, 2 * i), sc_ld(f, 2 * i + 1), r));
                sc_st(X, SC_T + i, sc_fold(sc_ld(w, 2 * i), sc_ld(w, 2 * i + 1), r));
            } else {
                sc_st(X, i, sc_ld(f, i)), sc_st(X, SC_T + i, sc_ld(w, i));
            }
        }
    }
    CoopConsts cc;
    TrRegs R{};
    if (wave == 0) cc = coop_load_consts(lane & 15u), R = tr_load(tr, lane);
    zk_syncthreads();
    for (unsigned t = 0; t < rounds; t++, n >>= 1) sc_small_round(WhirRound{}, X, SC_T, n, R, cc, proof_out + 8 * t, r_out + 4 * t, s_r);
    if (wave == 0) tr_store(tr, R, lane);
    if (fo)
        for (unsigned i = tid; i < n; i += SC_SW) sc_st(fo, i, sc_ld(X, i)), sc_st(wo, i, sc_ld(X, SC_T + i));
}

// coefficients folded by 2^k in one pass: out[y] = the k binary folds c_even + r_j c_odd of c[y 2^k ..]; cols (may be null): also
// the four coordinates as columns, col_stride apart (what the next codeword's NTT reads)
__global__ __launch_bounds__(256) void k_whir_cfold(const uint32_t* __restrict__ c, size_t n_out, unsigned k, const uint32_t* __restrict__ rs,
                                                    uint32_t* __restrict__ out, uint32_t* __restrict__ cols, size_t col_stride) {
    for (size_t y = (size_t)blockIdx.x * 256 + threadIdx.x; y < n_out; y += (size_t)gridDim.x * 256) {
        Ext v[16];
        const unsigned s = 1u << k;
        for (unsigned t = 0; t < s; t++) v[t] = sc_ld(c, (y << k) + t);
        for (unsigned j = 0; j < k; j++) {
            const Ext r = sc_ld(rs, j);
            for (unsigned t = 0; t < (s >> (j + 1)); t++) v[t] = ext_add(v[2 * t], ext_mul(r, v[2 * t + 1]));
        }
        sc_st(out, y, v[0]);
        if (cols)
            for (int q = 0; q < 4; q++) cols[q * col_stride + y] = v[0].c[q];
    }
}

// partial sums of sum_i c_i zeta^i: thread g takes the `per` consecutive coefficients from g * per and raises zeta to g * per itself
__global__ __launch_bounds__(256) void k_whir_ood(const uint32_t* __restrict__ c, size_t n, size_t per, const uint32_t* __restrict__ zeta_p,
                                                  uint32_t* __restrict__ partial) {
    const Ext z = sc_ld(zeta_p, 0);
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, i0 = g * per;
    Ext acc[1] = {ext_zero()};
    if (i0 < n) {
        Ext x = ext_pow(z, i0);
        const size_t i1 = i0 + per < n ? i0 + per : n;
        for (size_t i = i0; i < i1; i++) {
            acc[0] = ext_add(acc[0], ext_mul(sc_ld(c, i), x));
            x = ext_mul(x, z);
        }
    }
    sc_block_sum(acc, partial + blockIdx.x);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
void whir_eq_launch(hipStream_t st, uint32_t* w, unsigned mv, const uint32_t* pts) {
    hipLaunchKernelGGL(k_whir_weight, dim3((unsigned)((((size_t)1 << mv) + 255) / 256)), dim3(256), 0, st, w, mv, pts, 1u,
                       (const uint32_t*)nullptr, 1);
}

namespace {
unsigned grid_of(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(SC_NB, (n + 255) / 256)); }
std::vector<Ext> pow_point(Ext x, unsigned n) {
    std::vector<Ext> out(n);
    for (unsigned j = 0; j < n; j++) out[j] = x, x = ext_mul(x, x);
    return out;
}
}  // namespace

}  // namespace zk

struct zkhip_whir_commitment {
    zkhip_whir_params params{};
    unsigned m = 0;
    size_t n_cols = 0;
    zk::WhirCols cols{};          // the caller's evaluation columns
    uint32_t* d_coeffs = nullptr; // n_cols x 2^m monomial coefficients
    uint32_t* d_mat = nullptr;    // the committed matrix
    zkhip_tree* tree = nullptr;
    uint32_t root[8] = {};
};

namespace zk {

int whir_commit_cols(zkhip_ctx* ctx, const zkhip_whir_params* params, const WhirCols& cols, size_t n_cols, unsigned m,
                     zkhip_whir_commitment** out, uint32_t* root_out) {
    const WhirShape sh = whir_shape(params, m, n_cols);
    if (!sh.ok) return set_error(ctx, ZKHIP_ERR_INVALID, "whir: parameters do not fit m and n_cols");
    const unsigned b = params->log_blowup, k = params->fold_log, ln = m + b;
    const size_t N = (size_t)1 << ln, n = (size_t)1 << m;
    zkhip_whir_commitment* com = new zkhip_whir_commitment();
    com->params = *params, com->m = m, com->n_cols = n_cols, com->cols = cols;
    uint32_t* d_cw = nullptr;
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(ctx->stream);
        if (d_cw) (void)hipFree(d_cw);
        if (com->d_coeffs) (void)hipFree(com->d_coeffs);
        if (com->d_mat) (void)hipFree(com->d_mat);
        delete com;
        return rc;
    };
    if (hipMalloc(&d_cw, N * n_cols * 4) != hipSuccess || hipMalloc(&com->d_coeffs, n * n_cols * 4) != hipSuccess ||
        hipMalloc(&com->d_mat, N * n_cols * 4) != hipSuccess)
        return fail(set_error(ctx, ZKHIP_ERR_NOMEM, "whir: commitment buffers"));
    hipStream_t st = ctx->stream;
    {
        KernelScope ks(ctx, "whir_zeta");
        for (unsigned s = 0; s < m;) {
            const unsigned v = s == 0 ? std::min(m, WHIR_ZT) : std::min(m - s, WHIR_ZT - 4), lw = s == 0 ? 0 : std::min(s, WHIR_ZT - v);
            const size_t tiles = (size_t)1 << (m - v - lw);
            hipLaunchKernelGGL(k_whir_zeta, dim3((unsigned)tiles, (unsigned)n_cols), dim3(256), 0, st, cols, (int)(s == 0), d_cw, N, m, s, v, lw);
            s += v;
        }
    }
    if (hipGetLastError() != hipSuccess) return fail(set_error(ctx, ZKHIP_ERR_HIP, "whir: zeta launch"));
    if (hipMemcpy2DAsync(com->d_coeffs, n * 4, d_cw, N * 4, n * 4, n_cols, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemset2DAsync(d_cw + n, N * 4, 0, (N - n) * 4, n_cols, st) != hipSuccess)
        return fail(set_error(ctx, ZKHIP_ERR_HIP, "whir: coefficient copies"));
    int rc = ntt_batch(ctx, d_cw, ln, n_cols, N, false, true);
    if (rc != ZKHIP_OK) return fail(rc);
    {
        KernelScope ks(ctx, "whir_regroup");
        hipLaunchKernelGGL(k_whir_regroup, dim3(grid_of(N * n_cols)), dim3(256), 0, st, (const uint32_t*)d_cw, N, (unsigned)n_cols, ln, k, 0,
                           com->d_mat);
    }
    if (hipGetLastError() != hipSuccess) return fail(set_error(ctx, ZKHIP_ERR_HIP, "whir: regroup launch"));
    zkhip_matrix mat{com->d_mat, (size_t)1 << (ln - k), ln - k, n_cols << k};
    rc = zkhip_merkle_commit(ctx, &mat, 1, &com->tree, com->root);   // synchronises
    if (rc != ZKHIP_OK) return fail(rc);
    (void)hipFree(d_cw);
    d_cw = nullptr;
    if (root_out) memcpy(root_out, com->root, 32);
    *out = com;
    return ZKHIP_OK;
}

void whir_destroy(zkhip_ctx* ctx, zkhip_whir_commitment* com) {
    if (!com) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    if (com->tree) zkhip_tree_destroy(ctx, com->tree);
    if (com->d_coeffs) (void)hipFree(com->d_coeffs);
    if (com->d_mat) (void)hipFree(com->d_mat);
    delete com;
}

int whir_open_device(zkhip_ctx* ctx, zkhip_whir_commitment* com, DevTranscript* d_t, const uint32_t* point, uint32_t* values_out,
                     uint32_t* proof_out, size_t cap) {
    const zkhip_whir_params* prm = &com->params;
    const unsigned m = com->m, k = prm->fold_log, b = prm->log_blowup;
    const size_t n_cols = com->n_cols, n = (size_t)1 << m;
    const WhirShape sh = whir_shape(prm, m, n_cols);
    const WhirLayout L = whir_layout(prm, m, n_cols, sh);
    if (cap < L.total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, "whir: proof buffer too small");
    for (unsigned j = 0; j < 4 * m; j++)
        if (point[j] >= P) return set_error(ctx, ZKHIP_ERR_INVALID, "whir: point not canonical");
    unsigned max_q = 0;
    for (unsigned i = 0; i < sh.R; i++) max_q = std::max(max_q, prm->num_queries[i]);
    const unsigned ln1 = m + b - 1;   // the largest later codeword
    DevBufs B(ctx);
    // the later codewords' trees: declared after B, so destroyed after the stream drains and before B frees the matrices under them
    struct Trees {
        zkhip_ctx* ctx;
        std::vector<zkhip_tree*> list;
        ~Trees() {
            (void)hipStreamSynchronize(ctx->stream);
            for (zkhip_tree* t : list) zkhip_tree_destroy(ctx, t);
        }
    } trees{ctx};
    uint32_t *fA = B.get(4 * n), *wA = B.get(4 * n), *fB = B.get(2 * n), *wB = B.get(2 * n), *cA = B.get(4 * n), *cB = B.get(4 * (n >> k));
    uint32_t *ntt = sh.R > 1 ? B.get(4 * ((size_t)1 << ln1)) : nullptr;
    uint32_t *mat[2] = {sh.R > 1 ? B.get(4 * ((size_t)1 << ln1)) : nullptr, sh.R > 2 ? B.get(4 * ((size_t)1 << (ln1 - 1))) : nullptr};
    uint32_t *partial = B.get(4 * (size_t)ZKHIP_WHIR_MAX_COLS * SC_NB), *dP = B.get(L.total), *rs = B.get(4 * (size_t)k * sh.R);
    uint32_t *misc = B.get(64), *idx = B.get(max_q), *pts = B.get(4 * (size_t)(1 + max_q) * m);
    if (!fA || !wA || !fB || !wB || !cA || !cB || (sh.R > 1 && (!ntt || !mat[0])) || (sh.R > 2 && !mat[1]) || !partial || !dP || !rs ||
        !misc || !idx || !pts)
        return set_error(ctx, ZKHIP_ERR_NOMEM, "whir: opening buffers");
    uint32_t *alpha = misc, *zeta = misc + 4, *gamma = misc + 8;
    hipStream_t st = ctx->stream;
    ZK_HIP_CHECK(ctx, hipMemsetAsync(dP, 0, L.total * 4, st));
    {   // w = eq(z, .), the values, alpha, f and its coefficients
        std::vector<uint32_t> zm(4 * (size_t)m);
        for (size_t j = 0; j < zm.size(); j++) zm[j] = to_monty(point[j]);
        ZK_TRY(zkhip_h2d(ctx, pts, zm.data(), zm.size() * 4));
        {
            KernelScope ks(ctx, "whir_weight");
            hipLaunchKernelGGL(k_whir_weight, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wA, m, (const uint32_t*)pts, 1u,
                               (const uint32_t*)nullptr, 1);
        }
        const unsigned nb = grid_of(n);
        {
            KernelScope ks(ctx, "whir_dot");
            hipLaunchKernelGGL(k_whir_dot, dim3(nb), dim3(256), 0, st, com->cols, (unsigned)n_cols, (const uint32_t*)wA, n, partial);
        }
        {
            KernelScope ks(ctx, "whir_reduce");
            hipLaunchKernelGGL(k_whir_reduce, dim3(1), dim3(256), 0, st, (const uint32_t*)partial, nb, (unsigned)n_cols, dP);
        }
        ZK_HIP_CHECK(ctx, hipGetLastError());
        ZK_TRY(transcript_observe(ctx, d_t, dP, (uint32_t)(4 * n_cols), true));
        ZK_TRY(transcript_sample(ctx, d_t, alpha, nullptr, 4));
        WhirCols cc{};
        for (size_t c = 0; c < n_cols; c++) cc.p[c] = com->d_coeffs + c * n, cc.es[c] = 1;
        KernelScope ks(ctx, "whir_combine");
        hipLaunchKernelGGL(k_whir_combine, dim3(grid_of(n)), dim3(256), 0, st, com->cols, (unsigned)n_cols, n, (const uint32_t*)alpha, fA);
        hipLaunchKernelGGL(k_whir_combine, dim3(grid_of(n)), dim3(256), 0, st, cc, (unsigned)n_cols, n, (const uint32_t*)alpha, cA);
        ZK_HIP_CHECK(ctx, hipGetLastError());
    }
    std::vector<std::vector<uint32_t>> openings(sh.R);
    std::vector<std::vector<uint64_t>> qidx(sh.R);
    zkhip_tree* tree = com->tree;
    uint32_t *f = fA, *w = wA, *c = cA;
    unsigned ln = m + b;
    for (unsigned i = 0; i < sh.R; i++) {
        const bool last = i + 1 == sh.R;
        const unsigned mi = m - k * i, mn = mi - k;
        uint32_t* r_i = rs + 4 * (size_t)k * i;
        // the k sum-check rounds
        size_t sz = (size_t)1 << mi;   // entries after the pending fold
        const uint32_t* pending = nullptr;
        auto pass = [&](uint32_t* fo, uint32_t* wo, uint32_t* part) {   // sz / 2 pairs
            WhirPass p{};
            p.src.tab[0] = f, p.src.tab[1] = w, p.dst[0] = fo, p.dst[1] = wo, p.r = pending, p.n_pairs = sz / 2, p.partial = part;
            KernelScope ks(ctx, "whir_pass");
            hipLaunchKernelGGL(k_sc_pass, dim3(grid_of(sz / 2)), dim3(256), 0, st, p);
        };
        unsigned t = 0;
        for (; t < k && sz > SC_T; t++, sz >>= 1) {
            uint32_t *fo = f == fA ? fB : fA, *wo = w == wA ? wB : wA;
            pass(fo, wo, partial);
            {
                KernelScope ks(ctx, "whir_round_tr");
                hipLaunchKernelGGL(k_sc_round_tr<8>, dim3(1), dim3(64), 0, st, d_t, (const uint32_t*)partial, grid_of(sz / 2), dP + L.sc[i] + 8 * t,
                                   r_i + 4 * t);
            }
            ZK_HIP_CHECK(ctx, hipGetLastError());
            if (pending) f = fo, w = wo;
            pending = r_i + 4 * t;
        }
        if (t < k) {   // the rest in one workgroup
            uint32_t *fo = last ? nullptr : (f == fA ? fB : fA), *wo = last ? nullptr : (w == wA ? wB : wA);
            KernelScope ks(ctx, "whir_small");
            hipLaunchKernelGGL(k_whir_small, dim3(1), dim3(SC_SW), 0, st, d_t, (const uint32_t*)f, (const uint32_t*)w, pending, (unsigned)sz,
                               k - t, dP + L.sc[i] + 8 * t, r_i + 4 * t, fo, wo);
            ZK_HIP_CHECK(ctx, hipGetLastError());
            if (!last) f = fo, w = wo;
        } else if (!last) {   // fold with the last challenge
            uint32_t *fo = f == fA ? fB : fA, *wo = w == wA ? wB : wA;
            pass(fo, wo, nullptr);
            ZK_HIP_CHECK(ctx, hipGetLastError());
            f = fo, w = wo;
        }
        // the coefficients, folded by 2^k
        uint32_t* cn = c == cA ? cB : cA;
        const size_t nn = (size_t)1 << mn, Nn = (size_t)1 << (ln - 1);
        if (!last) ZK_HIP_CHECK(ctx, hipMemset2DAsync(ntt + nn, Nn * 4, 0, (Nn - nn) * 4, 4, st));
        {
            KernelScope ks(ctx, "whir_cfold");
            hipLaunchKernelGGL(k_whir_cfold, dim3(grid_of(nn)), dim3(256), 0, st, (const uint32_t*)c, nn, k, (const uint32_t*)r_i, cn,
                               last ? nullptr : ntt, Nn);
            ZK_HIP_CHECK(ctx, hipGetLastError());
        }
        c = cn;
        zkhip_tree* next = nullptr;
        if (!last) {
            // f_{i+1} on L_{i+1} = L_i^2: NTT of the four coordinate columns, regroup, commit
            ZK_TRY(ntt_batch(ctx, ntt, ln - 1, 4, Nn, false, true));
            uint32_t* mt = mat[i % 2];
            {
                KernelScope ks(ctx, "whir_regroup");
                hipLaunchKernelGGL(k_whir_regroup, dim3(grid_of(4 * Nn)), dim3(256), 0, st, (const uint32_t*)ntt, Nn, 4u, ln - 1, k, 1, mt);
                ZK_HIP_CHECK(ctx, hipGetLastError());
            }
            zkhip_matrix mx{mt, Nn >> k, ln - 1 - k, (size_t)4 << k};
            ZK_TRY(zkhip_merkle_commit(ctx, &mx, 1, &next, nullptr));
            trees.list.push_back(next);
            ZK_HIP_CHECK(ctx, hipMemcpyAsync(dP + L.mid[i], zkhip_tree_root_device(next), 32, hipMemcpyDeviceToDevice, st));
            ZK_TRY(convert_repr(ctx, dP + L.mid[i], 8, false));
            ZK_TRY(transcript_observe(ctx, d_t, dP + L.mid[i], 8, true));
            ZK_TRY(transcript_sample(ctx, d_t, zeta, nullptr, 4));
            const size_t per = (nn + 256 * SC_NB - 1) / (256 * SC_NB);   // coefficients per thread
            const unsigned nb = (unsigned)(((nn + per - 1) / per + 255) / 256);
            {
                KernelScope ks(ctx, "whir_ood");
                hipLaunchKernelGGL(k_whir_ood, dim3(nb), dim3(256), 0, st, (const uint32_t*)c, nn, per, (const uint32_t*)zeta, partial);
            }
            {
                KernelScope ks(ctx, "whir_reduce");
                hipLaunchKernelGGL(k_whir_reduce, dim3(1), dim3(256), 0, st, (const uint32_t*)partial, nb, 1u, dP + L.mid[i] + 8);
            }
            ZK_HIP_CHECK(ctx, hipGetLastError());
            ZK_TRY(transcript_observe(ctx, d_t, dP + L.mid[i] + 8, 4, true));
        } else {
            ZK_HIP_CHECK(ctx, hipMemcpyAsync(dP + L.mid[i], c, ((size_t)16) << sh.mf, hipMemcpyDeviceToDevice, st));
            ZK_TRY(convert_repr(ctx, dP + L.mid[i], (size_t)4 << sh.mf, false));
            ZK_TRY(transcript_observe(ctx, d_t, dP + L.mid[i], (uint32_t)(4u << sh.mf), true));
        }
        ZK_TRY(transcript_grind(ctx, d_t, prm->pow_bits[i], dP + L.pow[i]));
        const unsigned nq = prm->num_queries[i];
        ZK_TRY(transcript_sample_bits(ctx, d_t, idx, nq, ln - k));
        std::vector<uint32_t> h(4 + nq);   // zeta, indices
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), zeta, 16, hipMemcpyDeviceToHost, st));
        ZK_HIP_CHECK(ctx, hipMemcpyAsync(h.data() + 4, idx, 4 * (size_t)nq, hipMemcpyDeviceToHost, st));
        ZK_HIP_CHECK(ctx, hipStreamSynchronize(st));
        qidx[i].assign(h.begin() + 4, h.end());
        openings[i].resize(nq * L.qw[i]);
        ZK_TRY(zkhip_merkle_open(ctx, tree, qidx[i].data(), nq, openings[i].data(), openings[i].size()));
        if (!last) {
            ZK_TRY(transcript_sample(ctx, d_t, gamma, nullptr, 4));
            // the new constraints: the OOD point and the query points y = g^bitrev(idx), g of order 2^(ln - k), as (y, y^2, y^4, ..)
            std::vector<uint32_t> pv;
            pv.reserve(4 * (size_t)(1 + nq) * mn);
            auto push = [&](const Ext& x) {
                for (const Ext& e : pow_point(x, mn))
                    for (int q = 0; q < 4; q++) pv.push_back(e.c[q]);
            };
            push(Ext{{h[0], h[1], h[2], h[3]}});
            const uint32_t g = (two_adic_generator(ln - k));
            for (unsigned q = 0; q < nq; q++) push(ext_from_base(mpow(g, bitrev32((uint32_t)qidx[i][q], ln - k))));
            ZK_TRY(zkhip_h2d(ctx, pts, pv.data(), pv.size() * 4));
            KernelScope ks(ctx, "whir_weight");
            hipLaunchKernelGGL(k_whir_weight, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, w, mn, (const uint32_t*)pts, 1 + nq,
                               (const uint32_t*)gamma, 0);
            ZK_HIP_CHECK(ctx, hipGetLastError());
            tree = next, ln--;
        }
    }
    std::vector<uint32_t> proof(L.total);
    ZK_TRY(zkhip_d2h(ctx, proof.data(), dP, L.total * 4));
    for (unsigned i = 0; i < sh.R; i++) std::copy(openings[i].begin(), openings[i].end(), proof.begin() + L.q[i]);
    memcpy(proof_out, proof.data(), L.total * 4);
    if (values_out) memcpy(values_out, proof.data(), 16 * n_cols);
    return ZKHIP_OK;
}

// ---- the host verifier ------------------------------------------------------------------------------------------------------
namespace {
Ext coeff_eval(const std::vector<Ext>& c, const Ext* pt, unsigned n) {   // f~(pt) from 2^n monomial coefficients
    std::vector<Ext> t(c);
    for (unsigned j = 0; j < n; j++) {   // bind the lowest variable: c_even + x c_odd
        for (size_t y = 0; y < t.size() / 2; y++) t[y] = ext_add(t[2 * y], ext_mul(pt[j], t[2 * y + 1]));
        t.resize(t.size() / 2);
    }
    return t[0];
}
struct Cons {
    Ext coef;
    std::vector<Ext> pt;
    size_t at;   // index of the first challenge it is bound by
};
}  // namespace

int whir_verify_host(HostChallenger& ch, const zkhip_whir_params* prm, const uint32_t* root, unsigned m, size_t n_cols, const uint32_t* point,
                     const uint32_t* proof, size_t words, uint32_t* values_out) {
    const WhirShape sh = whir_shape(prm, m, n_cols);
    if (!sh.ok || !proof || !root || !point) return ZKHIP_ERR_VERIFY;
    const WhirLayout L = whir_layout(prm, m, n_cols, sh);
    if (words != L.total) return ZKHIP_ERR_VERIFY;
    for (size_t j = 0; j < words; j++)
        if (proof[j] >= P) return ZKHIP_ERR_VERIFY;
    for (unsigned j = 0; j < 4 * m; j++)
        if (point[j] >= P) return ZKHIP_ERR_VERIFY;
    for (int j = 0; j < 8; j++)
        if (root[j] >= P) return ZKHIP_ERR_VERIFY;
    const unsigned k = prm->fold_log, s = 1u << k;
    ch.observe_canon(proof, 4 * n_cols);
    const Ext alpha = ch.sample_ext();
    std::vector<Ext> apow(n_cols);
    Ext sigma = ext_zero(), a = ext_one();
    for (size_t c = 0; c < n_cols; c++) apow[c] = a, sigma = ext_add(sigma, ext_mul(a, ext_from_canon(proof + 4 * c))), a = ext_mul(a, alpha);
    std::vector<Cons> cons;
    cons.push_back(Cons{ext_one(), std::vector<Ext>(m), 0});
    for (unsigned j = 0; j < m; j++) cons[0].pt[j] = ext_from_canon(point + 4 * j);
    std::vector<Ext> rs_all;
    std::vector<Ext> final_c;
    uint32_t cur_root[8];
    memcpy(cur_root, root, 32);
    unsigned ln = m + prm->log_blowup;
    for (unsigned i = 0; i < sh.R; i++) {
        const bool last = i + 1 == sh.R;
        const unsigned mn = m - k * (i + 1);
        std::vector<Ext> rs(k);
        for (unsigned t = 0; t < k; t++) {
            const uint32_t* sw = proof + L.sc[i] + 8 * t;
            const Ext s0 = ext_from_canon(sw), s2 = ext_from_canon(sw + 4);
            ch.observe_canon(sw, 8);
            rs[t] = ch.sample_ext();
            const Ext sv[3] = {s0, ext_sub(sigma, s0), s2};
            sigma = poly_at(sv, 2, rs[t]);
        }
        rs_all.insert(rs_all.end(), rs.begin(), rs.end());
        Ext zeta{}, ood{};
        if (!last) {
            ch.observe_canon(proof + L.mid[i], 8);
            zeta = ch.sample_ext();
            ood = ext_from_canon(proof + L.mid[i] + 8);
            ch.observe_canon(proof + L.mid[i] + 8, 4);
        } else {
            final_c.resize((size_t)1 << sh.mf);
            for (size_t j = 0; j < final_c.size(); j++) final_c[j] = ext_from_canon(proof + L.mid[i] + 4 * j);
            ch.observe_canon(proof + L.mid[i], (size_t)4 << sh.mf);
        }
        if (!ch.check_witness(prm->pow_bits[i], proof[L.pow[i]])) return ZKHIP_ERR_VERIFY;
        const unsigned nq = prm->num_queries[i], lh = ln - k;
        const size_t width = (i == 0 ? n_cols : 4) << k;
        std::vector<Ext> ys(nq), folded(nq);
        const uint32_t g = (two_adic_generator(lh));
        for (unsigned q = 0; q < nq; q++) {
            const uint64_t id = ch.sample_bits(lh);
            const uint32_t* op = proof + L.q[i] + q * L.qw[i];
            const unsigned lhs = lh;
            const size_t wd = width;
            if (zkhip_mmcs_verify(cur_root, &lhs, &wd, 1, id, op) != ZKHIP_OK) return ZKHIP_ERR_VERIFY;
            std::vector<Ext> v(s);
            for (unsigned t = 0; t < s; t++) {
                if (i == 0) {
                    Ext e = ext_zero();
                    for (size_t c = 0; c < n_cols; c++) e = ext_add(e, ext_mul_base(apow[c], to_monty(op[c * s + t])));
                    v[t] = e;
                } else {
                    v[t] = ext_from_canon(op + 4 * t);
                }
            }
            for (unsigned j = 0; j < k; j++) {
                const uint64_t base = id << (k - j - 1);
                for (unsigned u = 0; u < (s >> (j + 1)); u++) v[u] = fold_row(base + u, ln - j - 1, rs[j], v[2 * u], v[2 * u + 1]);
            }
            folded[q] = v[0];
            ys[q] = ext_from_base(mpow(g, bitrev32((uint32_t)id, lh)));
        }
        if (!last) {
            const Ext gamma = ch.sample_ext();
            Ext gp = gamma;
            sigma = ext_add(sigma, ext_mul(gp, ood));
            cons.push_back(Cons{gp, pow_point(zeta, mn), rs_all.size()});
            for (unsigned q = 0; q < nq; q++) {
                gp = ext_mul(gp, gamma);
                sigma = ext_add(sigma, ext_mul(gp, folded[q]));
                cons.push_back(Cons{gp, pow_point(ys[q], mn), rs_all.size()});
            }
            for (int j = 0; j < 8; j++) cur_root[j] = proof[L.mid[i] + j];
            ln--;
        } else {
            for (unsigned q = 0; q < nq; q++) {
                const std::vector<Ext> pp = pow_point(ys[q], sh.mf);
                if (!ext_eq(coeff_eval(final_c, pp.data(), sh.mf), folded[q])) return ZKHIP_ERR_VERIFY;
            }
        }
    }
    Ext total = ext_zero();
    for (const Cons& c : cons) {
        const size_t nb = rs_all.size() - c.at;
        const Ext e = ext_mul(c.coef, eq_eval(c.pt.data(), rs_all.data() + c.at, nb));
        total = ext_add(total, ext_mul(e, coeff_eval(final_c, c.pt.data() + nb, sh.mf)));
    }
    if (!ext_eq(total, sigma)) return ZKHIP_ERR_VERIFY;
    if (values_out) memcpy(values_out, proof, 16 * n_cols);
    return ZKHIP_OK;
}

namespace {
Ext coords_to_ext(const uint32_t* v4) {   // sum_c X^c v_c, v_c = 4 canonical words each
    Ext acc = ext_zero();
    for (int c = 0; c < 4; c++) {
        Ext xc = ext_zero();
        xc.c[c] = to_monty(1);
        acc = ext_add(acc, ext_mul(xc, ext_from_canon(v4 + 4 * c)));
    }
    return acc;
}
size_t committed_words(const zkhip_whir_params* prm, unsigned log_n, bool num_ext) {
    const size_t g = zkhip_gkr_proof_words(log_n), w = zkhip_whir_proof_words(prm, log_n, num_ext ? 8 : 5);
    return g && w ? 8 + g + w : 0;
}
}  // namespace

}  // namespace zk

using namespace zk;

extern "C" {

size_t zkhip_whir_proof_words(const zkhip_whir_params* params, unsigned m, size_t n_cols) {
    const WhirShape sh = whir_shape(params, m, n_cols);
    return sh.ok ? whir_layout(params, m, n_cols, sh).total : 0;
}

int zkhip_whir_commit(zkhip_ctx* ctx, const zkhip_whir_params* params, const uint32_t* d_cols, size_t col_stride, size_t n_cols, unsigned m,
                      zkhip_whir_commitment** out, uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !d_cols || !out || n_cols < 1 || n_cols > ZKHIP_WHIR_MAX_COLS) return ZKHIP_ERR_INVALID;
    if (m > ZKHIP_WHIR_MAX_LOG_N || (n_cols > 1 && col_stride < ((size_t)1 << m))) return set_error(ctx, ZKHIP_ERR_INVALID, "whir: column shape");
    WhirCols cols{};
    for (size_t c = 0; c < n_cols; c++) cols.p[c] = d_cols + c * col_stride, cols.es[c] = 1;
    return whir_commit_cols(ctx, params, cols, n_cols, m, out, root_out);
}

int zkhip_whir_open(zkhip_ctx* ctx, zkhip_whir_commitment* com, zkhip_transcript* transcript, const uint32_t* point, uint32_t* values_out,
                    uint32_t* proof_out, size_t cap) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !com || !transcript || !point || !proof_out) return ZKHIP_ERR_INVALID;
    return whir_open_device(ctx, com, transcript->d, point, values_out, proof_out, cap);
}

void zkhip_whir_commitment_destroy(zkhip_ctx* ctx, zkhip_whir_commitment* com) {
    ZK_BIND_DEVICE(ctx);
    whir_destroy(ctx, com);
}

int zkhip_whir_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const uint32_t* root, unsigned m, size_t n_cols,
                      const uint32_t* point, const uint32_t* values, const uint32_t* proof, size_t words) {
    if ((n_prefix && !prefix) || !values) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    ZK_TRY(whir_verify_host(ch, params, root, m, n_cols, point, proof, words, nullptr));
    return memcmp(values, proof, 16 * n_cols) == 0 ? ZKHIP_OK : ZKHIP_ERR_VERIFY;
}

size_t zkhip_gkr_committed_proof_words(const zkhip_whir_params* params, unsigned log_n, int num_is_ext) {
    return committed_words(params, log_n, num_is_ext != 0);
}

int zkhip_gkr_committed_prove(zkhip_ctx* ctx, zkhip_transcript* transcript, const zkhip_whir_params* params, const uint32_t* d_num, int num_is_ext,
                              const uint32_t* d_den, unsigned log_n, uint32_t* proof_out, size_t cap) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !transcript || !params || !d_num || !d_den || !proof_out) return ZKHIP_ERR_INVALID;
    const bool ext = num_is_ext != 0;
    const size_t total = committed_words(params, log_n, ext), gw = zkhip_gkr_proof_words(log_n);
    if (!total || log_n > ZKHIP_WHIR_MAX_LOG_N) return set_error(ctx, ZKHIP_ERR_INVALID, "gkr_committed: parameters do not fit log_n");
    if (cap < total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, "gkr_committed: proof buffer too small");
    WhirCols cols{};
    size_t nc = 0;
    if (ext)
        for (int q = 0; q < 4; q++) cols.p[nc] = d_num + q, cols.es[nc++] = 4;
    else
        cols.p[nc] = d_num, cols.es[nc++] = 1;
    for (int q = 0; q < 4; q++) cols.p[nc] = d_den + q, cols.es[nc++] = 4;
    zkhip_whir_commitment* com = nullptr;
    ZK_TRY(whir_commit_cols(ctx, params, cols, nc, log_n, &com, proof_out));
    int rc = zkhip_transcript_observe(ctx, transcript, proof_out, 8);
    const uint32_t* d_res = nullptr;
    if (rc == ZKHIP_OK) rc = gkr_prove_device(ctx, transcript->d, d_num, ext, d_den, log_n, &d_res);
    std::vector<uint32_t> h(gw + 4 * (size_t)log_n + 8);
    if (rc == ZKHIP_OK) rc = zkhip_d2h(ctx, h.data(), d_res, h.size() * 4);
    if (rc == ZKHIP_OK) {
        memcpy(proof_out + 8, h.data(), gw * 4);
        rc = whir_open_device(ctx, com, transcript->d, h.data() + gw, nullptr, proof_out + 8 + gw, total - 8 - gw);
    }
    whir_destroy(ctx, com);
    return rc;
}

int zkhip_gkr_committed_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const uint32_t* proof, size_t words,
                               unsigned log_n, int num_is_ext, uint32_t* root_out, uint32_t* pq_out) {
    if ((n_prefix && !prefix) || !proof) return ZKHIP_ERR_INVALID;
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    const bool ext = num_is_ext != 0;
    const size_t total = committed_words(params, log_n, ext), gw = zkhip_gkr_proof_words(log_n);
    if (!total || words != total) return ZKHIP_ERR_VERIFY;
    for (int j = 0; j < 8; j++)
        if (proof[j] >= P) return ZKHIP_ERR_VERIFY;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    ch.observe_canon(proof, 8);
    std::vector<uint32_t> point(4 * (size_t)log_n);
    uint32_t claims[8];
    Ext root_pq[2];
    ZK_TRY(gkr_verify_host(ch, proof + 8, gw, log_n, point.data(), claims, root_pq));
    const size_t nc = ext ? 8 : 5;
    std::vector<uint32_t> vals(4 * nc);
    ZK_TRY(whir_verify_host(ch, params, proof, log_n, nc, point.data(), proof + 8 + gw, words - 8 - gw, vals.data()));
    const Ext num_v = ext ? coords_to_ext(vals.data()) : ext_from_canon(vals.data());
    const Ext den_v = coords_to_ext(vals.data() + 4 * (nc - 4));
    if (!ext_eq(num_v, ext_from_canon(claims)) || !ext_eq(den_v, ext_from_canon(claims + 4))) return ZKHIP_ERR_VERIFY;
    if (root_out) memcpy(root_out, proof, 32);
    if (pq_out) ext_to_canon(pq_out, root_pq[0]), ext_to_canon(pq_out + 4, root_pq[1]);
    return ZKHIP_OK;
}

}  // extern "C"
