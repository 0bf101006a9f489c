// zerocheck.hip -- the AIR zero-check over the stacked WHIR commitment: the main traces of a set of AIRs satisfy their main-trace
// constraints on every row.  Protocol, layout, limits and measurements: docs/zerocheck.md.  The independent model is
// tests/zerocheck_model.py.
//
// Device side, per AIR: eq(tau, .) (k_whir_weight); round 0 of the sum-check straight from the base-field trace, the constraint
// program interpreted in the base field once per point (k_zc_round0); the later rounds as one streaming pass each that folds every
// table with the previous challenge and interprets the program in the extension field (k_zc_pass), to the last round; the values
// from the last fold; the rotation reduction on the sum-check core (k_sc_pass, sc_small_round) and the columns' values at its point
// (k_zc_dot).  Then one stacked opening (stacking.hip).  The host verifier is at the end of the file.
#include "zerocheck_dev.hpp"

namespace zk {
namespace {
// the whole shape: plans, the stacked columns' heights and AIRs, the words before the stacked opening; false = refused
struct ZcShape {
    std::vector<ZcPlan> plans;
    std::vector<unsigned> lh, col_point, dims;
    size_t head = 8, total = 0;
};
bool zc_shape(const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, unsigned l, ZcShape* S) {
    if (!prm || !airs || n_airs < 1 || n_airs > ZKHIP_STACK_MAX_POINTS) return false;
    S->plans.resize(n_airs);
    size_t n_cols = 0;
    for (size_t a = 0; a < n_airs; a++) {
        if (!zc_plan(airs[a], &S->plans[a])) return false;
        n_cols += airs[a].width;
        if (n_cols > ZKHIP_STACK_MAX_COLS) return false;
        S->head += S->plans[a].proven.empty() ? 0 : S->plans[a].words();
        S->dims.push_back(airs[a].log_height);
        for (size_t c = 0; c < airs[a].width; c++) S->lh.push_back(airs[a].log_height), S->col_point.push_back((unsigned)a);
    }
    const size_t sw = zkhip_stack_proof_words(prm, S->lh.data(), S->lh.size(), l);
    if (!sw) return false;
    S->total = S->head + sw;
    return true;
}

// ---- the device prover ---------------------------------------------------------------------------------------------------------
int zc_prove(zkhip_ctx* ctx, const zkhip_whir_params* prm, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
             const uint32_t* const* pvs, unsigned l, DevTranscript* d_t, uint32_t* proof_out, size_t cap, uint32_t* root_out) {
    ZcShape S;
    if (!zc_shape(prm, airs, n_airs, l, &S)) return set_error(ctx, ZKHIP_ERR_INVALID, "zerocheck: the shape does not fit the limits");
    if (cap < S.total) return set_error(ctx, ZKHIP_ERR_SMALL_BUFFER, "zerocheck: proof buffer too small");
    size_t n_pv = 0, pt_words = 0;
    for (size_t a = 0; a < n_airs; a++) {
        if (!d_traces[a] || (airs[a].n_pvs && !pvs[a])) return set_error(ctx, ZKHIP_ERR_INVALID, "zerocheck: null trace or public values");
        for (size_t i = 0; i < airs[a].n_pvs; i++)
            if (pvs[a][i] >= P) return set_error(ctx, ZKHIP_ERR_INVALID, "zerocheck: public value not canonical");
        n_pv += airs[a].n_pvs, pt_words += 4 * (size_t)airs[a].log_height;
    }
    // 1. commit: every main column, AIRs in caller order
    std::vector<const uint32_t*> cols;
    for (size_t a = 0; a < n_airs; a++)
        for (size_t c = 0; c < airs[a].width; c++) cols.push_back(d_traces[a] + (c << airs[a].log_height));
    struct Com {
        zkhip_ctx* ctx;
        zkhip_stack_commitment* sc = nullptr;
        ~Com() { stack_destroy(ctx, sc); }
    } com{ctx};
    uint32_t root[8];
    ZK_TRY(stack_commit(ctx, prm, cols.data(), S.lh.data(), cols.size(), l, &com.sc, root));
    ZcBufs B(ctx);
    // device: [the words before the opening | the points r'_a (Montgomery)], then the root and the public values to observe
    uint32_t *dP = B.get(S.head + pt_words), *d_obs = B.get(8 + n_pv);
    if (!dP || !d_obs) return set_error(ctx, ZKHIP_ERR_NOMEM, "zerocheck: proof staging");
    std::vector<uint32_t> obs(root, root + 8);
    for (size_t a = 0; a < n_airs; a++) obs.insert(obs.end(), pvs[a], pvs[a] + airs[a].n_pvs);
    ZK_TRY(zkhip_h2d(ctx, d_obs, obs.data(), obs.size() * 4));
    ZK_TRY(transcript_observe(ctx, d_t, d_obs, (uint32_t)obs.size(), true));
    // 2. - 4. per AIR
    size_t off = 8, poff = S.head;
    for (size_t a = 0; a < n_airs; a++) {
        ZK_TRY(zc_prove_air<false>(ctx, d_t, S.plans[a], d_traces[a], pvs[a], dP + off, dP + poff));
        off += S.plans[a].proven.empty() ? 0 : S.plans[a].words();
        poff += 4 * (size_t)airs[a].log_height;
    }
    // 5. the one read-back before the opening: the words so far and the points
    std::vector<uint32_t> h(S.head + pt_words);
    ZK_TRY(zkhip_d2h(ctx, h.data(), dP, h.size() * 4));
    for (size_t i = S.head; i < h.size(); i++) h[i] = from_monty(h[i]);
    ZK_TRY(stack_open(ctx, com.sc, d_t, h.data() + S.head, S.dims.data(), n_airs, S.col_point.data(), nullptr, proof_out + S.head, cap - S.head));
    memcpy(proof_out, root, 32);
    memcpy(proof_out + 8, h.data() + 8, (S.head - 8) * 4);
    if (root_out) memcpy(root_out, root, 32);
    return ZKHIP_OK;
}

// ---- the host verifier ---------------------------------------------------------------------------------------------------------
int zc_verify(const zkhip_whir_params* prm, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
              const uint32_t* const* pvs, unsigned l, const uint32_t* proof, size_t words, uint32_t* root_out) {
    ZcShape S;
    if (!zc_shape(prm, airs, n_airs, l, &S)) return ZKHIP_ERR_INVALID;
    for (size_t a = 0; a < n_airs; a++) {
        if (airs[a].n_pvs && !pvs[a]) return ZKHIP_ERR_INVALID;
        for (size_t i = 0; i < airs[a].n_pvs; i++)
            if (pvs[a][i] >= P) return ZKHIP_ERR_INVALID;
    }
    for (size_t i = 0; i < n_prefix; i++)
        if (prefix[i] >= P) return ZKHIP_ERR_INVALID;
    if (words != S.total) return ZKHIP_ERR_VERIFY;
    for (size_t i = 0; i < S.head; i++)
        if (proof[i] >= P) return ZKHIP_ERR_VERIFY;
    HostChallenger ch;
    ch.observe_canon(prefix, n_prefix);
    ch.observe_canon(proof, 8);
    for (size_t a = 0; a < n_airs; a++) ch.observe_canon(pvs[a], airs[a].n_pvs);
    const Ext one = ext_one();
    std::vector<uint32_t> points;                 // r'_a, canonical, end to end
    std::vector<const uint32_t*> claimed(n_airs, nullptr);   // the w values the opening must show (null: none claimed)
    const uint32_t* q = proof + 8;
    for (size_t a = 0; a < n_airs; a++) {
        const ZcPlan& pl = S.plans[a];
        const unsigned m = pl.m, D = pl.D;
        const size_t w = pl.w, n_rot = pl.rot.size();
        std::vector<Ext> rp(m);
        if (pl.proven.empty()) {
            for (unsigned j = 0; j < m; j++) rp[j] = ch.sample_ext();
        } else {
            std::vector<Ext> tau(m), r(m);
            for (unsigned j = 0; j < m; j++) tau[j] = ch.sample_ext();
            const Ext alpha = ch.sample_ext();
            Ext claim = ext_zero();
            for (unsigned i = 0; i < m; i++, q += 4 * D) {
                Ext s[ZKHIP_ZEROCHECK_MAX_DEGREE + 1];
                s[0] = ext_from_canon(q), s[1] = ext_sub(claim, s[0]);
                for (unsigned e = 1; e < D; e++) s[e + 1] = ext_from_canon(q + 4 * e);
                ch.observe_canon(q, 4 * D);
                r[i] = ch.sample_ext();
                claim = poly_at(s, D, r[i]);
            }
            std::vector<Ext> v(w), vn(n_rot);
            for (size_t j = 0; j < w; j++) v[j] = ext_from_canon(q + 4 * j);
            for (size_t t = 0; t < n_rot; t++) vn[t] = ext_from_canon(q + 4 * (w + t));
            ch.observe_canon(q, 4 * (w + n_rot));
            const uint32_t* qv = q;
            q += 4 * (w + n_rot);
            Ext first = one, last = one;
            for (unsigned j = 0; j < m; j++) first = ext_mul(first, ext_sub(one, r[j])), last = ext_mul(last, r[j]);
            const Ext c = zc_eval_host(pl, v.data(), vn.data(), first, last, pvs[a], alpha);
            if (!ext_eq(ext_mul(eq_eval(tau.data(), r.data(), m), c), claim)) return ZKHIP_ERR_VERIFY;
            if (n_rot == 0) {
                rp = r, claimed[a] = qv;
            } else {
                const Ext lambda = ch.sample_ext();
                std::vector<Ext> lp(w + n_rot);
                Ext x = one;
                claim = ext_zero();
                for (size_t j = 0; j < w + n_rot; j++) lp[j] = x, claim = ext_add(claim, ext_mul(x, j < w ? v[j] : vn[j - w])), x = ext_mul(x, lambda);
                for (unsigned i = 0; i < m; i++, q += 8) {
                    const Ext s0 = ext_from_canon(q), s2 = ext_from_canon(q + 4);
                    ch.observe_canon(q, 8);
                    rp[i] = ch.sample_ext();
                    const Ext sv[3] = {s0, ext_sub(claim, s0), s2};
                    claim = poly_at(sv, 2, rp[i]);
                }
                Ext ua = ext_zero(), ub = ext_zero();
                for (size_t j = 0; j < w; j++) ua = ext_add(ua, ext_mul(lp[j], ext_from_canon(q + 4 * j)));
                for (size_t t = 0; t < n_rot; t++) ub = ext_add(ub, ext_mul(lp[w + t], ext_from_canon(q + 4 * pl.rot[t])));
                ch.observe_canon(q, 4 * w);
                claimed[a] = q, q += 4 * w;
                const Ext rhs = ext_add(ext_mul(ua, eq_eval(r.data(), rp.data(), m)), ext_mul(ub, zc_rot_eval(r.data(), rp.data(), m)));
                if (!ext_eq(rhs, claim)) return ZKHIP_ERR_VERIFY;
            }
        }
        for (unsigned j = 0; j < m; j++) {
            uint32_t c4[4];
            ext_to_canon(c4, rp[j]);
            points.insert(points.end(), c4, c4 + 4);
        }
    }
    const uint32_t* op = proof + S.head;
    ZK_TRY(stack_verify_host(ch, prm, proof, S.lh.data(), S.lh.size(), l, points.data(), S.dims.data(), n_airs, S.col_point.data(), op, words - S.head));
    size_t col = 0;
    for (size_t a = 0; a < n_airs; col += airs[a].width, a++)
        if (claimed[a] && memcmp(claimed[a], op + 4 * col, 16 * airs[a].width) != 0) return ZKHIP_ERR_VERIFY;
    if (root_out) memcpy(root_out, proof, 32);
    return ZKHIP_OK;
}
}  // namespace

}  // namespace zk

using namespace zk;

extern "C" {

size_t zkhip_zerocheck_proof_words(const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, unsigned log_stack) {
    ZcShape S;
    return zc_shape(params, airs, n_airs, log_stack, &S) ? S.total : 0;
}

int zkhip_zerocheck_prove(zkhip_ctx* ctx, const zkhip_whir_params* params, const zkhip_air* airs, size_t n_airs, const uint32_t* const* d_traces,
                          const uint32_t* const* pvs, unsigned log_stack, zkhip_transcript* transcript, uint32_t* proof_out, size_t cap,
                          uint32_t* root_out) {
    ZK_BIND_DEVICE(ctx);
    if (!ctx || !params || !airs || !d_traces || !pvs || !transcript || !proof_out) return ZKHIP_ERR_INVALID;
    return zc_prove(ctx, params, airs, n_airs, d_traces, pvs, log_stack, transcript->d, proof_out, cap, root_out);
}

int zkhip_zerocheck_verify(const zkhip_whir_params* params, const uint32_t* prefix, size_t n_prefix, const zkhip_air* airs, size_t n_airs,
                           const uint32_t* const* pvs, unsigned log_stack, const uint32_t* proof, size_t words, uint32_t* root_out) {
    if (!params || (n_prefix && !prefix) || !airs || !pvs || !proof) return ZKHIP_ERR_INVALID;
    return zc_verify(params, prefix, n_prefix, airs, n_airs, pvs, log_stack, proof, words, root_out);
}

}  // extern "C"
