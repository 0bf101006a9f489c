// fri_query_host.hpp -- zkhip_fri_query_host's body: one query's fold loop of the host verifier (verifier.hip, the `for l < n_layers` block
// of verify_where) on canonical words, with the values it passes through written out per layer.  It calls the verifier's own fold_row
// (host_challenger.hpp) and states the same join, eval += beta^2 ro; the Merkle openings of the loop are not its business (the chip
// claims them on a bus: air.py fri_query_air).  Plain C++ on the host: tests/fri_query_host_main.cpp compiles it on its own, together with
// verifier.hip, under the sanitizers.
#pragma once
#include "../../include/zkhip.h"
#include "host_challenger.hpp"

namespace zk {

inline int fri_query_canonical(uint64_t index, unsigned log_max, unsigned n_layers, const uint32_t* beta, const uint32_t* sibling, const uint32_t* has_ro,
                               const uint32_t* ro, const uint32_t* ro_top, uint32_t* e0, uint32_t* e1, uint32_t* eval) {
    if (!beta || !sibling || !has_ro || !ro || !ro_top || !e0 || !e1 || !eval) return ZKHIP_ERR_INVALID;
    // (the last row folds into a tree of height >= 1: n_layers <= log_max - 1; compared without adding, so no n_layers wraps past it)
    if (log_max > 27 || n_layers == 0 || n_layers >= log_max || (index >> log_max)) return ZKHIP_ERR_INVALID;
    for (int q = 0; q < 4; q++)
        if (ro_top[q] >= P) return ZKHIP_ERR_INVALID;
    for (unsigned l = 0; l < n_layers; l++) {
        if (has_ro[l] > 1) return ZKHIP_ERR_INVALID;
        for (int q = 0; q < 4; q++)
            if (beta[4 * l + q] >= P || sibling[4 * l + q] >= P || ro[4 * l + q] >= P || (!has_ro[l] && ro[4 * l + q])) return ZKHIP_ERR_INVALID;
    }
    Ext ev = ext_from_canon(ro_top);
    for (unsigned l = 0; l < n_layers; l++) {
        const unsigned log_len = log_max - l;
        const uint64_t il = index >> l;
        const Ext sib = ext_from_canon(sibling + 4 * l), b = ext_from_canon(beta + 4 * l);
        const Ext a0 = (il & 1) ? sib : ev, a1 = (il & 1) ? ev : sib;
        ext_to_canon(e0 + 4 * l, a0);
        ext_to_canon(e1 + 4 * l, a1);
        ev = fold_row((size_t)(il >> 1), log_len - 1, b, a0, a1);
        if (has_ro[l]) ev = ext_add(ev, ext_mul(ext_mul(b, b), ext_from_canon(ro + 4 * l)));
        ext_to_canon(eval + 4 * l, ev);
    }
    return ZKHIP_OK;
}

}  // namespace zk
