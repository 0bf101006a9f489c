// fri_final_host.hpp -- zkhip_fri_final_host's body: a query's last check of the host verifier (verifier.hip, the lines behind the
// `for l < n_layers` block of verify_where) on canonical words: the point xf = g_lvl^bitrev(k, lvl) of the last domain, lvl = log_blowup +
// log_final_poly_len and k = idx >> n_layers there, and Horner over the final polynomial's coefficients at it.  Written with the verifier's
// own field helpers (two_adic_generator, bitrev32, mpow, ext_mul_base); the comparison with the fold loop's value is the caller's (the chip
// receives that value on a bus: air.py fri_final_air).  Plain C++ on the host: tests/fri_final_host_main.cpp compiles it on its own, together
// with verifier.hip, under the sanitizers.
#pragma once
#include "../../include/zkhip.h"
#include "host_challenger.hpp"

namespace zk {

inline int fri_final_canonical(unsigned log_final_poly_len, unsigned lvl, uint64_t k, const uint32_t* coef, uint32_t* x_out, uint32_t* value_out) {
    if (!coef || !x_out || !value_out) return ZKHIP_ERR_INVALID;
    if (log_final_poly_len > ZKHIP_MAX_LOG_FINAL_POLY || lvl == 0 || lvl > 26 || (k >> lvl)) return ZKHIP_ERR_INVALID;
    const size_t n_fin = (size_t)1 << log_final_poly_len;
    for (size_t i = 0; i < 4 * n_fin; i++)
        if (coef[i] >= P) return ZKHIP_ERR_INVALID;
    // (the verifier skips the point when there is one coefficient; here it is an output, so it is always computed)
    const uint32_t xf = mpow(two_adic_generator(lvl), bitrev32((uint32_t)k, lvl));
    Ext want = ext_from_canon(coef + 4 * (n_fin - 1));
    for (size_t j = n_fin - 1; j-- > 0;) want = ext_add(ext_mul_base(want, xf), ext_from_canon(coef + 4 * j));
    x_out[0] = from_monty(xf);
    ext_to_canon(value_out, want);
    return ZKHIP_OK;
}

}  // namespace zk
