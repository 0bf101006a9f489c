// host_challenger.hpp -- the duplex challenger on the host (Montgomery words), what the host verifiers replay a proof's transcript
// with (csrc/verifier.hip, csrc/logup_gkr.hip).  The same sponge as the device transcript (csrc/transcript.hip).
#pragma once
#include <string.h>

#include "poseidon2.hpp"

namespace zk {

struct HostChallenger {
    uint32_t state[16];
    uint32_t in_buf[8], out_buf[8];
    unsigned n_in = 0, n_out = 0;
    HostChallenger() { memset(state, 0, sizeof state); }
    void duplex() {
        for (unsigned i = 0; i < n_in; i++) state[i] = in_buf[i];
        n_in = 0;
        poseidon2_permute_host(state);
        memcpy(out_buf, state, sizeof out_buf);
        n_out = 8;
    }
    void observe(uint32_t v_monty) {
        n_out = 0;
        in_buf[n_in++] = v_monty;
        if (n_in == 8) duplex();
    }
    void observe_canon(const uint32_t* v, size_t n) {
        for (size_t i = 0; i < n; i++) observe(to_monty(v[i]));
    }
    uint32_t sample() {
        if (n_in != 0 || n_out == 0) duplex();
        return out_buf[--n_out];
    }
    Ext sample_ext() {
        Ext e;
        for (int i = 0; i < 4; i++) e.c[i] = sample();
        return e;
    }
    uint32_t sample_bits(unsigned bits) { return from_monty(sample()) & (uint32_t)(((uint64_t)1 << bits) - 1); }
    bool check_witness(unsigned bits, uint32_t w_canon) {
        observe(to_monty(w_canon));
        return sample_bits(bits) == 0;
    }
};

// the field helpers every host verifier shares (csrc/verifier.hip)
Ext ext_from_canon(const uint32_t* p);                 // 4 canonical words -> Montgomery
void ext_to_canon(uint32_t* out, const Ext& e);         // Montgomery -> 4 canonical words
Ext poly_at(const Ext* s, unsigned d, const Ext& x);   // the polynomial of degree <= d through (j, s[j]), j = 0..d, at x
Ext eq_eval(const Ext* p, const Ext* x, size_t n);      // eq(p, x) = prod_j (p_j x_j + (1 - p_j)(1 - x_j))
// p3-fri `fold_row` for arity 2: pair k of a bit-reversed layer of 2^(log_n_out+1) values folded at beta
Ext fold_row(size_t k, unsigned log_n_out, const Ext& beta, const Ext& e0, const Ext& e1);

}  // namespace zk
