// hash_slice_host.hpp -- zkhip_hash_slice_host's body: p3's PaddingFreeSponge<_, 16, 8, 8> on canonical words.  The sponge itself is
// p2_hash_slice (poseidon2.hpp), the one loop the verifier's leaf hashing (verifier.hip verify_opening) runs as well; this only converts
// the words on the way in and out.  Plain C++ on the host: tests/mmcs_rows_sponge_main.cpp compiles it on its own under the sanitizers
// (-DZK_NO_HOST_AVX512: without csrc/poseidon2_avx512.cpp).
#pragma once
#include <vector>

#include "../../include/zkhip.h"
#include "poseidon2.hpp"

namespace zk {

inline int hash_slice_canonical(const uint32_t* in, size_t len, uint32_t out[8]) {
    if (!out || (len && !in)) return ZKHIP_ERR_INVALID;
    std::vector<uint32_t> m(len);
    for (size_t i = 0; i < len; i++) {
        if (in[i] >= P) return ZKHIP_ERR_INVALID;
        m[i] = to_monty(in[i]);
    }
    uint32_t dg[8];
    p2_hash_slice(m.data(), len, dg);
    for (int k = 0; k < 8; k++) out[k] = from_monty(dg[k]);
    return ZKHIP_OK;
}

}  // namespace zk
