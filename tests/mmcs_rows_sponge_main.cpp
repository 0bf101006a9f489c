// The host sponge on its own (zkvm-prover_amd/csrc/hash_slice_host.hpp: zkhip_hash_slice_host's body), for a sanitizer build:
// tests/test_mmcs_rows_cpu.py compiles this with -fsanitize=address,undefined -DZK_NO_HOST_AVX512 and compares what it prints with the
// oracle.  Words: seeded, with 0 and p - 1 among them; the buffers are heap blocks of exactly `len` words, so a read past the last
// partial block would be seen.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../zkvm-prover_amd/csrc/hash_slice_host.hpp"

int main() {
    const size_t lens[] = {0, 1, 7, 8, 9, 16, 17, 438};
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (size_t len : lens) {
        uint32_t* in = len ? (uint32_t*)std::malloc(len * 4) : nullptr;
        for (size_t i = 0; i < len; i++) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            in[i] = i % 5 == 0 ? 0u : i % 5 == 1 ? zk::P - 1u : (uint32_t)((seed >> 33) % zk::P);
        }
        uint32_t out[8];
        if (zk::hash_slice_canonical(in, len, out) != ZKHIP_OK) return 1;
        std::printf("%zu", len);
        for (size_t i = 0; i < len; i++) std::printf(" %u", in[i]);
        std::printf(" :");
        for (int k = 0; k < 8; k++) std::printf(" %u", out[k]);
        std::printf("\n");
        if (len) {
            in[len - 1] = zk::P;   // refused, and nothing written
            uint32_t keep[8] = {1, 2, 3, 4, 5, 6, 7, 8};
            if (zk::hash_slice_canonical(in, len, keep) != ZKHIP_ERR_INVALID || keep[0] != 1 || keep[7] != 8) return 2;
        }
        std::free(in);
    }
    return 0;
}
