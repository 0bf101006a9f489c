// The host's last check of a query on its own (zkvm-prover_amd/csrc/fri_final_host.hpp: zkhip_fri_final_host's body, with the verifier whose
// field helpers it calls), for a sanitizer build: tests/test_fri_final_cpu.py compiles this with -fsanitize=address,undefined
// -DZK_NO_HOST_AVX512 and compares what it prints with the twin.  Every buffer is a heap block of exactly the size the function may touch,
// so a read past the last coefficient or a write past an output would be seen.  Output: one line per case, `lfp lvl k | coef.. | x | value`.
#include <cstdio>
#include <cstdlib>

#include "../zkvm-prover_amd/csrc/fri_final_host.hpp"
#include "../zkvm-prover_amd/csrc/verifier.hip"

static uint64_t seed = 0x9E3779B97F4A7C15ull;
static uint32_t word(unsigned i) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return i % 7 == 0 ? 0u : i % 7 == 1 ? zk::P - 1u : (uint32_t)((seed >> 33) % zk::P);
}
static void put(const char* sep, const uint32_t* v, size_t n) {
    std::printf(" %s", sep);
    for (size_t i = 0; i < n; i++) std::printf(" %u", v[i]);
}

int main() {
    const struct { unsigned lfp, lvl; uint64_t k; } cases[] = {{0, 1, 0}, {0, 1, 1}, {1, 2, 3}, {3, 12, 0xABC}, {8, 26, (1ull << 26) - 1}, {8, 9, 1}, {5, 26, 0}};
    for (const auto& c : cases) {
        const size_t n = (size_t)4 << c.lfp;
        uint32_t *coef = (uint32_t*)std::malloc(4 * n), *x = (uint32_t*)std::malloc(4), *val = (uint32_t*)std::malloc(16);
        for (size_t i = 0; i < n; i++) coef[i] = word((unsigned)i + c.lfp);
        if (zk::fri_final_canonical(c.lfp, c.lvl, c.k, coef, x, val) != ZKHIP_OK) return 1;
        std::printf("%u %u %llu", c.lfp, c.lvl, (unsigned long long)c.k);
        put("|", coef, n), put("|", x, 1), put("|", val, 4);
        std::printf("\n");
        // refused, and nothing written: the last word equal to p; k one past the domain; lvl 0 and 27; one coefficient bit too many
        const uint32_t keep_x = x[0], keep_v = val[3];
        coef[n - 1] = zk::P;
        if (zk::fri_final_canonical(c.lfp, c.lvl, c.k, coef, x, val) != ZKHIP_ERR_INVALID || x[0] != keep_x || val[3] != keep_v) return 2;
        coef[n - 1] = 0;
        if (zk::fri_final_canonical(c.lfp, c.lvl, (uint64_t)1 << c.lvl, coef, x, val) != ZKHIP_ERR_INVALID || x[0] != keep_x || val[3] != keep_v) return 3;
        if (zk::fri_final_canonical(c.lfp, 0, 0, coef, x, val) != ZKHIP_ERR_INVALID || zk::fri_final_canonical(c.lfp, 27, c.k, coef, x, val) != ZKHIP_ERR_INVALID) return 4;
        // (refused before any of the exact-size blocks is read)
        if (zk::fri_final_canonical(9, c.lvl, c.k, coef, x, val) != ZKHIP_ERR_INVALID || zk::fri_final_canonical(0xFFFFFFFFu, c.lvl, c.k, coef, x, val) != ZKHIP_ERR_INVALID) return 5;
        if (x[0] != keep_x || val[3] != keep_v) return 6;
        std::free(coef), std::free(x), std::free(val);
    }
    return 0;
}
