// The host fold loop on its own (zkvm-prover_amd/csrc/fri_query_host.hpp: zkhip_fri_query_host's body, with the verifier whose fold_row it
// calls), for a sanitizer build: tests/test_fri_query_cpu.py compiles this with -fsanitize=address,undefined -DZK_NO_HOST_AVX512 and
// compares what it prints with the twin.  Every buffer is a heap block of exactly the size the function may touch, so a read or write past
// a call's last layer would be seen.  Output: one line per case, `index log_max n | beta.. | sibling.. | has_ro.. | ro.. | ro_top | e0.. |
// e1.. | eval..`.
#include <cstdio>
#include <cstdlib>

#include "../zkvm-prover_amd/csrc/fri_query_host.hpp"
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
    const struct { uint64_t index; unsigned log_max, n; } cases[] = {{0, 2, 1}, {3, 2, 1}, {5, 3, 2}, {(1ull << 27) - 1, 27, 26}, {0, 27, 26}, {0x2A5A5A5, 27, 13}, {77, 7, 6}};
    for (const auto& c : cases) {
        const size_t n = c.n;
        uint32_t *beta = (uint32_t*)std::malloc(16 * n), *sib = (uint32_t*)std::malloc(16 * n), *has = (uint32_t*)std::malloc(4 * n), *ro = (uint32_t*)std::malloc(16 * n),
                 *top = (uint32_t*)std::malloc(16), *e0 = (uint32_t*)std::malloc(16 * n), *e1 = (uint32_t*)std::malloc(16 * n), *ev = (uint32_t*)std::malloc(16 * n);
        for (size_t i = 0; i < 4 * n; i++) beta[i] = word((unsigned)i), sib[i] = word((unsigned)i + 3);
        for (size_t l = 0; l < n; l++) {
            has[l] = (uint32_t)((l + c.index) & 1);
            for (int q = 0; q < 4; q++) ro[4 * l + q] = has[l] ? word((unsigned)(4 * l + q) + 5) : 0u;
        }
        for (int q = 0; q < 4; q++) top[q] = word((unsigned)q + 1);
        if (zk::fri_query_canonical(c.index, c.log_max, c.n, beta, sib, has, ro, top, e0, e1, ev) != ZKHIP_OK) return 1;
        std::printf("%llu %u %u", (unsigned long long)c.index, c.log_max, c.n);
        put("|", beta, 4 * n), put("|", sib, 4 * n), put("|", has, n), put("|", ro, 4 * n), put("|", top, 4), put("|", e0, 4 * n), put("|", e1, 4 * n), put("|", ev, 4 * n);
        std::printf("\n");
        // refused, and nothing written: a word equal to p in the last layer; one layer too many
        const uint32_t keep = ev[4 * n - 1];
        sib[4 * n - 1] = zk::P;
        if (zk::fri_query_canonical(c.index, c.log_max, c.n, beta, sib, has, ro, top, e0, e1, ev) != ZKHIP_ERR_INVALID || ev[4 * n - 1] != keep) return 2;
        sib[4 * n - 1] = 0;
        if (zk::fri_query_canonical(c.index, c.n, c.n, beta, sib, has, ro, top, e0, e1, ev) != ZKHIP_ERR_INVALID || ev[4 * n - 1] != keep) return 3;
        // (a count at which n_layers + 1 wraps: refused before any of the exact-size blocks is read)
        if (zk::fri_query_canonical(c.index >> 1, c.log_max, 0xFFFFFFFFu, beta, sib, has, ro, top, e0, e1, ev) != ZKHIP_ERR_INVALID || ev[4 * n - 1] != keep) return 4;
        std::free(beta), std::free(sib), std::free(has), std::free(ro), std::free(top), std::free(e0), std::free(e1), std::free(ev);
    }
    return 0;
}
