// Host check of the deferred partial rounds (csrc/poseidon2.hpp, p2_internal_rounds_deferred): embedded in a whole permutation
// (poseidon2_permute_deferred) it must give, word for word, what the round-wise permutation gives -- the unrolled scalar form
// poseidon2_permute, which is what poseidon2_permute_host runs in this build (-DZK_NO_HOST_AVX512: one source, no vector object).
// Prints "ok <states>" and exits 0, or prints the first differing state and exits 1.  tests/test_poseidon2_deferred_cpu.py builds
// and runs it, once more under -fsanitize=undefined,address.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poseidon2.hpp"

using zk::P;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t next_word() {  // splitmix64, reduced to [0, p)
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % P);
}

static long checked = 0;
static bool check(const uint32_t in[16], const char* what) {
    uint32_t a[16], b[16];
    memcpy(a, in, sizeof a);
    memcpy(b, in, sizeof b);
    zk::poseidon2_permute_host(a);
    zk::poseidon2_permute_deferred(b);
    checked++;
    if (memcmp(a, b, sizeof a) == 0) return true;
    printf("MISMATCH (%s)\n in  :", what);
    for (int i = 0; i < 16; i++) printf(" %08x", in[i]);
    printf("\n want:");
    for (int i = 0; i < 16; i++) printf(" %08x", a[i]);
    printf("\n got :");
    for (int i = 0; i < 16; i++) printf(" %08x", b[i]);
    printf("\n");
    return false;
}

int main(int argc, char** argv) {
    const long n_random = argc > 1 ? atol(argv[1]) : 10000;
    bool ok = true;
    uint32_t s[16];
    // the table itself: every word a residue, the constants' slots hold rc - p
    for (int r = 0; r < 13; r++) {
        const int o = r * 16 + r * (r - 1) / 2;
        ok &= zk::Poseidon2DeferredConsts::T.v[o] + P == zk::Poseidon2Consts::RC[64 + r];
        for (int k = 1; k < 16 + r; k++) ok &= zk::Poseidon2DeferredConsts::T.v[o + k] < P;
    }
    for (int k = zk::P2D_FINAL_OFF; k < zk::P2D_WORDS; k++) ok &= zk::Poseidon2DeferredConsts::T.v[k] < P;
    if (!ok) return printf("MISMATCH (table range)\n"), 1;

    memset(s, 0, sizeof s);
    ok &= check(s, "all zero");
    for (int i = 0; i < 16; i++) s[i] = P - 1;
    ok &= check(s, "all p-1");
    for (int l = 0; l < 16; l++) {
        memset(s, 0, sizeof s);
        s[l] = P - 1;
        ok &= check(s, "one lane p-1");
    }
    for (int par = 0; par < 2; par++) {
        for (int i = 0; i < 16; i++) s[i] = ((i + par) & 1) ? P - 1 : 0;
        ok &= check(s, "alternating 0 / p-1");
    }
    const uint32_t special[] = {1u, (P - 1) / 2, (P + 1) / 2, 1u << 27, (uint32_t)((1ull << 31) % P), 0u, P - 1};
    const int n_special = sizeof special / sizeof special[0];
    for (int v = 0; v < 5; v++) {
        for (int i = 0; i < 16; i++) s[i] = special[v];
        ok &= check(s, "every lane one special value");
        for (int l = 0; l < 16; l++) {
            memset(s, 0, sizeof s);
            s[l] = special[v];
            ok &= check(s, "one lane special, rest 0");
            for (int i = 0; i < 16; i++) s[i] = i == l ? special[v] : P - 1;
            ok &= check(s, "one lane special, rest p-1");
        }
    }
    for (int rot = 0; rot < n_special; rot++) {
        for (int i = 0; i < 16; i++) s[i] = special[(i + rot) % n_special];
        ok &= check(s, "special values mixed");
    }
    for (long k = 0; k < n_random && ok; k++) {
        for (int i = 0; i < 16; i++) s[i] = next_word();
        if (k % 7 == 3) s[next_word() % 16] = special[next_word() % n_special];
        ok &= check(s, "random");
    }
    if (!ok) return 1;
    printf("ok %ld\n", checked);
    return 0;
}
