// Builds air.fri_query_air() with the C++ builder (include/zkhip_chips.hpp fri_query_air), without and with the two optional buses, and
// prints the programs; tests/test_fri_query_cpu.py compares them word for word with the Python builder's.
#include <cstdio>

#include "zkhip_air.hpp"
#include "zkhip_chips.hpp"

using namespace zkhip::air;

static void dump(const char* name, AirBuilder& b) {
    const std::vector<uint32_t> w = b.program();
    std::printf("%s %u", name, b.max_degree());
    for (uint32_t x : w) std::printf(" %u", x);
    std::printf("\n");
}

int main() {
    { AirBuilder b(61, 0); zkhip::chips::fri_query_air(b, 14, 11, 10, 15); dump("fri_query", b); }
    { AirBuilder b(61, 0); zkhip::chips::fri_query_air(b, 14, 11, 10, 15, 16, 17); dump("fri_query_all", b); }
    { AirBuilder b(61, 0); zkhip::chips::fri_query_air(b, 14, 11, 10, 15, -1, 17); dump("fri_query_final", b); }
    return 0;
}
