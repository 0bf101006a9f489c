// Builds air.reduced_opening_air() with the C++ builder (include/zkhip_chips.hpp reduced_opening_air), without and with the result bus, and
// prints the programs; tests/test_reduced_opening_cpu.py compares them word for word with the Python builder's.
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
    { AirBuilder b(18, 0); zkhip::chips::reduced_opening_air(b); dump("reduced_opening", b); }
    { AirBuilder b(18, 0); zkhip::chips::reduced_opening_air(b, 12); dump("reduced_opening_bus", b); }
    return 0;
}
