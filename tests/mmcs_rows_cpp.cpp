// Builds air.mmcs_rows_air() with the C++ builder (include/zkhip_chips.hpp mmcs_rows_air), without and with the values bus, and prints the
// programs; tests/test_mmcs_rows_cpu.py compares them word for word with the Python builder's.
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
    { AirBuilder b(56, 0); zkhip::chips::mmcs_rows_air(b, 11, 10); dump("mmcs_rows", b); }
    { AirBuilder b(56, 0); zkhip::chips::mmcs_rows_air(b, 11, 10, 12); dump("mmcs_rows_values", b); }
    return 0;
}
