// Builds air.fri_final_air() with the C++ builder (include/zkhip_chips.hpp fri_final_air) at log_final_poly_len 0, 3 and 8 and, with the
// optional coefficient bus, at 2, and prints the programs; tests/test_fri_final_cpu.py compares them word for word with the Python builder's.
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
    { AirBuilder b(19, 0); zkhip::chips::fri_final_air(b, 0, 14, 17); dump("fri_final_0", b); }
    { AirBuilder b(19, 0); zkhip::chips::fri_final_air(b, 3, 14, 17); dump("fri_final_3", b); }
    { AirBuilder b(19, 0); zkhip::chips::fri_final_air(b, 8, 14, 17); dump("fri_final_8", b); }
    { AirBuilder b(19, 0); zkhip::chips::fri_final_air(b, 2, 14, 17, 18); dump("fri_final_2_coeff", b); }
    return 0;
}
