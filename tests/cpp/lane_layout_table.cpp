// Prints lane_layout.hpp's position table for every FFT size whose workspace
// estimate is lane-ordered, one line per size: "C hc_pos(C, 0) ... hc_pos(C, C - 1)"
// (tests/test_lane_layout_cpu.py compares them with a forward enumeration).
#include <cstdio>

#include "lane_layout.hpp"

int main() {
    const int sizes[] = {128, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144};
    for (int C : sizes) {
        std::printf("%d", C);
        for (int b = 0; b < C; ++b) std::printf(" %d", ofdm::lane::hc_pos(C, b));
        std::printf("\n");
    }
    return 0;
}
