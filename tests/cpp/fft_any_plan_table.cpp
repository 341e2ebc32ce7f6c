// Prints fft_any_plan.hpp's plan of every FFT length, one line per C in
// 2 ... 8192 behind a header line "MAX_STAGES n":
//   "C CAP NT G ns | p_0 ... p_{ns-1} | m l (cp) m l (Lp) m l (L) per stage ... | m l (dC)"
// (tests/test_any_c_plan_cpu.py holds the lines to tests/any_c_cases.py).
// With the argument "fdiv" it checks the device's division
//   n / d = ((uint32_t)(((uint64_t)n * m) >> 32) + n) >> l
// in the host's arithmetic for every divisor d in 1 ... 8192 with make_fdiv(d):
// every n < 16384 (twice the largest LDS index a kernel forms), the last
// multiple of d below 2^24 and the number before it (the bound the header
// states), and prints "mismatches N".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "fft_any_plan.hpp"

using namespace ofdm::fany;

static uint32_t fdiv_host(uint32_t n, FDiv f) { return ((uint32_t)(((uint64_t)n * f.m) >> 32) + n) >> f.l; }

static int check_fdiv() {
    long long bad = 0;
    for (uint32_t d = 1; d <= (uint32_t)PLAN_MAX_C; ++d) {
        const FDiv f = make_fdiv(d);
        for (uint32_t n = 0; n < 16384; ++n) bad += fdiv_host(n, f) != n / d;
        const uint32_t top = ((1u << 24) - 1) / d * d;  // the last multiple of d below 2^24
        bad += fdiv_host(top, f) != top / d;
        bad += fdiv_host(top - 1, f) != (top - 1) / d;
    }
    std::printf("mismatches %lld\n", bad);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "fdiv") == 0) return check_fdiv();
    std::printf("MAX_STAGES %d\n", MAX_STAGES);
    for (int C = 2; C <= PLAN_MAX_C; ++C) {
        Plan pl;
        if (!make_plan(C, pl)) {
            std::printf("%d refused\n", C);
            continue;
        }
        const int cap = cap_of(C);
        std::printf("%d %d %d %d %d |", pl.C, cap, nt_of(cap), pl.G, pl.ns);
        for (int s = 0; s < pl.ns; ++s) std::printf(" %d", pl.p[s]);
        std::printf(" |");
        for (int s = 0; s < pl.ns; ++s)
            for (int k = 0; k < 3; ++k) std::printf(" %u %u", pl.m[k][s], pl.l[k][s]);
        std::printf(" | %u %u\n", pl.dC.m, pl.dC.l);
    }
    return 0;
}
