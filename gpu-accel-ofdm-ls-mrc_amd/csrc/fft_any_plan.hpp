// fft_any_plan.hpp -- the host side of fft_any.hip: the radix plan of an FFT
// length C in [2, 8192], its magic-number divisors and the LDS variant that
// takes it.  No HIP header: the host compiler reads this file alone
// (tests/cpp/fft_any_plan_table.cpp prints the plan of every length and
// tests/test_any_c_plan_cpu.py holds it to the rule stated above make_plan).
#pragma once

namespace ofdm {
namespace fany {

constexpr int MAX_STAGES = 16;
constexpr int PLAN_MAX_C = 8192;  // fft_any.hip asserts that this is FFT_ANY_MAX

// n / d for n < 2^24 as (umulhi(n, m) + n) >> l (round-up magic numbers,
// computed on the host: the stages divide by runtime sizes per butterfly)
struct FDiv {
    unsigned m, l;
};
inline FDiv make_fdiv(unsigned d) {
    const unsigned l = d > 1 ? 32 - __builtin_clz(d - 1) : 0;
    return FDiv{(unsigned)((((1ull << 32) * ((1ull << l) - d)) / d) + 1), l};
}

// flat arrays (read by a runtime stage index straight from the kernel
// arguments; an array of structs would be copied to scratch)
struct Plan {
    int C, G, ns;
    FDiv dC;
    int p[MAX_STAGES];
    unsigned m[3][MAX_STAGES], l[3][MAX_STAGES];
};

// LDS capacity (complex elements per buffer) of the variant that takes C
// and its threads per workgroup
constexpr int cap_of(int C) { return C <= 2048 ? 2048 : C <= 4096 ? 4096 : 8192; }
constexpr int nt_of(int cap) { return cap <= 4096 ? 256 : 512; }

// Radices in stage order: primes above 8 first (their direct stages are
// the slowest; never the fused last stage), then 8s, 7, 5, 4, 3, 2 -- the
// smallest last, so that the fused last stage of k_mrc_any has the most
// butterflies (C / p_last) to spread over the threads; a pure power of 8
// ends in 4 x 2 instead of 8 for the same reason.
inline bool make_plan(int C, Plan &pl) {
    if (C < 2 || C > PLAN_MAX_C) return false;
    pl.C = C;
    pl.G = cap_of(C) / C;
    pl.ns = 0;
    pl.dC = make_fdiv((unsigned)C);
    int f[32], nf = 0, n = C;
    int c2 = 0, c3 = 0, c5 = 0, c7 = 0;
    while (n % 2 == 0) { n /= 2; ++c2; }
    while (n % 3 == 0) { n /= 3; ++c3; }
    while (n % 5 == 0) { n /= 5; ++c5; }
    while (n % 7 == 0) { n /= 7; ++c7; }
    int big[16], nbig = 0;  // prime factors above 7
    for (int p = 11; n > 1; p += 2) {
        if (p * p > n) p = n;
        while (n % p == 0) {
            if (nbig == 16) return false;
            big[nbig++] = p;
            n /= p;
        }
    }
    for (int i = 0; i < nbig; ++i) f[nf++] = big[i];
    int tail2 = 0;  // radices 4 / 2 that follow the 8s
    if (c2 % 3 == 0 && c2 > 0 && c3 + c5 + c7 == 0) {  // pure power of 8 beside primes > 8 only
        for (int i = 0; i < c2 / 3 - 1; ++i) f[nf++] = 8;
        tail2 = 3;
    } else {
        for (int i = 0; i < c2 / 3; ++i) f[nf++] = 8;
        tail2 = c2 % 3;
    }
    for (int i = 0; i < c7; ++i) f[nf++] = 7;
    for (int i = 0; i < c5; ++i) f[nf++] = 5;
    if (tail2 == 2) f[nf++] = 4;
    if (tail2 == 3) f[nf++] = 4;
    for (int i = 0; i < c3; ++i) f[nf++] = 3;
    if (tail2 == 1 || tail2 == 3) f[nf++] = 2;
    if (nf > MAX_STAGES) return false;
    int Lp = 1;
    for (int i = 0; i < nf; ++i) {
        const int p = f[i];
        const FDiv d[3] = {make_fdiv((unsigned)(C / p)), make_fdiv((unsigned)Lp), make_fdiv((unsigned)(Lp * p))};
        for (int k = 0; k < 3; ++k) {
            pl.m[k][pl.ns] = d[k].m;
            pl.l[k][pl.ns] = d[k].l;
        }
        pl.p[pl.ns++] = p;
        Lp *= p;
    }
    return true;
}

}  // namespace fany
}  // namespace ofdm
