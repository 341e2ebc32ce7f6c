// tx_driver.cpp -- the reference's transmit calls (modRefSymbol, modOneSymbol;
// cpuLS.hpp:466-529) written against this package's cpuLS.hpp.  The prefix
// length is the ring header's `prefix` macro (-Dprefix=N).
//   tx_driver cols users [rows]
//     reads  Pilots.dat (modRefSymbol's file), X.bin (users x (cols-1)) and,
//            with rows > 0, W.bin (the zero-forcing matrix, reference layout)
//     writes REF.bin  (cols + prefix samples), REFX.bin (cols-1 rotated pilots),
//            ONE.bin  (users x (cols + prefix): modOneSymbol, chanMultiply = false),
//            ZF.bin   (rows x (cols + prefix): chanMultiply = true; rows > 0 only)
#include <cstdio>
#include <vector>

#include "cpuLS.hpp"

static std::vector<complexF> load(const char *path, size_t n) {
    std::vector<complexF> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(complexF), n, f) != n) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}
static void store(const char *path, const std::vector<complexF> &v) {
    FILE *f = std::fopen(path, "wb");
    std::fwrite(v.data(), sizeof(complexF), v.size(), f);
    std::fclose(f);
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int cols = std::atoi(argv[1]), users = std::atoi(argv[2]), rows = argc > 3 ? std::atoi(argv[3]) : 0;
    const size_t K = cols - 1, Cp = cols + prefix;
    std::vector<complexF> ref(Cp), refX(K);
    modRefSymbol(ref.data(), refX.data(), cols);
    store("REF.bin", ref);
    store("REFX.bin", refX);
    std::vector<complexF> X = load("X.bin", (size_t)users * K), one((size_t)users * Cp);
    modOneSymbol(one.data(), nullptr, X.data(), users, cols, users);
    store("ONE.bin", one);
    if (rows > 0) {
        std::vector<complexF> W = load("W.bin", (size_t)users * rows * K), zf((size_t)rows * Cp);
        modOneSymbol(zf.data(), W.data(), X.data(), rows, cols, users, true);
        store("ZF.bin", zf);
    }
    return 0;
}
