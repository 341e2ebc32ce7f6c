/*
 * tx_ref_standins.hpp -- force-included in front of the transmit functions
 * that tests/test_tx_ref_cpu.py extracts from the reference's cpuLS.hpp
 * (ifftShiftOneRow, ifftOneRow, addPrefix, matrix_readX,
 * multiplyWithChannelInv, modRefSymbol, modOneSymbol), read where they lie.
 *
 * TEST INFRASTRUCTURE ONLY.  complexF and the `prefix` macro come from the
 * reference's own ShMemSymBuff.hpp (found via -I, prefix set with -Dprefix=N).
 * The libraries those functions call are absent from the image; this file
 * holds the project's own stand-ins for exactly the entry points they use:
 *   fftwf_plan_dft_1d / fftwf_execute / fftwf_destroy_plan: a direct DFT of
 *       any length in float64, rounded once to float.  (A real FFTW_MEASURE
 *       plan may overwrite the arrays while it plans; this one does not.)
 *   clange_ for norm 'M': max |a(i, j)|;  cblas_csscal: x *= alpha;
 *   cblas_cgemm, cblas_cgemv, cgetrf_, cgetri_: abort -- the zero-forcing
 *       branch (chanMultiply = true) is not driven here.
 */
#include "ShMemSymBuff.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>
using namespace std;
static const char *g_tx_pilot_path = "Pilots.dat";
#define fileNameForX g_tx_pilot_path

typedef float fftwf_complex[2];
struct tx_fftw_plan {
    int n, sign;
    fftwf_complex *in, *out;
};
typedef tx_fftw_plan *fftwf_plan;
#define FFTW_FORWARD (-1)
#define FFTW_BACKWARD (+1)
#define FFTW_MEASURE 0u
#define FFTW_ESTIMATE 64u

static fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex *in, fftwf_complex *out, int sign, unsigned) {
    return new tx_fftw_plan{n, sign, in, out};
}
static void fftwf_execute(const fftwf_plan p) {
    const int n = p->n;
    const double pi = 3.14159265358979323846;
    std::vector<double> c(n), s(n), re(n), im(n);
    for (int k = 0; k < n; ++k) {
        c[k] = std::cos(2.0 * pi * k / n);
        s[k] = p->sign * std::sin(2.0 * pi * k / n);
        re[k] = p->in[k][0];
        im[k] = p->in[k][1];
    }
    for (int o = 0; o < n; ++o) {
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < n; ++k) {
            if (re[k] == 0.0 && im[k] == 0.0) continue;  // empty bins (a unit impulse is one term)
            const int e = (int)(((long long)o * k) % n);
            ar += re[k] * c[e] - im[k] * s[e];
            ai += re[k] * s[e] + im[k] * c[e];
        }
        p->out[o][0] = (float)ar;
        p->out[o][1] = (float)ai;
    }
}
static void fftwf_destroy_plan(fftwf_plan p) { delete p; }

[[noreturn]] static void tx_absent(const char *what) {
    std::fprintf(stderr, "tx_ref_standins: %s is not provided\n", what);
    std::abort();
}
enum { CblasColMajor = 102, CblasNoTrans = 111, CblasConjTrans = 113 };
extern "C" {
static float clange_(char *norm, int *m, int *n, complexF *A, int *lda, float *) {
    if (*norm != 'M') tx_absent("clange_ for a norm other than 'M'");
    float best = 0.f;
    for (int j = 0; j < *n; ++j)
        for (int i = 0; i < *m; ++i) {
            const float v = hypotf(A[(size_t)j * *lda + i].real, A[(size_t)j * *lda + i].imag);
            if (v > best || v != v) best = v;
        }
    return best;
}
static void cblas_csscal(int n, float alpha, float *x, int incx) {
    for (int i = 0; i < n; ++i) {
        x[2 * (size_t)i * incx] *= alpha;
        x[2 * (size_t)i * incx + 1] *= alpha;
    }
}
static void cblas_cgemv(int, int, int, int, const void *, const void *, int, const void *, int, const void *, void *,
                        int) {
    tx_absent("cblas_cgemv");
}
static void cblas_cgemm(int, int, int, int, int, int, const void *, const void *, int, const void *, int,
                        const void *, void *, int) {
    tx_absent("cblas_cgemm");
}
static void cgetrf_(int *, int *, complexF *, int *, int *, int *) { tx_absent("cgetrf_"); }
static void cgetri_(int *, complexF *, int *, int *, complexF *, int *, int *) { tx_absent("cgetri_"); }
}
