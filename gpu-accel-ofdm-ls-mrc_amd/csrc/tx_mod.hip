// tx_mod.hip -- OFDM modulator (ofdm_tx_modulate): the reference's transmit
// helpers modOneSymbol / modRefSymbol (cpuLS.hpp:466-529) with
// ifftShiftOneRow (119-132), ifftOneRow (152-162), the clange_ 'M' + csscal
// peak normalisation (521-523) and addPrefix (391-398) as ONE pass per row:
// K inputs read through the inverse of the bin placement, the backward
// transform, the row's peak, the scale, and the row stored once behind its
// cyclic prefix.  HBM traffic per row: K * 8 B read, (C + cp) * 8 B written.
//
// This file holds the C = 1024 kernel (one wave per row on the wave FFT of
// wave_fft1024.hpp) and the dispatch; every other C runs k_tx_any on the
// mixed-radix stage machinery (fft_any.hip).
#include "tx_map.hpp"
#include "wave_fft1024.hpp"

namespace ofdm {
namespace txm {

using namespace td1024;

constexpr int WAVES = 8;  // rows per workgroup pass; LDS 9.0 + 8 x 8.5 KiB: two workgroups per CU

// The finished row goes through the natural-order image of wave_fft1024.hpp
// (nat_img): conflict-free writes from row_fft's output order, and an even n and
// n + 1 in one aligned 16-B word for the wide store path.

typedef float f4v __attribute__((ext_vector_type(4)));

// WIDE: rows start 16-B aligned and cp is even -- 16-B stores; else 8-B.
template <bool WIDE>
__global__ void __launch_bounds__(64 * WAVES)
k_tx_mod1024(const float2 *__restrict__ X, long long ldx, long long nrows, int cp, int map, int norm, float scale,
             float2 *__restrict__ iq, float *__restrict__ peak) {
    __shared__ __attribute__((aligned(16))) float2 tw[TWBUF];
    __shared__ __attribute__((aligned(16))) float2 Tall[WAVES * TBUF];
    fill_twiddles(tw);
    __syncthreads();
    const int t = threadIdx.x & 63;
    float2 *T = Tall + (threadIdx.x >> 6) * TBUF;
    const int Cp = C + cp;
    for (long long row = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6); row < nrows;
         row += (long long)gridDim.x * WAVES) {
        // lane t holds bins t + 64 m, re/im swapped: IFFT(x) = swap(FFT(swap(x)))
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(X + row * ldx);
        float2 a[16], x[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int k = tx_src(t + 64 * m, C, map);
            unsigned long long v = 0;
            if (k >= 0) v = __builtin_nontemporal_load(src + k);
            const float2 f = __builtin_bit_cast(float2, v);
            a[m] = float2{f.y, f.x};
        }
        row_fft(a, t, T, tw, x);  // x[k] = swap(ifft)[lane_bin0(t) + 16 k]
        float m2 = x[0].x * x[0].x + x[0].y * x[0].y;
#pragma unroll
        for (int k = 1; k < 16; ++k) m2 = tx_max(m2, x[k].x * x[k].x + x[k].y * x[k].y);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m2 = tx_max(m2, __shfl_xor(m2, d));
        const float pk = __builtin_sqrtf(m2);
        const float s = tx_gain(pk, norm, scale);
        const int b0 = lane_bin0(t);
#pragma unroll
        for (int k = 0; k < 16; ++k) T[nat_img(b0 + 16 * k)] = float2{x[k].y * s, x[k].x * s};
        wave_lds_sync();
        float2 *o = iq + row * Cp;
        if (WIDE) {  // output samples 2 i, 2 i + 1 = row samples n, n + 1, n = (2 i - cp) mod C even
            const int np = Cp >> 1;
            for (int i = t; i < np; i += 64) {
                const int n = (2 * i + C - cp) & (C - 1);
                const float4 v = *reinterpret_cast<const float4 *>(T + nat_img(n));
                __builtin_nontemporal_store(f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f4v *>(o + 2 * i));
            }
        } else {
            for (int e = t; e < Cp; e += 64) {
                const float2 v = T[nat_img((e + C - cp) & (C - 1))];
                __builtin_nontemporal_store(__builtin_bit_cast(unsigned long long, v),
                                            reinterpret_cast<unsigned long long *>(o + e));
            }
        }
        if (peak && t == 0) peak[row] = pk;
        wave_lds_sync();  // the next row's transform writes T
    }
}

int cus() {
    static const int n = [] {
        int dev = 0, v = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            v = 256;
        return v;
    }();
    return n;
}

}  // namespace txm

hipError_t launch_tx_modulate(const float2 *X, long long ldx, long long nrows, int C, int cp, int map, int norm,
                              float scale, float2 *iq, float *peak, hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    if (C != txm::C) return launch_tx_any(X, ldx, nrows, C, cp, map, norm, scale, iq, peak, s);
    const long long blocks = (nrows + txm::WAVES - 1) / txm::WAVES, res = 2ll * txm::cus();
    const unsigned grid = (unsigned)(blocks < res ? blocks : res);  // persistent: the twiddles are filled once
    // 16-B stores need every row 16-B aligned: an even row length on a 16-B aligned buffer
    const bool wide = (cp & 1) == 0 && (reinterpret_cast<uintptr_t>(iq) & 15) == 0;
    if (wide)
        hipLaunchKernelGGL((txm::k_tx_mod1024<true>), dim3(grid), dim3(64 * txm::WAVES), 0, s, X, ldx, nrows, cp, map,
                           norm, scale, iq, peak);
    else
        hipLaunchKernelGGL((txm::k_tx_mod1024<false>), dim3(grid), dim3(64 * txm::WAVES), 0, s, X, ldx, nrows, cp, map,
                           norm, scale, iq, peak);
    return hipGetLastError();
}

}  // namespace ofdm
