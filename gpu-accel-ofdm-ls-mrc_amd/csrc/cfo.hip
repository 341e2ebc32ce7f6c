// cfo.hip -- carrier frequency offset (CFO): the cyclic-prefix estimator and
// the stand-alone derotator (include/ofdm_lsmrc.h, "carrier frequency offset").
//
// The reference's receive driver runs the radios on free-running oscillators
// unless told otherwise (rx_and_corr.cpp:116, --ref defaults to "internal"),
// and a frame is one pilot followed by data symbols combined against that one
// estimate: an offset of eps subcarrier spacings turns every later symbol by
// a further 2 pi eps (C + cp) / C.
//
// Convention (every CFO entry): eps is in subcarrier spacings, cycles per C
// samples.  A received frame is y[m] = x[m] e^{+2 pi i eps m / C}, m = s (C +
// cp) + i counting the frame's samples per antenna row from the first prefix
// sample of symbol 0, i in [0, C + cp).  Every frame has its own eps.  The
// correction is x'[f,s,r,i] = y[f,s,r,i] e^{-2 pi i eps_f m / C}; a non-finite
// eps_f acts as 0.
//
//   k_cfo_estimate  gamma_f = sum_s sum_r sum_{i = cp_skip .. cp-1}
//                   conj(y[f,s,r,i]) y[f,s,r,i+C];  eps_f = arg(gamma_f) / 2 pi
//                   in (-0.5, 0.5], 0 for gamma = 0.  One workgroup per frame
//                   reads the first and last cp samples of each row only; every
//                   thread sums its terms in float64 in a fixed order and the
//                   1024 partials meet in a fixed tree through LDS: no atomics,
//                   bit-identical from run to run, and the 465 408 terms of a
//                   101 x 64 x 72 frame lose nothing an f32 result could show.
//   k_cfo_derotate  x' for whole rows, prefix included, in place or out of
//                   place.  The phase at a row's start reaches hundreds of
//                   turns: it is reduced modulo one turn in float64, once per
//                   row; only the in-row part (under two turns) is formed in
//                   f32, through a range-reducing sincospi.  16-B nontemporal
//                   accesses on the 16-B aligned pairs of a row (rows are only
//                   8-B aligned when C + cp is odd: a leading / trailing sample
//                   goes alone).
// The fused C = 1024 receiver with the rotation in is frame_td.hip's
// (k_ls_td1024 / k_mrc_td1024_hlds under src_cfo); this derotator is the route for
// every other C.
#include "common.hpp"
#include "launch.hpp"

namespace ofdm {
namespace cfo {

typedef float f4v __attribute__((ext_vector_type(4)));
constexpr int EST_THREADS = 1024;
constexpr int ROT_THREADS = 256;

__device__ __forceinline__ float finite_or_zero(float e) {
    return (__builtin_bit_cast(unsigned, e) & 0x7f800000u) == 0x7f800000u ? 0.f : e;
}
// e^{2 pi i x}, x in turns (sincospi reduces the range exactly)
__device__ __forceinline__ float2 cis_turns(float x) {
    float sn, cs;
    sincospif(2.f * x, &sn, &cs);
    return float2{cs, sn};
}

// lw = log2 of the lanes across a row's prefix window (a power of two >= cp -
// cp_skip, at most EST_THREADS): thread (row slot rs, lane li) takes rows rs,
// rs + EST_THREADS >> lw, ... and samples cp_skip + li, + (1 << lw), ...
__global__ void __launch_bounds__(EST_THREADS) k_cfo_estimate(const float2 *__restrict__ iq, long long rows, int C,
                                                              int cp, int cp_skip, int lw,
                                                              float2 *__restrict__ gamma, float *__restrict__ eps) {
    __shared__ double sre[EST_THREADS], sim[EST_THREADS];
    const long long f = blockIdx.x;
    const int Cp = C + cp;
    const float2 *frame = iq + f * rows * Cp;
    const int li = threadIdx.x & ((1 << lw) - 1), rs = threadIdx.x >> lw;
    const int W = 1 << lw, RPP = EST_THREADS >> lw;
    double re = 0.0, im = 0.0;
    for (long long r = rs; r < rows; r += RPP) {
        const float2 *row = frame + r * Cp;
        for (int i = cp_skip + li; i < cp; i += W) {
            const float2 a = row[i], b = row[i + C];
            // conj(a) b
            re += (double)a.x * (double)b.x + (double)a.y * (double)b.y;
            im += (double)a.x * (double)b.y - (double)a.y * (double)b.x;
        }
    }
    sre[threadIdx.x] = re;
    sim[threadIdx.x] = im;
    __syncthreads();
    for (int n = EST_THREADS / 2; n > 0; n >>= 1) {
        if ((int)threadIdx.x < n) {
            sre[threadIdx.x] += sre[threadIdx.x + n];
            sim[threadIdx.x] += sim[threadIdx.x + n];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double gr = sre[0], gi = sim[0];
        if (gamma) gamma[f] = float2{(float)gr, (float)gi};
        double e = atan2(gi, gr) * 0.15915494309189535;  // / 2 pi; atan2(0, 0) = 0
        if (e <= -0.5) e = 0.5;                          // (-0.5, 0.5]
        eps[f] = (float)e;
    }
}

// One workgroup per row at a time (grid-stride): row = (f * S + s) * R + r.
__global__ void __launch_bounds__(ROT_THREADS) k_cfo_derotate(const float2 *in, float2 *out, long long nrows, int S,
                                                              int R, int C, int cp, const float *__restrict__ eps) {
    const int Cp = C + cp;
    const float invC = 1.f / (float)C;
    const double invCd = 1.0 / (double)C;
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const long long fs = row / R, f = fs / S;
        const int s = (int)(fs - f * S);
        const float e = finite_or_zero(eps[f]);
        // the row's start, s (C + cp) samples into the frame, modulo one turn
        const double turns = (double)e * (double)((long long)s * Cp) * invCd;
        const float ph0 = (float)(turns - __builtin_rint(turns));
        const float2 step = cis_turns(-e * invC);  // one sample on
        const long long g0 = row * Cp;             // the row's first sample in the buffer
        const float2 *src = in + g0;
        float2 *dst = out + g0;
        auto w = [&](int i) { return cis_turns(-(ph0 + e * (float)i * invC)); };
        const int head = (int)(g0 & 1);  // an odd start: sample 0 is the upper half of a 16-B word
        const int npair = (Cp - head) >> 1;
        if (threadIdx.x == 0) {
            if (head) dst[0] = cmul(src[0], w(0));
            const int last = head + 2 * npair;
            if (last < Cp) dst[last] = cmul(src[last], w(last));
        }
        const f4v *src4 = reinterpret_cast<const f4v *>(src + head);
        f4v *dst4 = reinterpret_cast<f4v *>(dst + head);
        for (int p = threadIdx.x; p < npair; p += ROT_THREADS) {
            const f4v v = __builtin_nontemporal_load(src4 + p);
            const float2 w0 = w(head + 2 * p), w1 = cmul(w0, step);
            const float2 a = cmul(float2{v.x, v.y}, w0), b = cmul(float2{v.z, v.w}, w1);
            __builtin_nontemporal_store(f4v{a.x, a.y, b.x, b.y}, dst4 + p);
        }
    }
}

}  // namespace cfo

hipError_t launch_cfo_estimate(const float2 *iq, long long nframes, int S, int R, int C, int cp, int cp_skip,
                               float2 *gamma, float *eps, hipStream_t s) {
    using namespace cfo;
    if (nframes <= 0) return hipSuccess;
    int lw = 0;
    while ((1 << lw) < cp - cp_skip && (1 << lw) < EST_THREADS) ++lw;
    const long long rows = (long long)S * R;
    for (long long f0 = 0; f0 < nframes; f0 += 0x7fffffffll) {  // one launch but for absurd batches
        const long long n = nframes - f0 < 0x7fffffffll ? nframes - f0 : 0x7fffffffll;
        hipLaunchKernelGGL(k_cfo_estimate, dim3((unsigned)n), dim3(EST_THREADS), 0, s,
                           iq + f0 * rows * (C + cp), rows, C, cp, cp_skip, lw, gamma ? gamma + f0 : nullptr, eps + f0);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_cfo_derotate(const float2 *in, float2 *out, long long nframes, int S, int R, int C, int cp,
                               const float *eps, hipStream_t s) {
    using namespace cfo;
    const long long nrows = nframes * S * R;
    if (nrows <= 0) return hipSuccess;
    // enough workgroups to fill the GPU several times over, each looping over rows
    const unsigned grid = (unsigned)(nrows < 16384 ? nrows : 16384);
    hipLaunchKernelGGL(k_cfo_derotate, dim3(grid), dim3(ROT_THREADS), 0, s, in, out, nrows, S, R, C, cp, eps);
    return hipGetLastError();
}

}  // namespace ofdm
