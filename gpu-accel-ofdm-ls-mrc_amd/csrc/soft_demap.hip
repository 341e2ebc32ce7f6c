// soft_demap.hip -- soft-decision output behind ofdm_frame_soft_demap and
// ofdm_frame_noise_estimate (no reference counterpart: the reference ends at
// the equalised symbols).
//
// Input of both kernels: the demodulated array z, flat [nframes][S-1][K] in
// the rotated order every receiver writes, and the |H|^2 sums P of the frame
// workspace, [nframes][C] by FFT bin at every C and for every estimator (the
// lane orders of the fused receivers concern Hc only).  The subcarrier at
// output position k is j = out_src(k, K) (common.hpp, odd and even K), and
// its post-combining gain is P[f*C + j + 1].
//
// Constellations: Gray-mapped, unit average energy, 3GPP TS 38.211 5.1.2-5.1.6
// (QPSK, 16-, 64-, 256-QAM; BPS = 2, 4, 6, 8 bits per symbol; a and the slicer
// are decision.hpp's, shared with the trackers).  Bit 2i comes
// from the real axis and bit 2i+1 from the imaginary axis, by the same
// per-axis function; llr > 0 <=> bit 0 more likely.  With x one axis of Z and
// a the half-distance between neighbouring points,
//
//   BPS  a           lambda_0   lambda_1           lambda_2               lambda_3
//   2    1/sqrt(2)   4a x
//   4    1/sqrt(10)  4a x       4a (2a - |x|)
//   6    1/sqrt(42)  4a x       4a (4a - |x|)      4a (2a - ||x| - 4a|)
//   8    1/sqrt(170) 4a x       4a (8a - |x|)      4a (4a - ||x| - 8a|)   4a (2a - |||x| - 8a| - 4a|)
//
// i.e. t_0 = x, t_i = 2a m_i - |t_{i-1}|, lambda_i = 4a t_i with
// m_i = 2^(BPS/2 - 1 - i); a = 0.70710678, 0.31622777, 0.15430335, 0.07669650.
// llr[2i] = scale * lambda_i(Re Z), llr[2i+1] = scale * lambda_i(Im Z),
// scale = P / noise_var[f].  This is the MAX-LOG approximation in its usual
// recursive (constant-slope) form, not the exact log-sum over the
// constellation: exact for QPSK, and for the higher orders exact max-log only
// in the decision regions next to each bit's boundary.
//
// ofdm_synth_frames' QPSK puts the POSITIVE axis where its data bit is SET
// (fft_synth.hip qpsk()), the complement of the 38.211 bit: a hard decision
// llr < 0 reads the generator's bit as 0.
//
//   k_soft_demap<BPS, OUT>  one workgroup per tile of 1024 consecutive
//       elements of the flat stream (rows of K are not 16-B aligned, the
//       stream is): two 16-B nontemporal loads per thread, the LLRs into an
//       LDS image of the tile's output bytes, then whole 16-B nontemporal
//       stores, 1 KiB contiguous per wave instruction, for every BPS and both
//       formats.  P and noise_var are gathered per element (4-B loads, L2
//       hits: one frame's P serves its S-1 symbols); one reciprocal per
//       element, none per bit.  OUT 0: float; OUT 1: signed byte
//       clamp(rint(llr * llr_scale), -127, 127), round-to-nearest-even, never
//       -128.  An element whose P or noise_var is not a positive finite
//       number gets llr = 0 (an erasure) in both formats.  A non-finite Z with
//       good P and noise_var gives its own element's LLRs by the formulas (NaN
//       from a NaN); OUT 1 stores a NaN llr as 0, an erasure too (quant8).
//   k_noise_estimate<BPS>  one workgroup per frame: the mean over the frame's
//       (s, k) of P |Z - slice(Z)|^2, slice = the nearest constellation point;
//       elements whose P is 0 or not finite are skipped (0 if none is left); a
//       non-finite Z that is not skipped makes the frame's value non-finite.
//       Each thread sums its elements in order into eight accumulators, the
//       workgroup adds them by a fixed tree in LDS: no atomics, the same bits
//       on every run.
#include "decision.hpp"
#include "launch.hpp"

namespace ofdm {

using dd::pos_finite;
using dd::qam_a;
using dd::slice_err;

constexpr int SD_TPB = 256, SD_TILE = 1024;

// the BPS/2 values lambda_i(x) * s of one axis, s4a = s * 4a
template <int BPS>
__device__ __forceinline__ void axis_llr(float x, float s4a, float (&l)[BPS / 2]) {
    constexpr float a = qam_a<BPS>();
    float t = x;
    l[0] = s4a * t;
#pragma unroll
    for (int i = 1; i < BPS / 2; ++i) {
        t = (float)(1 << (BPS / 2 - i)) * a - __builtin_fabsf(t);  // 2a m_i - |t_{i-1}|
        l[i] = s4a * t;
    }
}

// LLRs of one element, bit index fastest
template <int BPS>
__device__ __forceinline__ void elem_llr(float2 z, float p, float nvf, float (&l)[BPS]) {
    const bool ok = pos_finite(p) && pos_finite(nvf);
    const float s4a = ok ? (p * __builtin_amdgcn_rcpf(nvf)) * (4.f * qam_a<BPS>()) : 0.f;
    float re[BPS / 2], im[BPS / 2];
    axis_llr<BPS>(ok ? z.x : 0.f, s4a, re);
    axis_llr<BPS>(ok ? z.y : 0.f, s4a, im);
#pragma unroll
    for (int i = 0; i < BPS / 2; ++i) {
        l[2 * i] = re[i];
        l[2 * i + 1] = im[i];
    }
}

// A NaN LLR (a non-finite z with good P and noise_var) is an erasure, 0: the
// max / min below would return their other operand, a confident -127.
__device__ __forceinline__ unsigned quant8(float llr, float qs) {
    const float x = llr * qs;
    const float v = x == x ? __builtin_fminf(__builtin_fmaxf(x, -127.f), 127.f) : 0.f;
    return (unsigned)(int)__builtin_rintf(v) & 0xffu;
}

typedef float sd_f4 __attribute__((ext_vector_type(4)));
typedef unsigned sd_u4 __attribute__((ext_vector_type(4)));

template <int BPS, int OUT>
__global__ void __launch_bounds__(SD_TPB) k_soft_demap(const float2 *__restrict__ z, long long total, int K,
                                                       unsigned per_frame, int C, const float *__restrict__ P,
                                                       const float *__restrict__ nv, float llr_scale,
                                                       unsigned char *__restrict__ out) {
    constexpr int EB = OUT == 0 ? 4 * BPS : BPS;  // output bytes per element
    constexpr int PW = 2 * EB / 4;                // output dwords per element pair
    __shared__ __attribute__((aligned(16))) unsigned T[SD_TILE * EB / 4];
    const int tid = threadIdx.x;
    // where the tile starts: frame f0, element r0 of that frame, position k0 of its row
    const long long base = (long long)blockIdx.x * SD_TILE;
    const long long f0 = base / per_frame;
    const unsigned r0 = (unsigned)(base - f0 * per_frame);
    const unsigned k0 = r0 % (unsigned)K;
    const bool kbig = K >= SD_TILE - 1;        // k0 + o < 2 K
    const bool fbig = per_frame >= SD_TILE;    // r0 + o < 2 per_frame
    const long long left = total - base;
    const unsigned n = left < SD_TILE ? (unsigned)left : (unsigned)SD_TILE;

    float4 v[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const unsigned o = 2u * (unsigned)(it * SD_TPB + tid);
        v[it] = float4{0.f, 0.f, 0.f, 0.f};
        if (o + 1 < n) {
            const sd_f4 w = __builtin_nontemporal_load(reinterpret_cast<const sd_f4 *>(z + base + o));
            v[it] = float4{w.x, w.y, w.z, w.w};
        } else if (o < n) {
            const float2 w = z[base + o];
            v[it].x = w.x;
            v[it].y = w.y;
        }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const unsigned o = 2u * (unsigned)(it * SD_TPB + tid);
        float l[2][BPS];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned oe = o + h;
            float p = 0.f, nvf = 0.f;
            if (oe < n) {
                unsigned kk = k0 + oe;
                if (kbig) kk -= kk >= (unsigned)K ? (unsigned)K : 0u;
                else kk %= (unsigned)K;
                const unsigned r = r0 + oe;
                const unsigned df = fbig ? (r >= per_frame ? 1u : 0u) : r / per_frame;
                const long long f = f0 + df;
                p = P[f * C + out_src((int)kk, K) + 1];
                nvf = nv[f];
            }
            elem_llr<BPS>(h ? float2{v[it].z, v[it].w} : float2{v[it].x, v[it].y}, p, nvf, l[h]);
        }
        unsigned *dst = T + (o >> 1) * PW;
        if (OUT == 0) {
#pragma unroll
            for (int i = 0; i < 2 * BPS; ++i) dst[i] = __builtin_bit_cast(unsigned, l[i / BPS][i % BPS]);
        } else {
#pragma unroll
            for (int w = 0; w < PW; ++w) {
                unsigned d = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int i = 4 * w + b;
                    d |= quant8(l[i / BPS][i % BPS], llr_scale) << (8 * b);
                }
                dst[w] = d;
            }
        }
    }
    __syncthreads();
    // the tile's n * EB output bytes start 16-B aligned (SD_TILE * EB is a multiple of 16)
    const unsigned bytes = n * EB, full = bytes >> 4;
    unsigned char *ob = out + base * EB;
    for (unsigned c = tid; c < full; c += SD_TPB)
        __builtin_nontemporal_store(reinterpret_cast<const sd_u4 *>(T)[c], reinterpret_cast<sd_u4 *>(ob) + c);
    const unsigned rem = bytes & 15u;  // the last tile of the stream only
    if ((unsigned)tid < rem) ob[16 * full + tid] = reinterpret_cast<const unsigned char *>(T)[16 * full + tid];
}

template <int BPS>
__global__ void __launch_bounds__(SD_TPB) k_noise_estimate(const float2 *__restrict__ z, int K, unsigned per_frame,
                                                           int C, const float *__restrict__ P,
                                                           float *__restrict__ nv) {
    __shared__ float rs[SD_TPB];
    __shared__ unsigned rc[SD_TPB];
    const int tid = threadIdx.x;
    const long long f = blockIdx.x;
    const float2 *zf = z + f * per_frame;
    const float *Pf = P + f * C;
    const unsigned step = (unsigned)SD_TPB % (unsigned)K;
    unsigned k = (unsigned)tid % (unsigned)K;  // row position of element i = tid + 256 m
    constexpr int NU = 8;  // loads of z and of P in flight per thread
    float acc[NU] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    unsigned cnt = 0;
    auto add = [&](float &a, float2 w, float p) {
        if (pos_finite(p)) {
            const float dx = slice_err<BPS>(w.x), dy = slice_err<BPS>(w.y);
            a += p * (dx * dx + dy * dy);
            ++cnt;
        }
    };
    unsigned i0 = 0;
    for (; i0 + NU * SD_TPB <= per_frame; i0 += NU * SD_TPB) {  // whole chunks: every load issued, then the sums
        float2 w[NU];
        float p[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            w[u] = zf[i0 + u * SD_TPB + tid];
            p[u] = Pf[out_src((int)k, K) + 1];
            k += step;
            k -= k >= (unsigned)K ? (unsigned)K : 0u;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) add(acc[u], w[u], p[u]);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {  // the frame's last, partial chunk
        const unsigned i = i0 + u * SD_TPB + tid;
        if (i < per_frame) add(acc[u], zf[i], Pf[out_src((int)k, K) + 1]);
        k += step;
        k -= k >= (unsigned)K ? (unsigned)K : 0u;
    }
    rs[tid] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    rc[tid] = cnt;
    __syncthreads();
    for (int s = SD_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
            rs[tid] += rs[tid + s];
            rc[tid] += rc[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) nv[f] = rc[0] ? rs[0] / (float)rc[0] : 0.f;
}

bool soft_demap_supported(long long nframes, int S, int C) {
    const long long per_frame = (long long)(S - 1) * (C - 1);
    if (per_frame < 1 || per_frame > 0x7fffffffll - 2 * SD_TILE) return false;
    // one workgroup per tile / per frame, grid x below 2^31
    return nframes <= 0x7fffffffll && nframes <= (0x7fffffffll * SD_TILE) / per_frame;
}

hipError_t launch_soft_demap(const float2 *z, long long nframes, int S, int C, const float *P, const float *nv,
                             int bps, int fmt, float llr_scale, void *out, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    if (!soft_demap_supported(nframes, S, C) || (fmt != 0 && fmt != 1)) return hipErrorInvalidValue;
    const int K = C - 1;
    const unsigned per_frame = (unsigned)(S - 1) * (unsigned)K;
    const long long total = nframes * (long long)per_frame;
    const unsigned tiles = (unsigned)((total + SD_TILE - 1) / SD_TILE);
    unsigned char *o = static_cast<unsigned char *>(out);
    return dd::for_bps(bps, [&](auto b) {
        constexpr int BPS = decltype(b)::value;
        if (fmt == 0)
            hipLaunchKernelGGL((k_soft_demap<BPS, 0>), dim3(tiles), dim3(SD_TPB), 0, s, z, total, K, per_frame, C, P, nv,
                               llr_scale, o);
        else
            hipLaunchKernelGGL((k_soft_demap<BPS, 1>), dim3(tiles), dim3(SD_TPB), 0, s, z, total, K, per_frame, C, P, nv,
                               llr_scale, o);
        return hipGetLastError();
    });
}

hipError_t launch_noise_estimate(const float2 *z, long long nframes, int S, int C, const float *P, int bps,
                                 float *nv, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    if (!soft_demap_supported(nframes, S, C)) return hipErrorInvalidValue;
    const int K = C - 1;
    const unsigned per_frame = (unsigned)(S - 1) * (unsigned)K;
    return dd::for_bps(bps, [&](auto b) {
        hipLaunchKernelGGL(k_noise_estimate<decltype(b)::value>, dim3((unsigned)nframes), dim3(SD_TPB), 0, s, z, K,
                           per_frame, C, P, nv);
        return hipGetLastError();
    });
}

}  // namespace ofdm
