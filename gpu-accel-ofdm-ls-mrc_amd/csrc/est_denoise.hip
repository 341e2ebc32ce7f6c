// est_denoise.hip -- delay-domain denoising of the kept LS channel estimate
// (ofdm_frame_estimate_denoise, include/ofdm_lsmrc.h states the operation):
// every antenna row of the workspace estimate goes to the delay domain, the
// taps outside [0, taps_post) u [C - taps_pre, C) are zeroed, and the row
// comes back, in place, with the frame's |H|^2 sums rebuilt from it.  HBM
// traffic: the estimate read once and written once, P written once.
//
// This file holds the C = 1024 kernel for the lane-ordered workspace (one wave
// per row on the wave FFT of wave_fft1024.hpp) and the dispatch; every other C
// and the bin layout run k_denoise_any on the mixed-radix stage machinery
// (fft_any.hip).
#include "wave_fft1024.hpp"

namespace ofdm {
namespace dn1024 {

using namespace td1024;

constexpr int WAVES = 8;  // rows in flight per workgroup; LDS 9.0 + 8 x 8.5 KiB: two workgroups per CU

// One workgroup per frame, wave w the rows r = w, w + 8, ...  A row arrives as
// hc_load's 8 coalesced 16-B loads: lane t holds Hc[b0(t) + 16 k], which is
// row_fft's OUTPUT order.  row_fft wants sample t + 64 m in lane t, so the
// row goes through the wave's natural-order LDS image (nat_img: conflict-free
// ds_write_b64 from the output order, and each read of nat_img(t + 64 m) one
// contiguous image row) -- once as swap(H), H = conj(Hc), for the backward
// transform (IFFT(x) = swap(FFT(swap(x))), as k_tx_mod1024), and once as the
// masked taps for the forward one, whose output order is the Hc lane order
// again: the row leaves through hc_store.  The mask and the 1/C are applied
// in registers between the two.  Lane 0's slot 0 is bin 0: it enters as
// (H[1] + H[C-1]) / 2 (lane 4's slot 0 and lane 63's slot 15) and is stored
// back with the bits it was loaded with.
// P: a wave adds |H'|^2 of its rows in order of r into 16 registers per lane;
// the eight partial sums meet in LDS (each wave's image as 1024 floats by
// bin) and are added in order of the wave index: a fixed order, no atomics.
__global__ void __launch_bounds__(64 * WAVES)
k_denoise1024(float2 *__restrict__ Hc, float *__restrict__ P, int R, int taps_post, int taps_pre) {
    __shared__ __attribute__((aligned(16))) float2 tw[TWBUF];
    __shared__ __attribute__((aligned(16))) float2 Tall[WAVES * TBUF];
    static_assert(2 * sizeof(float2) * (TWBUF + WAVES * TBUF) <= 160 * 1024, "two workgroups per CU");
    static_assert(C * sizeof(float) <= TBUF * sizeof(float2), "a wave's partial P fits its image");
    fill_twiddles(tw);
    __syncthreads();
    const int t = threadIdx.x & 63, w = threadIdx.x >> 6;
    float2 *T = Tall + w * TBUF;
    const long long f = blockIdx.x;
    const int b0 = lane_bin0(t), keep_hi = C - taps_pre;
    const float inv = 1.f / C;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    for (int r = w; r < R; r += WAVES) {
        float4 *row = reinterpret_cast<float4 *>(Hc + (f * R + r) * C);
        float2 h[16], a[16], x[16];
        hc_load(row, t, h);
        const float2 kept0 = h[0];
        auto lane_val = [](float v, int lane) {
            return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
        };
        const float2 h1{lane_val(h[0].x, 4), lane_val(h[0].y, 4)}, hm{lane_val(h[15].x, 63), lane_val(h[15].y, 63)};
        if (t == 0) h[0] = float2{0.5f * (h1.x + hm.x), 0.5f * (h1.y + hm.y)};
        // swap(conj(h)) = (-h.y, h.x)
#pragma unroll
        for (int k = 0; k < 16; ++k) T[nat_img(b0 + 16 * k)] = float2{-h[k].y, h[k].x};
        wave_lds_sync();
#pragma unroll
        for (int m = 0; m < 16; ++m) a[m] = T[nat_img(t + 64 * m)];
        wave_lds_sync();
        row_fft(a, t, T, tw, x);  // x[k] = swap(C g)[b0 + 16 k]
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int n = b0 + 16 * k;
            const bool keep = n < taps_post || n >= keep_hi;
            T[nat_img(n)] = keep ? float2{x[k].y * inv, x[k].x * inv} : float2{0.f, 0.f};
        }
        wave_lds_sync();
#pragma unroll
        for (int m = 0; m < 16; ++m) a[m] = T[nat_img(t + 64 * m)];
        wave_lds_sync();
        row_fft(a, t, T, tw, x);  // x[k] = H'[b0 + 16 k]
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            acc[k] += x[k].x * x[k].x + x[k].y * x[k].y;
            h[k] = float2{x[k].x, -x[k].y};
        }
        if (t == 0) h[0] = kept0;
        hc_store(row, t, h);
    }
    wave_lds_sync();
    float *Tf = reinterpret_cast<float *>(T);
#pragma unroll
    for (int k = 0; k < 16; ++k) Tf[b0 + 16 * k] = acc[k];
    lds_barrier();
    const float *Pw = reinterpret_cast<const float *>(Tall);
    for (int b = threadIdx.x; b < C; b += 64 * WAVES) {
        float s = Pw[b];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) s += Pw[v * (2 * TBUF) + b];
        if (b >= 1) P[f * C + b] = s;
    }
}

}  // namespace dn1024

hipError_t launch_estimate_denoise(float2 *Hc, float *P, long long nframes, int R, int C, bool lane_order,
                                   int taps_post, int taps_pre, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    if (C != dn1024::C || !lane_order)
        return launch_denoise_any(Hc, P, nframes, R, C, lane_order, taps_post, taps_pre, s);
    if (R < 1 || taps_post < 1 || taps_pre < 0 || taps_post > C - taps_pre || nframes > 0x7fffffffll)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn1024::k_denoise1024, dim3((unsigned)nframes), dim3(64 * dn1024::WAVES), 0, s, Hc, P, R,
                       taps_post, taps_pre);
    return hipGetLastError();
}

}  // namespace ofdm
