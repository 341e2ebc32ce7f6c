// lane_layout.hpp -- the lane orders of the workspace estimate, stated once.
//
// A fused receiver keeps each Hc row (C float2 per frame and antenna) in the
// order its MRC kernel's lanes consume it, so that every wave load of the
// estimate is coalesced.  This header is the only place that says which
// position of such a row holds which bin: the LS kernels store through
// hc_pos, ofdm_frame_export_estimate reads back through it, and the FFT512
// family's MRC kernels name the bin of an accumulator with bin512 /
// bin_small.  Plain C++, callable from host and device
// (tests/test_lane_layout_cpu.py enumerates every table on the CPU).
#pragma once

#ifdef __HIPCC__
#define OFDM_HD __host__ __device__ __forceinline__
#else
#define OFDM_HD inline
#endif

namespace ofdm {
namespace lane {

// ---- FFT512 family (frame_td_fft512.hip) ----------------------------------
// C = 1536 W on W = 1, 2, 4 waves per data symbol: slot i = 8 j + d of lane
// L = 8 s + c of wave e holds bin 3 (W (s + 8 c + 64 d) + e) + j, stored at
// e * 1536 + i * 64 + L.
OFDM_HD int bin512(int W, int e, int L, int i) {
    return 3 * (W * ((L >> 3) + 8 * (L & 7) + 64 * (i & 7)) + e) + (i >> 3);
}
OFDM_HD int pos512(int W, int b) {
    const int q = b / 3, j = b - 3 * q, e = q % W, kk = q / W;
    return e * 1536 + (8 * j + (kk >> 6)) * 64 + 8 * (kk & 7) + ((kk >> 3) & 7);
}
// C = 64 P, P = 2, 4, 8, on one wave: slot d of lane-mod-8P lw = 8 s' + c
// holds bin s' + P c + 8 P d, stored at d * 8 P + lw.
OFDM_HD int bin_small(int P, int lw, int d) { return (lw >> 3) + P * (lw & 7) + 8 * P * d; }
OFDM_HD int pos_small(int P, int b) { return (b / (8 * P)) * (8 * P) + 8 * (b % P) + ((b / P) & 7); }

OFDM_HD bool is_fft512(int C) { return C == 1536 || C == 3072 || C == 6144; }
OFDM_HD bool is_small(int C) { return C == 128 || C == 256 || C == 512; }

// ---- C = 1024 / 2048 / 4096 (frame_td.hip, frame_td2048.hip, frame_td4096.hip)
// lane t of a wave owns the bins b0(t) + 16 k, b0(t) = (t >> 2) + 256 c(t & 3),
// c(a) = (a >> 1) + 2 (a & 1): the lane and the k of bin b < 1024
OFDM_HD int lane_of(int b, int &k) {
    const int q = b & 15, c = b >> 8;
    k = (b >> 4) & 15;
    return 4 * q + (((c & 1) << 1) | (c >> 1));
}

// Position of bin b < C inside one lane-ordered Hc row; a C without a lane
// order (and C = 0) is in bin layout: position = b.
OFDM_HD int hc_pos(int C, int b) {
    int k;
    if (is_fft512(C)) return pos512(C / 1536, b);
    if (is_small(C)) return pos_small(C / 64, b);
    if (C == 1024) {  // float4 (k >> 1) * 64 + t holds bins (k & ~1, k | 1) of lane t
        const int t = lane_of(b, k);
        return 2 * ((k >> 1) * 64 + t) + (k & 1);
    }
    if (C == 2048) {  // float4 k * 64 + t = (Hc[2 b'], Hc[2 b' + 1]), b' = b0(t) + 16 k
        const int t = lane_of(b >> 1, k);
        return 2 * (k * 64 + t) + (b & 1);
    }
    if (C == 4096) {  // float2 e * 2048 + h * 1024 + (k >> 1) * 128 + 2 t + (k & 1) = Hc[4 b' + 2 h + e]
        const int t = lane_of(b >> 2, k);
        return (b & 1) * 2048 + ((b >> 1) & 1) * 1024 + (k >> 1) * 128 + 2 * t + (k & 1);
    }
    return b;
}

}  // namespace lane
}  // namespace ofdm
