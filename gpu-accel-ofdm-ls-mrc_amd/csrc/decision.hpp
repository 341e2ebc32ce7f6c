// decision.hpp -- what the decision-directed stages behind the combiner share
// (soft_demap.hip, phase_track.hip, timing_track.hip): the constellation and its
// slicer, the wave-level pieces, the layout and the row load of the two
// trackers' frame-per-workgroup design, and the host-side dispatch over the
// modulation and over launch chunks.  Each once; a fix to the slicer is made
// here.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace ofdm {
namespace dd {

// ---- the constellation (3GPP TS 38.211 5.1.2-5.1.6, unit average energy) ----

// half the distance between neighbouring points of one axis
template <int BPS>
__device__ __forceinline__ constexpr float qam_a() {
    return BPS == 2 ? 0.70710678118654752f
         : BPS == 4 ? 0.31622776601683794f
         : BPS == 6 ? 0.15430334996209191f
                    : 0.076696498884737041f;
}

// the nearest point of one axis: a (2 t + 1), t = clamp(floor(x / 2a), -L, L - 1)
template <int BPS>
__device__ __forceinline__ float slice_axis(float x) {
    constexpr float a = qam_a<BPS>();
    constexpr float L = (float)(1 << (BPS / 2 - 1));
    float t = __builtin_floorf(x * (0.5f / a));
    t = __builtin_fminf(__builtin_fmaxf(t, -L), L - 1.f);
    return (2.f * t + 1.f) * a;
}
// x minus its nearest point
template <int BPS>
__device__ __forceinline__ float slice_err(float x) {
    return x - slice_axis<BPS>(x);
}

__device__ __forceinline__ bool pos_finite(float v) { return v > 0.f && v < __builtin_inff(); }
__device__ __forceinline__ bool is_finite(float v) {
    return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u;
}

// e^{-2 pi i turns}: reduced modulo one turn in float64, the rest in f32 (as cfo.hip does)
__device__ __forceinline__ float2 cis_neg_turns(double turns) {
    const float r = (float)(turns - __builtin_rint(turns));
    float sn, cs;
    sincospif(2.f * r, &sn, &cs);
    return float2{cs, -sn};
}

// ---- wave pieces ----

// v + (v of the lane DPP control CTRL names); every lane active
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(float, o);
}
// the sum over the wave's 64 lanes, the same bits in every lane
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the 8
    v = dpp_add<0x140>(v);  // row_mirror: the other 8 of the row of 16
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// a wave-uniform float64 as a scalar: a recursion's state stays out of the VGPRs
__device__ __forceinline__ double uniform(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// the sum over the wave's lanes of a float64, in a fixed order (once per frame)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));

// Row n's byte offset in its frame, as a scalar the compiler does not see
// through: the row's base stays in SGPRs with the element's 32-bit offset
// beside it, instead of one strength-reduced 64-bit VGPR pointer per element,
// row set and access (96 registers at 16 elements per thread).
__device__ __forceinline__ unsigned long long row_bytes(int n, int K) {
    const unsigned long long b = (unsigned long long)n * (unsigned)K * 8u;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// ---- the trackers' rows: one workgroup of TPB threads per frame ----
//
// Frames are the parallel dimension, the rows of a frame are a serial chain
// load -> rotate/slice/accumulate -> reduce -> atan2 -> rotate -> store, and
// its latency, not its bytes, is what can bound the kernel.  Thread t holds the
// elements k = c*TPB + t, c < CH, of a row (CH * TPB >= K) in registers: kc[c]
// the element's byte offset in a row, p[c] its P by output position (0 where P
// is not positive and finite), and the next two rows' elements in two more
// sets.  Rows are only 8-B aligned (K is odd for every even C): every access
// is one 8-B element per lane, 512 B contiguous per wave instruction,
// nontemporal both ways -- no head/tail case, and in place each thread writes
// its own elements only and uses nothing it read from another's.
//
// The setup of kc[] and p[] and the rotation of the rows through the three
// sets are written out in k_phase_track and in k_timing_track, not here: a
// function holding either loop is optimised on its own before it is inlined,
// and the kernels' instruction order, which their wait counters depend on
// (phase_track.hip, at the loop), comes out different.

// row min(n, last) of the frame at zf into one register set (the kernels call
// it through a local closure, `load`, over zf, last, K and kc)
template <int CH>
__device__ __forceinline__ void load_row(float2 (&r)[CH], const f2v *zf, int n, int last, int K,
                                         const unsigned (&kc)[CH]) {
    const char *zn = reinterpret_cast<const char *>(zf) + row_bytes(n < last ? n : last, K);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const f2v v = __builtin_nontemporal_load(reinterpret_cast<const f2v *>(zn + kc[c]));
        r[c] = float2{v.x, v.y};
    }
}

// ---- host side ----

// fn(std::integral_constant<int, BPS>) for the modulation's bits per symbol
template <class Fn>
hipError_t for_bps(int bps, Fn &&fn) {
    switch (bps) {
    case 2: return fn(std::integral_constant<int, 2>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}

// launch(f0, n) for the frames [f0, f0 + n) of every chunk that fits a grid: one launch but for absurd batches
template <class Launch>
hipError_t for_frame_chunks(long long nframes, Launch &&launch) {
    for (long long f0 = 0; f0 < nframes; f0 += 0x7fffffffll) {
        const long long n = nframes - f0 < 0x7fffffffll ? nframes - f0 : 0x7fffffffll;
        launch(f0, (unsigned)n);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dd
}  // namespace ofdm
