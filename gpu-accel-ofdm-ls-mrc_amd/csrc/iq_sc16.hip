// iq_sc16.hip -- sc16 IQ (what the radios put on the wire; the reference's
// drivers default otw to "sc16", rx_and_corr.cpp:112,283, and let UHD widen
// every sample to fc32 on the host CPU) to complex<float> on the device:
//   k_iq_sc16_to_cf32  out[i] = {float(re) * scale, float(im) * scale}
// The int16 -> float conversion is exact and the product rounds once, so the
// result is bit-exact against i16.astype(float32) * float32(scale) for any
// scale.  It is the route for every FFT length that has no sc16 receiver of
// its own (frame_td.hip has them for C = 1024): convert, then any fp32 entry.
#include "common.hpp"
#include "launch.hpp"

namespace ofdm {

typedef unsigned u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float2 sc16_to_cf32(unsigned v, float scale) {
    return float2{(float)(short)(v & 0xffffu) * scale, (float)((int)v >> 16) * scale};
}

// Each lane: one 16-B nontemporal load (4 samples, streamed once) and two
// 16-B stores (plain: the fp32 receiver that follows reads them from L2 while
// they are there); grid-stride over the n / 4 groups, then the n % 4 tail
// samples one lane each.
__global__ void __launch_bounds__(256) k_iq_sc16_to_cf32(const sc16 *__restrict__ in, long long n, float scale,
                                                         float2 *__restrict__ out) {
    const long long n4 = n >> 2;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const u4v *in4 = reinterpret_cast<const u4v *>(in);
    float4 *out4 = reinterpret_cast<float4 *>(out);
    for (long long i = gid; i < n4; i += stride) {
        const u4v v = __builtin_nontemporal_load(in4 + i);
        const float2 a = sc16_to_cf32(v.x, scale), b = sc16_to_cf32(v.y, scale);
        const float2 c = sc16_to_cf32(v.z, scale), d = sc16_to_cf32(v.w, scale);
        out4[2 * i] = float4{a.x, a.y, b.x, b.y};
        out4[2 * i + 1] = float4{c.x, c.y, d.x, d.y};
    }
    const long long i = 4 * n4 + gid;
    if (gid < 4 && i < n) out[i] = sc16_to_cf32(in[i].v, scale);
}

hipError_t launch_iq_sc16_to_cf32(const sc16 *in, long long n, float scale, float2 *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    // enough workgroups to fill the GPU several times over, each lane looping
    const long long want = ((n >> 2) + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
    hipLaunchKernelGGL(k_iq_sc16_to_cf32, dim3(grid), dim3(256), 0, s, in, n, scale, out);
    return hipGetLastError();
}

}  // namespace ofdm
