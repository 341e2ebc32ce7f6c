// llr_quant.hpp -- one LLR element of a decoder's input stream as an integer
// q in [-127, 127], for the channel decoders (viterbi.hip, ldpc.hip).  The
// rule is the one include/ofdm_lsmrc_decode.h states: OFDM_LLR_I8 (fmt 1)
// max(v, -127); OFDM_LLR_F32 (fmt 0) soft_demap.hip's int8 rule, NaN -> 0, so
// decoding f32 LLRs is bit-identical to decoding the demapper's bytes.
#pragma once
#include <hip/hip_runtime.h>

namespace ofdm {
namespace llrq {

// One LLR element of the codeword at element e0, as loaded: the float's bits or
// the sign-extended byte; x: its index in the codeword's stream, 0 at and
// beyond n_rx (never read).  quant() makes the integer q of the definition
// from it; the two are apart so that a load stays in flight until its
// register is needed.
__device__ __forceinline__ int load_raw(const void *llr, int fmt, long long e0, int x, int n_rx) {
    if (x >= n_rx) return 0;
    if (fmt == 1) return static_cast<const signed char *>(llr)[e0 + x];
    return __float_as_int(static_cast<const float *>(llr)[e0 + x]);
}
__device__ __forceinline__ int quant(int raw, int fmt, float scale) {
    if (fmt == 1) return raw < -127 ? -127 : raw;
    const float f = __int_as_float(raw) * scale;
    const float v = f == f ? __builtin_fminf(__builtin_fmaxf(f, -127.f), 127.f) : 0.f;  // soft_demap.hip quant8
    return (int)__builtin_rintf(v);
}

}  // namespace llrq
}  // namespace ofdm
