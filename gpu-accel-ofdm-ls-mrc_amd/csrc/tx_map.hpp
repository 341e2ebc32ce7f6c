// tx_map.hpp -- what the two modulator kernels (tx_mod.hip k_tx_mod1024,
// fft_any.hip k_tx_any) share: the inverse of the bin placement, the peak's
// maximum and the row gain.  Values of map / norm: OFDM_TX_MAP_* / OFDM_TX_NORM_*
// (include/ofdm_lsmrc.h).
#pragma once
#include "common.hpp"

namespace ofdm {

constexpr int TX_MAP_REFERENCE = 0, TX_MAP_RX = 1;
constexpr int TX_NORM_PEAK = 0, TX_NORM_SCALE = 1;

// The input position k whose value bin b of the transform carries, or -1 for
// an empty bin.
//   reference: modOneSymbol's d[0] = 0, d[k + 1] = X[k] (cpuLS.hpp:511) then
//     ifftShiftOneRow's three memmoves (119-132), h = C / 2: bin[i] = d[i + h]
//     (i < h), d[i - h] (h <= i < 2 h), and for odd C bin[C - 1] = d[C - 1];
//   rx: position k at bin out_src(k, K) + 1, i.e. bin j + 1 carries
//     k = out_pos_any(j, K); bin 0 empty -- what the receivers undo.
__device__ __forceinline__ int tx_src(int b, int C, int map) {
    if (map == TX_MAP_REFERENCE) {
        const int h = C / 2;
        return (b < h ? b + h : (b < 2 * h ? b - h : b)) - 1;
    }
    return b == 0 ? -1 : out_pos_any(b - 1, C - 1);
}

// max that keeps a NaN from either side (fmaxf drops it)
__device__ __forceinline__ float tx_max(float m, float v) { return (v > m || v != v) ? v : m; }

// the factor of a row whose peak |x| is pk: 1 / pk (the reference's
// maxval = 1 / clange_, cpuLS.hpp:521; an all-zero row: 0, so that it is
// stored as zeros, not the reference's 0 * inf), or the caller's scale
__device__ __forceinline__ float tx_gain(float pk, int norm, float scale) {
    if (norm != TX_NORM_PEAK) return scale;
    return pk == 0.f ? 0.f : 1.0f / pk;
}

}  // namespace ofdm
