/*
 * ofdm_lsmrc_timing.h -- sampling clock offset: decision-directed tracking of
 * the common phase and the timing drift of a frame's data symbols.  An
 * extension of ofdm_lsmrc.h: same library (libofdm_lsmrc.so), same
 * conventions, same error codes, no version step (OFDM_LSMRC_VERSION stays 2).
 * It is a header of its own for the reason ofdm_lsmrc_acquire.h gives: the main
 * header's symbol set stays what its tables list.
 *
 * Why: free-running oscillators (the reference's default, rx_and_corr.cpp:116)
 * drive the carrier and the sampling clock alike.  A sampling clock offset of
 * delta moves the FFT window of data symbol n by tau_n = delta n (C + cp)
 * samples against the pilot's; subcarrier nu is then turned by
 * 2 pi nu tau_n / C: a phase slope across the band that grows with every
 * symbol.  ofdm_frame_phase_track removes only its mean.  At C = 1024, cp = 72,
 * S = 101, 10 ppm is 1.1 samples by the last symbol, +-3.4 rad at the band
 * edge, and the receiver reports no error.
 *
 * Definition.  Inputs exactly as ofdm_frame_phase_track's: d_z, the demodulated
 * array [nframes][S-1][K] (K = C - 1) in the rotated order every receiver
 * writes, and P of a full estimate in the workspace: the gain at output
 * position k is P[f*C + out_src(k, K) + 1].
 *
 * Signed frequency of position k: with b = out_src(k, K) + 1, nu_k = b if
 * 2 b < C, otherwise b - C (the Nyquist bin counts as -C/2).
 *
 * Once per frame: `use` = the positions whose P is positive and finite; the
 * lower half L = use with nu < 0, the upper half U = use with nu > 0; the
 * centroids c_L = sum_L P nu / sum_L P and c_U = sum_U P nu / sum_U P in
 * float64; span = c_U - c_L.  Slope tracking is ON for the frame if L and U
 * are both non-empty and span is finite and positive.  Otherwise tau stays
 * exactly 0 for the whole frame and the frame is tracked as
 * ofdm_frame_phase_track tracks it (C = 2 is such a case: nu = -1 only).
 *
 * Rows n = 0 .. S-2 in order, from theta_-1 = theta_-2 = tau_-1 = tau_-2 = 0:
 *   1. phi = 2 theta_(n-1) - theta_(n-2),  psi = 2 tau_(n-1) - tau_(n-2)
 *   2. w_k = z_k e^{-i (phi + 2 pi nu_k psi / C)},  d_k = slice(w_k), the
 *      phase tracker's slicer (the nearest point of the 38.211 constellation)
 *   3. g_L = sum_{k in L} P_k w_k conj(d_k), g_U likewise, g = g_L + g_U
 *   4. Delta = atan2(Im g, Re g), 0 when g is 0 or not finite
 *   5. x = g_U conj(g_L);  beta = atan2(Im x, Re x), 0 when slope tracking is
 *      off or x is 0 or not finite
 *   6. theta_n = phi + Delta,  tau_n = psi + beta C / (2 pi span)
 *   7. d_out[n][k] = z_k e^{-i (theta_n + 2 pi nu_k tau_n / C)} for every k,
 *      skipped elements included
 *   8. d_phase[f][n] = theta_n (radians, unwrapped, f32; may be null),
 *      d_timing[f][n] = tau_n (samples, f32; may be null)
 * tau > 0 means "this symbol's window lies tau samples later than the
 * pilot's": z = d e^{+i (theta + 2 pi nu tau / C)}.  The sums are formed in
 * f32 in a fixed order, no atomics: bit-identical from run to run.  Range of
 * P: g_L and g_U must each be finite in f32 (about |sum| < 3.4e38; a row where
 * one is not has Delta = beta = 0, as for a non-finite symbol).  Within that
 * range g_L + g_U and g_U conj(g_L) are formed from the two sums scaled by
 * exact powers of two, so Delta and beta do not depend on the scale of P.
 * theta and tau are carried in float64; only phases modulo one turn go through an f32
 * sincospi (for even C a thread's rotations follow from its first by
 * wave-uniform f32 factors, within rounding of the per-element value).  One
 * bad (non-finite) symbol leaves Delta = beta = 0 for its row and does not
 * poison the frame.
 *
 * The sampling clock offset as a fraction (delta) is the slope of tau through
 * the origin: sum n' tau_(n'-1) / sum n'^2 / (C + cp), n' = 1 .. S-1 (the
 * binding's sampling_offset, the twin of residual_cfo; host arithmetic).
 *
 * ofdm_frame_timing_track: arguments, alignment, overlap, registry and refusal
 * rules are exactly ofdm_frame_phase_track's.  Before any device work, in this
 * order:
 *   OFDM_E_ARG          modulation not 2 / 4 / 6 / 8; nframes < 0; S < 2; R < 1
 *   OFDM_E_UNSUPPORTED  C outside [2, 8192]
 *   (nframes == 0 is a no-op here: OFDM_OK)
 *   OFDM_E_ARG          a null d_z, d_out or d_ws; d_z or d_out not 8-byte
 *                       aligned, d_phase or d_timing not 4-byte aligned; d_out
 *                       overlapping d_z other than d_out == d_z (in place);
 *                       d_phase overlapping d_z or d_out; d_timing overlapping
 *                       d_z, d_out or d_phase; a workspace that holds no full
 *                       estimate of this geometry
 * The workspace is only read; no work tickets; the sticky device status is
 * neither consulted nor cleared.
 *
 * ofdm_pipeline_set_timing_track: with modulation 2 / 4 / 6 / 8 every later
 * submit runs this tracker in place on the slot's output, where the phase
 * tracker would run, after whichever receiver form the submit used; when both
 * are set it runs INSTEAD of the phase tracker, which it contains.  0 is the
 * state of a new pipeline: a submit then enqueues exactly what it enqueues
 * without this call.  OFDM_E_ARG for a null pipeline or another modulation.
 *
 * Not covered: drift beyond the cyclic prefix and the sample drop or insert
 * that goes with it; correcting in the time domain or inside the receivers;
 * handing the pipeline's tau back to the caller; the host C++ mirrors (host/).
 */
#ifndef OFDM_LSMRC_TIMING_H_
#define OFDM_LSMRC_TIMING_H_

#include "ofdm_lsmrc.h"

#ifdef __cplusplus
extern "C" {
#endif

int ofdm_frame_timing_track(const ofdm_cf32 *d_z, long long nframes, int S, int R, int C,
                            const void *d_ws, size_t ws_bytes, int modulation, ofdm_cf32 *d_out,
                            float *d_phase  /* [nframes][S-1] or NULL */,
                            float *d_timing /* [nframes][S-1] or NULL */, ofdm_stream_t stream);
int ofdm_pipeline_set_timing_track(ofdm_pipeline *p, int modulation);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_LSMRC_TIMING_H_ */
