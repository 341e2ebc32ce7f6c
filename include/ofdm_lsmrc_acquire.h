/*
 * ofdm_lsmrc_acquire.h -- integer carrier frequency offset: acquisition of
 * |eps| >= 0.5 subcarrier spacings from the pilot symbol.  An extension of
 * ofdm_lsmrc.h: same library (libofdm_lsmrc.so), same conventions, same error
 * codes, no version step (OFDM_LSMRC_VERSION stays 2).  It is a header of its
 * own only so that the main header's symbol set stays what its tables list;
 * folding it into ofdm_lsmrc.h ("carrier frequency offset") is a later step.
 *
 * Why: the cyclic-prefix estimator (ofdm_frame_cfo_estimate) returns eps
 * modulo one subcarrier spacing.  Free-running oscillators (the reference's
 * default, rx_and_corr.cpp:116) differ by several spacings at the sample rates
 * its radios run; derotating by the fractional part alone leaves every bin on
 * a neighbour's pilot, and every decision wrong with no error code.  After
 * the fractional derotation an integer offset d is a cyclic shift of the pilot
 * symbol's spectrum by d bins; the differential product of neighbouring bins
 * cancels the channel wherever it is coherent over one bin (any channel
 * shorter than the prefix) and lines up with the pilots' own differential
 * sequence at exactly one shift.
 *
 * Definition (the CFO convention of ofdm_lsmrc.h: eps in subcarrier spacings,
 * y[m] = x[m] e^{+2 pi i eps m / C}, m counted per antenna row from the first
 * prefix sample of symbol 0).  For frame f, with e = d_eps_in[f], the f32 value
 * taken exactly (a non-finite value, or a null d_eps_in, acts as 0), K = C - 1,
 * X the rotated pilots as every receiver takes them, D = max_shift:
 *   1. x0[r][i] = y[f,0,r,cp_len+i] e^{-2 pi i e (cp_len+i) / C},  i < C
 *      (the pilot symbol, its prefix skipped: never read)
 *   2. Y[r][.] = forward unnormalised FFT of x0[r]
 *   3. Z[b] = sum_r Y[r][(b+1) mod C] conj(Y[r][b]),  b < C, in order of r
 *   4. q[j] = X[j+1] conj(X[j]),  j = 0 .. K-2  (bin j+1 to bin j+2)
 *   5. A(d) = sum_j Z[(j + 1 + d) mod C] conj(q[j]),  M(d) = |A(d)|,  d = -D .. D
 *   6. dh = the d of largest finite M; among equal M the smallest |d|, the
 *      negative before the positive; a non-finite M(d) is never chosen; if no
 *      M is finite and positive, dh = 0
 *   7. gate: if M(dh) < min_ratio * max_{d != dh} M(d) (the finite ones), dh := 0
 *      and the fractional estimate stands; min_ratio == 1 always accepts
 *   8. d_eps_out[f] = (float)((double)e + dh);  d_shift[f] = dh (int32, may be
 *      null);  d_metric[f][d + D] = (float)M(d), ungated (float [nframes][2D+1],
 *      may be null), so a caller can form its own confidence.
 * d_eps_out may equal d_eps_in (in place).  M is accumulated in float64 in a
 * fixed order, no atomics: bit-identical from run to run.
 *
 * Pilots whose differential sequence q is constant cannot be acquired this
 * way: every shift lines up equally well.  The reference's fallback fill
 * (ofdm_read_pilots without a file: fill + i fill in every bin) and any
 * constant-phase-ramp pilot are examples; their best-to-runner-up ratio is 1
 * and the gate leaves shift 0.  Measured with random QPSK pilots on 4-tap
 * channels: 9 - 17 at C = 1024 on four antennas, 4.9 - 9 at C = 256 on two,
 * 2.4 - 5.4 at C = 64 on one; noise-only frames 1.0 - 1.6.
 *
 * One pass over the pilot symbol (1/S of a frame's bytes), each row read once;
 * any 8 <= C <= 8192.  No workspace, no work tickets, no device allocation
 * inside the call; the sticky device status is neither consulted nor cleared.
 * Before any device work, in this order:
 *   OFDM_E_ARG          nframes < 0, S < 2, R < 1, cp_len < 0 or cp_len > C; a
 *                       null d_iq, d_X or d_eps_out with nframes > 0; d_iq not
 *                       16-byte aligned (rows need 8 bytes only: any cp_len);
 *                       max_shift < 1 or > OFDM_ACQ_MAX_SHIFT; a min_ratio that
 *                       is not finite or is < 1; d_eps_out overlapping d_metric
 *                       or d_shift
 *   OFDM_E_UNSUPPORTED  C outside [8, 8192]
 *   OFDM_E_ARG          4 * max_shift > C
 * nframes == 0 is a no-op (OFDM_OK); cp_len == 0 is valid (the pass needs no
 * prefix).
 *
 * ofdm_pipeline_set_cfo_search: with max_shift > 0 every later submit that runs
 * with ofdm_pipeline_set_cfo on enqueues, directly after
 * ofdm_frame_cfo_estimate, ofdm_frame_cfo_acquire in place on the slot's eps
 * array with the pipeline's device copy of X; everything after it is as
 * before (the _cfo receiver at C = 1024, the derotator and the fp32 forms
 * elsewhere, denoising and phase tracking as set).  An sc16 pipeline at
 * C != 1024 searches on its converted chunk.  max_shift == 0 turns the search
 * off, the state of a new pipeline: a submit then enqueues exactly what it
 * enqueues without this call.  While CFO is off the setting is stored and has
 * no effect.  OFDM_E_ARG for a null pipeline, max_shift < 0, > OFDM_ACQ_MAX_SHIFT
 * or with 4 * max_shift > C, or a min_ratio that is not finite or is < 1;
 * OFDM_E_UNSUPPORTED for max_shift > 0 on a pipeline with C < 8.
 *
 * Not covered: sc16 input without conversion, the host C++ mirrors (host/),
 * returning the pipeline's shifts to the caller, offsets beyond
 * +-OFDM_ACQ_MAX_SHIFT spacings.
 */
#ifndef OFDM_LSMRC_ACQUIRE_H_
#define OFDM_LSMRC_ACQUIRE_H_

#include "ofdm_lsmrc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_ACQ_MAX_SHIFT 64

int ofdm_frame_cfo_acquire(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                           const ofdm_cf32 *d_X, int max_shift, float min_ratio,
                           const float *d_eps_in /* nullable */, float *d_eps_out,
                           int *d_shift /* nullable */, float *d_metric /* nullable */, ofdm_stream_t stream);
int ofdm_pipeline_set_cfo_search(ofdm_pipeline *p, int max_shift, float min_ratio);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_LSMRC_ACQUIRE_H_ */
