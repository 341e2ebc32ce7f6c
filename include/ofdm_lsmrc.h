/*
 * ofdm_lsmrc.h -- C ABI of the MI355X (gfx950) OFDM uplink receiver hot path:
 * per-subcarrier Least-Squares channel estimation from a pilot symbol and
 * Maximal-Ratio-Combining demodulation of data symbols across RX antennas.
 *
 * Library: gpu-accel-ofdm-ls-mrc_amd/lib/libofdm_lsmrc.so (hand-written HIP
 * kernels for CDNA4; no CPU fallback -- every compute entry point runs on the
 * GPU and returns an error if it cannot).
 *
 * Conventions (all cite the reference bhargav0410/gpu-accel-ofdm-ls-mrc):
 *   R  = RX antennas (numOfRows), C = FFT size / subcarriers (dimension:
 *        any 2 <= C <= 8192, like the reference's FFTW / cuFFT plans; else
 *        OFDM_E_UNSUPPORTED), K = C - 1 used subcarriers (the DC bin is dropped,
 *        cpuLS.hpp:290-292), S = symbols per frame (lenOfBuffer), symbol 0 of
 *        a frame is the pilot, symbols 1..S-1 carry data.
 *   ofdm_cf32 = {float re, im}, layout-identical to complexF
 *        (ShMemSymBuff.hpp:86-89), cuFloatComplex and hipFloatComplex.
 *   A symbol is R rows of C (+prefix) samples, row-major by antenna
 *        (struct symbol, ShMemSymBuff.hpp:92-94); frames are consecutive
 *        symbols, batches are consecutive frames.
 *   Output of a data symbol: K values, shiftOneRow-rotated (cpuLS.hpp:135-149):
 *        out[k] = Z[(k + (K-1)/2) mod K], Z[j] = sum_r Y[r][j+1] conj(H[r][j])
 *        / sum_r |H[r][j]|^2, for odd K (even C); for even K (odd C) the
 *        three memmoves of shiftOneRow literally: out[k] = Z[k + K/2 - 1] for
 *        k < K/2, Z[k - K/2] for K/2 <= k < K-1, and out[K-1] = Z[K-1].
 *   Pointers named d_* are device pointers; `stream` is a hipStream_t (NULL =
 *   the default stream).  Calls are asynchronous on that stream.
 *   Return value: 0 (OFDM_OK) or a negative OFDM_E_* code; ofdm_last_error()
 *   describes the last failure on the calling thread.
 *   Alignment of device pointers (OFDM_E_ARG otherwise, before any device
 *   work): 16 bytes for the sample input of every frame, symbol and MRC entry
 *   -- d_iq / d_Y / d_sym of ofdm_frame_*, ofdm_symbols_demod, ofdm_mrc_demod
 *   and ofdm_mrc_numerator (rows inside the buffer need 8 bytes only, sc16 rows
 *   4: any cp_len works) -- and for the pointers an entry's own comment names;
 *   256 bytes for d_ws.  Every other pointer needs the natural alignment of its
 *   element only: 8 bytes for ofdm_cf32 and the 64-bit words, 4 for float.
 *
 * Degenerate and non-finite input.  No entry has data-dependent addressing: a
 * NaN, an Inf, a zero pilot X[k] or an all-zero pilot symbol is ordinary data,
 * and it changes only the outputs that depend on it (its footprint); every
 * other output holds the bits it holds without it.  f frame, s symbol (0 the
 * pilot), r antenna, b bin, j subcarrier (bin j + 1), pos(j) its output column:
 *   time-domain receivers (ofdm_frame_demod[_ex], _estimate + _combine, the
 *     _sc16 and _cfo forms, _ls_partial + _mrc_partial + ofdm_mrc_finalize,
 *     ofdm_symbols_demod): a time sample of a data row (f, s >= 1, r) reaches
 *     out[f][s-1][*]; one of a pilot row (f, 0, r) reaches out[f][*][*], the
 *     estimate rows of (f, r) and P[f]; the cyclic prefix is never read.
 *     X[k] = 0 reaches out[*][*][pos(k)] and the estimate and P at subcarrier
 *     k of every frame; an all-zero pilot symbol of frame f gives estimate 0,
 *     P[f] = 0 and out[f] = NaN (0 / 0) -- the cells the downstream stages
 *     skip.  d_eps[f] reaches frame f alone.
 *   frequency-domain receivers and the stage entries: Y[f][s >= 1][r][b]
 *     reaches out[f][s-1][pos(b-1)] alone, Y[f][0][r][b] reaches
 *     out[f][*][pos(b-1)], Hconj[r][b-1] and P[b-1]; bin 0 reaches nothing.
 *   ofdm_fft_rows, ofdm_tx_modulate: an element of row i reaches row i (and
 *     d_peak[i]).  ofdm_zf_detect / _apply: Y[n][r][k] or X[n][u][k] reaches
 *     out[n][*][k], Wt[u][r][k] reaches out[*][u][k] (detect) or out[*][r][k]
 *     (apply); ofdm_zf_precoder: H[u][r][k] reaches W[k] and Wt[*][*][k].
 *   per-frame outputs (ofdm_frame_cfo_estimate, ofdm_frame_cfo_acquire,
 *     ofdm_frame_noise_estimate, ofdm_frame_phase_track, ofdm_frame_estimate_
 *     denoise) and the pipeline's chunks: a sample of frame f reaches frame
 *     f's values alone -- in a pipeline neither the other frames of its chunk
 *     nor the later chunks that reuse the slot.
 * Amplitude range: every receiver output is unchanged, bit for bit, when the
 * IQ is scaled by a power of two (the exported estimate scales by it, P by its
 * square), as long as P = sum_r |H|^2 and 1 / P are NORMAL floats for every
 * used bin: the division is a hardware reciprocal (v_rcp_f32), which flushes
 * a subnormal P or 1 / P, so outside that range a bin's output is 0 or
 * non-finite where a true division would still answer.  P is a second power
 * of the FFT bins, themselves up to C times the samples: IQ of unit amplitude
 * times 2^+-40 is inside the range at every C and R <= 64, and is what the
 * tests exercise.  The per-frame CFO outputs scale likewise (gamma and the
 * acquisition metric by the square, eps and the shift not at all).
 */
#ifndef OFDM_LSMRC_H_
#define OFDM_LSMRC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ofdm_hbm_probe takes dst_bytes; OFDM_E_DEVICE, ofdm_device_status(_inject),
 *    ofdm_zf_detect_ex / ofdm_zf_apply_ex added (round 6) */
#define OFDM_LSMRC_VERSION 2

typedef struct ofdm_cf32 { float re, im; } ofdm_cf32;
/* One sc16 sample, 4 bytes: re in the low half of the little-endian dword --
 * std::complex<int16_t>, what a UHD rx_streamer delivers for the cpu format
 * "sc16" (see "sc16 IQ" below). */
typedef struct ofdm_sc16 { int16_t re, im; } ofdm_sc16;
typedef void *ofdm_stream_t; /* hipStream_t */

enum {
    OFDM_OK = 0,
    OFDM_E_ARG = -1,         /* invalid argument (shape, null, alignment) */
    OFDM_E_HIP = -2,         /* HIP runtime / launch failure */
    OFDM_E_UNSUPPORTED = -3, /* shape not supported by this build */
    OFDM_E_IO = -4,          /* file I/O */
    OFDM_E_DEVICE = -5       /* an EARLIER launch reported a fault from the device (see
                                ofdm_device_status); its output may be incomplete */
};

int ofdm_version(void);
const char *ofdm_last_error(void);

/* ---------------------------------------------------------------- host --- */

/* Pilot rotation of matrix_readX (cpuLS.hpp:105-112, gpuLS.cu:75-82):
 * X[j] = raw[(j + (K+1)/2) mod K].  raw may equal X. */
int ofdm_pilot_rotate(const ofdm_cf32 *raw, int K, ofdm_cf32 *X);

/* matrix_readX (cpuLS.hpp:80-117 / gpuLS::matrix_readX, gpuLS.cu:53-86):
 * read K raw complex floats from `path` and rotate.  If the file cannot be
 * opened every X[j] = fill + i*fill (the reference uses 0.707 on the CPU path,
 * cpuLS.hpp:84-90, and 1.0 on the GPU path, gpuLS.cu:57-63) and 1 is
 * returned. */
int ofdm_read_pilots(const char *path, int K, float fill, ofdm_cf32 *X);

/* ------------------------------------------------------ device: stages --- */

/* Batched forward (inverse != 0: backward) unnormalised C2C FFT of nrows
 * contiguous rows of C samples, in place or out of place.
 * Replaces gpuLS::batchedFFT (gpuLS.cu:343-349) / cufftPlan1d + cufftExecC2C
 * (gpuLS.cu:377-381, 441-445) and fftOneRow (cpuLS.hpp:165-174).
 * Any 2 <= C <= 8192: powers of two up to 4096 by radix-4 Stockham stages,
 * every other length by mixed-radix stages (radices 8, 4, 2, 3, 5, 7 and a
 * direct stage with double accumulation for larger prime factors). */
int ofdm_fft_rows(const ofdm_cf32 *d_in, ofdm_cf32 *d_out, long long nrows, int C, int inverse,
                  ofdm_stream_t stream);

/* LS channel estimate from one frequency-domain pilot symbol d_Y (R x C,
 * bin 0 = DC) and the rotated pilots d_X (K values):
 *   d_Hconj[r][j] = conj(Y[r][j+1] / X[j])  (R x K)
 *   d_Hsqrd[j]    = sum_r |Hconj[r][j]|^2   (K floats)
 * Replaces findHs (gpuLS.cu:158-182) + findDistSqrd (gpuLS.cu:185-209) and
 * the post-FFT part of firstVector (cpuLS.hpp:290-311). */
int ofdm_ls_estimate(const ofdm_cf32 *d_Y, const ofdm_cf32 *d_X, int R, int C, ofdm_cf32 *d_Hconj,
                     float *d_Hsqrd, ofdm_stream_t stream);

/* MRC demodulation of nsyms frequency-domain symbols d_Y (nsyms x R x C)
 * against one estimate: d_out (nsyms x K) = rotated sum_r Y Hconj / Hsqrd.
 * Replaces multiplyWithChannelConj + combineForMRC + shiftOneRow
 * (gpuLS.cu:109-125, 212-259) and the post-FFT part of doOneSymbol
 * (cpuLS.hpp:354-368). */
int ofdm_mrc_demod(const ofdm_cf32 *d_Y, long long nsyms, const ofdm_cf32 *d_Hconj,
                   const float *d_Hsqrd, int R, int C, ofdm_cf32 *d_out, ofdm_stream_t stream);

/* MRC numerator only (matrixMultThenSum, cpuLS.hpp:187-208):
 * d_num (nsyms x K, subcarrier order, not rotated) = sum_r Y[r][j+1] Hconj[r][j].
 * With a subset of antennas this is the partial numerator of the antenna-split
 * multi-GPU path. */
int ofdm_mrc_numerator(const ofdm_cf32 *d_Y, long long nsyms, const ofdm_cf32 *d_Hconj, int R,
                       int C, ofdm_cf32 *d_num, ofdm_stream_t stream);

/* Finalise (summed) numerators: elements [e0, e0+count) of a flat
 * [nframes][nsym][K] numerator array (d_num points at element e0) are divided
 * by d_Hsqrd[f][j] ([nframes][K]) and stored rotated into d_out, the full
 * [nframes][nsym][K] output array.  (combineForMRC's divide + shiftOneRow,
 * gpuLS.cu:254-256, 109-125.) */
int ofdm_mrc_finalize(const ofdm_cf32 *d_num, long long e0, long long count, int nsym, int K,
                      const float *d_Hsqrd, ofdm_cf32 *d_out, ofdm_stream_t stream);

/* Stage-wise operations behind the reference's per-stage GPU methods, which
 * materialise their intermediates (the fused entry points above do not):
 *   ofdm_channel_conj_product: d_prod[s][r][j] = Y[s][r][j+1] * Hconj[r][j]
 *       (nsyms x R x K; multiplyWithChannelConj, gpuLS.cu:212-233)
 *   ofdm_combine_products: d_out[s][k] = sum_r prod[s][r][j] / Hsqrd[j], at
 *       k = rotated position of j if rotate != 0, else k = j
 *       (combineForMRC [+ shiftOneRow], gpuLS.cu:236-259, 109-125)
 *   ofdm_shift_rows: shiftOneRow on nrows device rows of K, out of place
 *       (gpuLS.cu:109-125, cpuLS.hpp:135-149)
 *   ofdm_dist_sqrd: d_Hsqrd[j] = sum_r |H[r][j]|^2 of an R x K matrix
 *       (findDistSqrd, gpuLS.cu:185-209, cpuLS.hpp:211-228) */
int ofdm_channel_conj_product(const ofdm_cf32 *d_Y, long long nsyms, const ofdm_cf32 *d_Hconj,
                              int R, int C, ofdm_cf32 *d_prod, ofdm_stream_t stream);
int ofdm_combine_products(const ofdm_cf32 *d_prod, long long nsyms, const float *d_Hsqrd, int R,
                          int K, int rotate, ofdm_cf32 *d_out, ofdm_stream_t stream);
int ofdm_shift_rows(const ofdm_cf32 *d_in, long long nrows, int K, ofdm_cf32 *d_out,
                    ofdm_stream_t stream);
int ofdm_dist_sqrd(const ofdm_cf32 *d_H, int R, int K, float *d_Hsqrd, ofdm_stream_t stream);

/* ------------------------------------------------------ device: frames --- */

/* Workspace for ofdm_frame_demod / ofdm_frame_demod_freq and the two-stage
 * and antenna-split calls (bytes, 256-aligned pieces): per-frame channel
 * estimates [F][R][C], |H|^2 [F][C], one 64-bit word per frame (the
 * estimate flags of the one-launch C = 1024 demod below) and, for C outside
 * {1024, 2048, 4096}
 * (no fused kernel), a frequency-domain staging buffer of at most 256 MiB.
 * A workspace carries the estimate of ONE geometry: the calls that consume it
 * (ofdm_frame_combine, ofdm_frame_mrc_partial, ofdm_frame_export_estimate,
 * ofdm_frame_noise_estimate, ofdm_frame_soft_demap)
 * must pass the nframes, S, R, C and ws_bytes of the call that filled it, and
 * return OFDM_E_ARG otherwise (checked per process, on the host, by a registry
 * keyed on d_ws).  An estimate call clears the workspace's entry before it
 * launches and records it only after every launch was enqueued, so a failed
 * estimate leaves a workspace that the consumers refuse. */
size_t ofdm_frame_workspace_bytes(long long nframes, int S, int R, int C);

/* Work tickets.  The C = 1024 one-launch demod and the C = 2048 / 4096 MRC
 * kernels (ofdm_frame_demod, _combine, _mrc_partial(_range),
 * ofdm_symbols_demod) deal their blocks to workgroups at run time through 8
 * counter words in the workspace (after the flag words).  These entry points
 * therefore WRITE the workspace, ofdm_symbols_demod's const d_ws included.
 * A counter holds tag << 32 | count with a per-launch tag, so whatever the
 * words hold when a launch starts (zeros, an earlier launch's counts, an
 * estimate of another geometry, recycled memory) is claimed afresh and never
 * consumed as a count: no zeroing, release or registry state is needed for
 * them.  One workspace serves one launch at a time (one stream, as for its
 * estimate).  Two ticketed launches that overlap on one workspace either
 * both complete (a block may be processed twice: same bytes) or one of them
 * sees the other's tag and raises the sticky device status below.
 *
 * Sticky device status: a library-owned, host-mapped word that ticketed
 * launches set when they meet a counter they cannot trust.  Every ticketed
 * entry point reads it first (no synchronisation) and, if set, clears it and
 * returns OFDM_E_DEVICE without launching anything; ofdm_device_status()
 * does the same on demand (synchronise the stream first to see the status of
 * launches still in flight).  ofdm_device_status_inject() ORs `bits` into
 * the status (tests of the reporting path; no device needed). */
int ofdm_device_status(void);
int ofdm_device_status_inject(unsigned bits);

/* Drops what the registry above knows about d_ws.  Call it before the memory
 * is freed (or handed to another user): a workspace later allocated at the
 * same address then holds no estimate until an estimate call fills it, and
 * the consumers return OFDM_E_ARG instead of dividing by a stale |H|^2.  The
 * Python binding calls it from the workspace tensor's finaliser.  NULL or an
 * unknown pointer is a no-op; always returns OFDM_OK. */
int ofdm_workspace_release(const void *d_ws);

/* Frame-batched receiver on time-domain IQ (what ShMemSymBuff delivers):
 * d_iq = nframes x S x R x (C + cp_len) samples; the cyclic prefix of every
 * row is skipped (ShMemSymBuff.hpp:309-322), each row is FFT'd, symbol 0 of
 * each frame gives the LS estimate, symbols 1..S-1 are MRC-demodulated into
 * d_out = nframes x (S-1) x K.  Replaces demodOneFrameCUDA / demodOptimized
 * (gpuLS.cu:575-769) and the cpuLS_main loop (cpuLS_main.cpp:80-92), for a
 * whole batch of frames in one call.  C in {1024, 2048, 4096} runs the fused
 * one-pass kernels (FFT + LS, FFT + MRC + normalise + rotate); at C = 1024
 * both run in ONE launch (estimator workgroups publish each frame's estimate
 * to the MRC workgroups through the workspace's flag words, agent-scope
 * release/acquire), except on a stream being captured into a graph, where
 * the two launches are used.  Every other C in [2, 8192] runs FFT, LS
 * and MRC as stages through the workspace's staging buffer. */
int ofdm_frame_demod(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                     const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out,
                     ofdm_stream_t stream);

/* ofdm_frame_demod with its two scheduling choices exposed (same results,
 * same workspace contract):
 *   flow        OFDM_FLOW_AUTO (what ofdm_frame_demod does) or
 *               OFDM_FLOW_TWO_LAUNCH (estimate, then combine, as two launches
 *               on the stream, at every C);
 *   spin_ticks  one-launch path (C = 1024): how long, in ticks of the 100 MHz
 *               device clock, an MRC workgroup waits for the estimate of a
 *               frame it reads before it estimates that frame itself (the
 *               same code and bytes as the estimator workgroup); < 0 = the
 *               default (200 000 = 2 ms), 0 = never wait.  The result does
 *               not depend on it; a shared GPU that delays the estimator
 *               workgroups only trades the wait for a re-estimate. */
#define OFDM_FLOW_AUTO 0
#define OFDM_FLOW_TWO_LAUNCH 1
int ofdm_frame_demod_ex(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                        const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out, int flow,
                        long long spin_ticks, ofdm_stream_t stream);

/* The two stages of ofdm_frame_demod, for callers that pipeline or time them
 * separately: ofdm_frame_estimate FFTs the pilot symbol of every frame and
 * stores the LS estimate (Hconj, |H|^2) in d_ws (gpuLS::firstVector,
 * gpuLS.cu:351-408, per frame); ofdm_frame_combine MRC-demodulates the data
 * symbols against it (gpuLS::demodOneSymbol, gpuLS.cu:410-473, per symbol).
 * ofdm_frame_demod == estimate then combine on the same stream. */
int ofdm_frame_estimate(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                        const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_stream_t stream);
int ofdm_frame_combine(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                       void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out, ofdm_stream_t stream);

/* One frame's LS estimate out of a workspace filled by ofdm_frame_estimate /
 * ofdm_frame_demod / ofdm_frame_demod_freq / ofdm_frame_ls_partial (same
 * nframes, S, R, C), in the reference's layout: d_Hconj[r][j] = conj(Y0/X)
 * (R x K), d_Hsqrd[j] = sum_r |Hconj[r][j]|^2 (K floats; NULL = not wanted;
 * for an ls_partial workspace the local antennas' partial sum).  These are
 * the Hconj / Hsqrd outputs of demodOneFrameCUDA (gpuLS.cu:617-629) and
 * firstVector (gpuLS.cu:392-395), which the fused kernels keep in their own
 * lane order. */
int ofdm_frame_export_estimate(const void *d_ws, size_t ws_bytes, long long nframes, int S, int R, int C,
                               long long frame, ofdm_cf32 *d_Hconj, float *d_Hsqrd, ofdm_stream_t stream);

/* Delay-domain denoising of the kept LS estimate (no reference counterpart;
 * added without a version step: OFDM_LSMRC_VERSION stays 2).  The raw LS
 * estimate carries a data bin's worth of noise in every bin; a channel no
 * longer than the cyclic prefix occupies few taps, so the taps that cannot
 * hold channel energy are zeroed and the estimate's noise falls by (kept
 * taps) / C.  In place on a workspace that holds a FULL estimate of the same
 * nframes, S, R, C, ws_bytes, of any estimator (ofdm_frame_estimate, _demod,
 * _estimate_sc16, _demod_sc16, _estimate_freq, _demod_freq, _demod_freq_mfma;
 * lane order or bin layout).  For each frame f and antenna r, with
 * H[b] = conj(Hconj[b]) for the FFT bins b = 1 .. C-1 (the receivers drop
 * bin 0):
 *   1. H[0] := (H[1] + H[C-1]) / 2        (the one bin the pilot does not cover)
 *   2. g[n]  = (1/C) sum_b H[b] e^{+2 pi i b n / C},  n = 0 .. C-1
 *   3. g[n] := 0 unless n in [0, taps_post) or n in [C - taps_pre, C)
 *      (the pre-cursor taps hold the channel when frame sync put the FFT
 *      window inside the prefix)
 *   4. H'[b] = sum_n g[n] e^{-2 pi i b n / C}
 *   5. Hconj[b] := conj(H'[b]) and Hsqrd[f][b] := sum_r |H'[r][b]|^2 for
 *      b = 1 .. C-1, the sum in order of r (no atomics: bit-identical from
 *      run to run).
 * The bin-0 position of every row and Hsqrd[f][0] stay as the estimator left
 * them, as do the workspace's flags and ticket area and its registry entry:
 * ofdm_frame_combine, _combine_sc16, _combine_freq, ofdm_symbols_demod,
 * ofdm_frame_export_estimate, ofdm_frame_noise_estimate and
 * ofdm_frame_soft_demap take the denoised workspace as they take a raw one.
 * No work tickets; the sticky device status is neither consulted nor cleared.
 * OFDM_E_ARG, before any device work: a null workspace with nframes > 0, bad
 * geometry (S < 2, R < 1, C outside [2, 8192], nframes < 0), a workspace with
 * no estimate or one of another geometry, an antenna-split partial estimate
 * (ofdm_frame_ls_partial), taps_post < 1, taps_pre < 0 or taps_post + taps_pre
 * > C.  nframes == 0 is a no-op (OFDM_OK).  taps_post + taps_pre == C keeps
 * every tap: the kernels run and return the estimate to f32 rounding. */
int ofdm_frame_estimate_denoise(void *d_ws, size_t ws_bytes, long long nframes, int S, int R, int C,
                                int taps_post, int taps_pre, ofdm_stream_t stream);

/* Soft-decision output (no reference counterpart; added without a version
 * step: OFDM_LSMRC_VERSION stays 2).  Both calls read d_z, the demodulated
 * [nframes][S-1][K] array of a frame call (rotated order, 16-B aligned), and
 * the |H|^2 sums its estimate left in d_ws: P[j] = sum_r |H[r][j]|^2, stored
 * by FFT bin for every C and every estimator, so a workspace filled by any
 * FULL estimate of the same nframes, S, R, C, ws_bytes is accepted
 * (ofdm_frame_demod, _estimate, _demod_freq, _estimate_freq, _demod_freq_mfma).
 * OFDM_E_ARG for an antenna-split partial estimate (ofdm_frame_ls_partial),
 * another geometry, a workspace without an estimate, a modulation or format
 * not listed here, a null pointer with nframes > 0, or OFDM_LLR_I8 with an
 * llr_scale that is not positive and finite; nframes == 0 is a no-op
 * (OFDM_OK).  The workspace is only read: no work tickets, and the sticky
 * device status is neither consulted nor cleared.
 *
 * Constellations: Gray-mapped, unit average energy, 3GPP TS 38.211 5.1.3-5.1.6;
 * `modulation` is the number of bits per symbol.  For the element at
 * (f, s, k), whose subcarrier is j (the inverse of the output rotation
 * above), d_llr[((f*(S-1) + s)*K + k)*bps + b], b = 0..bps-1:
 *     llr[2i]   = P[f][j] / noise_var[f] * lambda_i(Re Z)
 *     llr[2i+1] = P[f][j] / noise_var[f] * lambda_i(Im Z)
 * with, a = 1/sqrt(2), 1/sqrt(10), 1/sqrt(42), 1/sqrt(170) for bps = 2, 4,
 * 6, 8 and m_i = 2^(bps/2 - 1 - i),
 *     t_0 = x,  t_i = 2 a m_i - |t_(i-1)|,  lambda_i(x) = 4 a t_i
 *     (16-QAM: 4a x, 4a (2a - |x|); 64-QAM: 4a x, 4a (4a - |x|),
 *      4a (2a - ||x| - 4a|); 256-QAM: 8a, 4a, 2a nested likewise).
 * llr > 0 <=> bit 0 more likely.  This is the MAX-LOG approximation in its
 * recursive constant-slope form, not the exact log-sum.  ofdm_synth_frames'
 * QPSK puts the positive axis where its data bit is SET, the complement of
 * the 38.211 bit: there a hard decision llr < 0 means generator bit 0.
 * An element whose P or noise_var is not positive and finite gets llr = 0.
 * A non-finite Z with good P and noise_var gives that element's own LLRs
 * from the formulas above (NaN from a NaN; +-Inf and finite values from an
 * Inf component) and touches no other element.
 *   OFDM_LLR_F32: d_llr holds floats.
 *   OFDM_LLR_I8:  d_llr holds signed bytes clamp(rint(llr * llr_scale), -127,
 *                 127), round-to-nearest-even; -128 is never produced; a NaN
 *                 llr is stored as 0, an erasure.
 * d_llr: nframes*(S-1)*K*bps values, 16-B aligned.
 *
 * ofdm_frame_noise_estimate: decision-directed, per frame,
 *     d_noise_var[f] = mean over (s, k) of P[f][j] |Z - slice(Z)|^2,
 * slice = the nearest point of the constellation; elements whose P is 0 or
 * not finite are skipped.  A non-finite Z at an element that is not skipped
 * makes d_noise_var[f] non-finite (the demapper then zeroes frame f's LLRs);
 * the other frames' values do not change.  Z - X has variance sigma^2 / P[j], so this
 * estimates the per-antenna bin noise INCLUDING the LS estimate's own error
 * (about twice sigma^2 with equal-energy pilots and data) -- the quantity the
 * LLR scale needs.  Fixed-order reduction: bit-identical from run to run. */
enum { OFDM_MOD_QPSK = 2, OFDM_MOD_QAM16 = 4, OFDM_MOD_QAM64 = 6, OFDM_MOD_QAM256 = 8 }; /* = bits/symbol */
enum { OFDM_LLR_F32 = 0, OFDM_LLR_I8 = 1 };
int ofdm_frame_noise_estimate(const ofdm_cf32 *d_z, long long nframes, int S, int R, int C, const void *d_ws,
                              size_t ws_bytes, int modulation, float *d_noise_var, ofdm_stream_t stream);
int ofdm_frame_soft_demap(const ofdm_cf32 *d_z, long long nframes, int S, int R, int C, const void *d_ws,
                          size_t ws_bytes, int modulation, const float *d_noise_var /* [nframes], device */,
                          int llr_format, float llr_scale, void *d_llr, ofdm_stream_t stream);

/* Per-symbol receiver (gpuLS::demodOneSymbol, gpuLS.cu:410-473, which runs
 * cuFFT + multiplyWithChannelConj + combineForMRC + a CPU shift per symbol):
 * nsym consecutive time-domain data symbols d_sym (nsym x R x (C + cp_len),
 * each row's cyclic prefix skipped) demodulated against the LS estimate of
 * frame `frame` of a workspace filled by ofdm_frame_estimate (any nframes and
 * S; R, C and ws_bytes must match), in ONE fused launch (FFT + MRC +
 * normalise + rotate, each row read once) -> d_out (nsym x K).  C in {1024,
 * 2048, 4096} (else OFDM_E_UNSUPPORTED); a frequency-domain or partial
 * estimate is refused with OFDM_E_ARG. */
int ofdm_symbols_demod(const ofdm_cf32 *d_sym, long long nsym, int R, int C, int cp_len, const void *d_ws,
                       size_t ws_bytes, long long frame, ofdm_cf32 *d_out, ofdm_stream_t stream);

/* ofdm_frame_demod on frequency-domain symbols (FFT done upstream, no prefix):
 * d_Y = nframes x S x R x C.  The LS + MRC of the reference's GPU path on
 * its own (findHs + findDistSqrd, gpuLS.cu:158-209; multiplyWithChannelConj +
 * combineForMRC + shiftOneRow, gpuLS.cu:109-125, 212-259, per frame as in
 * demodOneFrameCUDA, gpuLS.cu:575-675, after its cuFFT). */
int ofdm_frame_demod_freq(const ofdm_cf32 *d_Y, long long nframes, int S, int R, int C,
                          const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out,
                          ofdm_stream_t stream);

/* Its two stages (as ofdm_frame_estimate / ofdm_frame_combine): the LS
 * estimate of every frame's pilot symbol into d_ws, then the MRC of the data
 * symbols against it.  At every C that has a fused time-domain receiver --
 * 128, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144 -- the time-domain
 * ofdm_frame_estimate leaves its estimate in that receiver's lane order:
 * ofdm_frame_combine_freq refuses such a workspace and ofdm_frame_combine
 * refuses one filled here, with OFDM_E_ARG.  (Until round 4, C = 128 / 256 /
 * 512 had no fused receiver and their time-domain estimates were in the bin
 * layout, which ofdm_frame_combine_freq accepted.)  At every other C both
 * estimators write the bin layout, and each combine accepts either one. */
int ofdm_frame_estimate_freq(const ofdm_cf32 *d_Y, long long nframes, int S, int R, int C,
                             const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_stream_t stream);
int ofdm_frame_combine_freq(const ofdm_cf32 *d_Y, long long nframes, int S, int R, int C, void *d_ws,
                            size_t ws_bytes, ofdm_cf32 *d_out, ofdm_stream_t stream);

/* ofdm_frame_demod_freq with the antenna combine on the matrix cores: per
 * subcarrier the (S-1) x R x R-by-1 product sum_r Y[s][r] Hconj[r] as
 * v_mfma_f32 tiles (mrc_mfma.hip) -- the MFMA-cgemm formulation BASELINE
 * configs[4] asks to compare with the elementwise combine.  Same results
 * within f32 rounding (antenna order per MFMA block); C >= 64. */
int ofdm_frame_demod_freq_mfma(const ofdm_cf32 *d_Y, long long nframes, int S, int R, int C,
                               const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out,
                               ofdm_stream_t stream);

/* Antenna-split pieces (time-domain frames holding this GPU's R antennas):
 * partial |H|^2 per frame into d_P ([nframes][K], sum over the local
 * antennas; sum the partials across GPUs), and partial MRC numerators
 * d_num ([nframes][S-1][K], subcarrier order; sum across GPUs, then
 * ofdm_mrc_finalize).  d_ws as for ofdm_frame_demod. */
int ofdm_frame_ls_partial(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                          const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, float *d_P,
                          ofdm_stream_t stream);
int ofdm_frame_mrc_partial(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C,
                           int cp_len, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_num,
                           ofdm_stream_t stream);
/* ofdm_frame_mrc_partial for frames [f0, f0 + count) of a batch of nframes
 * whose estimate ONE ofdm_frame_ls_partial call put in d_ws (no reference
 * counterpart: the pipelined antenna split estimates the whole batch in one
 * launch and streams the MRC in chunks).  d_iq is the whole batch, d_num
 * [count][S-1][K].  OFDM_E_ARG for a range outside [0, nframes). */
int ofdm_frame_mrc_partial_range(const ofdm_cf32 *d_iq, long long nframes, long long f0, long long count, int S,
                                 int R, int C, int cp_len, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_num,
                                 ofdm_stream_t stream);

/* ---------------------------------------------------- streaming ingest --- */

/* Pipelined receiver for IQ that lives in HOST memory (the ShMemSymBuff ring,
 * a capture file): SURVEY.md 8(f) rank 2.  `depth` device slots of
 * `chunk_frames` frames each cycle through three HIP streams -- host->device
 * copy, compute (ofdm_frame_demod), device->host copy of the outputs -- so
 * PCIe traffic in both directions overlaps the kernels.  Replaces the
 * reference's per-symbol copy + sync on a fresh stream
 * (readNextSymbolCUDA, ShMemSymBuff_gpu.hpp:375-447; createStream 364-368)
 * and the host staging of demodOneFrame (gpuLS.cu:475-573).
 *   ofdm_pipeline_create: geometry as ofdm_frame_demod; X = the K rotated
 *       pilots (host or device pointer, copied).  Device = the current one.
 *   ofdm_pipeline_acquire: the next slot's device IQ buffer (chunk_frames x S
 *       x R x (C+cp_len)) and the copy stream; the caller enqueues its own
 *       host->device copies on that stream (the ring reader does), then
 *   ofdm_pipeline_submit: demodulates the first nframes frames of that slot
 *       and copies the nframes x (S-1) x K outputs to `out` (host or device;
 *       NULL = leave them in the slot) on the output stream.
 *   ofdm_pipeline_demod: acquire + copy + submit over nframes host frames.
 *   ofdm_pipeline_sync: waits for everything submitted.
 *   ofdm_pipeline_set_denoise: with taps_post > 0 every later submit runs
 *       estimate -> ofdm_frame_estimate_denoise(taps_post, taps_pre) ->
 *       combine on the compute stream instead of ofdm_frame_demod (the sc16
 *       forms on an sc16 pipeline at C = 1024; at another C the chunk is
 *       converted and the fp32 forms run).  taps_post == 0 (with taps_pre ==
 *       0) turns it off, the state of a new pipeline: a submit then enqueues
 *       exactly what it enqueues without this call.  OFDM_E_ARG for a null
 *       pipeline, a negative value, taps_pre without taps_post, or taps_post +
 *       taps_pre > C.
 * Each call makes the pipeline's device current and restores the caller's
 * current device before returning.  A failed submit releases its slot (those
 * frames are not demodulated); the pipeline stays usable.
 * Calls return before the copies finish: `iq` and `out` must stay valid until
 * ofdm_pipeline_sync.  For copies that overlap, host buffers must be
 * page-locked (ofdm_host_register); pageable buffers work but serialise. */
typedef struct ofdm_pipeline ofdm_pipeline;
int ofdm_pipeline_create(int S, int R, int C, int cp_len, const ofdm_cf32 *X, int chunk_frames,
                         int depth, ofdm_pipeline **out);
int ofdm_pipeline_destroy(ofdm_pipeline *p);
int ofdm_pipeline_acquire(ofdm_pipeline *p, ofdm_cf32 **d_iq, ofdm_stream_t *copy_stream);
int ofdm_pipeline_submit(ofdm_pipeline *p, long long nframes, ofdm_cf32 *out);
int ofdm_pipeline_demod(ofdm_pipeline *p, const ofdm_cf32 *iq, long long nframes,
                        ofdm_cf32 *out);
int ofdm_pipeline_sync(ofdm_pipeline *p);
int ofdm_pipeline_set_denoise(ofdm_pipeline *p, int taps_post, int taps_pre);

/* Page-lock / release a host range for asynchronous DMA (hipHostRegister). */
int ofdm_host_register(void *p, size_t bytes);
int ofdm_host_unregister(void *p);

/* ------------------------------------------------------------ sc16 IQ --- */

/* Frames as the radios deliver them (no version step: OFDM_LSMRC_VERSION
 * stays 2).  The reference's drivers default the over-the-wire format to
 * sc16 (rx_and_corr.cpp:112,283, tx_same_seq_no_udp.cpp:108) and have UHD
 * widen every sample to fc32 on the host CPU (stream_args_t("fc32", otw))
 * before it enters the ring; the entries below take the 4-byte samples
 * themselves, so a host-fed receiver moves half the bytes over PCIe, keeps
 * half the IQ in HBM, and the radio process converts nothing.
 *
 * Layout: today's [nframes][S][R][C + cp_len], the element an ofdm_sc16.
 * Semantics: every *_sc16 entry is DEFINED as its fp32 counterpart applied to
 *     x = (float)i16 * scale        per component,
 * scale finite and > 0 (else OFDM_E_ARG): 1.0f / 32767 is UHD's convention,
 * 2^-15 the power of two.  Results agree with that definition to f32
 * rounding (the scale may be applied after the transform, which is linear);
 * the demodulated output does not depend on scale, the estimate does: Hconj
 * and Hsqrd in the workspace are in the units of x.
 *
 * ofdm_iq_convert_sc16: d_out[i] = {(float)re * scale, (float)im * scale}
 *     for n samples, one rounding each -- bit-exact for any scale.  d_in and
 *     d_out 16-B aligned; n == 0 is a no-op.  It is the route for every FFT
 *     length without an sc16 receiver: convert, then call any fp32 entry.
 * ofdm_frame_estimate_sc16 / _combine_sc16 / _demod_sc16: the two-launch
 *     C = 1024 receiver (ofdm_frame_estimate, ofdm_frame_combine, and
 *     ofdm_frame_demod_ex(OFDM_FLOW_TWO_LAUNCH)) instantiated on the sample
 *     type: each IQ row is read once, as 4 KiB.  Any other valid C returns
 *     OFDM_E_UNSUPPORTED before any device work (use ofdm_iq_convert_sc16).
 *     d_iq 16-B aligned; rows need 4-byte alignment only, so any cp_len
 *     works.  The workspace is the fp32 one (ofdm_frame_workspace_bytes, same
 *     layout, same registry rules), so ofdm_frame_export_estimate,
 *     ofdm_frame_noise_estimate, ofdm_frame_soft_demap and the fp32
 *     ofdm_frame_combine work on an sc16 estimate, and ofdm_frame_combine_sc16
 *     on an fp32 one.  The sticky device status is consulted as in the fp32
 *     entries.
 * ofdm_pipeline_create_sc16: an ofdm_pipeline whose slots hold sc16, so the
 *     host->device copy is half the bytes at every valid C.  At C = 1024 a
 *     submit runs ofdm_frame_demod_sc16; at every other C each slot also owns
 *     an fp32 buffer of chunk_frames frames (chunk_frames * S * R * (C +
 *     cp_len) * 8 bytes of device memory per slot, on top of the 4-byte
 *     slot), and a submit converts into it on the compute stream and runs
 *     ofdm_frame_demod.  ofdm_pipeline_acquire_sc16 / _demod_sc16 are the
 *     sc16 forms of acquire / demod; submit, sync and destroy are shared.
 *     The fp32 acquire / demod on an sc16 pipeline, and the sc16 ones on an
 *     fp32 pipeline, return OFDM_E_ARG. */
int ofdm_iq_convert_sc16(const ofdm_sc16 *d_in, long long n, float scale, ofdm_cf32 *d_out, ofdm_stream_t stream);
int ofdm_frame_demod_sc16(const ofdm_sc16 *d_iq, long long nframes, int S, int R, int C, int cp_len, float scale,
                          const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out, ofdm_stream_t stream);
int ofdm_frame_estimate_sc16(const ofdm_sc16 *d_iq, long long nframes, int S, int R, int C, int cp_len, float scale,
                             const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_stream_t stream);
int ofdm_frame_combine_sc16(const ofdm_sc16 *d_iq, long long nframes, int S, int R, int C, int cp_len, float scale,
                            void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out, ofdm_stream_t stream);
int ofdm_pipeline_create_sc16(int S, int R, int C, int cp_len, float scale, const ofdm_cf32 *X, int chunk_frames,
                              int depth, ofdm_pipeline **out);
int ofdm_pipeline_acquire_sc16(ofdm_pipeline *p, ofdm_sc16 **d_iq, ofdm_stream_t *copy_stream);
int ofdm_pipeline_demod_sc16(ofdm_pipeline *p, const ofdm_sc16 *iq, long long nframes, ofdm_cf32 *out);

/* ------------------------------------------ carrier frequency offset --- */
/* The reference's receive driver defaults its clock reference to "internal"
 * (rx_and_corr.cpp:116): free-running oscillators.  A frame is one pilot and
 * then data symbols combined against that one estimate, so a carrier
 * frequency offset (CFO) of eps subcarrier spacings turns every later symbol
 * by a further 2 pi eps (C + cp_len) / C.  These entries estimate eps per
 * frame from the cyclic prefix and remove it.
 *
 * Conventions: eps is in subcarrier spacings, cycles per C samples.  A
 * received frame is y[m] = x[m] e^{+2 pi i eps m / C}, m = s (C + cp_len) + i
 * counting the frame's samples per antenna row from the first prefix sample
 * of symbol 0, i in [0, C + cp_len).  Every frame has its own eps: d_eps is
 * float[nframes] on the device.  Every *_cfo entry is DEFINED as its fp32
 * counterpart applied to x'[f,s,r,i] = y[f,s,r,i] e^{-2 pi i eps_f m / C}, the
 * f32 value d_eps[f] taken exactly; a non-finite d_eps[f] acts as 0.  The
 * estimate left in the workspace is the estimate of x': ofdm_frame_export_
 * estimate, the soft output, ofdm_frame_estimate_denoise and either combine
 * work on it unchanged (the same fp32 workspace, size and registry rules).
 *
 * ofdm_frame_cfo_estimate: gamma_f = sum_s sum_r sum_{i = cp_skip .. cp_len-1}
 *     conj(y[f,s,r,i]) y[f,s,r,i+C]; d_eps[f] = atan2(Im gamma, Re gamma) /
 *     2 pi in (-0.5, 0.5], 0 for gamma = 0.  cp_skip leaves out the head of the
 *     prefix that the previous symbol's echo spoils.  d_gamma (ofdm_cf32
 *     [nframes]) may be null, d_eps may not.  Any 2 <= C <= 8192; only the
 *     first and last cp_len samples of each row are read.  Summed in a fixed
 *     order in float64, no atomics: bit-identical from run to run.  A NaN
 *     among the samples read makes d_gamma[f] and d_eps[f] NaN (the *_cfo
 *     entries then take that frame's eps as 0); an Inf makes d_gamma[f]
 *     non-finite and d_eps[f] NaN or a meaningless value in (-0.5, 0.5].  The
 *     other frames' values do not change.
 *     OFDM_E_ARG, before any device work: cp_len < 1, cp_skip outside
 *     [0, cp_len), bad geometry as in the other frame entries, a null pointer
 *     with nframes > 0.  nframes == 0 is a no-op.
 * ofdm_frame_cfo_derotate: d_out = x' for whole frames, prefix included.
 *     d_out == d_in is allowed, any other overlap is OFDM_E_ARG.  The route
 *     for every C without a derotating receiver (as ofdm_iq_convert_sc16 is
 *     for sc16).  Both buffers 16-byte aligned.
 * ofdm_frame_estimate_cfo / _combine_cfo / _demod_cfo: the two-launch
 *     C = 1024 receiver with the rotation applied as each row is loaded (each
 *     IQ row still read once).  Any other valid C returns OFDM_E_UNSUPPORTED
 *     before any device work (use ofdm_frame_cfo_derotate and the fp32 entry);
 *     a null d_eps with nframes > 0 is OFDM_E_ARG.  Sticky device status as in
 *     the fp32 entries.
 *   Phase accuracy (the derotator and the fused receiver alike): the phase at
 *     a symbol's start, eps s (C + cp_len) / C turns, is reduced modulo one
 *     turn in float64; only the part inside a symbol is formed in f32.
 * ofdm_pipeline_set_cfo: with on != 0 every later submit estimates eps per
 *     frame of the chunk (cp_skip as above) into a per-slot device array on
 *     the compute stream; at C = 1024 it then runs the _cfo receiver, at any
 *     other C it derotates the slot in place and runs the fp32 forms (with
 *     ofdm_pipeline_set_denoise also on: estimate -> denoise -> combine in
 *     their _cfo or derotated forms).  An sc16 pipeline at C != 1024 estimates
 *     and derotates on its converted fp32 buffer; an sc16 pipeline at
 *     C = 1024 returns OFDM_E_UNSUPPORTED.  OFDM_E_ARG for a null pipeline
 *     and, with on != 0, cp_len == 0 or cp_skip outside [0, cp_len).  on == 0
 *     (the state of a new pipeline): a submit enqueues exactly what it
 *     enqueues without this call.
 * Not covered: sc16 x CFO in one kernel, fused derotating receivers for other
 *     C, the one-launch demod, ofdm_symbols_demod, the antenna-split partials,
 *     the frequency-domain entries, integer offsets (|eps| >= 0.5: the
 *     estimator cannot see them; ofdm_lsmrc_acquire.h finds them from the
 *     pilot symbol: ofdm_frame_cfo_acquire, ofdm_pipeline_set_cfo_search),
 *     returning the pipeline's estimates to the caller, and the host C++
 *     mirrors (host/). */
int ofdm_frame_cfo_estimate(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len, int cp_skip,
                            ofdm_cf32 *d_gamma, float *d_eps, ofdm_stream_t stream);
int ofdm_frame_cfo_derotate(const ofdm_cf32 *d_in, ofdm_cf32 *d_out, long long nframes, int S, int R, int C,
                            int cp_len, const float *d_eps, ofdm_stream_t stream);
int ofdm_frame_estimate_cfo(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                            const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, const float *d_eps,
                            ofdm_stream_t stream);
int ofdm_frame_combine_cfo(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len, void *d_ws,
                           size_t ws_bytes, ofdm_cf32 *d_out, const float *d_eps, ofdm_stream_t stream);
int ofdm_frame_demod_cfo(const ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                         const ofdm_cf32 *d_X, void *d_ws, size_t ws_bytes, ofdm_cf32 *d_out, const float *d_eps,
                         ofdm_stream_t stream);
int ofdm_pipeline_set_cfo(ofdm_pipeline *p, int on, int cp_skip);

/* ------------------------------------------------------ phase tracking --- */

/* Decision-directed carrier phase tracking between the combiner and the
 * demapper (no reference counterpart; added without a version step:
 * OFDM_LSMRC_VERSION stays 2).  A frame is one pilot and then up to 100 data
 * symbols combined against that one estimate: whatever offset the prefix
 * estimator leaves, eps_res, turns every later symbol by a further
 * 2 pi eps_res (C + cp_len) / C, and oscillator phase noise adds to it.
 *
 * ofdm_frame_phase_track reads d_z, the demodulated [nframes][S-1][K] array of
 * a frame call (rotated order), and the |H|^2 sums P its estimate left in
 * d_ws (as the soft output reads them: P[f][j(k)], j(k) the subcarrier at
 * output position k), and writes the derotated array d_out and, if d_phase is
 * not null, the tracked phase of every data symbol.  For frame f the rows
 * n = 0 .. S-2 (data symbols 1 .. S-1) are processed in order from
 * theta_(-1) = theta_(-2) = 0 (the pilot symbol is phase 0 by construction):
 *   1. phi = theta_(n-1) + (theta_(n-1) - theta_(n-2))
 *      (linear extrapolation: a constant drift costs nothing)
 *   2. w_k = z_k e^{-i phi},  d_k = slice(w_k), the nearest point of the
 *      38.211 constellation (`modulation` as in the soft output): per axis
 *      t = clamp(floor(x / 2a), -L, L-1), L = 2^(bps/2 - 1), point a (2t + 1)
 *   3. g = sum_k P[f][j(k)] w_k conj(d_k); elements whose P is not positive
 *      and finite are skipped.  Fixed-order reduction, no atomics:
 *      bit-identical from run to run.
 *   4. delta = atan2(Im g, Re g), 0 when g is 0 or not finite (one bad symbol
 *      does not poison the rest of the frame);  theta_n = phi + delta
 *   5. d_out[f][n][k] = z_k e^{-i theta_n} for every k, skipped elements
 *      included;  d_phase[f*(S-1) + n] = theta_n in radians, unwrapped
 *      (cumulative: tens of radians over 100 symbols), f32.
 * theta is carried in float64; only its value modulo one turn goes through
 * an f32 sincos.  The slope of d_phase over a frame gives the residual offset
 * back: eps_res = sum_n' n' theta_(n'-1) / sum_n' n'^2 * C / (2 pi (C + cp_len)),
 * n' = 1 .. S-1.
 * d_z and d_out: 8-byte aligned, d_out == d_z (in place) or disjoint; d_phase
 * disjoint from both.  The workspace goes through the registry as for
 * ofdm_frame_soft_demap: any FULL estimate of the same nframes, S, R, C,
 * ws_bytes; it is only read, no work tickets, and the sticky device status is
 * neither consulted nor cleared.  Before any device work: OFDM_E_ARG for a
 * modulation not listed, nframes < 0, S < 2, R < 1, a null or misaligned d_z,
 * d_out or d_ws with nframes > 0, buffers that overlap otherwise, an
 * antenna-split partial estimate, another geometry or a workspace without an
 * estimate; OFDM_E_UNSUPPORTED for C outside [2, 8192].  nframes == 0 is a
 * no-op (OFDM_OK).
 *
 * ofdm_pipeline_set_phase_track: with modulation 2, 4, 6 or 8 every later
 * submit runs the tracker in place on the slot's output, on the compute
 * stream, after whichever receiver form the submit used (fp32, sc16, CFO,
 * denoise) and before the copy-out.  0 turns it off (the state of a new
 * pipeline): a submit then enqueues exactly what it enqueues without this
 * call.  OFDM_E_ARG for a null pipeline or another modulation.  The
 * per-symbol phases are not handed back (as the CFO estimates are not).
 * Not covered: the tracker fused into the receivers' epilogues, tracking on
 * pilot subcarriers, and returning the pipeline's phases. */
int ofdm_frame_phase_track(const ofdm_cf32 *d_z, long long nframes, int S, int R, int C, const void *d_ws,
                           size_t ws_bytes, int modulation, ofdm_cf32 *d_out,
                           float *d_phase /* [nframes][S-1] or NULL */, ofdm_stream_t stream);
int ofdm_pipeline_set_phase_track(ofdm_pipeline *p, int modulation);

/* ------------------------------------------------------ PN frame sync --- */

/* Frame synchronisation of the receive driver, on
 * the device.  ofdm_pn_correlate replaces the sliding correlator of
 * rx_and_corr.cpp:332-360: for channel ch = 0..R-1 and lag i = 0..N-L in that
 * order, v = |sum_j pn[j] * buf[ch][i+j]| / L (no conjugate, as the
 * reference); the first (ch, i) with v >= thres is the hit.  d_buf: R rows of
 * N samples; d_pn: L samples.  *d_pos (device) = ch * (N-L+1) + i, or -1 if
 * no lag reaches thres.  d_mag (optional, R x (N-L+1) floats, NULL = not
 * stored) receives v for every lag (then no lag is skipped).  The index is
 * bit-exact with the reference: each lag is summed in its f32 order.
 *
 * ofdm_pn_extract replaces the copy_buff assembly (rx_and_corr.cpp:370-392)
 * and copy_to_shared_mem (64-87): with lag = *d_pos mod (N-L+1), each
 * channel's N-L samples after the PN -- d_buf1[ch][lag+L..N) then
 * d_buf2[ch][0..lag) -- are cut into nsym symbols of C+cp samples with the
 * cyclic prefix dropped, d_sym[s][ch][k] = seq[s*(C+cp)+cp+k]: the ring's
 * symbol layout, ready for ofdm_frame_demod (cp_len 0).  Nothing is written
 * when *d_pos < 0.  nsym*(C+cp) <= N-L. */
int ofdm_pn_correlate(const ofdm_cf32 *d_buf, int R, long long N, const ofdm_cf32 *d_pn, int L,
                      float thres, long long *d_pos, float *d_mag, ofdm_stream_t stream);
int ofdm_pn_extract(const ofdm_cf32 *d_buf1, const ofdm_cf32 *d_buf2, int R, long long N, int L,
                    const long long *d_pos, int C, int cp, int nsym, ofdm_cf32 *d_sym,
                    ofdm_stream_t stream);

/* ------------------------------------------------------ zero forcing --- */

/* Multi-user zero forcing, U users x R antennas per
 * subcarrier, K subcarriers (the reference passes cols and uses K = cols-1).
 *
 * ofdm_zf_precoder replaces createZeroForcingMatrix (cpuLS.hpp:415-447):
 *   d_H: users x rows x K channel cube, the layout the reference hands to
 *   rotCube (cpuLS.hpp:400-413, X[user*rows*cols + row*cols + col]); it is
 *   not modified (the reference rotates it in place).  Per subcarrier k,
 *   A(u, r) = H[u][r][k], G = A A^H, W = A^H G^-1 (R x U), inverted by
 *   Gauss-Jordan with partial pivoting in f32 (the reference: cgetrf +
 *   cgetri; results agree to f32 rounding of a well-conditioned G, not
 *   bit-for-bit).  Outputs (either may be NULL, not both):
 *     d_W  [K][U][R]: W(r, u) at d_W[k*R*U + u*R + r] -- the reference's H
 *          output (cgemm ldc = rows, cpuLS.hpp:440);
 *     d_Wt [U][R][K]: W(r, u) at d_Wt[(u*R + r)*K + k] -- the layout
 *          ofdm_zf_apply / ofdm_zf_detect read (subcarrier-fastest).
 * ofdm_zf_transpose: d_W (reference layout) -> d_Wt.
 * ofdm_zf_apply replaces multiplyWithChannelInv (cpuLS.hpp:449-463, cgemv
 *   per subcarrier) for nsym symbols at once: d_Y[s][r][k] = sum_u W(r, u)
 *   d_X[s][u][k]  (X: nsym x U x K, Y: nsym x R x K).
 * ofdm_zf_detect (uplink counterpart, no reference function):
 *   d_X[s][u][k] = sum_r conj(W(r, u)) d_Y[s][r][k] -- W^H = G^-1 A is the
 *   pseudo-inverse of the R x U uplink channel A^H.
 * Limits: 1 <= users <= OFDM_ZF_MAX_USERS, users*rows <= OFDM_ZF_MAX_USERS_X_ROWS. */
#define OFDM_ZF_MAX_USERS 32
#define OFDM_ZF_MAX_USERS_X_ROWS 8192
int ofdm_zf_precoder(const ofdm_cf32 *d_H, int users, int rows, int K, ofdm_cf32 *d_W, ofdm_cf32 *d_Wt,
                     ofdm_stream_t stream);
int ofdm_zf_transpose(const ofdm_cf32 *d_W, int users, int rows, int K, ofdm_cf32 *d_Wt,
                      ofdm_stream_t stream);
int ofdm_zf_apply(const ofdm_cf32 *d_Wt, const ofdm_cf32 *d_X, int users, int rows, int K, long long nsym,
                  ofdm_cf32 *d_Y, ofdm_stream_t stream);
int ofdm_zf_detect(const ofdm_cf32 *d_Wt, const ofdm_cf32 *d_Y, int users, int rows, int K, long long nsym,
                   ofdm_cf32 *d_X, ofdm_stream_t stream);
/* ofdm_zf_apply on row-padded layouts (no reference counterpart):
 * d_X[(s*users + u)*ldx + k] and d_Y[(s*rows + r)*ldy + k], ldx, ldy >= K
 * (ldx = ldy = K is ofdm_zf_apply); pitches other than K need K >= 2,
 * rows >= 8 and users <= 40 (else OFDM_E_UNSUPPORTED). */
int ofdm_zf_apply_ex(const ofdm_cf32 *d_Wt, const ofdm_cf32 *d_X, long long ldx, int users, int rows, int K,
                     long long nsym, ofdm_cf32 *d_Y, long long ldy, ofdm_stream_t stream);
/* ofdm_zf_detect on row-padded layouts (no reference counterpart):
 * d_Y[(s*rows + r)*ldy + k] and d_X[(s*users + u)*ldx + k], ldy, ldx >= K
 * (the pad is neither read nor written; ldy = ldx = K is ofdm_zf_detect).
 * Rows padded to a multiple of 16 elements (K = 1023 -> 1024) start on
 * 128-B lines, so no part of a line is left for another workgroup to
 * complete.  Pitches other than K need rows <= 72 (else OFDM_E_UNSUPPORTED). */
int ofdm_zf_detect_ex(const ofdm_cf32 *d_Wt, const ofdm_cf32 *d_Y, long long ldy, int users, int rows, int K,
                      long long nsym, ofdm_cf32 *d_X, long long ldx, ofdm_stream_t stream);

/* ------------------------------------------------------ OFDM modulator --- */

/* The reference's transmit helpers in one pass per row (no version step:
 * OFDM_LSMRC_VERSION stays 2): modOneSymbol / modRefSymbol
 * (cpuLS.hpp:466-529) = bin placement with ifftShiftOneRow (119-132), the
 * backward transform (ifftOneRow, 152-162), the per-row peak normalisation
 * (clange_ 'M' then cblas_csscal, 521-523) and addPrefix (391-398).
 *
 * Input:  d_X[row*ldx + k], k < K = C - 1, ldx >= K; the pad is never read.
 *         ldx = K is the layout of modOneSymbol's X and of ofdm_zf_apply's
 *         output, ldx = 1024 takes ofdm_zf_apply_ex's padded rows (K = 1023).
 * Output: d_iq[row*(C+cp_len) + n]: the prefix (the row's last cp_len
 *         samples) first, then its C samples (addPrefix, cpuLS.hpp:394-395) --
 *         the ring's `symbol` layout, so nrows = F*S*R rows written in order
 *         are directly an input of ofdm_frame_demod.
 *         d_peak (NULL = not wanted): d_peak[row] = max_n |x[n]| of the
 *         transformed row BEFORE scaling, |x| = sqrt(re^2 + im^2) -- what
 *         clange_ returns; with OFDM_TX_NORM_PEAK the gain 1/d_peak[row] a
 *         caller needs to undo.
 * Bin placement (which bin of the transform carries X[k]):
 *   OFDM_TX_MAP_REFERENCE  modOneSymbol's, literally (cpuLS.hpp:511-513):
 *         d[0] = 0, d[k+1] = X[k], then ifftShiftOneRow's three memmoves with
 *         h = C/2 (integer): bin[i] = d[i+h] (i < h), bin[i] = d[i-h]
 *         (h <= i < 2h) and, for odd C, bin[C-1] = d[C-1] left in place.  For
 *         even C, X[k] sits at bin (k + 1 + C/2) mod C: bin C/2 is empty and
 *         bin 0 (DC) carries X[C/2 - 1], which the receivers drop
 *         (cpuLS.hpp:290-292) -- the reference's transmitter and receiver do
 *         not agree; reproduced, not repaired.
 *   OFDM_TX_MAP_RX  the placement the receivers undo: row position k at bin
 *         out_src(k) + 1, out_src the inverse of shiftOneRow's output rotation
 *         (cpuLS.hpp:135-149, the three memmoves for any K, even K included);
 *         bin 0 empty.  A frame whose symbol 0 is the RAW pilot file order
 *         (before matrix_readX's rotation, cpuLS.hpp:105-112) and whose
 *         symbols 1..S-1 are data rows comes back from ofdm_frame_demod(X =
 *         ofdm_pilot_rotate(raw)) as those data rows.
 * Transform: backward, unnormalised, e^(+2 pi i n k / C) (FFTW_BACKWARD,
 *   cpuLS.hpp:157).
 * Scaling:
 *   OFDM_TX_NORM_PEAK   row * (1 / max_n |x[n]|) (maxval = 1 / clange_, then
 *         csscal, cpuLS.hpp:521-523; `scale` ignored).  An all-zero row is
 *         stored as zeros with d_peak = 0; the reference would store NaN
 *         (0 * (1/0)).
 *   OFDM_TX_NORM_SCALE  row * scale (scale = 1: the bare unnormalised IFFT).
 *   Non-finite inputs propagate.
 * Limits: 2 <= C <= 8192, 0 <= cp_len <= C, nrows >= 0; d_X, d_iq 8-B
 * aligned.  Anything else is OFDM_E_ARG, before any device work; nrows == 0
 * is OFDM_OK and launches nothing.  C = 1024 runs one wave per row (16-B
 * stores when cp_len is even and d_iq is 16-B aligned), every other C one
 * workgroup per row on the mixed-radix stages of ofdm_fft_rows. */
#define OFDM_TX_MAP_REFERENCE 0
#define OFDM_TX_MAP_RX 1
#define OFDM_TX_NORM_PEAK 0
#define OFDM_TX_NORM_SCALE 1
int ofdm_tx_modulate(const ofdm_cf32 *d_X, long long ldx, long long nrows, int C, int cp_len, int map, int norm,
                     float scale, ofdm_cf32 *d_iq, float *d_peak /* nullable */, ofdm_stream_t stream);

/* --------------------------------------------------- synthetic frames --- */

/* Deterministic synthetic frames for tests and benchmarks:
 * H ~ CN(0,1) per (frame, antenna, subcarrier), pilot = d_X, data = QPSK,
 * bins j+1 carry H x (bin 0 empty), y = IFFT(Y)/sqrt(C) + CN(0, noise_std^2)
 * with a cyclic prefix (freq_domain = 0), or y = Y + noise (freq_domain = 1,
 * cp_len ignored).  Frame f of the buffer is global frame frame0 + f; antenna
 * r is global antenna r0 + r (antenna-split shards). */
int ofdm_synth_frames(ofdm_cf32 *d_iq, long long nframes, int S, int R, int C, int cp_len,
                      const ofdm_cf32 *d_X, unsigned long long seed, long long frame0,
                      float noise_std, int freq_domain, int r0, ofdm_stream_t stream);

/* Adds to *d_errors the number of demodulated symbols in d_out
 * (nframes x (S-1) x K) whose QPSK hard decision differs from the synthetic
 * data of ofdm_synth_frames(seed, frame0). */
int ofdm_count_symbol_errors(const ofdm_cf32 *d_out, long long nframes, int S, int C,
                             unsigned long long seed, long long frame0,
                             unsigned long long *d_errors, ofdm_stream_t stream);

/* Host-mirror helper (no reference counterpart): an order-sensitive 64-bit
 * hash of `bytes` (a multiple of 4) of device memory into *d_hash (device).
 * gpuLS::demodOneSymbol hashes the caller's Hconj / Hsqrd to tell whether
 * they still hold the estimate firstVector exported (gpuLS.cu:410-473 reads
 * them afresh for every symbol). */
int ofdm_buffer_hash(const void *d_buf, size_t bytes, unsigned long long *d_hash, ofdm_stream_t stream);

/* Box probe for bench.py (no reference counterpart): mode 0 copies `bytes`
 * from d_src to d_dst, mode 1 reads them (d_dst receives 1024 x 256 float
 * partial sums, OFDM_HBM_PROBE_SINK_BYTES): every wave streams 16 KiB chunks
 * with 16 non-temporal 16-B loads per lane in flight -- the receivers' access
 * pattern.  `bytes` and both pointers 16-B aligned; dst_bytes = the size of
 * d_dst, at least `bytes` (mode 0) or OFDM_HBM_PROBE_SINK_BYTES (mode 1),
 * else OFDM_E_ARG. */
#define OFDM_HBM_PROBE_SINK_BYTES (1024 * 256 * 4)
int ofdm_hbm_probe(int mode, const void *d_src, void *d_dst, size_t bytes, size_t dst_bytes,
                   ofdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_LSMRC_H_ */
