/*
 * ofdm_lsmrc_decode.h -- Viterbi decoding of constraint-length-7 convolutional
 * codes on the demapper's LLRs.  An extension of ofdm_lsmrc.h: same library
 * (libofdm_lsmrc.so), same conventions, same error codes, no version step
 * (OFDM_LSMRC_VERSION stays 2).  It is a header of its own for the reason
 * ofdm_lsmrc_acquire.h gives: the main header's symbol set stays what its
 * tables list.
 *
 * Why: ofdm_frame_soft_demap writes "soft output for a channel decoder", and
 * OFDM_LLR_I8 exists only as a decoder's input format.  Without a decoder on
 * the device a user who wants bits copies every LLR to the host, more bytes
 * than the receiver's own output.  The code is the K = 7 one of 802.11, DVB
 * and CCSDS (0133 / 0171 octal at rate 1/2, with 0165 at rate 1/3, and the
 * punctured rates 2/3 and 3/4); any other generators of 7 bits are taken too.
 * Metrics are integers on int8 LLRs: the result is defined exactly, below.
 *
 * The code (ofdm_conv_code).  n_out = 2 or 3 coded bits per input bit;
 * generators g[i], 7 bits each, 1..127: bit 6 taps the current input bit u_t,
 * bit 6-d taps u_(t-d); g[2] is ignored when n_out == 2.  terminated = 1: six
 * zero tail bits were encoded, start and end state 0; terminated = 0:
 * truncated, start state 0, end at the best state.  punct_period p: 0 =
 * unpunctured, else p >= 1 and p * n_out <= 32; bit (t mod p) * n_out + i of
 * punct_mask set <=> coded bit i of step t was sent (802.11 rate 2/3: p = 2,
 * mask 0x7; rate 3/4: p = 3, mask 0x27).
 *
 * Steps and positions.  L information bits make T = L + 6 steps when
 * terminated, T = L otherwise.  Mother position (t, i) is coded bit i of step
 * t; it was sent iff p = 0 or its mask bit is set.  n_rx is the number of sent
 * positions among the T * n_out (ofdm_conv_coded_len: host arithmetic, no
 * device call).  Codeword c reads its n_rx LLRs at elements c * cw_stride ..
 * c * cw_stride + n_rx - 1 of d_llr, in the order (t, i), t slow, unsent
 * positions skipped.  No element outside those ranges is read or influences
 * any output.  d_llr needs only its element type's alignment: a codeword may
 * start at any element.
 *
 * Quantisation, to an integer q in [-127, 127] per position:
 *   OFDM_LLR_I8   q = max(value, -127); llr_scale is not consulted.
 *   OFDM_LLR_F32  q = clamp(rint(llr * llr_scale), -127, 127), round to nearest
 *                 even, NaN -> 0, +-Inf -> +-127: ofdm_frame_soft_demap's int8
 *                 rule, so decoding f32 LLRs with scale s is bit-identical to
 *                 decoding the bytes the demapper writes with llr_scale = s
 *                 from the same values.
 * An unsent position has q = 0.  llr > 0 <=> bit 0 more likely, as in the main
 * header.
 *
 * Trellis.  State s_t holds u_(t-1) at bit 5 .. u_(t-6) at bit 0; register
 * r = (u_t << 6) | s_t; coded bit c_i = parity(r & g[i]); next state
 * s_(t+1) = r >> 1.  Branch metric = sum_i (1 - 2 c_i) q(t, i), in integers;
 * the path metric is maximised.  At step t state s' has two candidates
 * b = 0, 1 with r = (s' << 1) | b: predecessor r & 63, input bit s' >> 5.  The
 * larger candidate survives; on equality b = 0 survives.  Only paths that start
 * in state 0 exist.  End state: 0 when terminated, otherwise the state with the
 * largest metric, the lowest index on equality.  The traceback from the end
 * state gives u_0 .. u_(T-1); the output is u_0 .. u_(L-1).  These rules make
 * the output unique; the kernel's arithmetic reproduces every comparison
 * (int32 metrics: |metric| <= 65536 * 3 * 127 < 2^25).
 *
 * Outputs.  Bits are packed: bit t of codeword c is bit (t & 7) of byte
 * c * out_stride + (t >> 3) of d_bits.  Exactly ceil(L / 8) bytes per codeword
 * are written, pad bits 0; the stride's other bytes are not touched.
 * d_metric[c], when d_metric is not null, is sum_j (1 - 2 c^_j) q_j over the
 * n_rx received positions, c^ the re-encoding of the decoded bits, tail
 * included: the surviving path's metric, int32.  No atomics; bit-identical
 * from run to run.
 *
 * ofdm_conv_coded_len and ofdm_viterbi_workspace_bytes check the code and L
 * (and ncw) as ofdm_viterbi_decode does and make no device call.
 *
 * Workspace.  ofdm_viterbi_workspace_bytes is 0 while T <= 4096 (the survivor
 * decisions, 8 bytes per step, stay in LDS; d_scratch may then be null) and
 * 8 * T * min(ncw, 1024) bytes beyond: one launch round keeps at most 1024
 * long codewords resident, further ones reuse the slots.  That is within
 * 8 * T * min(ncw, 4096) + 4096 for every ncw.  d_scratch needs 8-byte
 * alignment; its contents before and after a call mean nothing.
 *
 * ofdm_viterbi_decode, before any device work, in this order:
 *   OFDM_E_ARG          a null code; n_out not 2 or 3; a generator outside
 *                       1..127; punct_period < 0 or p * n_out > 32; punct_mask
 *                       bits at or above p * n_out (p = 0: any mask bit); a
 *                       mask with no sent bit; L < 1; ncw < 0
 *   OFDM_E_UNSUPPORTED  L > 65530 (up to there T <= 65536)
 *   OFDM_E_ARG          llr_format not OFDM_LLR_F32 / OFDM_LLR_I8; OFDM_LLR_F32
 *                       with an llr_scale that is not positive and finite;
 *                       cw_stride < n_rx; out_stride < ceil(L / 8)
 *   (ncw == 0 is a no-op here: OFDM_OK)
 *   OFDM_E_ARG          a null d_llr or d_bits; scratch_bytes below
 *                       ofdm_viterbi_workspace_bytes, or a null d_scratch where
 *                       that is not 0; d_llr misaligned for its element type,
 *                       d_metric not 4-byte aligned, d_scratch not 8-byte
 *                       aligned; d_bits, d_metric, d_scratch (the bytes the call
 *                       uses) or the LLR range overlapping one another
 * No work tickets; the sticky device status is neither consulted nor cleared.
 *
 * Not covered: tail-biting, soft output (SOVA / BCJR), other constraint
 * lengths, an encoder on the device, interleavers, a pipeline hook, the host
 * C++ mirrors (host/).
 */
#ifndef OFDM_LSMRC_DECODE_H_
#define OFDM_LSMRC_DECODE_H_

#include "ofdm_lsmrc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ofdm_conv_code {
    int      n_out;        /* coded bits per input bit: 2 or 3 */
    int      g[3];         /* generators, 7 bits each, 1..127; g[2] ignored when n_out == 2 */
    int      terminated;   /* 1: six zero tail bits, end state 0; 0: truncated, end at the best state */
    int      punct_period; /* p: 0 = unpunctured, else 1 <= p and p * n_out <= 32 */
    unsigned punct_mask;   /* bit (t mod p) * n_out + i set <=> coded bit i of step t was sent */
} ofdm_conv_code;

int ofdm_conv_coded_len(const ofdm_conv_code *code, int L, long long *n_rx);
int ofdm_viterbi_workspace_bytes(const ofdm_conv_code *code, int L, long long ncw, size_t *bytes);
int ofdm_viterbi_decode(const void *d_llr, int llr_format, float llr_scale, long long cw_stride,
                        long long ncw, int L, const ofdm_conv_code *code,
                        unsigned char *d_bits, long long out_stride, int *d_metric /* [ncw] or NULL */,
                        void *d_scratch, size_t scratch_bytes, ofdm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_LSMRC_DECODE_H_ */
