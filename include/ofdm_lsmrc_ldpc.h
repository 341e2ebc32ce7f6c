/*
 * ofdm_lsmrc_ldpc.h -- layered min-sum decoding of quasi-cyclic LDPC codes on
 * the demapper's LLRs.  An extension of ofdm_lsmrc.h: same library
 * (libofdm_lsmrc.so), same conventions, same error codes, no version step
 * (OFDM_LSMRC_VERSION stays 2).  It is a header of its own for the reason
 * ofdm_lsmrc_acquire.h gives: the other headers' symbol sets stay what their
 * tables list.
 *
 * Why: ofdm_lsmrc_decode.h decodes the K = 7 convolutional code of 802.11a/g,
 * DVB and CCSDS.  5G NR data channels and 802.11n/ac/ax use quasi-cyclic LDPC
 * codes; without a decoder for them on the device every LLR is copied to the
 * host.  The caller supplies the base matrix, so no standard's tables live
 * here.  The arithmetic is integer and defined exactly, below: the output is
 * unique, bit for bit.
 *
 * The code (ofdm_qc_ldpc, host arrays).  mb base rows, nb base columns,
 * lifting size Z, in row-compressed form: row_ptr[mb + 1] (row_ptr[0] = 0,
 * nnz = row_ptr[mb]), col[nnz], shift[nnz].  Entry e of base row r
 * (row_ptr[r] <= e < row_ptr[r + 1]) is the Z x Z identity cyclically shifted
 * by shift[e]: check r * Z + i is connected to variable
 * col[e] * Z + ((i + shift[e]) mod Z), 0 <= i < Z.  N = nb * Z variables,
 * M = mb * Z checks.  Limits: 2 <= Z <= 384, 1 <= mb < nb, N <= 32768, every
 * row of degree 2 .. 32, columns strictly increasing within a row (so no
 * variable appears twice in a layer and a layer's Z checks touch disjoint
 * variables), 0 <= shift < Z.
 *
 * Handle.  ofdm_ldpc_code_create checks the code and copies it; the caller's
 * arrays may go afterwards.  It makes no device call.  In this order:
 *   OFDM_E_ARG          a null code or handle pointer; null row_ptr, col or
 *                       shift; mb < 1; nb <= mb; Z < 2; row_ptr[0] != 0; a row
 *                       of degree below 2 (a decreasing row_ptr included); a
 *                       column outside 0 .. nb - 1 or not above its predecessor
 *                       in the row; a shift outside 0 .. Z - 1
 *   OFDM_E_UNSUPPORTED  (a code that is valid but for its size) Z > 384; a row
 *                       of degree above 32; N > 32768
 * Every OFDM_E_ARG fault of any row answers before a size limit does.
 * ofdm_ldpc_code_destroy releases the handle and its device table; a null or
 * unknown handle is OFDM_E_ARG.  A destroyed handle is unknown to every entry.
 * The base table (4 * (mb + 1 + nnz) bytes) reaches the device at the first
 * ofdm_ldpc_decode with that handle that launches anything, by one allocation
 * and one synchronous copy on the current device, and stays there until
 * destroy; every refusal comes before that and needs no device.  Under stream
 * capture: make the first decode with a handle before the capture begins.
 * Later decodes are one kernel launch on `stream` and capture like any other;
 * a first decode inside a capture fails with OFDM_E_HIP (the copy is not
 * capturable) and the capture is lost.  A handle serves the device its table
 * went to.
 *
 * Input.  Codeword c reads n_rx LLRs at elements c * cw_stride ..
 * c * cw_stride + n_rx - 1 of d_llr; they are positions pos0 ..
 * pos0 + n_rx - 1 of the codeword.  Every other position has q = 0 (punctured
 * leading columns, a punctured tail: no copy needed).  Quantisation to an
 * integer q in [-127, 127] is ofdm_viterbi_decode's:
 *   OFDM_LLR_I8   q = max(value, -127); llr_scale is not consulted.
 *   OFDM_LLR_F32  q = clamp(rint(llr * llr_scale), -127, 127), round to nearest
 *                 even, NaN -> 0, +-Inf -> +-127: ofdm_frame_soft_demap's int8
 *                 rule, so decoding f32 LLRs with scale s is bit-identical to
 *                 decoding the bytes the demapper writes with llr_scale = s.
 * llr > 0 <=> bit 0 more likely.  d_llr needs only its element type's
 * alignment; a codeword may start at any element.  No element outside the
 * stated ranges is read or influences any output.
 *
 * Arithmetic, all in integers.  The posterior L[v] starts at q_v; the
 * check-to-variable messages R start at 0.  One iteration is the base rows
 * r = 0 .. mb - 1 in order (layers); within a layer the Z checks are
 * independent.  For a check with edges j = 0 .. d - 1, in the row's column
 * order, to the variables v_j:
 *   T_j   = L[v_j] - R_j;   s_j = (T_j < 0);   a_j = |T_j|
 *   S     = xor of all s_j
 *   idx   = the first j attaining min a_j;  min1 = a_idx;
 *   min2  = min over j != idx of a_j
 *   mu_j  = min2 if j == idx, else min1
 *   mu'_j = min(127, max(0, ((mu_j * norm16) >> 4) - offset))
 *   R'_j  = -mu'_j if S xor s_j, else mu'_j
 *   L[v_j] = clamp(T_j + R'_j, -16383, 16383);   R_j <- R'_j
 * norm16 in 1 .. 16 and offset in 0 .. 127: (16, 0) is plain min-sum, (12, 0)
 * normalised by 0.75, (16, b) offset min-sum.  With |R| <= 127 no 16-bit
 * intermediate overflows.  After an iteration x_v = (L[v] < 0); the syndrome
 * is zero iff every check's xor of its x is 0.
 *   early_stop = 1: stop after the first iteration whose syndrome is zero
 *                   (at most max_iter iterations).
 *   early_stop = 0: exactly max_iter iterations, the syndrome evaluated once,
 *                   at the end.
 * d_iters[c], when d_iters is not null, is +k, the iterations run, when the
 * final syndrome is zero, and -k otherwise.
 *
 * Output: the first n_bits of x, packed as the Viterbi decoder packs: bit t of
 * codeword c is bit (t & 7) of byte c * out_stride + (t >> 3) of d_bits.
 * Exactly ceil(n_bits / 8) bytes per codeword are written, pad bits 0; the
 * stride's other bytes are not touched.  No atomics; bit-identical from run
 * to run.
 *
 * Workspace.  The kernel keeps L (2 N bytes) and the messages (one byte per
 * edge, nnz * Z) of a codeword in LDS while 2 N + nnz * Z <= 65536:
 * ofdm_ldpc_workspace_bytes is then 0 and d_scratch may be null.  Beyond, the
 * messages live in d_scratch: nnz * Z * min(ncw, 1024) bytes (a launch keeps
 * at most 1024 such codewords resident, further ones reuse the slots), which
 * is within 32 * M * min(ncw, 1024) for every code and ncw.  d_scratch needs
 * no alignment; its contents before and after a call mean nothing.
 *
 * ofdm_ldpc_workspace_bytes: OFDM_E_ARG for a null or destroyed handle,
 * ncw < 0, a null bytes pointer, in this order; no device call.
 *
 * ofdm_ldpc_decode, before any device work, in this order:
 *   OFDM_E_ARG  a null or destroyed handle
 *   OFDM_E_ARG  llr_format not OFDM_LLR_F32 / OFDM_LLR_I8; OFDM_LLR_F32 with an
 *               llr_scale that is not positive and finite; pos0 < 0, n_rx < 1
 *               or pos0 + n_rx > N; cw_stride < n_rx; n_bits outside 1 .. N;
 *               out_stride < ceil(n_bits / 8); max_iter outside 1 .. 1000;
 *               norm16 outside 1 .. 16; offset outside 0 .. 127; early_stop not
 *               0 or 1; ncw < 0
 *   (ncw == 0 is a no-op here: OFDM_OK)
 *   OFDM_E_ARG  a null d_llr or d_bits; scratch_bytes below
 *               ofdm_ldpc_workspace_bytes, or a null d_scratch where that is
 *               not 0; d_llr misaligned for its element type; d_iters not
 *               4-byte aligned; d_bits, d_iters, d_scratch (the bytes the call
 *               uses) or the LLR range (gaps included) overlapping one another
 * No work tickets; the sticky device status is neither consulted nor cleared.
 *
 * Not covered: the NR / 802.11n base-graph tables themselves, filler bits and
 * repetition in rate matching, an encoder on the device, a pipeline that
 * delivers bits, soft output, the host C++ mirrors (host/).
 */
#ifndef OFDM_LSMRC_LDPC_H_
#define OFDM_LSMRC_LDPC_H_

#include "ofdm_lsmrc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ofdm_qc_ldpc {
    int        mb;      /* base rows (layers) */
    int        nb;      /* base columns, > mb */
    int        Z;       /* lifting size, 2 .. 384 */
    const int *row_ptr; /* [mb + 1], row_ptr[0] = 0; row r holds entries row_ptr[r] .. row_ptr[r + 1] - 1 */
    const int *col;     /* [nnz] base column of each entry, strictly increasing within a row */
    const int *shift;   /* [nnz] circulant shift of each entry, 0 .. Z - 1 */
} ofdm_qc_ldpc;

typedef struct ofdm_ldpc_code *ofdm_ldpc_code_t;

int ofdm_ldpc_code_create(const ofdm_qc_ldpc *code, ofdm_ldpc_code_t *handle);
int ofdm_ldpc_code_destroy(ofdm_ldpc_code_t handle);
int ofdm_ldpc_workspace_bytes(ofdm_ldpc_code_t code, long long ncw, size_t *bytes);
int ofdm_ldpc_decode(const void *d_llr, int llr_format, float llr_scale, long long cw_stride, long long ncw,
                     ofdm_ldpc_code_t code, int pos0, int n_rx, int max_iter, int norm16, int offset, int early_stop,
                     int n_bits, unsigned char *d_bits, long long out_stride, int *d_iters /* [ncw] or NULL */,
                     void *d_scratch, size_t scratch_bytes, ofdm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OFDM_LSMRC_LDPC_H_ */
