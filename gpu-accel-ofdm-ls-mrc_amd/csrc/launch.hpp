// launch.hpp -- internal host-side launchers for the LS/MRC kernels.
// Arguments are validated by the C-ABI layer (capi.cpp) before these run;
// every launcher returns hipGetLastError() of its launch(es).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <set>
#include <tuple>

namespace ofdm {

// Opts `kernel` into `bytes` of dynamic LDS (launches above 64 KiB need it)
// once per (kernel, device, size) in this process; thread-safe, so a process
// driving several GPUs or launching from several host threads is covered.
inline hipError_t opt_in_lds(const void *kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::tuple<const void *, int, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(kernel, dev, bytes);
    if (done.count(key)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert(key);
    return e;
}

// Sets ofdm_last_error() for the calling thread and returns `code`.
int set_error(int code, const char *msg);

// The work tickets of ONE launch of a ticketed receiver (wave_fft1024.hpp,
// take_unit): set = 8 counter words 128 B apart (the workspace's ticket
// area); tag = this launch's value, never 0, in the high half of every word
// the launch counts in (a word holding anything else is claimed afresh, so
// no stale or foreign value is ever consumed as a count); status = the
// library's host-mapped sticky status word (capi.cpp, OFDM_E_DEVICE), or null.
struct Tickets {
    unsigned long long *set;
    unsigned *status;
    unsigned tag;
};
// status bits a ticketed launch raises
constexpr unsigned TK_FOREIGN = 1u;     // a count of another launch in a fetch_add result
constexpr unsigned TK_RANGE = 2u;       // a count beyond units + grid
constexpr unsigned TK_CONTENDED = 4u;   // a claim that did not settle in 64 compare-and-swaps

// Generic batched row FFT (Stockham in LDS), in place or out of place.
// Row i is read from in + i*in_stride + in_off and written to
// out + i*out_stride + out_off.  Any 2 <= C <= FFT_ANY_MAX: powers of two up
// to 4096 run the radix-4 kernel (fft_synth.hip), every other length the
// mixed-radix one (fft_any.hip).
constexpr int FFT_ANY_MAX = 8192;
hipError_t launch_fft_rows(const float2 *in, long long in_stride, int in_off, float2 *out,
                           long long out_stride, int out_off, long long nrows, int C,
                           bool inverse, float scale, hipStream_t s);
// The mixed-radix kernel alone (any C in [2, FFT_ANY_MAX]).
hipError_t launch_fft_any(const float2 *in, long long in_stride, int in_off, float2 *out,
                          long long out_stride, int out_off, long long nrows, int C, bool inverse,
                          float scale, hipStream_t s);
// ... with input row i at in + (i / in_rb) * in_bstride + (i % in_rb) * in_stride
// + in_off (e.g. the R pilot rows of every frame of a batch in one launch).
hipError_t launch_fft_any_b(const float2 *in, long long in_stride, long long in_rb, long long in_bstride,
                            int in_off, float2 *out, long long out_stride, int out_off, long long nrows, int C,
                            bool inverse, float scale, hipStream_t s);
bool fft_any_supported(int C);
// The FFT512 family (frame_td_fft512.hip: C = 128, 256, 512, 1536 on one wave
// per symbol, 3072 on a pair, 6144 on a quad): LS from FFT'd pilot rows
// (staging, frame stride R*C) into the lane-order Hc (lane_layout.hpp) +
// bin-layout P, and the fused MRC.  Other C: hipErrorInvalidValue.
bool lane512_supported(int C);
hipError_t launch_ls_lane512(int C, const float2 *Y, long long nframes, int R, const float2 *X, float2 *Hl, float *P,
                             hipStream_t s);
hipError_t launch_mrc_lane512(int C, const float2 *iq, long long nframes, int S, int R, int prefix, const float2 *Hl,
                              const float *P, float2 *out, int mode, hipStream_t s);
// Fused any-C MRC (fft_any.hip k_mrc_any): data symbols of frames
// iq + f*S*R*(C+prefix) (symbols 1..S-1) against the staged estimate in the
// bin layout (Hc [F][R][C], P [F][C]); mode 0: out[q][out_pos_any(j)] =
// sum_r Y*Hc / P, mode 1: out[q][j] = sum_r Y*Hc.
hipError_t launch_mrc_any(const float2 *iq, long long nframes, int S, int R, int C, int prefix, const float2 *Hc,
                          const float *P, float2 *out, int mode, hipStream_t s);

// LS channel estimate on frequency-domain pilot symbols.
// Pilot of frame f: Y + f*frame_stride, R rows of C bins.
// Hconj(f, r, j) at Hc + f*hc_fstride + r*hc_ld + j + hc_jofs  (j = 0..K-1)
// P(f, j)        at P  + f*p_fstride + j + p_jofs
// (reference layout: hc_ld = K, jofs = 0; bin layout: hc_ld = C, jofs = 1).
hipError_t launch_ls_freq(const float2 *Y, long long frame_stride, long long nframes, int R,
                          int C, const float2 *X, float2 *Hc, long long hc_fstride, int hc_ld,
                          int hc_jofs, float *P, long long p_fstride, int p_jofs, hipStream_t s);

// MRC on frequency-domain data symbols.  Data symbol q (q < nframes*nsym)
// belongs to frame q / nsym and lives at
// Y + (q / nsym)*frame_stride + (q % nsym)*sym_stride (R rows of C bins).
// mode 0: full demod  out[q][out_pos(j)] = (sum_r Y*Hc) / P
// mode 1: numerator   out[q][j] = sum_r Y*Hc  (antenna-split partial)
hipError_t launch_mrc_freq(const float2 *Y, long long frame_stride, long long sym_stride,
                           long long nframes, int nsym, int R, int C, const float2 *Hc,
                           long long hc_fstride, int hc_ld, int hc_jofs, const float *P,
                           long long p_fstride, int p_jofs, float2 *out, int mode,
                           hipStream_t s);

// The same combine on the matrix cores (mrc_mfma.hip): bin-layout Hc
// (hc_ld = C, DC slot zero), bin-indexed P (P[f*p_fstride + b]); C >= 64.
hipError_t launch_mrc_freq_mfma(const float2 *Y, long long frame_stride, long long sym_stride,
                                long long nframes, int nsym, int R, int C, const float2 *Hc,
                                long long hc_fstride, const float *P, long long p_fstride,
                                float2 *out, int mode, hipStream_t s);

// Finalise antenna-split numerators: elements [e0, e0+count) of the flat
// [nframes][nsym][K] numerator array (num points at element e0) are divided
// by P[f][j] and stored rotated into out ([nframes][nsym][K], full array).
hipError_t launch_mrc_finalize(const float2 *num, long long e0, long long count, int nsym,
                               int K, const float *P, float2 *out, hipStream_t s);

// One sc16 sample as the radio puts it on the wire (ofdm_sc16: int16 re in
// the low half of the little-endian dword, int16 im in the high half).
struct sc16 {
    unsigned v;
};
// The sample source of the two-launch C = 1024 receiver: fp32 frames (f32), or
// sc16 frames (i16: x = (float)i16 * scale; rows need 4-byte alignment only),
// exactly one of the two non-null.  eps (fp32 frames only, may be null): one
// carrier frequency offset per frame, in subcarrier spacings; the kernels then
// receive the derotated frames (cfo.hip states the convention).
struct Iq1024 {
    const float2 *f32;
    const sc16 *i16;
    float scale;
    const float *eps;
};
inline Iq1024 iq_f32(const float2 *iq, const float *eps = nullptr) { return {iq, nullptr, 1.f, eps}; }
inline Iq1024 iq_sc16(const sc16 *iq, float scale) { return {nullptr, iq, scale, nullptr}; }

// Fused time-domain receiver, C = 1024 (32 x 32 wave FFT), the same kernels
// instantiated on the sample source.
// Frames: src + f*S*R*(C+prefix); pilot = symbol 0, data = symbols 1..S-1.
// Workspace: Hc [F][R][C] (bin layout), P [F][C], in the units of x whatever
// the source, so a workspace serves any source's MRC.
hipError_t launch_ls_td1024(const Iq1024 &src, long long nframes, int S, int R, int prefix, const float2 *X,
                            float2 *Hc, float *P, int partial, hipStream_t s);
hipError_t launch_mrc_td1024(const Iq1024 &src, long long nframes, int S, int R, int prefix, const float2 *Hc,
                             const float *P, float2 *out, int mode, hipStream_t s);
// Both in one grid (frame_td.hip k_demod_td1024): estimator workgroups
// publish each frame's estimate through flags[f] = epoch (agent scope), the
// MRC workgroups wait for it.  flags: nframes words in the workspace; epoch:
// a per-launch value no flag holds.  mode 0 (full demod) only.
hipError_t launch_demod_td1024(const float2 *iq, long long nframes, int S, int R, int prefix, const float2 *X,
                               float2 *Hc, float *P, float2 *out, Tickets tk,
                               unsigned long long *flags, unsigned long long epoch, long long spin_ticks,
                               hipStream_t s);

// out[i] = {float(re) * scale, float(im) * scale}, i < n (iq_sc16.hip); in
// and out 16-B aligned.
hipError_t launch_iq_sc16_to_cf32(const sc16 *in, long long n, float scale, float2 *out, hipStream_t s);

// Carrier frequency offset (cfo.hip states the convention; eps: one offset per
// frame, in subcarrier spacings).  cfo_estimate: gamma[f] (may be null) and
// eps[f] = arg(gamma[f]) / 2 pi from the cyclic prefixes of frame f, samples
// cp_skip .. cp-1 of every row; any C.  cfo_derotate: out = in e^{-2 pi i eps m
// / C} over whole rows, out == in or disjoint.  The C = 1024 receiver on the
// derotated frames: launch_{ls,mrc}_td1024 with Iq1024::eps.
hipError_t launch_cfo_estimate(const float2 *iq, long long nframes, int S, int R, int C, int cp, int cp_skip,
                               float2 *gamma, float *eps, hipStream_t s);
hipError_t launch_cfo_derotate(const float2 *in, float2 *out, long long nframes, int S, int R, int C, int cp,
                               const float *eps, hipStream_t s);
// Integer offset from the pilot symbol (fft_any.hip k_acquire_any;
// include/ofdm_lsmrc_acquire.h states the definition): eps_out[f] = eps_in[f]
// (null or non-finite: 0) + the shift in [-max_shift, max_shift] whose pilot
// differential correlation is largest and passes the min_ratio gate; shift
// [nframes] and metric [nframes][2 max_shift + 1] may be null; eps_out may be
// eps_in.  8 <= C <= FFT_ANY_MAX, 1 <= max_shift <= 64, 4 max_shift <= C.
hipError_t launch_cfo_acquire(const float2 *iq, long long nframes, int S, int R, int C, int cp, const float2 *X,
                              int max_shift, float min_ratio, const float *eps_in, float *eps_out, int *shift,
                              float *metric, hipStream_t s);

// Stage-wise operations of the reference's per-stage gpuLS methods (stages.hip).
// fused time-domain receiver, C = 2048 (frame_td2048.hip); same contracts
hipError_t launch_ls_td2048(const float2 *iq, long long nframes, int S, int R, int prefix,
                            const float2 *X, float2 *Hc, float *P, int partial, hipStream_t s);
hipError_t launch_mrc_td2048(const float2 *iq, long long nframes, int S, int R, int prefix,
                             const float2 *Hc, const float *P, float2 *out, int mode, Tickets tk,
                             hipStream_t s);
// fused time-domain receiver, C = 4096 (frame_td4096.hip); same contracts
hipError_t launch_ls_td4096(const float2 *iq, long long nframes, int S, int R, int prefix,
                            const float2 *X, float2 *Hc, float *P, int partial, hipStream_t s);
hipError_t launch_mrc_td4096(const float2 *iq, long long nframes, int S, int R, int prefix,
                             const float2 *Hc, const float *P, float2 *out, int mode, Tickets tk,
                             hipStream_t s);
hipError_t launch_conj_product(const float2 *Y, long long nsyms, int R, int C, const float2 *Hc,
                               float2 *prod, hipStream_t s);
hipError_t launch_combine(const float2 *prod, long long nsyms, int R, int K, const float *P,
                          int rotate, float2 *out, hipStream_t s);
hipError_t launch_shift_rows(const float2 *in, long long nrows, int K, float2 *out, hipStream_t s);
hipError_t launch_hash_words(const void *d, long long nwords, unsigned long long *h, hipStream_t s);
hipError_t launch_zero_words(unsigned long long *p, int n, hipStream_t s);
hipError_t launch_dist_sqrd(const float2 *H, int R, int K, float *P, hipStream_t s);
// One frame's workspace estimate (Hc rows of C float2: lane_order = the
// fused LS kernel for C wrote them, else bin layout; P bin-indexed) ->
// Hconj [R][K], Hsqrd [K] (may be null).
hipError_t launch_export_estimate(const float2 *Hc, const float *P, int R, int C, bool lane_order,
                                  float2 *Hconj, float *Hsqrd, hipStream_t s);

// Delay-domain denoising of the workspace estimate, in place
// (est_denoise.hip; ofdm_frame_estimate_denoise states the operation): Hc
// [nframes][R][C] rows in C's lane order (lane_order) or in bin layout, P
// [nframes][C] bin-indexed.  The bin-0 position of every row keeps its bits
// and P[f][0] is not written.  1 <= taps_post, 0 <= taps_pre, taps_post +
// taps_pre <= C.  C = 1024 in lane order runs the wave kernel k_denoise1024,
// everything else launch_denoise_any (fft_any.hip k_denoise_any: any C and
// either layout).
hipError_t launch_estimate_denoise(float2 *Hc, float *P, long long nframes, int R, int C, bool lane_order,
                                   int taps_post, int taps_pre, hipStream_t s);
hipError_t launch_denoise_any(float2 *Hc, float *P, long long nframes, int R, int C, bool lane_order, int taps_post,
                              int taps_pre, hipStream_t s);

// Soft output (soft_demap.hip).  z: the demodulated [nframes][S-1][K] array
// (16-B aligned), P: the workspace's bin-indexed |H|^2 [nframes][C], bps in
// {2, 4, 6, 8}.  noise_estimate: nv[f] = mean of P |Z - slice(Z)|^2 over frame
// f.  soft_demap: llr [nframes][S-1][K][bps] (16-B aligned), fmt 0 = float,
// 1 = signed byte clamp(rint(llr * llr_scale), -127, 127).  Both need
// soft_demap_supported (a frame's (S-1)*K and the grid below 2^31), else
// hipErrorInvalidValue.
bool soft_demap_supported(long long nframes, int S, int C);
hipError_t launch_noise_estimate(const float2 *z, long long nframes, int S, int C, const float *P, int bps,
                                 float *nv, hipStream_t s);
hipError_t launch_soft_demap(const float2 *z, long long nframes, int S, int C, const float *P, const float *nv,
                             int bps, int fmt, float llr_scale, void *out, hipStream_t s);

// Decision-directed phase tracking (phase_track.hip states the recursion).
// z, out: [nframes][S-1][K] (8-B aligned; out == z or disjoint), P: the
// workspace's bin-indexed |H|^2 [nframes][C], bps in {2, 4, 6, 8}, phase:
// [nframes][S-1] radians, unwrapped (may be null).  2 <= C <= 8192, S >= 2.
hipError_t launch_phase_track(const float2 *z, long long nframes, int S, int C, const float *P, int bps, float2 *out,
                              float *phase, hipStream_t s);

// Decision-directed phase and timing tracking (timing_track.hip states the
// recursion, include/ofdm_lsmrc_timing.h the definition).  Arguments as
// launch_phase_track's; timing: [nframes][S-1] samples (may be null).
hipError_t launch_timing_track(const float2 *z, long long nframes, int S, int C, const float *P, int bps, float2 *out,
                               float *phase, float *timing, hipStream_t s);

// Viterbi decoder for K = 7 convolutional codes (viterbi.hip states the
// kernel, include/ofdm_lsmrc_decode.h the definition).  llr: fmt 0 floats, 1
// signed bytes, codeword c at element c*cw_stride, n_rx elements; T steps of
// n_out coded bits, generators g, puncturing (p, mask) as ofdm_conv_code's;
// bits: ceil(L/8) bytes at c*out_stride; metric [ncw] (may be null); scratch:
// viterbi_scratch_bytes(T, ncw) bytes, 8-B aligned (null where that is 0).
constexpr int VIT_LDS_STEPS = 4096;      // decisions of up to this many steps stay in LDS (8 B per step)
constexpr int VIT_ROUND_LDS = 65536;     // workgroups of a launch, each taking codewords in turn: decisions in LDS ...
constexpr int VIT_ROUND_SCRATCH = 1024;  // ... and in scratch (one 8*T-byte slot each)
size_t viterbi_scratch_bytes(int T, long long ncw);
hipError_t launch_viterbi(const void *llr, int fmt, float llr_scale, long long cw_stride, long long ncw, int L, int T,
                          long long n_rx, int n_out, const int *g, int terminated, int p, unsigned mask,
                          unsigned char *bits, long long out_stride, int *metric, void *scratch, hipStream_t s);

// Layered min-sum decoder for quasi-cyclic LDPC codes (ldpc.hip states the
// kernel, include/ofdm_lsmrc_ldpc.h the definition).  d_tab: the base table on
// the device, row_ptr[mb + 1] then one word per entry, (shift << 16) | col * Z;
// N = nb * Z; llr, bits as the Viterbi decoder's, the window (pos0, n_rx);
// iters [ncw] (may be null); scratch: ldpc_scratch_bytes(...) bytes (null
// where that is 0).  ldpc_plan: a codeword's L and messages stay in LDS while
// they fit LDPC_LDS_BYTES, G codewords to a workgroup of one wave while
// G * Z <= 64; beyond, the messages take a scratch slot per workgroup.
constexpr int LDPC_LDS_BYTES = 65536;     // 2 N + nnz * Z up to here: messages in LDS
constexpr int LDPC_ROUND_LDS = 16384;     // workgroups of a launch, each taking codeword groups in turn: messages in LDS ...
constexpr int LDPC_ROUND_SCRATCH = 1024;  // ... and in scratch (one nnz * Z-byte slot each)
struct LdpcPlan {
    bool msg_lds;  // messages in LDS
    int G;         // codewords per workgroup
    int threads;   // of a workgroup: G * Z rounded up to whole waves
    size_t lds;    // dynamic LDS bytes
    size_t slot;   // scratch bytes per workgroup
};
LdpcPlan ldpc_plan(int N, int Z, int nnz);
size_t ldpc_scratch_bytes(int N, int Z, int nnz, long long ncw);
hipError_t launch_ldpc(const void *llr, int fmt, float llr_scale, long long cw_stride, long long ncw, const int *d_tab,
                       int mb, int N, int Z, int nnz, int pos0, int n_rx, int max_iter, int norm16, int offset,
                       int early_stop, int n_bits, unsigned char *bits, long long out_stride, int *iters, void *scratch,
                       hipStream_t s);

// OFDM modulator (tx_mod.hip; any C but 1024: fft_any.hip k_tx_any): row i =
// X + i*ldx (K values, through the bin placement `map`) -> backward FFT ->
// iq + i*(C+cp): the last cp samples, then the C samples, times 1/peak
// (norm 0) or scale (norm 1); peak[i] = max_n |x[n]| before scaling (may be
// null).  2 <= C <= FFT_ANY_MAX, 0 <= cp <= C, ldx >= C - 1.
hipError_t launch_tx_modulate(const float2 *X, long long ldx, long long nrows, int C, int cp, int map, int norm,
                              float scale, float2 *iq, float *peak, hipStream_t s);
hipError_t launch_tx_any(const float2 *X, long long ldx, long long nrows, int C, int cp, int map, int norm,
                         float scale, float2 *iq, float *peak, hipStream_t s);

// Synthetic frames: time-domain (freq_domain=0, rows of C+prefix with a
// cyclic prefix) or frequency-domain (freq_domain=1, rows of C) IQ.
hipError_t launch_synth(float2 *iq, long long nframes, int S, int R, int C, int prefix,
                        const float2 *X, uint64_t seed, long long frame0, float noise_std,
                        int freq_domain, int r0, hipStream_t s);
// Hard-decision QPSK errors of demodulated output against the synthetic data.
// HBM probes (bench.py): mode 0 float4 copy src -> dst, mode 1 float4 read
// of src (dst: 1024 x 256 floats of sums); n4 float4s
hipError_t launch_hbm_probe(int mode, const void *src, void *dst, long long n4, hipStream_t s);
hipError_t launch_count_errors(const float2 *out, long long nframes, int S, int C,
                               uint64_t seed, long long frame0, unsigned long long *errors,
                               hipStream_t s);

// PN frame sync (pn_sync.hip): first (channel, lag) whose |correlation| / L
// reaches thres, as ch * (N-L+1) + lag in *pos (-1: none); mag optional.
hipError_t launch_pn_correlate(const float2 *buf, int R, long long N, const float2 *pn, int L,
                               float thres, long long *pos, float *mag, hipStream_t s);
hipError_t launch_pn_extract(const float2 *buf1, const float2 *buf2, int R, long long N, int L,
                             const long long *pos, int C, int cp, int nsym, float2 *sym,
                             hipStream_t s);

// Zero forcing (zf.hip).  Hin [U][R][K]; W [K][U][R] (reference layout, may be
// null); Wt [U][R][K] (subcarrier-fastest, may be null).  1 <= U <= 32,
// U*R <= 8192 (checked by capi.cpp).
size_t zf_precoder_lds_bytes(int U, int R);
hipError_t launch_zf_precoder(const float2 *Hin, int U, int R, int K, float2 *W, float2 *Wt,
                              hipStream_t s);
hipError_t launch_zf_transpose(const float2 *W, int U, int R, int K, float2 *Wt, hipStream_t s);
// apply: Y[s][r][k] = sum_u W(r,u) X[s][u][k]; detect: X[s][u][k] = sum_r conj(W(r,u)) Y[s][r][k].
// The kernel follows from (U, R, K) alone.  Apply: the 16-B-lane W-stationary kernel for K >= 2 and
// R >= 8, else register tiles (fed through LDS for 5 <= R < 8 with U >= 8).  Detect: register tiles for R < 8 or U <= 8, the W-stationary MFMA
// kernel for R <= 72, else the LDS-fed MFMA kernels.  A grid past 2^31 - 1 blocks: hipErrorInvalidValue.
hipError_t launch_zf_apply(const float2 *Wt, const float2 *X, int U, int R, int K, long long nsym,
                           float2 *Y, hipStream_t s);
hipError_t launch_zf_detect(const float2 *Wt, const float2 *Y, int U, int R, int K, long long nsym,
                            float2 *X, hipStream_t s);
// ... with row pitches (elements, >= K); pitched apply: K >= 2, R >= 8, U <= 40
bool zf_apply_pitched_supported(int U, int R, int K);
hipError_t launch_zf_apply_ld(const float2 *Wt, const float2 *X, long long ldx, int U, int R, int K, long long nsym,
                              float2 *Y, long long ldy, hipStream_t s);
// ... with row pitches ldy / ldx (elements, >= K); pitched calls need R <= 72
bool zf_detect_pitched_supported(int U, int R);
hipError_t launch_zf_detect_ld(const float2 *Wt, const float2 *Y, long long ldy, int U, int R, int K,
                               long long nsym, float2 *X, long long ldx, hipStream_t s);

}  // namespace ofdm
