// frame_td.hip -- fused time-domain receiver for C = 1024 subcarriers.
//
// Replaces the reference's frame flow demodOneFrameCUDA (gpuLS.cu:575-675):
// batched cuFFT over all rows -> findHs -> findDistSqrd ->
// multiplyWithChannelConj -> combineForMRC -> shiftOneRow, six launches that
// each re-read the frame from global memory.  Here the time-domain IQ is read
// exactly once:
//
//   k_ls_td1024  one workgroup per frame: FFT the pilot rows (symbol 0),
//                Hc = conj(Y/X) stored bin-indexed [F][R][C], P = sum_r |Hc|^2.
//   k_mrc_td1024_hlds one wave (64 lanes) per data symbol, 8 per workgroup:
//                for every antenna row a 1024-point FFT in registers + one
//                LDS transpose, then acc += Y * Hc in registers (the Hc row
//                staged in LDS once per workgroup, the next IQ row
//                prefetched); finally acc / P stored at the rotated output
//                position.
//
// 1024-point FFT on one wave (four-step, N = 64 x 16): lane t holds
// x[t + 64 m], m < 16.
//   A[t][k2]  = FFT16_m(x[t + 64 m]) * W1024^(t k2)                 k2 < 16
//   X[k2 + 16 k1] = DFT64_t(A[t][k2])                                k1 < 64
// The 64-point DFTs run on lane quads after an LDS transpose: lane
// t = 4 q + a (q = k2, a < 4) holds A[a + 4 l'][q], l' < 16, and
//   B_a[k'] = FFT16_l'(A[a + 4 l'][q]) * W64^(a k')                   k' < 16
//   X[q + 16 (k' + 16 c)] = sum_a B_a[k'] W4^(a c)                    c < 4
// the last sum being a radix-2 x 2 exchange inside the quad (DPP).  Lane
// (q, a) finally owns bins b = q + 256 c(a) + 16 k', c(a) = (a >> 1) + 2 (a & 1).
#include "launch.hpp"
#include "wave_fft1024.hpp"
#include "diag.hpp"

OFDM_DIAG_TU(td1024)


namespace ofdm {
namespace td1024 {

// ---------------------------------------------------------------------------
// LS: one workgroup (NW waves) per frame; wave w takes antenna rows w, w+NW,
// ... and keeps a partial |H|^2 per bin; partials are added in wave order
// through LDS (deterministic; for R <= NW this is findDistSqrd's sequential
// antenna order, cpuLS.hpp:211-228).  partial != 0: antenna-split mode (DC
// slot of P = 0).  P is written bin-indexed [F][C]; Hc lane-ordered
// [F][R][8][64] float4.  NW = 4 for large batches; NW = 16 (one antenna row
// per wave up to R = 16, 148 KiB of LDS) when the batch has too few frames to
// fill the GPU with 4-wave workgroups (BASELINE configs[1]: 100 frames x 16
// antennas -- the frame's rows are transformed side by side instead of four
// after one another).
// ---------------------------------------------------------------------------
// IQ = sc16: the raw integers are transformed and the estimate multiplied by
// `scale` (ignored for float2), so Hc and P are in the units of x = i16 * scale.
constexpr int LS_WAVES = 4;

// ---------------------------------------------------------------------------
// Carrier frequency offset (cfo.hip states the convention): the src_cfo kernels
// transform x'[n] = y[n] e^{-2 pi i eps (m0 + n) / C}, m0 = s (C + prefix) +
// prefix the frame-sample index of the symbol's first FFT sample.  Lane t holds
// n = t + 64 m, so the rotation of a row splits three ways:
//   e^{-2 pi i eps m0 / C}    one factor per symbol: commutes with the FFT
//                             and the antenna sum, applied once per output
//                             (the MRC epilogue; the LS multiplies h by its
//                             conjugate).  m0 reaches tens of turns: reduced
//                             modulo one turn in float64.
//   e^{-2 pi i eps 64 m / C}  15 wave-uniform constants (Rot::cr / ci,
//                             SGPRs), applied to the row in front of the
//                             16-point transform over m.
//   e^{-2 pi i eps t / C}     one factor per lane: commutes with that
//                             transform.  Where every wave of the workgroup
//                             has the same eps (the LS; an MRC workgroup inside
//                             one frame) it is folded into the workgroup's copy
//                             of the first twiddle table, k2 = 0 apart;
//                             otherwise (a straddling MRC workgroup) each
//                             twiddle is multiplied by it from two registers.
// A non-finite eps acts as 0.
//
// The rotation is a compile-time policy of the C = 1024 kernels and row
// functions (SRC = src_cfo), not a copy of them.  Every `if constexpr (CFO<...>)`
// site must leave the src_plain instantiations with no CFO state at all -- no
// Rot, no eps, no phase: an empty NoRot is passed, never a Rot of ones -- so
// that their code stays what it was without the policy.  Checked when the
// policy went in by comparing the gfx950 instruction streams of the seven
// src_plain kernels with those of the separate kernels before it (DESIGN.md
// 4.13): same mnemonics, same registers, operands equal up to the source order
// of commutative adds.  A change to one of these sites repeats that comparison.
// ---------------------------------------------------------------------------
struct Rot {
    float2 l;               // e^{-2 pi i eps t / C} of this lane
    float cr[15], ci[15];   // e^{-2 pi i eps 64 m / C}, m = 1..15 (wave-uniform)
};
struct NoRot {};
// The sample-source policy and what the kernels' last argument is under it.
struct src_plain {
    using arg = float;  // the sc16 scale (ignored for float2)
    using rot = NoRot;
};
struct src_cfo {
    using arg = const float *__restrict__;  // eps: one offset per frame
    using rot = Rot;
};
template <class T>
constexpr bool CFO = __is_same(T, src_cfo) || __is_same(T, Rot);

__device__ __forceinline__ float cfo_eps(const float *eps, long long f) {
    const float e = eps[f];
    return (__builtin_bit_cast(unsigned, e) & 0x7f800000u) == 0x7f800000u ? 0.f : e;
}
// e^{2 pi i x}, x in turns (range-reduced by sincospi)
__device__ __forceinline__ float2 cis_turns(float x) {
    float sn, cs;
    sincospif(2.f * x, &sn, &cs);
    return float2{cs, sn};
}
__device__ __forceinline__ float uniform_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
// e^{sign 2 pi i eps m0 / C} for a frame-sample index m0 (wave-uniform): the
// turns reduced to [-0.5, 0.5] in float64 before the f32 sincospi
__device__ __forceinline__ float2 cfo_symbol_phase(float eps, long long m0, float sign) {
    const double turns = (double)eps * (double)m0 * (1.0 / C);
    const float2 p = cis_turns(sign * (float)(turns - __builtin_rint(turns)));
    return float2{uniform_f(p.x), uniform_f(p.y)};
}
// every lane of the wave active; t the lane index
__device__ __forceinline__ Rot make_rot(float eps, int t) {
    Rot r;
    r.l = cis_turns(-eps * (float)t * (1.f / C));
    const float2 c = cis_turns(-eps * (float)(t & 15) * (64.f / C));  // lane m < 16 holds constant m
#pragma unroll
    for (int m = 1; m < 16; ++m) {
        r.cr[m - 1] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c.x), m));
        r.ci[m - 1] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c.y), m));
    }
    return r;
}
__device__ __forceinline__ void rot_row(float2 (&a)[16], const Rot &rot) {
#pragma unroll
    for (int m = 1; m < 16; ++m) a[m] = cmul(a[m], float2{rot.cr[m - 1], rot.ci[m - 1]});
}
// row_fft (wave_fft1024.hpp) of the rotated row; tw's first table carries the
// lane factor in every entry, k2 = 0 included (k_ls_td1024 folds it in)
__device__ __forceinline__ void row_fft_rot(float2 (&a)[16], int t, float2 *T, const float2 *tw, const Rot &rot,
                                            float2 (&x)[16]) {
    rot_row(a, rot);
    fft16_fma(a);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) a[k2] = cmul(a[k2], tw[t * TW1P + k2]);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) T[k2 * TP + t] = a[k2];
    wave_lds_sync();
    const int q = t >> 2, qa = t & 3;
#pragma unroll
    for (int l = 0; l < 16; ++l) x[l] = T[q * TP + qa + 4 * l];
    wave_lds_sync();
    fft16_fma(x);
    const float2 *tw2 = tw + TW1BUF + qa * TW2P;
    const float g = quad_g(qa);
    x[0] = float2{g * x[0].x, g * x[0].y};
#pragma unroll
    for (int k = 1; k < 16; ++k) x[k] = cmul(x[k], tw2[k]);
    quad_dft(x, qa);
}

// SRC = src_cfo: the estimate of x' (fp32 rows; `last` is eps).
template <int NW, class IQ, class SRC>
__global__ void __launch_bounds__(64 * NW) k_ls_td1024(const IQ *__restrict__ iq, int S, int R,
                                                       int prefix, const float2 *__restrict__ X,
                                                       float2 *__restrict__ Hc, float *__restrict__ P,
                                                       int partial, typename SRC::arg last) {
    static_assert(!(CFO<SRC> && is_sc16<IQ>), "the CFO policy covers fp32 rows");
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    float2 *tw = lds;
    const int w = threadIdx.x >> 6;
    const int t = threadIdx.x & 63;
    float2 *T = lds + TWBUF + w * TBUF;
    fill_twiddles(tw);
    [[maybe_unused]] typename SRC::rot rot;
    [[maybe_unused]] float2 p0;
    if constexpr (CFO<SRC>) {
        const float e = uniform_f(cfo_eps(last, blockIdx.x));
        // the lane factor into the table entries this thread has just written
        for (int i = threadIdx.x; i < TW1BUF; i += blockDim.x)
            if (i % TW1P < 16) tw[i] = cmul(tw[i], cis_turns(-e * (float)(i / TW1P) * (1.f / C)));
        rot = make_rot(e, t);
        p0 = cfo_symbol_phase(e, prefix, 1.f);  // conj(Y' / X) = conj(Y / X) e^{+2 pi i eps prefix / C}
    }
    __syncthreads();

    const long long f = blockIdx.x;
    const int Cp = C + prefix;
    const IQ *pilot = iq + f * (long long)S * R * Cp + prefix;
    float4 *Hf = reinterpret_cast<float4 *>(Hc + f * (long long)R * C);
    const int b0 = lane_bin0(t);
    float2 xp[16];  // rotated pilots of this lane's subcarriers
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int b = b0 + 16 * k;
        xp[k] = b > 0 ? X[b - 1] : float2{1.f, 0.f};
    }
    float p[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = 0.f;
    for (int r = w; r < R; r += NW) {
        float2 a[16], x[16];
        if constexpr (is_sc16<IQ>) {
            unsigned raw[16];
            row_load(pilot + (long long)r * Cp, t, raw);
            widen_row(raw, a);
        } else {
            row_load(pilot + (long long)r * Cp, t, a);
        }
        if constexpr (CFO<SRC>)
            row_fft_rot(a, t, T, tw, rot, x);
        else
            row_fft(a, t, T, tw, x);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float2 h = ls_conj(x[k], xp[k]);
            if constexpr (is_sc16<IQ>) h = float2{h.x * last, h.y * last};
            if constexpr (CFO<SRC>) h = cmul(h, p0);
            if (b0 + 16 * k == 0) h = float2{0.f, 0.f};
            x[k] = h;
            p[k] = p[k] + (h.x * h.x) + (h.y * h.y);
        }
        hc_store(Hf + (long long)r * (C / 2), t, x);
    }
    __syncthreads();
    float *pp = reinterpret_cast<float *>(lds + TWBUF);  // [NW][C], reuses T
    static_assert(NW * C * sizeof(float) <= NW * TBUF * sizeof(float2), "partials fit the transpose images");
#pragma unroll
    for (int k = 0; k < 16; ++k) pp[w * C + b0 + 16 * k] = p[k];
    __syncthreads();
    float *Pf = P + f * C;
    const int nw = R < NW ? R : NW;  // waves that hold rows
    for (int b = threadIdx.x; b < C; b += blockDim.x) {
        float sum = pp[b];
        for (int i = 1; i < nw; ++i) sum = sum + pp[i * C + b];
        Pf[b] = b == 0 ? (partial ? 0.f : 1.f) : sum;
    }
}

// ---------------------------------------------------------------------------
// MRC with the channel estimates staged in LDS (HLDS): the 8 waves of a
// workgroup walk the antenna rows in lockstep; each thread prefetches 16 B of
// the next Hc row into a register before the FFT, the workgroup stores the
// row to LDS once and every wave reads its 16 values from there -- one
// dwordx4 per thread per row instead of eight per lane, and only LDS latency
// in front of the MAC.  LDS per workgroup is exactly 80 KiB (2 per CU):
//   TW1s [15][64] W1024^(c k2), k2 = 1..15     7680 B (k2-major: conflict free)
//   TW2s [16][4]  g(a) W64^(a k')                512 B
//   T    8 x [16][68] transpose images        69632 B (pitch 68: conflict free)
//   Hfree  Hc float4s 0..255                    4096 B
// and Hc float4s 256..511 live in the 16 unused 4-float2 row tails of the
// 8 transpose images (never touched by the transposes).  Both halves are
// read with per-lane affine addresses and no bank conflicts.
// ---------------------------------------------------------------------------

// The row transform of every C = 1024 kernel in this file (estimator
// workgroups, the bounded-wait fallback, the shared and non-shared row loops,
// split_unit, the two-launch pair): plain f32, table twiddles, fused-FMA
// 16-point transforms (fft16_fma, common.hpp).
__device__ __forceinline__ void fft_a(float2 (&a)[16], int t, float2 *T, const float2 *tw1) {
    hlds::row_fft_a<0, false, true>(a, t, T, tw1);
}
__device__ __forceinline__ void fft_b(int t, float2 *T, const float2 *tw2, float2 (&x)[16]) {
    hlds::row_fft_b<0, false, true>(t, T, tw2, x);
}
// fft_a of the row rotated by rot.  FOLDED: tw1 is the workgroup's table with
// the lane factor folded in (k2 = 1..15).
template <bool FOLDED>
__device__ __forceinline__ void fft_a_rot(float2 (&a)[16], int t, float2 *T, const float2 *tw1, const Rot &rot) {
    rot_row(a, rot);
    fft16_fma(a);
    a[0] = cmul(a[0], rot.l);
#pragma unroll
    for (int k2 = 1; k2 < 16; ++k2) {
        const float2 w = tw1[(k2 - 1) * 64 + t];
        a[k2] = cmul(a[k2], FOLDED ? w : cmul(w, rot.l));
    }
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) T[hlds::swz(k2, t)] = a[k2];
}
// acc += x * v, matrixMultThenSum (cpuLS.hpp:203-204) with the antennas in
// order, as two chained FMAs per component (64 VALU per row for the 16 bins;
// the reference's rounding order, products summed first and then added,
// compiles to mul + fma + add: 96).
__device__ __forceinline__ void mac(float2 &acc, float2 x, float vx, float vy) {
    acc.x = __builtin_fmaf(-x.y, vy, __builtin_fmaf(x.x, vx, acc.x));
    acc.y = __builtin_fmaf(x.y, vx, __builtin_fmaf(x.x, vy, acc.y));
}


// One antenna row of the sc16 loop (one row buffer; the fp32 rows are
// hlds_row_pp's): a[] holds this row on entry and
// the next row (`next`, when PREF) on exit.  The thread's 16 B of the Hc row
// are a buffer load -- hc: the frame's estimates, hoff: the byte offset of
// (row, this wave's 1 KiB), in SGPRs; the lane's offset is formed here -- so
// that no per-thread 64-bit pointer stays live across the loop.
typedef int v4i_t __attribute__((ext_vector_type(4)));
template <bool PREF, class IQ>
__device__ __forceinline__ void hlds_row_pf(const IQ *next, __amdgpu_buffer_rsrc_t hc, int hoff, int t,
                                            row_reg_t<IQ> (&a)[16],
                                            float2 *T, const float2 *tw1, const float2 *tw2,
                                            const float4 *lo, const float4 *hi, float4 *mine,
                                            float2 (&acc)[16]) {
    using namespace hlds;
    float2 x[16];
    if constexpr (is_sc16<IQ>) {
        // widened only now: converting behind the load would put the wait for
        // the prefetched row in front of the previous row's second FFT half
        float2 af[16];
        widen_row(a, af);
        fft_a(af, t, T, tw1);
    } else {
        fft_a(a, t, T, tw1);
    }
    // a row is 512 float4: each of the 512 threads moves 16 B
    const float4 hreg = __builtin_bit_cast(float4, (v4i_t)__builtin_amdgcn_raw_buffer_load_b128(hc, t * 16, hoff, 0));
    __builtin_amdgcn_sched_barrier(0);
    if (PREF) row_load<true>(next, t, a);
    fft_b(t, T, tw2, x);
    // sc16: the second FFT half stays in front of the exchange, as the fp32
    // loop has it (left free, the scheduler moves it between the two barriers
    // and the allocator then spills six accumulators across the loop, whose
    // reloads wait for the prefetched row: 128 VGPRs + 24 B of scratch
    // against 112 and none)
    if constexpr (is_sc16<IQ>) __builtin_amdgcn_sched_barrier(0);
    lds_barrier();  // every wave is done with the previous Hc row
    *mine = hreg;
    lds_barrier();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 v = i < 4 ? lo[i * 64] : hi[(i - 4) * TS];  // 2 images = TS float4s
        mac(acc[2 * i], x[2 * i], v.x, v.y);
        mac(acc[2 * i + 1], x[2 * i + 1], v.z, v.w);
    }
}

// One antenna row of the ping-pong loop: cur[] holds this row, nxt[] takes
// the next one (`next`, when PREF).  fp32: the second FFT half lands in cur[]
// again (dead once the first half has written it to the transpose image), so
// the row costs no register set beyond cur + nxt + acc and nxt[] is free to
// take loads from the row's start.  sc16: cur / nxt are the 16 raw dwords,
// widened here.  The next row's 16 loads are issued in pieces -- PP_A before
// the first FFT half, PP_B between the halves, PP_C behind the second half,
// the rest behind the Hc exchange: all 16 at the row's start (in flight for
// the whole row) measured no faster than the parent, whose 16 sit between
// the halves; what pays is that a wave never issues more than a few loads
// at once.  The thread's 16 B of the Hc row are a buffer
// load -- hc: the frame's estimates, hoff: the byte offset of (row, this
// wave's 1 KiB), in SGPRs; the lane's offset is formed here, so that no
// per-thread 64-bit pointer stays live across the loop -- issued in front of
// the row's loads: the wait for it before the exchange leaves them in flight.
// The scheduler barriers pin each piece to its place and keep the second FFT
// half in front of the exchange (left free in the sc16 loop, the scheduler
// moved it between the two barriers and the allocator spilled accumulators).
// ROT = Rot: the row rotated (fft_a_rot<true>: tw1 with the lane factor folded in).
constexpr int PP_A = 4, PP_B = 8, PP_C = 4;
template <bool PREF, class IQ, class ROT>
__device__ __forceinline__ void hlds_row_pp(const IQ *next, __amdgpu_buffer_rsrc_t hc, int hoff, int t,
                                            row_reg_t<IQ> (&cur)[16], row_reg_t<IQ> (&nxt)[16],
                                            float2 *T, const float2 *tw1, const float2 *tw2,
                                            const float4 *lo, const float4 *hi, float4 *mine,
                                            float2 (&acc)[16], const ROT &rot) {
    using namespace hlds;
    static_assert(PP_A >= 0 && PP_B >= 0 && PP_C >= 0 && PP_A + PP_B + PP_C <= 16, "the row's 16 loads");
    const float4 hreg = __builtin_bit_cast(float4, (v4i_t)__builtin_amdgcn_raw_buffer_load_b128(hc, t * 16, hoff, 0));
    if (PREF) row_load_part<0, PP_A>(next, t, nxt);
    __builtin_amdgcn_sched_barrier(0);
    auto rest = [&](float2 (&x)[16]) {
        if constexpr (CFO<ROT>)
            fft_a_rot<true>(x, t, T, tw1, rot);
        else
            fft_a(x, t, T, tw1);
        __builtin_amdgcn_sched_barrier(0);
        if (PREF) row_load_part<PP_A, PP_A + PP_B>(next, t, nxt);
        __builtin_amdgcn_sched_barrier(0);
        fft_b(t, T, tw2, x);
        __builtin_amdgcn_sched_barrier(0);
        if (PREF) row_load_part<PP_A + PP_B, PP_A + PP_B + PP_C>(next, t, nxt);
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();  // every wave is done with the previous Hc row
        *mine = hreg;
        lds_barrier();
        if (PREF) row_load_part<PP_A + PP_B + PP_C, 16>(next, t, nxt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = i < 4 ? lo[i * 64] : hi[(i - 4) * TS];  // 2 images = TS float4s
            mac(acc[2 * i], x[2 * i], v.x, v.y);
            mac(acc[2 * i + 1], x[2 * i + 1], v.z, v.w);
        }
    };
    if constexpr (is_sc16<IQ>) {
        float2 x[16];
        widen_row(cur, x);
        rest(x);
    } else {
        rest(cur);
    }
}

// Antenna-row loop.  SHARED: the workgroup's 8 symbols share one frame and
// the Hc row goes through LDS; the rows alternate between two register
// buffers (hlds_row_pp; the loop is unrolled by two, so no prefetched
// register is ever moved), the next row's loads spread over the current row.
// Otherwise (a workgroup straddling a frame boundary) each wave loads its
// own Hc row from L2.  sc16 rows (IQ = sc16) go through the transform and
// the MAC as raw integers (|sums| <= 2^15 * 1024 * R: exact headroom in f32);
// the scale is applied once per output, in the epilogue.
// R0: row 0 is already in this wave's transpose image, DMA'd there at the
// workgroup's start (row0_dma) and landed (vmcnt drained, barrier passed).
template <bool R0, class IQ>
__device__ __forceinline__ void row0(const IQ *sym, int t, const float2 *T, row_reg_t<IQ> (&a)[16]) {
    if constexpr (R0) {
        static_assert(!is_sc16<IQ>, "sc16 rows are only 4-byte aligned: no 16-B row-0 DMA");
        // this wave's DMA (the compiler does not count asm loads).  The builtin,
        // not an asm string: the compiler's own counter bookkeeping then knows
        // that nothing is outstanding here -- a load it still held pending
        // from a path in front of the rows (the fallback estimate's pilots)
        // otherwise becomes a vmcnt(1) at the head of the unrolled row loop,
        // in front of the next row's loads
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) alone (expcnt 7, lgkmcnt 15)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int m = 0; m < 16; ++m) a[m] = T[t + 64 * m];
    } else {
        row_load<true>(sym, t, a);
    }
}
// Row 0 of this wave's symbol (8 KiB) into its transpose image by LDS-DMA:
// no registers held, in flight through the table fill (and the estimate
// wait of the one-launch kernel).  The image's row tails carry other waves'
// Hc words only from row 0's exchange on, after every wave has read row 0.
__device__ __forceinline__ void row0_dma(const float2 *sym, int t, float2 *T) {
    const char *src = reinterpret_cast<const char *>(sym) + t * 16;
    const unsigned dst = lds_addr(T);
#pragma unroll
    for (int j = 0; j < 8; ++j) dma16(src + j * 1024, dst + j * 1024);
}

template <bool SHARED, bool R0 = false, class IQ, class ROT = NoRot>
__device__ __forceinline__ void hlds_rows(const IQ *sym, int Cp, int R, const float4 *Hf, int t,
                                          float2 *T, const float2 *tw1, const float2 *tw2,
                                          float2 *T0, float4 *hfree, float2 (&acc)[16], const ROT &rot = {}) {
    static_assert(!CFO<ROT> || (R0 && !is_sc16<IQ>), "rotated rows: fp32 with row-0 DMA");
    using namespace hlds;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = float2{0.f, 0.f};
    if constexpr (SHARED) {
        row_reg_t<IQ> a[16];
        const int tl = lane_here();  // the caller's t need not stay live up to here
        const float4 *lo = hfree + tl;
        const float4 *hi = hslot(T0, hfree, 256 + tl);
        float4 *mine = hslot(T0, hfree, threadIdx.x);
        // the frame's R rows of 8 KiB; a row is 512 float4, 64 per wave
        const __amdgpu_buffer_rsrc_t hc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(Hf), (short)0, R * (C * 8), 0x00020000);
        const int hw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 1024;
        if constexpr (is_sc16<IQ>) {
            // sc16 keeps one row buffer and the prefetch behind the first FFT
            // half: with the ping-pong rows its R = 16 x 100-frame batch ran
            // 6 % slower.  The last row is peeled so that the
            // prefetch is unconditional: the wait for the Hc word before the
            // exchange is then vmcnt(16), not 0
            row0<R0>(sym, tl, T, a);
            for (int r = 0; r + 1 < R; ++r)
                hlds_row_pf<true>(sym + (long long)(r + 1) * Cp, hc, r * (C * 8) + hw, lane_here(), a, T, tw1, tw2,
                                  lo, hi, mine, acc);
            hlds_row_pf<false>(sym, hc, (R - 1) * (C * 8) + hw, lane_here(), a, T, tw1, tw2, lo, hi, mine, acc);
        } else {
            row_reg_t<IQ> b[16];
            // rows in pairs, a -> b -> a, while two more rows follow; then the
            // last row (R odd) or the last two (R even), the final one without a
            // prefetch
            auto row = [&](auto pref, int r, row_reg_t<IQ>(&cur)[16], row_reg_t<IQ>(&nxt)[16]) {
                hlds_row_pp<decltype(pref)::value>(sym + (long long)(r + 1) * Cp, hc, r * (C * 8) + hw, lane_here(), cur,
                                                   nxt, T, tw1, tw2, lo, hi, mine, acc, rot);
            };
            int r = 0;
            if ((R & 1) == 0) {
                row0<R0>(sym, tl, T, b);
                row(std::true_type{}, 0, b, a);
                r = 1;
            } else {
                row0<R0>(sym, tl, T, a);
            }
            for (; r + 2 < R; r += 2) {
                row(std::true_type{}, r, a, b);
                row(std::true_type{}, r + 1, b, a);
            }
            row(std::false_type{}, r, a, b);
        }
    } else {
        for (int r = 0; r < R; ++r) {
            float2 a[16], x[16], h[16];
            if constexpr (is_sc16<IQ>) {
                unsigned raw[16];
                if (r == 0)
                    row0<R0>(sym, t, T, raw);
                else
                    row_load<true>(sym + (long long)r * Cp, t, raw);
                widen_row(raw, a);
            } else if (r == 0) {
                row0<R0>(sym, t, T, a);
            } else {
                row_load<true>(sym + (long long)r * Cp, t, a);
            }
            if constexpr (CFO<ROT>)
                fft_a_rot<false>(a, t, T, tw1, rot);
            else
                fft_a(a, t, T, tw1);
            fft_b(t, T, tw2, x);
            __builtin_amdgcn_sched_barrier(0);
            hc_load(Hf + (long long)r * (C / 2), t, h);
#pragma unroll
            for (int k = 0; k < 16; ++k) mac(acc[k], x[k], h[k].x, h[k].y);
        }
    }
}

// Epilogue of one symbol (mode 0: normalise by P): stage the K outputs in
// this wave's transpose image (free after the last row; its padding tails
// still hold other waves' Hc words, so index it as [16][TP]) at their final
// positions, then store them as 16 contiguous 512-B nontemporal wave stores
// instead of 4 scattered 128-B runs per instruction.
// SCALED (the sc16 receiver, whose acc is in raw integer units): scale folded
// into the reciprocal (mode 0) or applied to the numerator (mode 1).
template <bool SCALED = false>
__device__ __forceinline__ void hlds_epilogue(const float2 (&acc)[16], const float *P, long long f, long long q,
                                              int t, float2 *T, float2 *__restrict__ out, int mode,
                                              float scale = 1.f) {
    const int b0 = lane_bin0(t);
    float2 *o = out + q * K;
    const float *Pf = P + f * C + b0;
    // all 16 |H|^2 loads issued before the first use (under the DC-bin
    // condition the compiler issued them one at a time, each behind a
    // vmcnt(0) wait; neutral at 4 waves/SIMD)
    float pv[16];
    if ((mode & 1) == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) pv[k] = Pf[16 * k];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int b = b0 + 16 * k;
        float2 v = acc[k];
        int j = b - 1;
        if ((mode & 1) == 0) {
            // acc * (1 / P): one reciprocal (v_rcp_f32, 1 ulp) and two
            // products instead of two IEEE divisions (10 instructions each);
            // within 2 ulp of the reference's division (cpuLS.hpp:364-368)
            float rp = __builtin_amdgcn_rcpf(pv[k]);
            if constexpr (SCALED) rp = rp * scale;
            v = float2{acc[k].x * rp, acc[k].y * rp};
            j = out_pos(b > 0 ? b - 1 : 0, K);
        } else if constexpr (SCALED) {
            v = float2{acc[k].x * scale, acc[k].y * scale};
        }
        if (b > 0) T[(j >> 6) * hlds::TP + (j & 63)] = v;
    }
    wave_lds_sync();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int j = t + 64 * m;
        if (j < K) {
            const float2 v = T[m * hlds::TP + t];
            // nontemporal (streaming) stores: 2-3 % faster than plain ones
            __builtin_nontemporal_store(__builtin_bit_cast(unsigned long long, v),
                                        reinterpret_cast<unsigned long long *>(o + j));
        }
    }
}

// 8 waves = 8 consecutive data symbols per workgroup, XCD-grouped block order
// (blocks b and b+8 share an XCD under round-robin dispatch, so a frame's
// workgroups share its Hc rows in one L2; speed only, never correctness).
// mode 0: out[q][out_pos(j)] = acc / P;  mode 1: out[q][j] = acc (numerator).
// IQ = sc16: `last` is the scale (ignored for float2) that turns the raw
// integers into samples.  SRC = src_cfo: `last` is eps, the rows are those of
// x' and the estimate is that of x'.
template <bool R0, class IQ, class SRC>
__global__ void __attribute__((amdgpu_flat_work_group_size(512, 512), amdgpu_waves_per_eu(4, 4)))
k_mrc_td1024_hlds(const IQ *__restrict__ iq, int S, int R, int prefix, const float2 *__restrict__ Hc,
                  const float *__restrict__ P, float2 *__restrict__ out, long long nq, long long nblocks,
                  long long per_xcd, int mode, typename SRC::arg last) {
    static_assert(!CFO<SRC> || (R0 && !is_sc16<IQ>), "the CFO policy covers fp32 rows with row-0 DMA");
    using namespace hlds;
    constexpr int HW = WAVES;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    float2 *tw1 = lds, *tw2 = lds + TW1S;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t = threadIdx.x & 63;
    float2 *T = lds + TW1S + TW2S + w * TS;
    float2 *T0 = lds + TW1S + TW2S;
    float4 *hfree = reinterpret_cast<float4 *>(T0 + HW * TS);
    const long long pb = blockIdx.x;
    const long long lb = (pb & 7) * per_xcd + (pb >> 3);  // XCD-grouped logical block
    if (lb >= nblocks) return;

    // every wave takes part in the per-row barriers: tail waves duplicate the
    // last symbol and do not store
    const int nsym = S - 1;
    const long long qw = lb * HW + w;
    const bool store = qw < nq;
    const long long q = store ? qw : nq - 1;
    // the workgroup's Hc rows come from the frame of its first symbol; a
    // workgroup straddling two frames falls back to per-wave L2 loads
    const long long f = uniform64(q / nsym);  // wave-uniform: SGPRs across the row loop
    const long long f0 = (lb * HW) / nsym;
    const long long fl = ((lb * HW + HW - 1 < nq ? lb * HW + HW - 1 : nq - 1)) / nsym;
    const int s = 1 + (int)(q % nsym);
    const int Cp = C + prefix;
    const IQ *sym = iq + (f * S + s) * (long long)R * Cp + prefix;
    if constexpr (R0) row0_dma(sym, t, T);
    fill(tw1, tw2);
    [[maybe_unused]] float e;
    typename SRC::rot rot;
    if constexpr (CFO<SRC>) {
        // this wave's frame: every wave of a workgroup inside one frame has the
        // same offset, and each thread folds its lane factor into the table
        // entries it has just written itself (fill: i = threadIdx.x, + 512;
        // i % 64 = t)
        e = uniform_f(cfo_eps(last, f));
        rot = make_rot(e, t);
        if (f0 == fl) {
            for (int i = threadIdx.x; i < TW1S; i += blockDim.x) tw1[i] = cmul(tw1[i], rot.l);
        }
    }
    __syncthreads();

    float2 acc[16];
    if (f0 == fl)
        hlds_rows<true, R0>(sym, Cp, R, reinterpret_cast<const float4 *>(Hc + f0 * (long long)R * C), t, T,
                                 tw1, tw2, T0, hfree, acc, rot);
    else
        hlds_rows<false, R0>(sym, Cp, R, reinterpret_cast<const float4 *>(Hc + f * (long long)R * C), t, T,
                                tw1, tw2, T0, hfree, acc, rot);
    if (!store) return;
    if constexpr (CFO<SRC>) {
        // the symbol's start phase, once per output
        const float2 ps = cfo_symbol_phase(e, (long long)s * Cp + prefix, -1.f);
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = cmul(acc[k], ps);
    }
    if constexpr (is_sc16<IQ>)
        hlds_epilogue<true>(acc, P, f, q, lane_here(), T, out, mode, last);
    else
        hlds_epilogue(acc, P, f, q, lane_here(), T, out, mode);
}


// ---------------------------------------------------------------------------
// One-launch frame demodulation (ofdm_frame_demod at C = 1024): the reference
// runs demodOneFrameCUDA as dependent launches (gpuLS.cu:575-675); here the
// LS of every frame and the MRC of every data symbol share ONE grid.
// Workgroups 0 .. nls-1 (nls = nframes rounded up to 8, so the MRC blocks
// keep their XCD grouping) each estimate one frame -- FFT of its R pilot
// rows, Hc = conj(Y/X) into the workspace in lane order, P = sum_r |Hc|^2 --
// and publish it with an agent-scope release and a 64-bit flag (cdna_hip_
// programming.md Guideline 16, R1: plain stores, every storing wave's
// vmcnt(0), barrier, one lane's release fence + vmcnt(0) + relaxed agent
// flag store).  The MRC workgroups behind them poll the flags of the (one or
// two) frames they read with one lane, relaxed, then ONE agent acquire, a
// vmcnt(0) and a barrier before any Hc / P load.  Flags hold a per-launch
// 64-bit epoch (never reused; a workspace's flags need no reset).  The wait
// is bounded: a workgroup that has not seen its flag after SPIN_TICKS of
// the 100 MHz wall clock estimates the frame itself (the same bytes) and
// goes on, so no dispatch-order or residency assumption is needed for a
// correct result -- in-order dispatch only makes the wait short.
// ---------------------------------------------------------------------------
// LS of frame f by one 8-wave workgroup in the HLDS LDS layout (tables
// filled): wave w takes rows w, w + 8, ...; partial |H|^2 added in wave
// order through the transpose images (the k_ls_td1024<8> order).
__device__ __forceinline__ void hlds_ls_frame(const float2 *__restrict__ iq, int S, int R, int prefix,
                                              const float2 *__restrict__ X, float2 *Hc, float *P, long long f,
                                              int w, int t, float2 *T, float2 *T0, const float2 *tw1,
                                              const float2 *tw2, unsigned long long *mx = nullptr) {
    using namespace hlds;
    (void)mx;  // diagnostic build: phase stamps
    const int Cp = C + prefix;
    const float2 *pilot = iq + f * (long long)S * R * Cp + prefix;
    float4 *Hf = reinterpret_cast<float4 *>(Hc + f * (long long)R * C);
    const int b0 = lane_bin0(t);
    float2 xp[16];  // rotated pilots of this lane's subcarriers
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int b = b0 + 16 * k;
        xp[k] = b > 0 ? X[b - 1] : float2{1.f, 0.f};
    }
    float p[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = 0.f;
    for (int r = w; r < R; r += WAVES) {
        float2 a[16], x[16];
        const int tl = lane_here();
        row_load<true>(pilot + (long long)r * Cp, tl, a);
        fft_a(a, tl, T, tw1);
        fft_b(tl, T, tw2, x);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float2 h = ls_conj(x[k], xp[k]);  // divideOneRow + conj (cpuLS.hpp:233-244)
            if (b0 + 16 * k == 0) h = float2{0.f, 0.f};
            x[k] = h;
            p[k] = p[k] + (h.x * h.x) + (h.y * h.y);
        }
        // hc_store's layout, write-through (sc1): visible at agent scope once vmcnt drains
#pragma unroll
        for (int i = 0; i < 8; ++i) store16_wt(Hf, R * C * 8, (r * (C / 2) + i * 64 + tl) * 16, x[2 * i], x[2 * i + 1]);
        if (r == w) {
            OFDM_DIAG_MARKP(mx, 1)
        }
    }
    OFDM_DIAG_MARKP(mx, 2)
    __syncthreads();  // every wave is done with its transpose image
    float *pp = reinterpret_cast<float *>(T0);  // [WAVES][C], over the images
#pragma unroll
    for (int k = 0; k < 16; ++k) pp[w * C + b0 + 16 * k] = p[k];
    __syncthreads();
    float *Pf = P + f * C;
    const int nw = R < WAVES ? R : WAVES;
    for (int b = threadIdx.x; b < C; b += blockDim.x) {
        float sum = pp[b];
        for (int i = 1; i < nw; ++i) sum = sum + pp[i * C + b];
        const float v = b == 0 ? 1.f : sum;
        store4_wt(Pf + b, v);
    }
    OFDM_DIAG_MARKP(mx, 3)
    __syncthreads();  // pp (the transpose images) read before they are reused
}

// A half unit of the one-launch demod's schedule tail: four consecutive data
// symbols q0 .. q0+3 with each symbol's antenna rows split over two waves
// (wave w: symbol w & 3, rows [0, R0) for w < 4, [R0, R) for w >= 4), so the
// unit takes about half a block's time.  Each wave reads its own Hc rows
// (L2; no shared row, the two halves of the workgroup are at different rows),
// the second-half waves hand their sums over through their transpose images
// and the first-half waves add them (first half + second half) and store.
// Every wave reaches the one workgroup barrier.
__device__ __forceinline__ void split_unit(const float2 *__restrict__ iq, int S, int R, int prefix, const float2 *Hc,
                                           const float *P, float2 *__restrict__ out, long long nq, long long q0, int w,
                                           int t, float2 *T, float2 *T0, const float2 *tw1, const float2 *tw2) {
    const int nsym = S - 1, Cp = C + prefix, hh = w >> 2, R0 = (R + 1) >> 1;
    const long long qw = q0 + (w & 3);
    const bool store = qw < nq;
    const long long q = store ? qw : nq - 1;
    const long long f = q / nsym;
    const int s = 1 + (int)(q % nsym);
    const float2 *sym = iq + (f * S + s) * (long long)R * Cp + prefix;
    const float4 *Hf = reinterpret_cast<const float4 *>(Hc + f * (long long)R * C);
    float2 acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = float2{0.f, 0.f};
    const int r1 = hh ? R : R0;
    for (int r = hh ? R0 : 0; r < r1; ++r) {
        float2 a[16], x[16], h[16];
        row_load<true>(sym + (long long)r * Cp, t, a);
        fft_a(a, t, T, tw1);
        fft_b(t, T, tw2, x);
        __builtin_amdgcn_sched_barrier(0);
        hc_load(Hf + (long long)r * (C / 2), t, h);
#pragma unroll
        for (int k = 0; k < 16; ++k) mac(acc[k], x[k], h[k].x, h[k].y);  // antennas in order per half
    }
    if (hh) {
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k * hlds::TP + t] = acc[k];
    }
    __syncthreads();
    if (hh) return;
    const float2 *Tp = T0 + (w + 4) * hlds::TS;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float2 v = Tp[k * hlds::TP + t];
        acc[k] = float2{acc[k].x + v.x, acc[k].y + v.y};
    }
    if (store) hlds_epilogue(acc, P, f, q, t, T, out, 0);
}

// The estimate is stored write-through (sc1: 16-B Hc stores, 4-B agent
// atomic P stores) and published without a release fence, whose L2
// write-back would also flush the output lines the MRC workgroups of the
// same XCD left dirty (wave_fft1024.hpp: publish_flag / consume_flags;
// same-process A/B vs plain stores + release fence: equal to 1 % faster,
// DESIGN.md 4.6).
__global__ void __attribute__((amdgpu_flat_work_group_size(512, 512), amdgpu_waves_per_eu(4, 4)))
k_demod_td1024(const float2 *__restrict__ iq, int S, int R, int prefix, const float2 *__restrict__ X, float2 *Hc,
               float *P, float2 *__restrict__ out, long long nq, long long nblocks, Tickets tk, long long k0, long long split, unsigned long long *flags, unsigned long long epoch,
               int nls, long long nframes, long long spin_ticks) {
    using namespace hlds;
    constexpr int HW = WAVES;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    float2 *tw1 = lds, *tw2 = lds + TW1S;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t = threadIdx.x & 63;
    float2 *T = lds + TW1S + TW2S + w * TS;
    float2 *T0 = lds + TW1S + TW2S;
    float4 *hfree = reinterpret_cast<float4 *>(T0 + HW * TS);
    OFDM_DIAG_BEGIN()

    // Frames this workgroup estimates itself, [e0, e1]: an estimator
    // workgroup its own frame; an MRC workgroup none, or -- when a flag it
    // waits for is not published within spin_ticks -- the frames it reads.
    // ONE call site of hlds_ls_frame for both, so that both run the same
    // inlined code and write the same bytes (two inlined copies
    // could contract differently).
    const bool estimator = (int)blockIdx.x < nls;
    // MRC workgroups: the logical block (8 consecutive data symbols) is a
    // work ticket (take_block: own XCD's range first, then the others'),
    // kept in SGPRs
    auto first_frame = [&](long long lb) { return (lb * HW) / (S - 1); };
    auto last_frame = [&](long long lb) { return ((lb * HW + HW - 1 < nq ? lb * HW + HW - 1 : nq - 1)) / (S - 1); };
    const int nsym = S - 1, Cp = C + prefix;
    // this wave's symbol of logical block lb (the last one for tail waves)
    auto sym_of = [&](long long lb) {
        const long long qw = lb * HW + w, q = qw < nq ? qw : nq - 1;
        return iq + ((q / nsym) * S + 1 + q % nsym) * (long long)R * Cp + prefix;
    };
    long long e0 = 1, e1 = 0, lb = 0;
    int um = 0;  // unit mode: 0 the whole block, 1 / 2 its first / second four symbols, rows split over waves
    if (estimator) {
        e0 = e1 = blockIdx.x;
        if (e0 >= nframes) return;
        // the estimates are the first round's critical path: the estimator
        // waves issue ahead of receiver waves on the same SIMDs (same process,
        // configs[1] 0.295 -> 0.292 ms on one box, equal on another;
        // profiles/r6/r6s_*, r6t_*)
        __builtin_amdgcn_s_setprio(3);
        fill(tw1, tw2);
        __syncthreads();
        OFDM_DIAG_MARKN(0)
    } else {
        // the table loads first: in flight through the work ticket
        FillRegs fr;
        fill_load(fr);
        lb = wg_take_unit(tk, nblocks, k0, (long long)blockIdx.x - nls, split,
                          reinterpret_cast<long long *>(hfree + 255));
        if (lb < 0) return;  // every block taken
        OFDM_DIAG_MARKN(0)
        um = (int)(lb & 3);
        lb >>= 2;
        fill_store(tw1, tw2, fr);
        // then row 0 of the wave's symbol into its transpose image by LDS-DMA
        // and a first look at the estimate flags, in flight together: a
        // block's start costs about two memory round trips (ticket, then
        // DMA / flags), not four
        const long long f0 = first_frame(lb), fl = last_frame(lb);
        if (!um) row0_dma(sym_of(lb), t, T);
        bool seen_before = false;
        if (threadIdx.x == 0)
            seen_before = __hip_atomic_load((gu64 *)(flags + f0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch &&
                          __hip_atomic_load((gu64 *)(flags + fl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch;
        OFDM_DIAG_MARKN(1)
        // wait for the estimates of frames f0 .. fl (hfree, not used before
        // the rows, carries the outcome); not published in time: estimate
        // here (identical bytes) and read them back behind an acquire of our own
        if (!consume_flags(flags, f0, fl, epoch, spin_ticks, reinterpret_cast<int *>(hfree), seen_before)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // row 0's DMA landed before the images are reused
            __syncthreads();
            e0 = f0;
            e1 = fl;
        }
    }
    for (long long ff = e0; ff <= e1; ++ff)
        hlds_ls_frame(iq, S, R, prefix, X, Hc, P, ff, w, t, T, T0, tw1, tw2, OFDM_DIAG_ARG);
    if (estimator) {
        OFDM_DIAG_MARK()
        publish_flag(flags + e0, epoch, w == 0 && lane_here() == 0);
        OFDM_DIAG_END_SLOT(td1024, epoch);
        return;
    }
    if (e0 <= e1) {
        acquire_all();
        if (!um) row0_dma(sym_of(lb), t, T);  // the estimate used the images: row 0 again
    }
    OFDM_DIAG_MARK()

    if (um) {  // a half unit of the schedule's tail (launch_demod_td1024)
        split_unit(iq, S, R, prefix, Hc, P, out, nq, lb * HW + 4 * (um - 1), w, t, T, T0, tw1, tw2);
        OFDM_DIAG_END_SLOT(td1024, epoch);
        return;
    }
    const long long qw = lb * HW + w;
    const bool store = qw < nq;
    const long long q = store ? qw : nq - 1;
    const long long f = q / nsym;
    const long long f0 = first_frame(lb), fl = last_frame(lb);
    const float2 *sym = sym_of(lb);
    float2 acc[16];
    if (f0 == fl)
        hlds_rows<true, true>(sym, Cp, R, reinterpret_cast<const float4 *>(Hc + f0 * (long long)R * C), t, T,
                              tw1, tw2, T0, hfree, acc);
    else
        hlds_rows<false, true>(sym, Cp, R, reinterpret_cast<const float4 *>(Hc + f * (long long)R * C), t, T,
                               tw1, tw2, T0, hfree, acc);
    OFDM_DIAG_MARKN(2)
    if (store) hlds_epilogue(acc, P, f, q, lane_here(), T, out, 0);
    OFDM_DIAG_END_SLOT(td1024, epoch);
}

}  // namespace td1024

namespace {
// `last`: the kernels' last argument under SRC (the sc16 scale, or eps)
template <class SRC, class IQ>
hipError_t ls_td1024(const IQ *iq, long long nframes, int S, int R, int prefix, typename SRC::arg last,
                     const float2 *X, float2 *Hc, float *P, int partial, hipStream_t s) {
    using namespace td1024;
    if (nframes <= 0) return hipSuccess;
    if (nframes > 0x7fffffffll) return hipErrorInvalidValue;
    // 4-wave workgroups unless they leave the GPU under-filled: fewer than
    // 2 waves per SIMD (2048 waves) with rows left to spread
    if (nframes * LS_WAVES < 2048 && R > LS_WAVES) {
        auto k16 = k_ls_td1024<16, IQ, SRC>;
        const size_t lds = (TWBUF + 16 * TBUF) * sizeof(float2);
        if (hipError_t e = opt_in_lds(reinterpret_cast<const void *>(k16), (int)lds); e != hipSuccess) return e;
        hipLaunchKernelGGL(k16, dim3((unsigned)nframes), dim3(64 * 16), lds, s, iq, S, R, prefix, X, Hc, P, partial,
                           last);
        return hipGetLastError();
    }
    const size_t lds = (TWBUF + LS_WAVES * TBUF) * sizeof(float2);
    hipLaunchKernelGGL((k_ls_td1024<LS_WAVES, IQ, SRC>), dim3((unsigned)nframes), dim3(64 * LS_WAVES), lds, s, iq, S,
                       R, prefix, X, Hc, P, partial, last);
    return hipGetLastError();
}

template <class SRC, class IQ>
hipError_t mrc_td1024(const IQ *iq, long long nframes, int S, int R, int prefix, typename SRC::arg last,
                      const float2 *Hc, const float *P, float2 *out, int mode, hipStream_t s) {
    using namespace td1024;
    const long long nq = nframes * (S - 1);
    if (nq <= 0) return hipSuccess;
    const long long nb = (nq + hlds::WAVES - 1) / hlds::WAVES;
    const long long pxcd = (nb + 7) / 8;
    if (pxcd * 8 > 0x7fffffffll) return hipErrorInvalidValue;
    // R0: each wave's row 0 DMA'd into its transpose image ahead of the table
    // fill (same process, bit-identical: R=16 x 100 frames 0.301 -> 0.293 ms,
    // R=64 x 400 3.961 -> 3.922; profiles/r3/r3p_row0_dma_ab.jsonl).  The
    // one-launch kernel takes it too since round 6, once its receivers ran
    // without scratch (profiles/r6/r6m2_*).
    // sc16 rows are only 4-byte aligned (any cp_len): their row 0 comes by
    // naturally aligned dword loads like every other row, not by 16-B DMA.
    auto kern = k_mrc_td1024_hlds<!is_sc16<IQ>, IQ, SRC>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(pxcd * 8)), dim3(64 * hlds::WAVES), hlds::LDS_BYTES, s, iq, S, R,
                       prefix, Hc, P, out, nq, nb, pxcd, mode, last);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_ls_td1024(const Iq1024 &src, long long nframes, int S, int R, int prefix, const float2 *X,
                            float2 *Hc, float *P, int partial, hipStream_t s) {
    using namespace td1024;
    if (src.i16) return ls_td1024<src_plain>(src.i16, nframes, S, R, prefix, src.scale, X, Hc, P, partial, s);
    if (src.eps) return ls_td1024<src_cfo>(src.f32, nframes, S, R, prefix, src.eps, X, Hc, P, partial, s);
    return ls_td1024<src_plain>(src.f32, nframes, S, R, prefix, 1.f, X, Hc, P, partial, s);
}
hipError_t launch_mrc_td1024(const Iq1024 &src, long long nframes, int S, int R, int prefix, const float2 *Hc,
                             const float *P, float2 *out, int mode, hipStream_t s) {
    using namespace td1024;
    if (src.i16) return mrc_td1024<src_plain>(src.i16, nframes, S, R, prefix, src.scale, Hc, P, out, mode, s);
    if (src.eps) return mrc_td1024<src_cfo>(src.f32, nframes, S, R, prefix, src.eps, Hc, P, out, mode, s);
    return mrc_td1024<src_plain>(src.f32, nframes, S, R, prefix, 1.f, Hc, P, out, mode, s);
}

// One-launch LS + MRC (ofdm_frame_demod, mode 0).  flags: nframes 64-bit
// words of the workspace; epoch: a value none of them holds (per launch);
// spin_ticks: how long (100 MHz ticks) an MRC workgroup waits for a frame's
// flag before it estimates the frame itself (< 0: SPIN_TICKS).
hipError_t launch_demod_td1024(const float2 *iq, long long nframes, int S, int R, int prefix, const float2 *X,
                               float2 *Hc, float *P, float2 *out, Tickets tk,
                               unsigned long long *flags, unsigned long long epoch, long long spin_ticks,
                               hipStream_t s) {
    using namespace td1024;
    const long long nq = nframes * (S - 1);
    if (nq <= 0) return hipSuccess;
    const long long nb = (nq + hlds::WAVES - 1) / hlds::WAVES;
    const long long nls = (nframes + 7) / 8 * 8;
    // the first TWO rounds static (k0 = twice the XCD's resident workgroups
    // per XCD range: a second-round unit costs no ticket round trip before
    // its row 0 and flags are in flight; configs[1] 0.292 -> 0.280 ms, R = 64
    // x 100 frames 1.043 -> 1.008 ms, larger batches equal; 1.5 / 3 static
    // rounds 0.288 / 0.286 ms: profiles/r6/r6ag_*, r6ah_*), then work tickets
    // with the schedule's tail in half units: the last k1 blocks of every
    // XCD range (k1 = the XCD's resident workgroups) -- the last rounds end on
    // units of about half a block's time (R >= 2)
    const long long k1 = ticket_k0(2), k0 = 2 * k1, split = R >= 2 ? k1 : 0;
    const long long g = ticket_grid(nb, 8 * split);
    if (g + nls > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_demod_td1024, dim3((unsigned)(nls + g)), dim3(64 * hlds::WAVES), hlds::LDS_BYTES, s, iq,
                       S, R, prefix, X, Hc, P, out, nq, nb, tk, k0, split, flags, epoch, (int)nls, nframes,
                       spin_ticks < 0 ? SPIN_TICKS : spin_ticks);
    return hipGetLastError();
}

}  // namespace ofdm
