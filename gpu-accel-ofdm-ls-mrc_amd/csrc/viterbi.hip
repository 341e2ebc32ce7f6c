// viterbi.hip -- Viterbi decoder for constraint-length-7 convolutional codes
// on the demapper's LLRs, behind ofdm_viterbi_decode
// (include/ofdm_lsmrc_decode.h states the definition in full; no reference
// counterpart).
//
// One wave per codeword, lane = trellis state.  State s' at step t has the
// candidates b = 0, 1 with register r = (s' << 1) | b: predecessor r & 63,
// coded bits parity(r & g[i]).  The path metric is maximised, b = 0 survives
// on equality.  Integer metrics (int32; |metric| < 2^25 at T <= 65536), so
// every comparison is exact and the result is the definition's bit for bit.
//
//   k_viterbi<NOUT, PUNCT>  a workgroup of one wave takes codewords
//       blockIdx.x, + gridDim.x, ...  Per codeword:
//       forward pass  the metric of state `lane` lives in that lane.  The
//           two predecessor metrics come from lanes (2 lane) & 63 and
//           (2 lane + 1) & 63 by ds_bpermute; each lane's 2 NOUT branch signs
//           are constants of the code, formed once; the step's LLRs are
//           wave-uniform (readlane, below), so a candidate is NOUT
//           v_mad_i32_i24 on its predecessor metric.  The 64 survivor
//           decisions of a step are one __ballot word, which v_writelane puts
//           into lane (t & 63) of a register pair; every 64 steps the wave
//           stores 64 words with one 8-B access per lane.  Paths that do not
//           start in state 0 carry -2^30: they lose every comparison against a
//           real path and all are gone after six steps.
//       LLRs  lane l loads element base + l of the codeword's stream, one
//           element per lane (so any element alignment serves), and the value
//           is quantised to an integer in [-127, 127] (int8: max(v, -127);
//           f32: the demapper's int8 rule): one datapath serves both formats.
//           A step's LLRs are v_readlane at wave-uniform positions.  Elements
//           at or beyond n_rx are never read.
//           !PUNCT: 64 steps consume exactly NOUT registers of 64 LLRs, so
//           the 64 steps are unrolled and every readlane and writelane has a
//           constant lane; the next block's NOUT loads are in flight, as
//           loaded, while a block runs, and are quantised when it ends.
//           PUNCT: a step's positions follow from the mask (punctured ones
//           are 0 and consume nothing), so the step loop is not unrolled and
//           tracks its stream position; two quantised registers and a third
//           in flight.
//       decisions  8 B per step: in LDS while T <= VIT_LDS_STEPS (32 KiB,
//           five waves a CU at the longest), else in the workgroup's slot of
//           the scratch buffer.  Lane l stores and later reads exactly the
//           words t = 64 k + l, so no ordering between lanes is needed.
//       traceback  serial and wave-uniform (SALU), 64 words per 8-B access per
//           lane, then 64 unrolled steps on a 64-bit shift register sr whose
//           low six bits are the state: b = bit (sr & 63) of step t's word,
//           sr = (sr << 1) | b.  b is bit 0 of the predecessor state, u_(t-6),
//           so after the steps t0 + n - 1 .. t0 bit k of sr is u_(t0 + k - 6),
//           and sr >> 6, with the six bits a full block shifts out put back
//           from the state the block began with, is u_t0 .. u_(t0 + 63) in
//           output order; lanes 0..7 store its bytes.  Exactly ceil(L/8) bytes
//           per codeword are written, pad bits 0.
//       end state  0, or the best state, lowest index on equality (wave max,
//           ballot, find-first); metric: that state's path metric.
// No atomics, no private segment.
#include "launch.hpp"
#include "llr_quant.hpp"

namespace ofdm {
namespace vit {

constexpr int NEG = -(1 << 30);

// v_writelane_b32: `old` with lane `lane` replaced by the wave-uniform `value`.
// This clang has no __builtin_amdgcn_writelane; the declaration binds the LLVM
// intrinsic by its name, so the compiler schedules it and pads its hazards as
// it does for the readlane builtin (an asm statement would get neither).
extern "C" __device__ int ofdm_vit_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// One LLR element as loaded and its integer q in [-127, 127]: shared with ldpc.hip.
using llrq::load_raw;
using llrq::quant;

// One add-compare-select step on the wave's 64 metrics; step t's decision
// word goes to lane `sel` of (dlo, dhi).
template <int NOUT>
__device__ __forceinline__ void acs(int &pm, const int (&q)[NOUT], const int (&sg)[2][NOUT], int a0, int a1, int sel,
                                    int &dlo, int &dhi) {
    int c0 = __builtin_amdgcn_ds_bpermute(a0, pm), c1 = __builtin_amdgcn_ds_bpermute(a1, pm);
#pragma unroll
    for (int i = 0; i < NOUT; ++i) {
        c0 += __mul24(sg[0][i], q[i]);
        c1 += __mul24(sg[1][i], q[i]);
    }
    const bool d1 = c1 > c0;
    pm = d1 ? c1 : c0;
    const unsigned long long w = __ballot(d1);
    dlo = ofdm_vit_writelane((int)(unsigned)w, sel, dlo);
    dhi = ofdm_vit_writelane((int)(unsigned)(w >> 32), sel, dhi);
}

template <int NOUT, bool PUNCT>
__global__ void __launch_bounds__(64) k_viterbi(const void *__restrict__ llr, int fmt, float scale, long long cw_stride,
                                                long long ncw, int L, int T, int n_rx, int g0, int g1, int g2,
                                                int terminated, int p, unsigned mask, unsigned char *__restrict__ bits,
                                                long long out_stride, int *__restrict__ metric,
                                                unsigned long long *__restrict__ scratch) {
    extern __shared__ unsigned long long s_dec[];
    const int lane = threadIdx.x;
    const bool in_lds = scratch == nullptr;
    unsigned long long *g_dec = in_lds ? nullptr : scratch + (size_t)blockIdx.x * (size_t)T;
    const int nbytes = (L + 7) >> 3;

    // branch signs of this state's two candidates
    const int g[3] = {g0, g1, g2};
    int sg[2][NOUT];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < NOUT; ++i) sg[b][i] = 1 - 2 * (__popc((((lane << 1) | b) & 127) & g[i]) & 1);
    const int a0 = ((2 * lane) & 63) << 2, a1 = a0 + 4;  // ds_bpermute byte addresses of the predecessors

    for (long long cw = blockIdx.x; cw < ncw; cw += gridDim.x) {
        const long long e0 = cw * cw_stride;
        int pm = lane == 0 ? 0 : NEG;
        int dlo = 0, dhi = 0;
        auto store_decisions = [&](int t0) {  // the words of steps t0 .. t0 + 63, those below T
            const int idx = t0 + lane;
            if (idx < T) {
                const unsigned long long v = ((unsigned long long)(unsigned)dhi << 32) | (unsigned)dlo;
                if (in_lds)
                    s_dec[idx] = v;
                else
                    g_dec[idx] = v;
            }
        };
        if constexpr (!PUNCT) {
            int cur[NOUT], raw[NOUT];
#pragma unroll
            for (int i = 0; i < NOUT; ++i) cur[i] = quant(load_raw(llr, fmt, e0, 64 * i + lane, n_rx), fmt, scale);
#pragma unroll
            for (int i = 0; i < NOUT; ++i) raw[i] = load_raw(llr, fmt, e0, 64 * (NOUT + i) + lane, n_rx);
            int t0 = 0;
            for (; t0 + 64 <= T; t0 += 64) {  // the full blocks: no exit inside, so the 64 steps unroll
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    int q[NOUT];
#pragma unroll
                    for (int i = 0; i < NOUT; ++i) q[i] = __builtin_amdgcn_readlane(cur[(j * NOUT + i) >> 6], (j * NOUT + i) & 63);
                    acs<NOUT>(pm, q, sg, a0, a1, j, dlo, dhi);
                }
                store_decisions(t0);
#pragma unroll
                for (int i = 0; i < NOUT; ++i) {
                    cur[i] = quant(raw[i], fmt, scale);
                    raw[i] = load_raw(llr, fmt, e0, (t0 + 128) * NOUT + 64 * i + lane, n_rx);
                }
            }
            for (int j = 0; j < T - t0; ++j) {  // the last T & 63 steps, lanes by index
                int q[NOUT];
#pragma unroll
                for (int i = 0; i < NOUT; ++i) {
                    const int e = j * NOUT + i;
                    q[i] = __builtin_amdgcn_readlane(cur[0], e & 63);
#pragma unroll
                    for (int r = 1; r < NOUT; ++r) {
                        const int v = __builtin_amdgcn_readlane(cur[r], e & 63);
                        q[i] = (e >> 6) == r ? v : q[i];
                    }
                }
                acs<NOUT>(pm, q, sg, a0, a1, j, dlo, dhi);
            }
            if (T & 63) store_decisions(t0);
        } else {
            int base = 0, pos = 0, ph = 0, t = 0;
            int cur = quant(load_raw(llr, fmt, e0, lane, n_rx), fmt, scale);
            int nxt = quant(load_raw(llr, fmt, e0, 64 + lane, n_rx), fmt, scale);
            int raw = load_raw(llr, fmt, e0, 128 + lane, n_rx);
            while (t < T) {
                // the steps that begin in `cur` (wave-uniform); cur and nxt do not change in here
                for (; t < T && pos - base < 64; ++t) {
                    int q[NOUT];
                    const unsigned sent = mask >> (ph * NOUT);
#pragma unroll
                    for (int i = 0; i < NOUT; ++i) {
                        q[i] = 0;
                        if ((sent >> i) & 1u) {
                            const int d = pos - base;  // 0 .. 66
                            const int lo = __builtin_amdgcn_readlane(cur, d & 63), hi = __builtin_amdgcn_readlane(nxt, d & 63);
                            q[i] = d < 64 ? lo : hi;
                            ++pos;
                        }
                    }
                    if (++ph == p) ph = 0;
                    acs<NOUT>(pm, q, sg, a0, a1, t & 63, dlo, dhi);
                    if ((t & 63) == 63) store_decisions(t - 63);
                }
                cur = nxt;
                nxt = quant(raw, fmt, scale);
                base += 64;
                raw = load_raw(llr, fmt, e0, base + 128 + lane, n_rx);
            }
            if (T & 63) store_decisions(T & ~63);
        }

        int end = 0;
        if (!terminated) {
            int mx = pm;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int other = __shfl_xor(mx, o);
                mx = other > mx ? other : mx;
            }
            end = __ffsll((long long)__ballot(pm == mx)) - 1;
        }
        end = __builtin_amdgcn_readfirstlane(end);
        const int fm = __builtin_amdgcn_readlane(pm, end);
        if (metric && lane == 0) metric[cw] = fm;

        unsigned char *ob = bits + cw * out_stride;
        unsigned long long sr = (unsigned long long)end;
        int vlo = 0, vhi = 0;
        auto load_decisions = [&](int t0) {
            const int idx = t0 + lane;
            unsigned long long v = 0;
            if (idx < T) v = in_lds ? s_dec[idx] : g_dec[idx];
            vlo = (int)(unsigned)v;
            vhi = (int)(unsigned)(v >> 32);
        };
        auto back = [&](int j) {  // one step back through lane j's word
            const unsigned long long word = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(vhi, j) << 32) |
                                            (unsigned)__builtin_amdgcn_readlane(vlo, j);
            sr = (sr << 1) | ((word >> (sr & 63ull)) & 1ull);
        };
        // u_t0 .. u_(t0 + n - 1) after the block's n steps; st: the state the block began with (at t0 + n)
        auto store_bits = [&](int t0, int n, unsigned long long st) {
            if (t0 < L) {
                unsigned long long u = sr >> 6;
                if (n > 58) u |= st << (n - 6);
                if (L - t0 < 64) u &= (1ull << (L - t0)) - 1ull;
                const int byte = (t0 >> 3) + lane;
                if (lane < 8 && byte < nbytes) ob[byte] = (unsigned char)(u >> (8 * lane));
            }
        };
        int tb = (T - 1) >> 6;
        if (T & 63) {  // the last, partial block: lanes by index
            const unsigned long long st = sr & 63ull;
            load_decisions(tb << 6);
            for (int j = (T & 63) - 1; j >= 0; --j) back(j);
            store_bits(tb << 6, T & 63, st);
            --tb;
        }
        for (; tb >= 0; --tb) {  // full blocks, unrolled
            const unsigned long long st = sr & 63ull;
            load_decisions(tb << 6);
#pragma unroll
            for (int j = 63; j >= 0; --j) back(j);
            store_bits(tb << 6, 64, st);
        }
    }
}

}  // namespace vit

size_t viterbi_scratch_bytes(int T, long long ncw) {
    if (T <= VIT_LDS_STEPS || ncw <= 0) return 0;
    const long long slots = ncw < VIT_ROUND_SCRATCH ? ncw : VIT_ROUND_SCRATCH;
    return (size_t)8 * (size_t)T * (size_t)slots;
}

hipError_t launch_viterbi(const void *llr, int fmt, float llr_scale, long long cw_stride, long long ncw, int L, int T,
                          long long n_rx, int n_out, const int *g, int terminated, int p, unsigned mask,
                          unsigned char *bits, long long out_stride, int *metric, void *scratch, hipStream_t s) {
    if (ncw <= 0) return hipSuccess;
    if (L < 1 || T < L || T > 65536 || (n_out != 2 && n_out != 3) || n_rx < 1 || n_rx > 3ll * T || (fmt != 0 && fmt != 1))
        return hipErrorInvalidValue;
    const bool in_lds = T <= VIT_LDS_STEPS;
    if (!in_lds && !scratch) return hipErrorInvalidValue;
    // decisions in LDS: one workgroup per codeword up to the round, the dispatcher keeps every CU full;
    // in scratch: as many workgroups as there are slots
    const long long round = in_lds ? VIT_ROUND_LDS : VIT_ROUND_SCRATCH;
    const unsigned grid = (unsigned)(ncw < round ? ncw : round);
    const size_t lds = in_lds ? (size_t)8 * T : 0;
    unsigned long long *sc = in_lds ? nullptr : static_cast<unsigned long long *>(scratch);
    const bool punct = p > 0 && mask != (p * n_out >= 32 ? ~0u : (1u << (p * n_out)) - 1u);
    const int g2 = n_out == 3 ? g[2] : 0;
#define OFDM_VIT_LAUNCH(N, P)                                                                                        \
    hipLaunchKernelGGL((vit::k_viterbi<N, P>), dim3(grid), dim3(64), lds, s, llr, fmt, llr_scale, cw_stride, ncw, L, \
                       T, (int)n_rx, g[0], g[1], g2, terminated, p, mask, bits, out_stride, metric, sc)
    if (n_out == 2) {
        if (punct)
            OFDM_VIT_LAUNCH(2, true);
        else
            OFDM_VIT_LAUNCH(2, false);
    } else {
        if (punct)
            OFDM_VIT_LAUNCH(3, true);
        else
            OFDM_VIT_LAUNCH(3, false);
    }
#undef OFDM_VIT_LAUNCH
    return hipGetLastError();
}

}  // namespace ofdm
