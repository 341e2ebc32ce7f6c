// ldpc.hip -- layered integer min-sum decoder for quasi-cyclic LDPC codes on
// the demapper's LLRs, behind ofdm_ldpc_decode (include/ofdm_lsmrc_ldpc.h
// states the definition in full; no reference counterpart).
//
// A workgroup owns one codeword (G codewords when G * Z <= 64: one wave, lane
// t serves codeword t / Z).  The thread is the row index i inside the
// circulant, so a layer (base row) is one check per thread and ceil(Z / 64)
// waves.
//
//   k_ldpc<MSG_LDS>  workgroups take codeword groups blockIdx.x, + gridDim.x ...
//       posterior  L[v], int16, in LDS ([G][N]); position v of the codeword is
//           element v - pos0 of its stream inside the window, 0 outside; the
//           quantiser is the Viterbi decoder's (llr_quant.hpp).
//       base table  row_ptr[mb + 1], then one word per entry: col * Z in the
//           low 16 bits (< 32768), the shift above.  Addresses are wave-uniform,
//           so the compiler reads it through the scalar cache.
//       a check  two passes over the row's d <= 32 edges, four edges at a time
//           (their loads in flight together), nothing indexed by a runtime
//           value kept in registers: pass 1 reads L and R of each edge and
//           keeps min1, min2, idx and the signs as a 32-bit word; pass 2
//           reads them again and writes L and R.  The rotation (i + shift) mod
//           Z is an LDS address.  A layer's checks touch disjoint variables
//           (columns strictly increasing in a row), so the passes need no
//           barrier between them: one workgroup barrier per layer.
//       messages  R per edge, one byte (|R| <= 127), at [entry][i]: in LDS
//           behind L (MSG_LDS), else in the workgroup's slot of the scratch
//           buffer; a thread reads only bytes it wrote itself.  The first
//           iteration takes R = 0 without reading, so nothing is cleared.
//       syndrome  a pass of its own after an iteration (every one with
//           early_stop, else the last): one L read per edge, the check's
//           parity is the sign of the xor of its L values.  Per codeword it
//           is a ballot (G > 1) or an OR through two alternating sets of LDS
//           flags, one per wave, written by plain stores.
//       output  thread b packs byte b from eight L signs; exactly
//           ceil(n_bits / 8) bytes, pad bits 0.
// No atomics, no private segment.
#include "launch.hpp"
#include "llr_quant.hpp"

namespace ofdm {
namespace ldpc {

constexpr int MAXT = 384;  // threads of a workgroup: the largest Z
constexpr int LCLAMP = 16383;
constexpr int U = 4;  // edges of a check in flight together

// OR of `p` over the workgroup, one barrier: each wave's lane 0 stores its
// ballot's verdict, every thread reads the flags of all waves.  Two sets in
// turn, so a call's stores cannot meet the previous call's reads.
__device__ __forceinline__ bool wg_or(bool p, int *flags, int &turn) {
    const int nw = (blockDim.x + 63) >> 6;
    int *f = flags + 8 * turn;
    turn ^= 1;
    const bool w = __ballot(p) != 0ull;
    if ((threadIdx.x & 63) == 0) f[threadIdx.x >> 6] = w;
    __syncthreads();
    int r = 0;
    for (int k = 0; k < nw; ++k) r |= f[k];
    return r != 0;
}

template <bool MSG_LDS>
__global__ void __launch_bounds__(MAXT) k_ldpc(const void *__restrict__ llr, int fmt, float scale, long long cw_stride,
                                               long long ncw, const int *__restrict__ tab, int mb, int N, int Z, int nnz,
                                               int G, int pos0, int n_rx, int max_iter, int norm16, int offset,
                                               int early_stop, int n_bits, unsigned char *__restrict__ bits,
                                               long long out_stride, int *__restrict__ iters_out,
                                               signed char *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) int s_mem[];  // flags [2][8], L [G][N] int16, R [G][nnz * Z] int8
    int *s_flags = s_mem;
    short *s_lam = reinterpret_cast<short *>(s_mem + 16);
    const int tid = threadIdx.x;
    const int cwl = tid / Z, i = tid - cwl * Z;
    const bool lane_on = cwl < G;
    const int nnzZ = nnz * Z;
    const int *row_ptr = tab;
    const unsigned *edge = reinterpret_cast<const unsigned *>(tab + mb + 1);
    short *lam = s_lam + (lane_on ? cwl : 0) * N;
    signed char *msg;
    if constexpr (MSG_LDS)
        msg = reinterpret_cast<signed char *>(s_lam + G * N) + (lane_on ? cwl : 0) * nnzZ + i;
    else
        msg = scratch + (size_t)blockIdx.x * (size_t)nnzZ + i;
    const unsigned long long mymask = (G > 1 && lane_on) ? ((1ull << Z) - 1ull) << (cwl * Z) : 0ull;
    const int nbytes = (n_bits + 7) >> 3;
    const long long ngroups = (ncw + G - 1) / G;
    int turn = 0;

    // the variable of edge word w for this thread: col * Z + (i + shift) mod Z
    auto var = [&](unsigned w) {
        const unsigned x = (unsigned)i + (w >> 16);  // below 2 Z
        const unsigned y = x - (unsigned)Z;          // wraps above x where x < Z
        return (int)((w & 0xffffu) + (y < x ? y : x));
    };

    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        for (int k = tid; k < G * N; k += blockDim.x) {
            const int g = k / N, v = k - g * N;
            const long long cw = grp * G + g;
            const int x = v - pos0;
            int q = 0;
            if (cw < ncw && x >= 0 && x < n_rx) q = llrq::quant(llrq::load_raw(llr, fmt, cw * cw_stride, x, n_rx), fmt, scale);
            s_lam[k] = (short)q;
        }
        __syncthreads();

        const long long cw = grp * G + cwl;
        const bool on = lane_on && cw < ncw;
        bool done = !on, ok = false;
        int iters = 0;
        for (int it = 1; it <= max_iter; ++it) {
            const bool first = it == 1;
            for (int r = 0; r < mb; ++r) {
                const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
                if (!done) {
                    // U edges at a time, their loads issued together: an index past the row reads the
                    // row's last edge again (pass 1 ignores it, pass 2 stores the same values twice)
                    int min1 = 0x7fffffff, min2 = 0x7fffffff, idx = 0;
                    unsigned sw = 0;
                    for (int e = e0; e < e1; e += U) {
                        int t[U];
                        unsigned w[U];
#pragma unroll
                        for (int k = 0; k < U; ++k) w[k] = edge[e + k < e1 ? e + k : e1 - 1];
#pragma unroll
                        for (int k = 0; k < U; ++k) {
                            const int ek = e + k < e1 ? e + k : e1 - 1;
                            const int m = msg[ek * Z];
                            t[k] = (int)lam[var(w[k])] - (first ? 0 : m);
                        }
#pragma unroll
                        for (int k = 0; k < U; ++k) {
                            const bool in_row = e + k < e1;  // wave-uniform: the masks below are scalars
                            const int a = (t[k] < 0 ? -t[k] : t[k]) | (in_row ? 0 : 0x7fffffff);
                            sw |= (unsigned)(t[k] >> 31) & (in_row ? 1u << (e + k - e0) : 0u);
                            const int lo = a < min2 ? a : min2;
                            min2 = lo > min1 ? lo : min1;  // min1 <= min2: the second smallest of (a, min1, min2)
                            idx = a < min1 ? e + k : idx;
                            min1 = a < min1 ? a : min1;
                        }
                    }
                    const unsigned flip = (__popc(sw) & 1u) ? ~sw : sw;  // bit j: S xor s_j
                    int m1 = ((min1 * norm16) >> 4) - offset, m2 = ((min2 * norm16) >> 4) - offset;
                    m1 = m1 < 0 ? 0 : (m1 > 127 ? 127 : m1);
                    m2 = m2 < 0 ? 0 : (m2 > 127 ? 127 : m2);
                    for (int e = e0; e < e1; e += U) {
                        int t[U], a[U];
                        unsigned w[U];
#pragma unroll
                        for (int k = 0; k < U; ++k) w[k] = edge[e + k < e1 ? e + k : e1 - 1];
#pragma unroll
                        for (int k = 0; k < U; ++k) {
                            const int ek = e + k < e1 ? e + k : e1 - 1;
                            const int m = msg[ek * Z];
                            a[k] = var(w[k]);
                            t[k] = (int)lam[a[k]] - (first ? 0 : m);
                        }
#pragma unroll
                        for (int k = 0; k < U; ++k) {
                            const int ek = e + k < e1 ? e + k : e1 - 1;
                            const int mag = ek == idx ? m2 : m1;
                            const int neg = -(int)((flip >> (ek - e0)) & 1u);  // 0 or -1
                            const int rn = (mag ^ neg) - neg;
                            int l = t[k] + rn;
                            l = l < -LCLAMP ? -LCLAMP : (l > LCLAMP ? LCLAMP : l);
                            lam[a[k]] = (short)l;
                            msg[ek * Z] = (signed char)rn;
                        }
                    }
                }
                __syncthreads();
            }
            if (early_stop || it == max_iter) {
                bool bad = false;
                if (!done) {
                    for (int r = 0; r < mb; ++r) {
                        const int e0 = row_ptr[r], e1 = row_ptr[r + 1];
                        int x = 0;
#pragma unroll 4
                        for (int e = e0; e < e1; ++e) x ^= (int)lam[var(edge[e])];
                        bad |= x < 0;
                    }
                }
                bool mybad, more;
                if (G > 1) {  // one wave
                    mybad = (__ballot(bad) & mymask) != 0ull;
                    if (!done) {
                        iters = it;
                        done = ok = !mybad;
                    }
                    more = __ballot(!done) != 0ull;
                    __syncthreads();
                } else {
                    mybad = more = wg_or(bad, s_flags, turn);
                    if (!done) {
                        iters = it;
                        done = ok = !mybad;
                    }
                }
                if (!more) break;
            }
        }

        if (on && i == 0 && iters_out) iters_out[cw] = ok ? iters : -iters;
        // byte b of codeword g: bits 8 b .. 8 b + 7 below n_bits
        for (int k = tid; k < G * nbytes; k += blockDim.x) {
            const int g = k / nbytes, b = k - g * nbytes;
            const long long c = grp * G + g;
            if (c < ncw) {
                const short *l = s_lam + g * N + 8 * b;
                unsigned v = 0;
                for (int j = 0; j < 8; ++j)
                    if (8 * b + j < n_bits) v |= (unsigned)(l[j] < 0) << j;
                bits[c * out_stride + b] = (unsigned char)v;
            }
        }
        __syncthreads();  // L is loaded anew
    }
}

}  // namespace ldpc

LdpcPlan ldpc_plan(int N, int Z, int nnz) {
    LdpcPlan p;
    const long long per = 2ll * N + (long long)nnz * Z;
    p.msg_lds = per <= LDPC_LDS_BYTES;
    p.G = 1;
    if (p.msg_lds && Z <= 32) {
        const long long fit = LDPC_LDS_BYTES / per;
        p.G = (int)(fit < 64 / Z ? fit : 64 / Z);
    }
    p.threads = ((p.G * Z + 63) / 64) * 64;
    // the flags, L, then (at a 2-byte boundary already) the messages
    p.lds = 64 + (size_t)p.G * (p.msg_lds ? (size_t)per : (size_t)2 * N);
    p.slot = p.msg_lds ? 0 : (size_t)nnz * Z;
    return p;
}

size_t ldpc_scratch_bytes(int N, int Z, int nnz, long long ncw) {
    const LdpcPlan p = ldpc_plan(N, Z, nnz);
    if (p.msg_lds || ncw <= 0) return 0;
    return p.slot * (size_t)(ncw < LDPC_ROUND_SCRATCH ? ncw : LDPC_ROUND_SCRATCH);
}

hipError_t launch_ldpc(const void *llr, int fmt, float llr_scale, long long cw_stride, long long ncw, const int *d_tab,
                       int mb, int N, int Z, int nnz, int pos0, int n_rx, int max_iter, int norm16, int offset,
                       int early_stop, int n_bits, unsigned char *bits, long long out_stride, int *iters, void *scratch,
                       hipStream_t s) {
    if (ncw <= 0) return hipSuccess;
    if (!d_tab || mb < 1 || Z < 2 || Z > ldpc::MAXT || N < 2 * Z || N > 32768 || N % Z || nnz < 2 * mb || nnz > 32 * mb ||
        pos0 < 0 || n_rx < 1 || pos0 + n_rx > N || n_bits < 1 || n_bits > N || max_iter < 1 || norm16 < 1 || norm16 > 16 ||
        offset < 0 || offset > 127 || (fmt != 0 && fmt != 1))
        return hipErrorInvalidValue;
    const LdpcPlan p = ldpc_plan(N, Z, nnz);
    if (!p.msg_lds && !scratch) return hipErrorInvalidValue;
    const long long groups = (ncw + p.G - 1) / p.G;
    const long long round = p.msg_lds ? LDPC_ROUND_LDS : LDPC_ROUND_SCRATCH;
    const unsigned grid = (unsigned)(groups < round ? groups : round);
    signed char *sc = p.msg_lds ? nullptr : static_cast<signed char *>(scratch);
#define OFDM_LDPC_LAUNCH(M)                                                                                           \
    do {                                                                                                              \
        if (p.lds > 65536) {                                                                                          \
            const hipError_t e = opt_in_lds(reinterpret_cast<const void *>(&ldpc::k_ldpc<M>), (int)p.lds);            \
            if (e != hipSuccess) return e;                                                                            \
        }                                                                                                             \
        hipLaunchKernelGGL((ldpc::k_ldpc<M>), dim3(grid), dim3(p.threads), p.lds, s, llr, fmt, llr_scale, cw_stride,  \
                           ncw, d_tab, mb, N, Z, nnz, p.G, pos0, n_rx, max_iter, norm16, offset, early_stop, n_bits,  \
                           bits, out_stride, iters, sc);                                                              \
    } while (0)
    if (p.msg_lds)
        OFDM_LDPC_LAUNCH(true);
    else
        OFDM_LDPC_LAUNCH(false);
#undef OFDM_LDPC_LAUNCH
    return hipGetLastError();
}

}  // namespace ofdm
