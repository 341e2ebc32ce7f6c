// phase_track.hip -- decision-directed carrier phase tracking between the
// combiner and the demapper, behind ofdm_frame_phase_track (no reference
// counterpart: the reference ends at the equalised symbols).
//
// A frame is one pilot and up to 100 data symbols combined against that one
// estimate; whatever carrier offset is left turns every later symbol a little
// further.  Input: the demodulated array z, flat [nframes][S-1][K] in the
// rotated order every receiver writes, and the |H|^2 sums P of the frame
// workspace, [nframes][C] by FFT bin (soft_demap.hip: the subcarrier at output
// position k is j = out_src(k, K), its gain P[f*C + j + 1]).
//
// Per frame, rows n = 0 .. S-2 in order, state theta_-1 = theta_-2 = 0 (the
// pilot is phase 0 by construction):
//   1. phi = theta_(n-1) + (theta_(n-1) - theta_(n-2))   a constant drift costs nothing
//   2. w_k = z_k e^{-i phi},  d_k = slice(w_k): the nearest point of the 38.211
//      constellation, per axis t = clamp(floor(x / 2a), -L, L-1), point a (2t+1)
//      (decision.hpp, slice_axis: the slicer of the noise estimate too)
//   3. g = sum_k P_k w_k conj(d_k) over the elements whose P is positive and finite
//   4. delta = atan2(Im g, Re g), 0 when g is 0 or not finite;  theta_n = phi + delta
//   5. out[n][k] = z_k e^{-i theta_n} for every k;  phase[f][n] = theta_n (unwrapped)
// theta is carried in float64; only its value modulo one turn goes through an
// f32 sincospi (as cfo.hip does).
//
//   k_phase_track<BPS, CH, TPB>  one workgroup of TPB threads per frame, the
//       trackers' rows of decision.hpp (thread t holds the elements
//       k = c*TPB + t, c < CH, of a row and P in registers); a row's loads are
//       issued two rows ahead and stay in flight while those rows reduce.
//       g: per thread over c in order, then within the wave by
//       DPP butterflies (quad, half-row, row: every lane holds its row's sum)
//       and the four row sums in lane order; the wave sums meet through one of
//       two LDS slot sets (row parity), so one barrier per row suffices: a wave
//       cannot write the set of row n+2 before every wave has passed the
//       barrier of row n+1, i.e. has read row n's.  Every thread then adds the
//       wave sums in wave order: no atomics, the same bits on every run.
//       <4, 256> serves K <= 1024, <8, 1024> every K up to 8192.
#include "decision.hpp"
#include "launch.hpp"

namespace ofdm {
namespace pt {

using namespace dd;

// e^{-i theta}
__device__ __forceinline__ float2 cis_neg(double theta) { return cis_neg_turns(theta * 0.15915494309189535); }  // / 2 pi

// z and out may be the same buffer (in place): no __restrict__ on them
template <int BPS, int CH, int TPB>
__global__ void __launch_bounds__(TPB) k_phase_track(const float2 *z, int nrows, int K, int C,
                                                     const float *__restrict__ P, float2 *out,
                                                     float *__restrict__ phase) {
    constexpr int NW = TPB / 64;
    __shared__ float2 slot[2][NW];
    const int tid = threadIdx.x;
    const long long f = blockIdx.x;
    const long long per_frame = (long long)nrows * K;
    const f2v *zf = reinterpret_cast<const f2v *>(z + f * per_frame);
    f2v *of = reinterpret_cast<f2v *>(out + f * per_frame);
    const float *Pf = P + f * C;

    // element c of this thread: k = c*TPB + tid; past the row's end the load
    // is clamped to the last element (no branch around a load: the waits stay
    // counted) and P = 0 keeps it out of the sum; only the store is guarded
    // (twin: k_timing_track's setup, see decision.hpp)
    unsigned kc[CH];  // byte offset in the row
    float p[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int k = c * TPB + tid, kk = k < K ? k : K - 1;
        kc[c] = (unsigned)kk * 8u;
        const float v = Pf[out_src(kk, K) + 1];
        p[c] = k < K && pos_finite(v) ? v : 0.f;
    }
    const int last = nrows - 1;
    auto load = [&](float2(&r)[CH], int n) { load_row(r, zf, n, last, K, kc); };
    double th1 = 0.0, th2 = 0.0;  // theta_(n-1), theta_(n-2)
    auto do_row = [&](const float2(&cur)[CH], int n) {
        const double phi = th1 + (th1 - th2);
        const float2 e = cis_neg(phi);
        float gx = 0.f, gy = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float2 w = cmul(cur[c], e);
            const float dx = slice_axis<BPS>(w.x), dy = slice_axis<BPS>(w.y);
            // P w conj(d); a skipped element (P = 0) adds nothing, whatever w is
            const float tx = p[c] * (w.x * dx + w.y * dy), ty = p[c] * (w.y * dx - w.x * dy);
            gx += p[c] > 0.f ? tx : 0.f;
            gy += p[c] > 0.f ? ty : 0.f;
        }
        gx = wave_sum(gx);
        gy = wave_sum(gy);
        float2 *sl = slot[n & 1];
        if ((tid & 63) == 0) sl[tid >> 6] = float2{gx, gy};
        __syncthreads();
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float2 v = sl[w];
            sx += v.x;
            sy += v.y;
        }
        const float delta = is_finite(sx) && is_finite(sy) ? atan2f(sy, sx) : 0.f;  // atan2(0, 0) = 0
        const double th = phi + (double)delta;
        th2 = th1;
        th1 = th;
        const float2 r = cis_neg(th);
        char *on = reinterpret_cast<char *>(of) + row_bytes(n, K);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const float2 v = cmul(cur[c], r);
            if (c * TPB + tid < K) __builtin_nontemporal_store(f2v{v.x, v.y}, reinterpret_cast<f2v *>(on + kc[c]));
        }
        if (phase && tid == 0) phase[f * nrows + n] = (float)th;
    };
    // three register sets, rows rotating through them (no copy, so nothing
    // waits for a load before its row is due): row n + 2's loads go out
    // before row n is touched, stay in flight while rows n and n + 1 reduce,
    // and are older than row n's stores, so the wait for a row's data (the
    // counter is in issue order) never waits for the row before's stores.
    // Past the frame's end the loads repeat the last row and are not used.
    // (twin: the same rotation in k_timing_track, see decision.hpp)
    float2 r0[CH], r1[CH], r2[CH];
    load(r0, 0);
    __builtin_amdgcn_sched_barrier(0);  // row 0's loads all older than row 1's, as in the loop
    load(r1, 1);
    int n = 0;
    // whole triples without an exit inside the loop: a break would merge its
    // path into the loop header and the wait there would fall back to "all
    // but the loads just issued", stores of the row before included
    for (; n + 3 <= nrows; n += 3) {
        load(r2, n + 2);
        do_row(r0, n);
        load(r0, n + 3);
        do_row(r1, n + 1);
        load(r1, n + 4);
        do_row(r2, n + 2);
    }
    if (n < nrows) do_row(r0, n);
    if (n + 1 < nrows) do_row(r1, n + 1);
}

}  // namespace pt

hipError_t launch_phase_track(const float2 *z, long long nframes, int S, int C, const float *P, int bps, float2 *out,
                              float *phase, hipStream_t s) {
    if (nframes <= 0) return hipSuccess;
    if (S < 2 || C < 2 || C > 8 * 1024) return hipErrorInvalidValue;
    const int K = C - 1, nrows = S - 1;
    const long long per_frame = (long long)nrows * K;
    return dd::for_bps(bps, [&](auto b) {
        constexpr int BPS = decltype(b)::value;
        return dd::for_frame_chunks(nframes, [&](long long f0, unsigned n) {
            const float2 *zi = z + f0 * per_frame;
            float2 *oi = out + f0 * per_frame;
            const float *Pi = P + f0 * C;
            float *ph = phase ? phase + f0 * nrows : nullptr;
            if (K <= 4 * 256)
                hipLaunchKernelGGL((pt::k_phase_track<BPS, 4, 256>), dim3(n), dim3(256), 0, s, zi, nrows, K, C, Pi, oi, ph);
            else
                hipLaunchKernelGGL((pt::k_phase_track<BPS, 8, 1024>), dim3(n), dim3(1024), 0, s, zi, nrows, K, C, Pi, oi,
                                   ph);
        });
    });
}

}  // namespace ofdm
