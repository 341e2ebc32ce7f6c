// timing_track.hip -- decision-directed tracking of the common phase AND the
// timing drift of a frame's data symbols, behind ofdm_frame_timing_track
// (include/ofdm_lsmrc_timing.h states the definition in full; no reference
// counterpart).  The twin of phase_track.hip: same inputs, same frame-per-
// workgroup design (decision.hpp holds what the two share), one
// more state variable.
//
// A sampling clock offset moves the FFT window of data symbol n by tau_n
// samples against the pilot's; subcarrier nu is then turned by
// 2 pi nu tau_n / C, a slope across the band that grows with every symbol and
// of which the phase tracker removes only the mean.  Signed frequency of output
// position k: b = out_src(k, K) + 1, nu = b if 2 b < C, else b - C.
//
// Per frame, once: the P-weighted centroids of nu over the lower (nu < 0) and
// the upper (nu > 0) half of the used positions, span = c_U - c_L, float64;
// slope tracking is on when both halves are non-empty.  Rows n = 0 .. S-2 in
// order, from theta = tau = 0:
//   1. phi = 2 theta_(n-1) - theta_(n-2),  psi = 2 tau_(n-1) - tau_(n-2)
//   2. w_k = z_k e^{-i (phi + 2 pi nu_k psi / C)},  d_k = slice(w_k)
//   3. g_L, g_U = sum P_k w_k conj(d_k) over the two halves,  g = g_L + g_U
//   4. delta = atan2(g), 0 when g is not finite
//   5. beta = atan2(g_U conj(g_L)), 0 when tracking is off or it is not finite
//      (4 and 5 from g_L and g_U scaled by exact powers of two: any finite pair gives its angles)
//   6. theta_n = phi + delta,  tau_n = psi + beta C / (2 pi span)
//   7. out[n][k] = z_k e^{-i (theta_n + 2 pi nu_k tau_n / C)} for every k
// theta and tau are carried in float64 (wave-uniform, kept in SGPRs).
//
//   k_timing_track<BPS, CH, TPB, REG>  k_phase_track's design: one workgroup
//       per frame, thread t holds k = c*TPB + t, c < CH, and P in registers,
//       three rotating row sets with loads two rows ahead, scalar row bases,
//       8-B nontemporal lane accesses, DPP wave sums, two LDS slot sets by row
//       parity and one barrier per row.  New: four partial sums per row (g_L
//       and g_U) instead of two, and the per-element rotation.
//       REG (every even C, where nu_k = k - C/2 + (k >= C/2)): a thread's
//       elements are TPB positions apart, so element c + 1's rotation is
//       element c's times the wave-uniform e^{-2 pi i TPB psi / C}, times
//       e^{-2 pi i psi / C} once where the thread's elements cross DC.  Per
//       thread and phase that is one sincospi for element 0 (its angle
//       reduced modulo one turn in float64) and one shared by the two uniform
//       factors (lane 0 computes the one, lane 1 the other; readlane), not CH.
//       !REG (odd C: out_src's three segments make nu non-monotonic in k):
//       every element's angle is reduced in float64 and goes through its own
//       sincospi; correctness only, no odd C is a product format.
//       nu and the half flag are derived from k, not kept.
//       <4, 256> serves K <= 1024, <8, 1024> every K up to 8192 (!REG:
//       <16, 512>, whose register budget holds a sincospi per element).
#include "decision.hpp"
#include "launch.hpp"

namespace ofdm {
namespace tt {

using namespace dd;

// the signed frequency of output position k (any C)
__device__ __forceinline__ int signed_bin(int k, int K, int C) {
    const int b = out_src(k, K) + 1;
    return 2 * b < C ? b : b - C;
}

// z and out may be the same buffer (in place): no __restrict__ on them
template <int BPS, int CH, int TPB, bool REG>
__global__ void __launch_bounds__(TPB) k_timing_track(const float2 *z, int nrows, int K, int C,
                                                      const float *__restrict__ P, float2 *out,
                                                      float *__restrict__ phase, float *__restrict__ timing) {
    constexpr int NW = TPB / 64;
    __shared__ f4v slot[2][NW];
    __shared__ double cen[NW][4];
    const int tid = threadIdx.x;
    const long long f = blockIdx.x;
    const long long per_frame = (long long)nrows * K;
    const f2v *zf = reinterpret_cast<const f2v *>(z + f * per_frame);
    f2v *of = reinterpret_cast<f2v *>(out + f * per_frame);
    const float *Pf = P + f * C;
    const int half = C >> 1;  // REG: position k is in the upper half iff k >= C/2

    // element c of this thread (twin: k_phase_track's setup, which says why;
    // see decision.hpp), with the sums for the centroids
    unsigned kc[CH];  // byte offset in the row
    float p[CH];
    double sl = 0.0, snl = 0.0, su = 0.0, snu = 0.0;  // sum P, sum P nu of the two halves
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int k = c * TPB + tid, kk = k < K ? k : K - 1;
        kc[c] = (unsigned)kk * 8u;
        const float v = Pf[out_src(kk, K) + 1];
        p[c] = k < K && pos_finite(v) ? v : 0.f;
        const int nu = signed_bin(kk, K, C);
        const double pd = (double)p[c], pn = pd * (double)nu;
        sl += nu < 0 ? pd : 0.0;
        snl += nu < 0 ? pn : 0.0;
        su += nu > 0 ? pd : 0.0;
        snu += nu > 0 ? pn : 0.0;
    }
    // the centroids, float64, in a fixed order: lanes by butterflies, waves in order
    sl = wave_sum_f64(sl);
    snl = wave_sum_f64(snl);
    su = wave_sum_f64(su);
    snu = wave_sum_f64(snu);
    if ((tid & 63) == 0) {
        cen[tid >> 6][0] = sl;
        cen[tid >> 6][1] = snl;
        cen[tid >> 6][2] = su;
        cen[tid >> 6][3] = snu;
    }
    __syncthreads();
    sl = snl = su = snu = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        sl += cen[w][0];
        snl += cen[w][1];
        su += cen[w][2];
        snu += cen[w][3];
    }
    // P is positive and finite where it counts: a half is non-empty iff its sum is positive,
    // and then c_L < 0 < c_U, so the span is positive and finite
    const bool on = __builtin_amdgcn_readfirstlane((int)(sl > 0.0 && su > 0.0)) != 0;
    const double span = on ? snu / su - snl / sl : 1.0;
    const double kappa = uniform((double)C / (6.283185307179586 * span));  // samples per radian of beta
    const double invC = uniform(1.0 / (double)C);

    const int last = nrows - 1;
    auto load = [&](float2(&r)[CH], int n) { load_row(r, zf, n, last, K, kc); };
    // e^{-i (theta + 2 pi nu_k tau / C)} for the thread's elements in order of c:
    // fn(c, rotation)
    auto rotations = [&](double theta, double tau, auto &&fn) {
        const double t0 = theta * 0.15915494309189535;  // turns
        const double u = tau * invC;                    // turns per bin
        if constexpr (REG) {
            // lane 0: the step between a thread's elements, lane 1: the extra bin across DC
            const float2 su2 = cis_neg_turns(((tid & 63) == 0 ? (double)TPB : 1.0) * u);
            const float2 step{lane_value(su2.x, 0), lane_value(su2.y, 0)};
            const float2 one{lane_value(su2.x, 1), lane_value(su2.y, 1)};
            const float2 step1 = cmul(step, one);
            const int nu0 = tid - half + (tid >= half ? 1 : 0);
            float2 rot = cis_neg_turns(t0 + (double)nu0 * u);
            fn(0, rot);
#pragma unroll
            for (int c = 1; c < CH; ++c) {
                const int k = c * TPB + tid;
                const bool cross = k >= half && k - TPB < half;
                rot = cmul(rot, float2{cross ? step1.x : step.x, cross ? step1.y : step.y});
                fn(c, rot);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int nu = signed_bin((int)(kc[c] >> 3), K, C);
                fn(c, cis_neg_turns(t0 + (double)nu * u));
            }
        }
    };
    auto upper = [&](int c) -> bool {
        if constexpr (REG) return c * TPB + tid >= half;
        else return signed_bin((int)(kc[c] >> 3), K, C) > 0;
    };

    double th1 = 0.0, th2 = 0.0, ta1 = 0.0, ta2 = 0.0;  // theta, tau of rows n-1, n-2
    auto do_row = [&](const float2(&cur)[CH], int n) {
        const double phi = th1 + (th1 - th2);
        const double psi = ta1 + (ta1 - ta2);  // stays exactly 0 while tracking is off
        float lx = 0.f, ly = 0.f, ux = 0.f, uy = 0.f;
        rotations(phi, psi, [&](int c, float2 e) {
            const float2 w = cmul(cur[c], e);
            const float dx = slice_axis<BPS>(w.x), dy = slice_axis<BPS>(w.y);
            // P w conj(d); a skipped element (P = 0) adds nothing, whatever w is
            const float tx = p[c] * (w.x * dx + w.y * dy), ty = p[c] * (w.y * dx - w.x * dy);
            const bool use = p[c] > 0.f, up = upper(c);
            lx += use && !up ? tx : 0.f;
            ly += use && !up ? ty : 0.f;
            ux += use && up ? tx : 0.f;
            uy += use && up ? ty : 0.f;
        });
        lx = wave_sum(lx);
        ly = wave_sum(ly);
        ux = wave_sum(ux);
        uy = wave_sum(uy);
        f4v *sw = slot[n & 1];
        if ((tid & 63) == 0) sw[tid >> 6] = f4v{lx, ly, ux, uy};
        __syncthreads();
        f4v s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < NW; ++w) s += sw[w];
        // Both angles are taken from sums scaled by powers of two (exact): any finite g_L and g_U
        // give the Delta and beta their values have, where g_L + g_U or g_U conj(g_L) formed as
        // they stand would leave f32's range.
        const int el = __builtin_amdgcn_frexp_expf(__builtin_fmaxf(__builtin_fabsf(s.x), __builtin_fabsf(s.y)));
        const int eu = __builtin_amdgcn_frexp_expf(__builtin_fmaxf(__builtin_fabsf(s.z), __builtin_fabsf(s.w)));
        // g = g_L + g_U on the larger half's scale: each term at most 1
        const int eg = el > eu ? el : eu;
        const float gx = __builtin_ldexpf(s.x, -eg) + __builtin_ldexpf(s.z, -eg);
        const float gy = __builtin_ldexpf(s.y, -eg) + __builtin_ldexpf(s.w, -eg);
        const float delta = is_finite(gx) && is_finite(gy) ? atan2f(gy, gx) : 0.f;  // atan2(0, 0) = 0
        // g_U conj(g_L), each factor on its own scale: a largest component in [0.5, 1)
        const float glx = __builtin_ldexpf(s.x, -el), gly = __builtin_ldexpf(s.y, -el);
        const float gux = __builtin_ldexpf(s.z, -eu), guy = __builtin_ldexpf(s.w, -eu);
        const float xx = gux * glx + guy * gly, xy = guy * glx - gux * gly;
        const float beta = on && is_finite(xx) && is_finite(xy) ? atan2f(xy, xx) : 0.f;
        const double th = uniform(phi + (double)delta);
        const double ta = uniform(psi + (double)beta * kappa);
        th2 = th1;
        th1 = th;
        ta2 = ta1;
        ta1 = ta;
        char *dst = reinterpret_cast<char *>(of) + row_bytes(n, K);
        rotations(th, ta, [&](int c, float2 r) {
            const float2 v = cmul(cur[c], r);
            if (c * TPB + tid < K) __builtin_nontemporal_store(f2v{v.x, v.y}, reinterpret_cast<f2v *>(dst + kc[c]));
        });
        if (tid == 0) {
            if (phase) phase[f * nrows + n] = (float)th;
            if (timing) timing[f * nrows + n] = (float)ta;
        }
    };
    // three register sets, rows rotating through them (twin: the same
    // rotation in k_phase_track, which says why it has this shape; see
    // decision.hpp)
    float2 r0[CH], r1[CH], r2[CH];
    load(r0, 0);
    __builtin_amdgcn_sched_barrier(0);
    load(r1, 1);
    int n = 0;
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

}  // namespace tt

hipError_t launch_timing_track(const float2 *z, long long nframes, int S, int C, const float *P, int bps, float2 *out,
                               float *phase, float *timing, hipStream_t s) {
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
            float *tm = timing ? timing + f0 * nrows : nullptr;
            if (K <= 4 * 256 && C % 2 == 0)
                hipLaunchKernelGGL((tt::k_timing_track<BPS, 4, 256, true>), dim3(n), dim3(256), 0, s, zi, nrows, K, C, Pi,
                                   oi, ph, tm);
            else if (K <= 4 * 256)
                hipLaunchKernelGGL((tt::k_timing_track<BPS, 4, 256, false>), dim3(n), dim3(256), 0, s, zi, nrows, K, C, Pi,
                                   oi, ph, tm);
            else if (C % 2 == 0)
                hipLaunchKernelGGL((tt::k_timing_track<BPS, 8, 1024, true>), dim3(n), dim3(1024), 0, s, zi, nrows, K, C,
                                   Pi, oi, ph, tm);
            else  // a sincospi per element does not fit 128 registers: half the threads, twice the budget
                hipLaunchKernelGGL((tt::k_timing_track<BPS, 16, 512, false>), dim3(n), dim3(512), 0, s, zi, nrows, K, C,
                                   Pi, oi, ph, tm);
        });
    });
}

}  // namespace ofdm
