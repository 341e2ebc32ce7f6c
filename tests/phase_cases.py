"""Shared generator and float64 model of the phase-tracking tests
(include/ofdm_lsmrc.h, "phase tracking").

The model IS the definition of ofdm_frame_phase_track: for every frame the
rows n = 0 .. S-2 in order, from theta_-1 = theta_-2 = 0,
    phi = theta_(n-1) + (theta_(n-1) - theta_(n-2))
    w_k = z_k e^{-i phi},  d_k = slice(w_k)
    g = sum_k P_k w_k conj(d_k)      over the k whose P_k is positive and finite
    delta = atan2(Im g, Re g), 0 when g is 0 or not finite
    theta_n = phi + delta,  out[n][k] = z_k e^{-i theta_n}
in float64 on the f32 input.  The slicer is discontinuous, so the model also
returns the smallest distance of any w_k to a decision threshold, in units of
the constellation's half-distance a: a parity test is meaningful only where
that margin is far above what f32 rounding moves w by (every such test
asserts margin >= 1e-3).

Generated cases are built once per key and returned read-only."""
import numpy as np

A = {2: 1 / np.sqrt(2.0), 4: 1 / np.sqrt(10.0), 6: 1 / np.sqrt(42.0), 8: 1 / np.sqrt(170.0)}
MARGIN_MIN = 1e-3

_cache = {}


def out_src(K):
    """j[k]: the subcarrier at output position k (common.hpp out_src), int (K,)."""
    k = np.arange(K)
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return np.where(k < n2, k + h, np.where(k < n2 + h, k - n2, k))


def p_by_position(hsqrd):
    """(..., K) |H|^2 by subcarrier (frame_export_estimate's Hsqrd) -> by output position."""
    return np.asarray(hsqrd)[..., out_src(np.asarray(hsqrd).shape[-1])]


def slice_points(w, bps):
    """The nearest constellation point of every element of w (complex128)."""
    a, L = A[bps], 1 << (bps // 2 - 1)

    def axis(x):
        t = np.clip(np.floor(x / (2 * a)), -L, L - 1)
        return a * (2 * t + 1)

    return axis(w.real) + 1j * axis(w.imag)


def threshold_margin(w, bps):
    """Smallest distance of any finite element of w to a decision threshold
    (x = 2 a m, |m| <= L - 1, on either axis), in units of a."""
    a, L = A[bps], 1 << (bps // 2 - 1)
    best = np.inf
    for x in (w.real, w.imag):
        x = x[np.isfinite(x)]
        if x.size:
            u = x / (2 * a)
            m = np.clip(np.rint(u), -(L - 1), L - 1)
            best = min(best, float(np.min(np.abs(u - m)) * 2))
    return best


def track(z, P, bps):
    """z (F, N, K) complex, P (F, K) aligned with z's last axis ->
    (out complex128 (F, N, K), theta float64 (F, N), margin)."""
    z = np.asarray(z).astype(np.complex128)
    P = np.asarray(P).astype(np.float64)
    F, N, K = z.shape
    out = np.empty_like(z)
    theta = np.zeros((F, N))
    margin = np.inf
    for f in range(F):
        use = np.isfinite(P[f]) & (P[f] > 0)
        th1 = th2 = 0.0
        for n in range(N):
            phi = th1 + (th1 - th2)
            w = z[f, n] * np.exp(-1j * phi)
            d = slice_points(w, bps)
            if use.any():
                margin = min(margin, threshold_margin(w[use], bps))
            with np.errstate(invalid="ignore", over="ignore"):
                g = np.sum(P[f, use] * w[use] * np.conj(d[use]))
            delta = np.arctan2(g.imag, g.real) if np.isfinite(g.real) and np.isfinite(g.imag) else 0.0
            th = phi + delta
            th2, th1 = th1, th
            theta[f, n] = th
            out[f, n] = z[f, n] * np.exp(-1j * th)
    return out, theta, margin


def residual_cfo(theta, C, cp):
    """The slope of theta through the origin over n' = 1 .. N, in subcarrier spacings."""
    n = np.arange(1, theta.shape[-1] + 1, dtype=np.float64)
    return (theta * n).sum(-1) / (n * n).sum() * C / (2 * np.pi * (C + cp))


def symbol_errors(out, truth, bps):
    """Elements whose hard decision differs from the transmitted point."""
    a = A[bps]
    d = slice_points(np.asarray(out).astype(np.complex128), bps)
    return int(np.count_nonzero(np.abs(d - truth) > a))


def case(F, N, K, bps, step, jitter, snr_db, seed=0):
    """dict(z complex64 (F, N, K), d complex128: the transmitted points,
    theta_true (F, N)).  z = d e^{i theta_true[n]} + noise at snr_db;
    theta_true: the cumulative sum of step * (1, -1.3, 0.6, ...)[f] plus
    N(0, jitter^2) per symbol."""
    key = (F, N, K, bps, step, jitter, snr_db, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, F, N, K, bps])
    a, L = A[bps], 1 << (bps // 2 - 1)
    lv = a * (2 * np.arange(-L, L) + 1)
    d = rng.choice(lv, (F, N, K)) + 1j * rng.choice(lv, (F, N, K))
    scale = np.array([(1.0, -1.3, 0.6, -0.2)[f % 4] for f in range(F)])
    inc = step * scale[:, None] + jitter * rng.standard_normal((F, N))
    theta_true = np.cumsum(inc, axis=1)
    sigma = 10.0 ** (-snr_db / 20.0)
    noise = sigma / np.sqrt(2.0) * (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape))
    z = (d * np.exp(1j * theta_true)[:, :, None] + noise).astype(np.complex64)
    out = dict(z=z, d=d, theta_true=theta_true)
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out
