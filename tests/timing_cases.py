"""Shared generators and float64 model of the timing-tracking tests
(include/ofdm_lsmrc_timing.h).

The model IS the definition of ofdm_frame_timing_track.  Signed frequency of
output position k: b = out_src(k, K) + 1, nu_k = b if 2 b < C else b - C.  Once
per frame: use = P positive and finite, L = use & (nu < 0), U = use & (nu > 0),
span = sum_U P nu / sum_U P - sum_L P nu / sum_L P; slope tracking is on when L
and U are non-empty and span is finite and positive.  Rows n = 0 .. S-2 in
order, from theta = tau = 0:
    phi = 2 theta_(n-1) - theta_(n-2),  psi = 2 tau_(n-1) - tau_(n-2)
    w_k = z_k e^{-i (phi + 2 pi nu_k psi / C)},  d_k = slice(w_k)
    g_L = sum_L P_k w_k conj(d_k),  g_U likewise,  g = g_L + g_U
    Delta = atan2(Im g, Re g), 0 when g is 0 or not finite
    x = g_U conj(g_L);  beta = atan2(Im x, Re x), 0 when tracking is off or x is 0 or not finite
    theta_n = phi + Delta,  tau_n = psi + beta C / (2 pi span)
    out[n][k] = z_k e^{-i (theta_n + 2 pi nu_k tau_n / C)}
in float64 on the f32 input.  As in phase_cases, the model also returns the
smallest distance of any used w_k to a decision threshold in units of a.

Generated cases are built once per key and returned read-only."""
import numpy as np

import cfo_cases as cc
import phase_cases as pc
from phase_cases import out_src, slice_points, symbol_errors, threshold_margin  # noqa: F401  (the slicer is shared)

SIGMA = 0.05  # per time sample, the time-domain frames

_cache = {}


def signed_bins(K):
    """nu[k]: the signed frequency of output position k, int (K,); the Nyquist bin is -C/2."""
    C = K + 1
    b = out_src(K) + 1
    return np.where(2 * b < C, b, b - C)


def track(z, P, bps):
    """z (F, N, K) complex in output-position order, P (F, K) aligned with it ->
    (out complex128 (F, N, K), theta float64 (F, N), tau float64 (F, N), margin)."""
    z = np.asarray(z).astype(np.complex128)
    P = np.asarray(P).astype(np.float64)
    F, N, K = z.shape
    C = K + 1
    nu = signed_bins(K).astype(np.float64)
    out = np.empty_like(z)
    theta, tau = np.zeros((F, N)), np.zeros((F, N))
    margin = np.inf
    for f in range(F):
        use = np.isfinite(P[f]) & (P[f] > 0)
        lo, up = use & (nu < 0), use & (nu > 0)
        on, span = False, 1.0
        if lo.any() and up.any():
            span = (P[f, up] * nu[up]).sum() / P[f, up].sum() - (P[f, lo] * nu[lo]).sum() / P[f, lo].sum()
            on = bool(np.isfinite(span) and span > 0)
        th1 = th2 = ta1 = ta2 = 0.0
        for n in range(N):
            phi, psi = 2 * th1 - th2, 2 * ta1 - ta2
            w = z[f, n] * np.exp(-1j * (phi + 2 * np.pi * nu * psi / C))
            d = slice_points(w, bps)
            if use.any():
                margin = min(margin, threshold_margin(w[use], bps))
            with np.errstate(invalid="ignore", over="ignore"):
                gl = np.sum(P[f, lo] * w[lo] * np.conj(d[lo]))
                gu = np.sum(P[f, up] * w[up] * np.conj(d[up]))
                g = gl + gu
                x = gu * np.conj(gl)
            delta = np.arctan2(g.imag, g.real) if np.isfinite(g.real) and np.isfinite(g.imag) else 0.0
            beta = np.arctan2(x.imag, x.real) if on and np.isfinite(x.real) and np.isfinite(x.imag) else 0.0
            th = phi + delta
            ta = psi + beta * C / (2 * np.pi * span) if on else 0.0
            th2, th1, ta2, ta1 = th1, th, ta1, ta
            theta[f, n], tau[f, n] = th, ta
            out[f, n] = z[f, n] * np.exp(-1j * (th + 2 * np.pi * nu * ta / C))
    return out, theta, tau, margin


def sampling_offset(tau, C, cp):
    """The slope of tau through the origin over n' = 1 .. N, as a fraction of a sample per sample."""
    n = np.arange(1, tau.shape[-1] + 1, dtype=np.float64)
    return (tau * n).sum(-1) / (n * n).sum() / (C + cp)


CYCLE = (1.0, -1.3, 0.6, -0.2)


def case(F, N, K, bps, step, jitter, snr_db, dstep, seed=0):
    """dict(z complex64 (F, N, K), d: the transmitted points, theta_true, tau_true (F, N)).
    z = d e^{i (theta_true[n] + 2 pi nu tau_true[n] / C)} + noise: phase_cases.case
    (the same theta steps and noise) with the timing slope on top; tau_true is
    the cumulative sum of dstep * (1, -1.3, 0.6, -0.2)[f] samples per symbol."""
    key = ("case", F, N, K, bps, step, jitter, snr_db, dstep, seed)
    if key in _cache:
        return _cache[key]
    c = pc.case(F, N, K, bps, step, jitter, snr_db, seed)
    scale = np.array([CYCLE[f % 4] for f in range(F)])
    tau_true = np.cumsum(np.broadcast_to(dstep * scale[:, None], (F, N)), axis=1)
    nu = signed_bins(K).astype(np.float64)
    slope = np.exp(2j * np.pi * nu[None, None, :] * tau_true[:, :, None] / (K + 1))
    z = (c["z"].astype(np.complex128) * slope).astype(np.complex64)  # rotated noise is the same noise
    out = dict(z=z, d=c["d"], theta_true=c["theta_true"], tau_true=tau_true)
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def frames(F, S, R, C, cp, eps, delta, seed=0, sigma=SIGMA):
    """cfo_cases.frames' construction with a sampling clock offset: symbol s of
    frame f is delayed by tau_s = delta_f s (C + cp) samples, i.e. its spectrum
    is multiplied by e^{+2 pi i nu tau_s / C} (nu the signed bin, Nyquist
    negative) before the inverse FFT.  dict(y complex64 (F, S, R, C + cp),
    X complex64 (K,), eps float32 (F,), delta float64 (F,), data (F, S-1, K):
    the transmitted QPSK by bin)."""
    key = ("frames", F, S, R, C, cp, tuple(np.float32(eps).tolist()), tuple(np.float64(delta).tolist()), seed, sigma)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, F, S, R, C, cp])
    eps = np.asarray(eps, np.float32)
    delta = np.asarray(delta, np.float64)
    assert eps.shape == (F,) and delta.shape == (F,)
    K = C - 1
    X = cc._qpsk(rng, K).astype(np.complex64)
    D = np.zeros((F, S, C), np.complex128)
    D[:, :, 1:] = cc._qpsk(rng, (F, S, K))
    D[:, 0, 1:] = X
    b = np.arange(C)
    nu = np.where(2 * b < C, b, b - C).astype(np.float64)
    tau = delta[:, None] * np.arange(S)[None, :] * (C + cp)                       # (F, S)
    shifted = D * np.exp(2j * np.pi * nu[None, None, :] * tau[:, :, None] / C)
    h = (rng.standard_normal((F, R, cc.TAPS)) + 1j * rng.standard_normal((F, R, cc.TAPS))) / np.sqrt(2 * cc.TAPS)
    Hf = np.fft.fft(h, C, axis=-1)
    body = np.fft.ifft(shifted[:, :, None, :] * Hf[:, None, :, :], axis=-1) * np.sqrt(C)
    x = np.concatenate([body[..., C - cp:], body], axis=-1) if cp else body
    y = x * cc.rotation(eps, S, C, cp, +1.0)
    y = y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    out = dict(y=y.astype(np.complex64), X=X, eps=eps, delta=delta, data=D[:, 1:, 1:])
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def receive(c, cp):
    """The float64 LS + MRC receiver on a frame set, in output-position order: (z (F, S-1, K), P (F, K))."""
    Y = np.fft.fft(c["y"][..., cp:].astype(np.complex128), axis=-1)[..., 1:]
    H = Y[:, 0] / c["X"]
    Pw = (np.abs(H) ** 2).sum(1)
    z = (Y[:, 1:] * np.conj(H)[:, None]).sum(2) / Pw[:, None]
    j = out_src(z.shape[-1])
    return z[..., j], Pw[..., j]
