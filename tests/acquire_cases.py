"""Shared generator and float64 model of the integer carrier offset tests
(include/ofdm_lsmrc_acquire.h).

The model IS the definition of ofdm_frame_cfo_acquire.  For frame f, with
e = eps_in[f] as the float64 of its f32 value (non-finite, or eps_in None: 0),
K = C - 1, X the rotated pilots, D = max_shift:
    x0[r][i] = y[f,0,r,cp+i] e^{-2 pi i e (cp+i) / C},  i < C
    Y[r]     = FFT(x0[r])                         (forward, unnormalised)
    Z[b]     = sum_r Y[r][(b+1) mod C] conj(Y[r][b])
    q[j]     = X[j+1] conj(X[j]),  j = 0 .. K-2
    A(d)     = sum_j Z[(j + 1 + d) mod C] conj(q[j]),  M(d) = |A(d)|,  d = -D .. D
    dh       = the d of largest finite M (equal M: smallest |d|, the negative
               first; none finite and positive: 0)
    gate     dh := 0 if M(dh) < min_ratio * max_{d != dh} M(d) (the finite ones)
    eps_out  = f32(e + dh)
in float64 on the f32 input.  `ratio` is M(dh) / max_{d != dh} M(d) of the
ungated dh (0 where M(dh) is not positive): a parity test on the shift is
meaningful only where it is far above 1, and every such test asserts it.

Frames are cfo_cases.frames' recipe with the pilots a parameter (constant
pilots, the reference's fallback fill, are a case here) and an optional
noise-only mode.  Generated cases are built once per key and returned
read-only."""
import numpy as np

import cfo_cases as cc

_cache = {}


def constant_pilots(K, fill=0.707):
    """matrix_readX's fallback (cpuLS.hpp:84-90): fill + i fill in every bin."""
    return np.full(K, fill + 1j * fill, np.complex64)


def random_pilots(K, seed=0):
    return cc._qpsk(np.random.default_rng([seed, K]), K).astype(np.complex64)


def frames(F, S, R, C, cp, eps, X, seed=0, noise_only=False):
    """dict(y complex64 (F, S, R, C + cp), X complex64 (K,), eps float32 (F,),
    clean complex64, data (F, S-1, K)) as cfo_cases.frames, with symbol 0
    carrying the given X; noise_only: y is the sigma = 0.02 noise alone."""
    X = np.asarray(X, np.complex64)
    K = C - 1
    assert X.shape == (K,)
    eps = np.asarray(eps, np.float32)
    assert eps.shape == (F,)
    key = (F, S, R, C, cp, tuple(eps.tolist()), X.tobytes(), seed, noise_only)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, F, S, R, C, cp])
    D = np.zeros((F, S, C), np.complex128)
    D[:, :, 1:] = cc._qpsk(rng, (F, S, K))
    D[:, 0, 1:] = X
    h = (rng.standard_normal((F, R, cc.TAPS)) + 1j * rng.standard_normal((F, R, cc.TAPS))) / np.sqrt(2 * cc.TAPS)
    Hf = np.fft.fft(h, C, axis=-1)
    body = np.fft.ifft(D[:, :, None, :] * Hf[:, None, :, :], axis=-1) * np.sqrt(C)
    x = np.concatenate([body[..., C - cp:], body], axis=-1) if cp else body
    clean = x.astype(np.complex64)
    y = np.zeros_like(x) if noise_only else x * cc.rotation(eps, S, C, cp, +1.0)
    y = y + cc.SIGMA * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    out = dict(y=y.astype(np.complex64), X=X.copy(), eps=eps, clean=clean, data=D[:, 1:, 1:])
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def priority(D):
    """The shifts in the order ties are resolved: 0, -1, +1, -2, +2, ..."""
    return [0] + [s * k for k in range(1, D + 1) for s in (-1, 1)]


def acquire(y, X, cp, D, eps_in=None, min_ratio=2.0):
    """y (F, S, R, C + cp) complex64, X (K,), eps_in (F,) float32 or None ->
    (shift int32 (F,), eps_out float32 (F,), M float64 (F, 2 D + 1), ratio float64 (F,))."""
    y = np.asarray(y)
    F, S, R, Cp = y.shape
    C = Cp - cp
    K = C - 1
    X = np.asarray(X).astype(np.complex128)
    if eps_in is None:
        e = np.zeros(F)
    else:
        e = np.asarray(eps_in, np.float32).astype(np.float64)
        e = np.where(np.isfinite(e), e, 0.0)
    m = cp + np.arange(C, dtype=np.float64)
    q = X[1:] * np.conj(X[:-1])                      # (K-1,)
    j = np.arange(K - 1)
    shift = np.zeros(F, np.int32)
    M = np.zeros((F, 2 * D + 1))
    ratio = np.zeros(F)
    gate = np.float64(np.float32(min_ratio))
    with np.errstate(all="ignore"):
        for f in range(F):
            x0 = y[f, 0, :, cp:].astype(np.complex128) * np.exp(-2j * np.pi * e[f] * m / C)[None, :]
            Y = np.fft.fft(x0, axis=-1)
            Z = (np.roll(Y, -1, axis=-1) * np.conj(Y)).sum(0)
            for d in range(-D, D + 1):
                M[f, d + D] = np.abs(np.sum(Z[(j + 1 + d) % C] * np.conj(q)))
            best, dh = 0.0, 0
            for d in priority(D):
                v = M[f, d + D]
                if np.isfinite(v) and v > best:
                    best, dh = v, d
            rest = [M[f, d + D] for d in range(-D, D + 1) if d != dh and np.isfinite(M[f, d + D])]
            runner = max(rest + [0.0])
            top = M[f, dh + D]
            ratio[f] = (top / runner if runner > 0 else np.inf) if top > 0 else 0.0
            if top < gate * runner:
                dh = 0
            shift[f] = dh
    eps_out = (e + shift).astype(np.float32)
    return shift, eps_out, M, ratio
