"""Shared generator and float64 references of the carrier-frequency-offset
tests (include/ofdm_lsmrc.h, "carrier frequency offset").

A frame: random QPSK on bins 1..C-1 of every symbol (symbol 0 carries the
pilots X), IFFT, a random 4-tap channel per antenna applied circularly (so the
prefix is exactly cyclic), the prefix, the per-frame rotation
y[m] = x[m] e^{+2 pi i eps m / C} (m = s (C + cp) + i, counted per antenna row
from the first prefix sample of symbol 0), sigma = 0.02 noise; time samples of
unit rms before the channel.  Everything is built once per key and returned
read-only."""
import numpy as np

EPS_CYCLE = (0.03, -0.2, 0.45, 0.0, -0.004)
SIGMA = 0.02
TAPS = 4

_cache = {}


def _qpsk(rng, shape):
    a = np.sqrt(0.5)
    return rng.choice([-a, a], shape) + 1j * rng.choice([-a, a], shape)


def phase_index(S, C, cp):
    """m[s, i] = s (C + cp) + i, int64 (S, C + cp)."""
    return (np.arange(S, dtype=np.int64)[:, None] * (C + cp)) + np.arange(C + cp, dtype=np.int64)[None, :]


def rotation(eps, S, C, cp, sign):
    """e^{sign 2 pi i eps_f m / C}, float64 (F, S, 1, C + cp); the phase reduced
    modulo one turn exactly (eps as the float64 of its f32 value)."""
    eps = np.asarray(eps, np.float32).astype(np.float64)
    eps = np.where(np.isfinite(eps), eps, 0.0)
    turns = eps[:, None, None] * phase_index(S, C, cp)[None] / C
    turns -= np.rint(turns)
    return np.exp(sign * 2j * np.pi * turns)[:, :, None, :]


def derotate_ref(y, eps, cp):
    """x' = y e^{-2 pi i eps_f m / C} in float64 on the f32 input, rounded to complex64."""
    F, S, R, Cp = y.shape
    return (y.astype(np.complex128) * rotation(eps, S, Cp - cp, cp, -1.0)).astype(np.complex64)


def gamma_ref(y, cp, cp_skip=0):
    """(gamma (F,) complex128, eps (F,) float64) of the prefix estimator on the f32 input."""
    C = y.shape[-1] - cp
    a = y[..., cp_skip:cp].astype(np.complex128)
    b = y[..., C + cp_skip:C + cp].astype(np.complex128)
    g = (np.conj(a) * b).sum(axis=(1, 2, 3))
    return g, np.arctan2(g.imag, g.real) / (2 * np.pi)


def frames(F, S, R, C, cp, eps=None, seed=0):
    """dict(y complex64 (F, S, R, C + cp), X complex64 (K,), eps float32 (F,),
    clean complex64: the frames without rotation or noise -- what a receiver
    makes of them is the transmitted data at its output positions --, data
    (F, S-1, K): the transmitted QPSK by bin)."""
    key = (F, S, R, C, cp, None if eps is None else tuple(np.float32(eps).tolist()), seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, F, S, R, C, cp])
    if eps is None:
        eps = [EPS_CYCLE[f % len(EPS_CYCLE)] for f in range(F)]
    eps = np.asarray(eps, np.float32)
    assert eps.shape == (F,)
    K = C - 1
    X = _qpsk(rng, K).astype(np.complex64)
    D = np.zeros((F, S, C), np.complex128)
    D[:, :, 1:] = _qpsk(rng, (F, S, K))
    D[:, 0, 1:] = X
    h = (rng.standard_normal((F, R, TAPS)) + 1j * rng.standard_normal((F, R, TAPS))) / np.sqrt(2 * TAPS)
    Hf = np.fft.fft(h, C, axis=-1)                                   # (F, R, C)
    body = np.fft.ifft(D[:, :, None, :] * Hf[:, None, :, :], axis=-1) * np.sqrt(C)
    x = np.concatenate([body[..., C - cp:], body], axis=-1) if cp else body
    clean = x.astype(np.complex64)
    y = x * rotation(eps, S, C, cp, +1.0)
    y = y + SIGMA * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    out = dict(y=y.astype(np.complex64), X=X, eps=eps, clean=clean, data=D[:, 1:, 1:])
    for v in out.values():
        v.setflags(write=False)
    _cache[key] = out
    return out


def decision_errors(out, truth):
    """Outputs whose QPSK decision (either bit) differs from `truth`'s."""
    return int(np.count_nonzero((np.signbit(out.real) != np.signbit(truth.real)) |
                                (np.signbit(out.imag) != np.signbit(truth.imag))))
