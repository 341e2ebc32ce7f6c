"""Seeded pilots whose modulus is not 1, and the plain reference of the LS
estimate they go through (a shared helper module, like zf_cases.py).

Every other generator of the suite draws +-0.70710678 +- 0.70710678i or ones,
so that the division by |x|^2 in ls_conj (csrc/common.hpp) divides by 1.  The
families here keep |x|^2 away from 1:

  fill_gpu  all 1 + 1j         the reference's GPU fallback pilots (gpuLS.cu:57-63), |x|^2 = 2
  fill_cpu  all 0.707 + 0.707j its CPU fallback (matrix_readX), |x|^2 = 0.999698
  boosted   modulus 2^U(-1, 1), phase U[0, 2 pi) per bin: +-6 dB, |Re x| != |Im x|
  wide      modulus 2^e, e in -20 .. 20 without 0, arbitrary phase: only for entries that take
            frequency-domain symbols (an f32 FFT cannot resolve a bin 2^-40
            below its row); |x|^2 stays a normal float
"""
import numpy as np

import helpers

FAMILIES = ("fill_gpu", "fill_cpu", "boosted", "wide")
FILL_FAMILIES = ("fill_gpu", "fill_cpu")


def pilots(family, K, seed=0):
    """(K,) complex64 pilots of `family`."""
    rng = np.random.default_rng([seed, K])
    if family == "fill_gpu":
        return np.full(K, 1 + 1j, np.complex64)
    if family == "fill_cpu":
        return np.full(K, 0.707 + 0.707j, np.complex64)
    if family == "boosted":
        mod = 2.0 ** rng.uniform(-1, 1, K)
    elif family == "wide":
        e = rng.integers(-20, 20, K)
        mod = 2.0 ** np.where(e >= 0, e + 1, e)  # -20 .. -1, 1 .. 20: one draw in 41 of 2^0 would be a unit pilot
    else:
        raise ValueError(family)
    return (mod * np.exp(2j * np.pi * rng.uniform(0, 1, K))).astype(np.complex64)


def ls128(Y, X):
    """The plain reference in complex128 on the same f32 inputs: Y (..., R, C)
    frequency-domain pilot symbol, X (K,) -> (Hconj = conj(Y[..., 1:] / X)
    (..., R, K), P = sum_r |Hconj|^2 (..., K))."""
    Y = np.asarray(Y, np.complex64).astype(np.complex128)
    X = np.asarray(X, np.complex64).astype(np.complex128)
    H = np.conj(Y[..., 1:] / X)
    return H, np.sum(np.abs(H) ** 2, axis=-2)


def elementwise(got, ref, rtol=helpers.RTOL):
    """|got - ref| <= rtol |ref| for every element, all values finite: the
    metric for the `wide` family, where helpers.parity's rms floor would hide
    the small bins.  Returns the largest relative error."""
    got = np.asarray(got, np.complex128).ravel()
    ref = np.asarray(ref, np.complex128).ravel()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "non-finite output"
    assert np.all(np.isfinite(ref)), "non-finite reference"
    if ref.size == 0:
        return 0.0
    err, mag = np.abs(got - ref), np.abs(ref)
    assert np.all(err <= rtol * mag), (
        f"element-wise relative error {np.max(err / np.maximum(mag, 1e-300)):.3e} > {rtol:g}")
    return float(np.max(err / np.maximum(mag, 1e-300)))


def compare(family, got, ref):
    """The metric the issue sets per family: elementwise for `wide`, helpers.parity for the rest."""
    if family == "wide":
        return elementwise(got, ref)
    return helpers.parity(got, ref)


# The stage-entry shapes (R, C) of ofdm_ls_estimate, shared by the CPU and the GPU file.
STAGE_SHAPES = [(1, 4), (3, 7), (5, 64), (16, 1024)]


def stage_input(family, R, C, noise=0.01, seed=0):
    """-> (Y (R, C) complex64, X (K,), H_true (R, K) complex128): Y[:, 1:] = H_true X + noise |X| n, bin 0 noise
    only.  With noise 0 the f32 rounding of Y is all that separates conj(Hconj) from H_true."""
    K = C - 1
    X = pilots(family, K, seed)
    rng = np.random.default_rng([seed, R, C, 7])
    H = (rng.standard_normal((R, K)) + 1j * rng.standard_normal((R, K))) / np.sqrt(2)
    n = (rng.standard_normal((R, C)) + 1j * rng.standard_normal((R, C))) / np.sqrt(2)
    Y = np.zeros((R, C), np.complex128)
    Y[:, 1:] = H * X.astype(np.complex128)
    Y[:, 1:] += noise * np.abs(X.astype(np.complex128)) * n[:, 1:]
    Y[:, 0] = noise * n[:, 0]
    return Y.astype(np.complex64), X, H
