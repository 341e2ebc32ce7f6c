"""The float64 numpy statement of ofdm_frame_estimate_denoise
(include/ofdm_lsmrc.h), shared by test_denoise_gpu, test_footprint_cpu and
test_footprint_gpu."""
import numpy as np


def ref_denoise(Hconj, C, tp, tq):
    """The float64 statement: Hconj (..., R, K) -> (Hconj' (..., R, K), Hsqrd' (..., K))."""
    Hconj = np.asarray(Hconj, np.complex128)
    H = np.zeros(Hconj.shape[:-1] + (C,), np.complex128)
    H[..., 1:] = np.conj(Hconj)
    H[..., 0] = (H[..., 1] + H[..., C - 1]) / 2
    g = np.fft.ifft(H, axis=-1)
    n = np.arange(C)
    g[..., ~((n < tp) | (n >= C - tq))] = 0
    Hp = np.fft.fft(g, axis=-1)[..., 1:]
    return np.conj(Hp), np.sum(np.abs(Hp) ** 2, axis=-2)
