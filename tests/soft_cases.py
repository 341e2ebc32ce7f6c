"""The float64 numpy statement of the soft-output formulas in
include/ofdm_lsmrc.h (ofdm_frame_soft_demap, ofdm_frame_noise_estimate) and the
f32 bound on an LLR, shared by test_soft_demap_gpu, test_footprint_cpu and
test_footprint_gpu."""
import numpy as np

A = {2: 1 / np.sqrt(2), 4: 1 / np.sqrt(10), 6: 1 / np.sqrt(42), 8: 1 / np.sqrt(170)}


def out_src(K):
    """subcarrier at output position k (shiftOneRow, odd and even K)"""
    k = np.arange(K)
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return np.where(k < n2, k + h, np.where(k < n2 + h, k - n2, k))


def ref_lambdas(x, bps):
    a = A[bps]
    t, out = x, []
    for i in range(bps // 2):
        if i:
            t = 2 * a * 2.0 ** (bps // 2 - 1 - i) - np.abs(t)
        out.append(4 * a * t)
    return out


def ref_llr(Z, scale, bps):
    """float64 max-log LLRs [..., bps], bit index fastest; scale broadcasts over Z"""
    Z = Z.astype(np.complex128)
    re, im = ref_lambdas(Z.real, bps), ref_lambdas(Z.imag, bps)
    out = np.empty(Z.shape + (bps,))
    for i in range(bps // 2):
        out[..., 2 * i] = scale * re[i]
        out[..., 2 * i + 1] = scale * im[i]
    return out


def ref_slice(Z, bps):
    a, L = A[bps], 2 ** (bps // 2 - 1)

    def axis(x):
        return (2 * np.clip(np.floor(x / (2 * a)), -L, L - 1) + 1) * a

    return axis(Z.real) + 1j * axis(Z.imag)


def ref_noise_var(Z, Pk, bps):
    """[F]: mean over (s, k) of P |Z - slice(Z)|^2; Pk [F, 1, K] in output order"""
    Z = Z.astype(np.complex128)
    return np.mean(Pk * np.abs(Z - ref_slice(Z, bps)) ** 2, axis=(1, 2))


def llr_bound(Z, scale):
    Z = Z.astype(np.complex128)
    return (1e-5 * scale * (np.abs(Z.real) + np.abs(Z.imag) + 1))[..., None]
