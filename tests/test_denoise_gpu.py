"""ofdm_frame_estimate_denoise on the GPU against a float64 numpy statement of
the operation in include/ofdm_lsmrc.h, applied to the GPU's own LS estimate
(ofdm_frame_export_estimate of every frame before denoising), so that both
sides start from identical inputs.

Frames are built in numpy: a channel of L taps CN(0, 1/L) per (frame,
antenna), rolled `shift` samples towards negative delays where the window
keeps pre-cursor taps, unit-modulus QPSK pilots and data on the bins 1 .. C-1,
complex noise of variance sigma^2 per antenna bin, an inverse FFT and a
cyclic prefix.

Bounds (none taken from what the kernels return):
  estimate  helpers.parity at the project's RTOL = 1e-5 (norm-relative and
            element-wise with the rms floor) on Hconj and on Hsqrd: two f32
            transforms of C <= 8192 points err by about log2(C) 2^-24 of the
            row's rms each, 2e-6 at the most.
  consumers the same parity against the float64 MRC formula on the exported
            denoised estimate; bit equality where two entries run one kernel.
  benefit   the float64 statement is asserted first (so the inputs are proven
            suitable), then the GPU figure within 1e-3 relative of it.

Hsqrd is compared with the same parity metric (1e-5 of max(|ref|, rms(ref))):
with R = 1 a bin in a deep fade holds a |H'|^2 far below the row's rms, and
the transforms' error is relative to the rms, not to the bin.

Measured on an MI355X: Hconj 2.1e-8 - 1.6e-7 norm-relative and
at most 6.3e-7 element-wise, Hsqrd 2.3e-8 - 2.4e-7 and at most 7.5e-7, over
every shape of this file.
"""
import functools

import numpy as np
import pytest

from any_c_cases import CALLER_LENGTHS
from denoise_cases import ref_denoise  # the float64 statement
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

A = np.float32(0.70710678)


# ------------------------------------------------------------------ builders

def qpsk(rng, shape):
    return (rng.choice([-A, A], shape) + 1j * rng.choice([-A, A], shape)).astype(np.complex64)


def out_src(K):
    """subcarrier at output position k (shiftOneRow, odd and even K)"""
    k = np.arange(K)
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return np.where(k < n2, k + h, np.where(k < n2 + h, k - n2, k))


@functools.lru_cache(maxsize=None)
def make_frames(F, S, R, C, cp, L, shift=0, sigma=0.05, seed=0):
    """-> iq (F, S, R, C + cp) complex64, X (K,) pilots, Htrue (F, R, C), data (F, S-1, K) by subcarrier.
    Computed once per argument set and shared; callers do not modify the arrays."""
    rng = np.random.default_rng(seed)
    K = C - 1
    X = qpsk(rng, K)
    h = np.zeros((F, R, C), np.complex128)
    h[..., :L] = (rng.standard_normal((F, R, L)) + 1j * rng.standard_normal((F, R, L))) / np.sqrt(2 * L)
    h = np.roll(h, -shift, axis=-1)
    H = np.fft.fft(h, axis=-1)
    data = qpsk(rng, (F, S - 1, K))
    tx = np.zeros((F, S, 1, C), np.complex128)
    tx[:, 0, 0, 1:] = X
    tx[:, 1:, 0, 1:] = data
    Y = H[:, None] * tx
    Y = Y + sigma * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2)
    Y[..., 0] = 0
    x = np.fft.ifft(Y, axis=-1)
    iq = np.concatenate([x[..., C - cp:], x], axis=-1) if cp else x
    for a in (X, H, data):
        a.setflags(write=False)
    iq = np.ascontiguousarray(iq.astype(np.complex64))
    iq.setflags(write=False)
    return iq, X, H, data


def ref_mrc(iq, cp, Hconj, P):
    """float64 MRC of the data symbols: iq (F, S, R, C + cp), Hconj (F, R, K), P (F, K) -> (F, S-1, K) rotated."""
    Y = np.fft.fft(np.asarray(iq[:, 1:, :, cp:], np.complex128), axis=-1)[..., 1:]
    Z = np.sum(Y * np.asarray(Hconj, np.complex128)[:, None], axis=2) / np.asarray(P, np.float64)[:, None]
    return Z[..., out_src(Z.shape[-1])]


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cached inputs are read-only


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def export_all(ofdm, ws, F, S, R, C):
    """(Hconj (F, R, K), Hsqrd (F, K)) of every frame, on the host."""
    import torch
    hp = [ofdm.frame_export_estimate(ws, F, S, R, C, f) for f in range(F)]
    return host(torch.stack([h for h, _ in hp])), host(torch.stack([p for _, p in hp]))


def same_bits(a, b):
    import torch
    bits = lambda t: (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.uint8)
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def up256(n):
    return (n + 255) & ~255


def estimate(ofdm, dev, iq, X, cp, how="td"):
    """A workspace holding the estimate of `iq`: "td" frame_estimate, "freq" frame_estimate_freq (bin layout)."""
    import torch
    F, S, R, Cp = iq.shape
    C = Cp - cp
    ws = ofdm.workspace(F, S, R, C, dev)
    Xd = to_dev(X, dev)
    if how == "td":
        d = to_dev(iq, dev)
        ofdm.frame_estimate(d, Xd, cp, ws)
    else:
        d = torch.fft.fft(to_dev(iq[..., cp:], dev), dim=-1).contiguous()
        ofdm.frame_estimate_freq(d, Xd, ws)
    return ws, d, Xd


def check_denoise(ofdm, dev, F, S, R, C, cp, L, tp, tq, shift=0, how="td", seed=0):
    iq, X, _, _ = make_frames(F, S, R, C, cp, L, shift, 0.05, seed)
    ws, d, _ = estimate(ofdm, dev, iq, X, cp, how)
    H0, P0 = export_all(ofdm, ws, F, S, R, C)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, tp, tq)
    H1, P1 = export_all(ofdm, ws, F, S, R, C)
    if tp + tq == C:
        Href, Pref = H0, P0  # every tap kept: the estimate before denoising
    else:
        Href, Pref = ref_denoise(H0, C, tp, tq)
    eh = parity(H1, Href, RTOL)
    ep = parity(P1, Pref, RTOL)
    print(f"denoise F={F} S={S} R={R} C={C} {how} window=({tp},{tq}): Hconj norm-rel {eh[0]:.2e} elem-rel {eh[1]:.2e}, "
          f"Hsqrd norm-rel {ep[0]:.2e} elem-rel {ep[1]:.2e}")
    return ws, d, iq, H1, P1


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("R", [5, 1])
@pytest.mark.parametrize("window", [(1, 0), (16, 0), (24, 8), (1019, 5), (1024, 0)])
def test_c1024_lane_order(ofdm, dev, R, window):
    tp, tq = window
    check_denoise(ofdm, dev, 3, 2, R, 1024, 7, 16, tp, tq, shift=min(tq, 5))


@pytest.mark.parametrize("window", [(16, 0), (24, 8)])
def test_c1024_bin_layout(ofdm, dev, window):
    tp, tq = window
    check_denoise(ofdm, dev, 3, 2, 5, 1024, 0, 16, tp, tq, shift=min(tq, 5), how="freq")


@pytest.mark.parametrize("C,L,window", [
    (256, 8, (12, 4)), (1536, 16, (24, 8)), (2048, 16, (24, 8)), (4096, 16, (24, 8)),   # each lane order
    (600, 12, (16, 4)), (7, 2, (3, 1)), (4, 2, (2, 1)),                                 # bin layout: mixed radix, prime, tiny
] + [(C, 12, (16, 4)) for C in CALLER_LENGTHS])  # a prime above 8, a 7 and a 5 in one plan per capacity; 7 * 7
def test_other_c(ofdm, dev, C, L, window):
    tp, tq = window
    check_denoise(ofdm, dev, 2, 2, 3, C, min(5, C), L, tp, tq, shift=min(tq, 3))


def test_c8192(ofdm, dev):
    check_denoise(ofdm, dev, 1, 2, 2, 8192, 9, 16, 24, 8, shift=5)


def test_frequency_domain_estimate_other_c(ofdm, dev):
    """a bin-layout workspace at a C whose time-domain estimate would be in lane order"""
    check_denoise(ofdm, dev, 2, 2, 3, 2048, 0, 16, 24, 8, shift=5, how="freq")


# ------------------------------------------------------- untouched regions

@pytest.mark.parametrize("C", [1024, 256, 600])
def test_untouched_regions_then_combine(ofdm, dev, C):
    """Bin 0 of every Hc row (position 0 in every layout of lane_layout.hpp), P[f][0] and the flag and ticket
    area keep their bits; frame_combine then runs on the same workspace and matches the float64 MRC."""
    import torch
    F, S, R, cp = 3, 3, 5, 7
    iq, X, _, _ = make_frames(F, S, R, C, cp, 8, 3, 0.05, 1)
    ws, d, _ = estimate(ofdm, dev, iq, X, cp)
    torch.cuda.synchronize()
    nh, npb, nfl = up256(F * R * C * 8), up256(F * C * 4), up256(F * 8)
    Hc = ws[:F * R * C * 8].view(torch.complex64).view(F, R, C)
    P = ws[nh:nh + F * C * 4].view(torch.float32).view(F, C)
    Hc[:, :, 0] = 12345.0 + 6789.0j  # sentinels: neither read into a result nor written
    P[:, 0] = 424242.0
    before = ws.clone()
    H0, _ = export_all(ofdm, ws, F, S, R, C)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 12, 4)
    torch.cuda.synchronize()
    after = ws.clone()
    bHc = before[:F * R * C * 8].view(torch.complex64).view(F, R, C)
    aHc = after[:F * R * C * 8].view(torch.complex64).view(F, R, C)
    assert same_bits(aHc[:, :, 0], bHc[:, :, 0])
    assert not same_bits(aHc[:, :, 1:], bHc[:, :, 1:])
    assert same_bits(after[nh:nh + F * C * 4].view(torch.float32).view(F, C)[:, 0],
                     before[nh:nh + F * C * 4].view(torch.float32).view(F, C)[:, 0])
    assert torch.equal(after[nh + npb:nh + npb + nfl + 4096], before[nh + npb:nh + npb + nfl + 4096])
    H1, P1 = export_all(ofdm, ws, F, S, R, C)
    Href, Pref = ref_denoise(H0, C, 12, 4)
    parity(H1, Href, RTOL)
    parity(P1, Pref, RTOL)
    out = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_combine(d, cp, ws, out)
    parity(host(out), ref_mrc(iq, cp, H1, P1), RTOL)
    ofdm.device_status()


# ------------------------------------------------------------ launch rounds

def test_grid_loop_third_round(ofdm, dev):
    """One workgroup per frame, a persistent grid of 4 workgroups per CU at C <= 2048: 2 * grid + 3 frames
    drive the frame loop (and its prefetch across frames) to a third round with a remainder."""
    import torch
    C, R, S, cp = 64, 3, 2, 0
    grid = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    F = 2 * grid + 3
    assert F > 2 * grid and F % grid != 0
    check_denoise(ofdm, dev, F, S, R, C, cp, 4, 6, 2, shift=2)


def test_row_groups_with_a_remainder(ofdm, dev):
    """R = 19 rows at C = 256: groups of 8, 8 and 3 rows of one frame through one workgroup in order."""
    check_denoise(ofdm, dev, 2, 2, 19, 256, 4, 8, 12, 4, shift=3)


# -------------------------------------------------------------- determinism

@pytest.mark.parametrize("C", [1024, 256])
def test_bit_identical_from_run_to_run(ofdm, dev, C):
    import torch
    F, S, R, cp = 3, 2, 19, 7
    iq, X, _, _ = make_frames(F, S, R, C, cp, 8, 3, 0.05, 2)
    ws, _, _ = estimate(ofdm, dev, iq, X, cp)
    torch.cuda.synchronize()
    saved = ws.clone()
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 12, 4)
    torch.cuda.synchronize()
    first = ws.clone()
    ws.copy_(saved)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 12, 4)
    torch.cuda.synchronize()
    assert torch.equal(ws, first)
    assert not torch.equal(first, saved)


# ---------------------------------------------------------------- consumers

@pytest.mark.parametrize("C", [1024, 256])
def test_frame_combine_on_the_denoised_estimate(ofdm, dev, C):
    import torch
    F, S, R, cp = 3, 3, 5, 7
    ws, d, iq, H1, P1 = check_denoise(ofdm, dev, F, S, R, C, cp, 8, 12, 4, shift=3, seed=3)
    out = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_combine(d, cp, ws, out)
    parity(host(out), ref_mrc(iq, cp, H1, P1), RTOL)
    if C == 1024:  # the per-symbol receiver on frame 1: the same kernel, bit for bit
        z = ofdm.symbols_demod(d[1, 1:].contiguous(), ws, cp, frame=1)
        assert same_bits(z, out[1])


def test_sc16_estimate_denoise_combine(ofdm, dev):
    import torch
    F, S, R, C, cp = 3, 3, 5, 1024, 7
    iq, X, _, _ = make_frames(F, S, R, C, cp, 8, 3, 0.05, 3)
    scale = 2.0 ** -17  # |x| ~ 1 / sqrt(C) with peaks near 0.1: samples of a few thousand counts
    q = np.stack([np.rint(iq.real / scale), np.rint(iq.imag / scale)], axis=-1)
    assert np.abs(q).max() < 32767
    iq16 = to_dev(q.astype(np.int16), dev)
    Xd = to_dev(X, dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_sc16(iq16, Xd, cp, ws, scale=scale)
    H0, _ = export_all(ofdm, ws, F, S, R, C)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 12, 4)
    H1, P1 = export_all(ofdm, ws, F, S, R, C)
    Href, Pref = ref_denoise(H0, C, 12, 4)
    parity(H1, Href, RTOL)
    parity(P1, Pref, RTOL)
    out = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_combine_sc16(iq16, cp, ws, out, scale=scale)
    xq = (q[..., 0] + 1j * q[..., 1]) * scale
    parity(host(out), ref_mrc(xq, cp, H1, P1), RTOL)


def test_refusals_that_need_a_registered_workspace(ofdm, dev):
    """an estimate of another geometry and an antenna-split partial estimate: OFDM_E_ARG, nothing changed"""
    import torch
    F, S, R, C, cp = 2, 2, 3, 1024, 7
    iq, X, _, _ = make_frames(F, S, R, C, cp, 8, 0, 0.05, 4)
    ws, d, Xd = estimate(ofdm, dev, iq, X, cp)
    torch.cuda.synchronize()
    before = ws.clone()
    with pytest.raises(ofdm.OfdmError, match="holds no estimate"):
        ofdm.frame_estimate_denoise(ofdm.workspace(F, S, R, C, dev), F, S, R, C, 16, 0)
    for args in ((F + 1, S, R, C), (F, S + 1, R, C), (F, S, R + 1, C), (F, S, R, 512)):
        with pytest.raises(ofdm.OfdmError, match="workspace estimate is for"):
            ofdm.frame_estimate_denoise(ws, *args, 16, 0)
    with pytest.raises(ofdm.OfdmError, match="taps_post"):
        ofdm.frame_estimate_denoise(ws, F, S, R, C, 1020, 5)
    torch.cuda.synchronize()
    assert torch.equal(ws, before)
    ofdm.frame_ls_partial(d, Xd, cp, ws)
    torch.cuda.synchronize()
    partial = ws.clone()
    with pytest.raises(ofdm.OfdmError, match="partial"):
        ofdm.frame_estimate_denoise(ws, F, S, R, C, 16, 0)
    torch.cuda.synchronize()
    assert torch.equal(ws, partial)


@pytest.mark.parametrize("C", [1024, 256])
def test_pipeline_set_denoise(ofdm, dev, C):
    """set_denoise against the direct three calls, and off against a pipeline that never heard of it: bit for bit"""
    import torch
    F, S, R, cp = 5, 3, 4, 7
    iq, X, _, _ = make_frames(F, S, R, C, cp, 8, 3, 0.05, 5)
    d, Xd = to_dev(iq, dev), to_dev(X, dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    want = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_estimate(d, Xd, cp, ws)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 12, 4)
    ofdm.frame_combine(d, cp, ws, want)
    raw = ofdm.frame_demod(d, Xd, cp)
    torch.cuda.synchronize()
    assert not same_bits(raw, want)

    def run(configure):
        out = np.full((F, S - 1, C - 1), np.nan, np.complex64)
        with ofdm.Pipeline(S, R, C, X, cp, chunk_frames=2, depth=2) as pl:
            configure(pl)
            pl.demod(iq, out)
            pl.sync()
        return torch.from_numpy(out).to(dev)

    assert same_bits(run(lambda pl: pl.set_denoise(12, 4)), want)
    never = run(lambda pl: None)

    def on_then_off(pl):
        pl.set_denoise(12, 4)
        pl.set_denoise(0)

    assert same_bits(run(on_then_off), never)
    with ofdm.Pipeline(S, R, C, X, cp, chunk_frames=2, depth=2) as pl:
        for bad in ((C, 1), (-1, 0), (4, -1), (0, 3)):
            with pytest.raises(ofdm.OfdmError, match="ofdm_pipeline_set_denoise"):
                pl.set_denoise(*bad)
        pl.set_denoise(C - 1, 1)


# ------------------------------------------------------------- what it buys

SIGMA = 0.05


@functools.lru_cache(maxsize=None)
def benefit_run(R, sigma):
    """(F, S, C) = (8, 8, 1024), L = 16, window (16, 0): raw and denoised estimates, GPU and float64 model."""
    import torch
    import ofdm_lsmrc as ofdm
    dev = torch.device("cuda:0")
    F, S, C, cp, L = 8, 8, 1024, 16, 16
    iq, X, Htrue, data = make_frames(F, S, R, C, cp, L, 0, sigma, 7)
    ws, d, _ = estimate(ofdm, dev, iq, X, cp)
    H0, P0 = export_all(ofdm, ws, F, S, R, C)
    z0 = ofdm.frame_demod(d, to_dev(X, dev), cp, ws=ofdm.workspace(F, S, R, C, dev))
    nv0 = host(ofdm.frame_noise_estimate(z0, ws, F, S, R, C, ofdm.MOD_QPSK))
    ofdm.frame_estimate_denoise(ws, F, S, R, C, 16, 0)
    H1, P1 = export_all(ofdm, ws, F, S, R, C)
    z1 = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_combine(d, cp, ws, z1)
    nv1 = host(ofdm.frame_noise_estimate(z1, ws, F, S, R, C, ofdm.MOD_QPSK))
    Hm, Pm = ref_denoise(H0, C, 16, 0)
    return dict(iq=iq, cp=cp, Htrue=Htrue[..., 1:], data=data[..., out_src(C - 1)], H0=H0, P0=P0, H1=H1, P1=P1, Hm=Hm,
                Pm=Pm, z0=host(z0), z1=host(z1), nv0=nv0, nv1=nv1)


def slice_qpsk(Z):
    return (np.where(Z.real >= 0, A, -A) + 1j * np.where(Z.imag >= 0, A, -A)).astype(np.complex128)


def model_noise(Z, P):
    """mean over (s, k) of P |Z - slice(Z)|^2 per frame; Z rotated, P by subcarrier"""
    Pk = np.asarray(P, np.float64)[:, None, out_src(P.shape[-1])]
    return np.mean(Pk * np.abs(Z - slice_qpsk(Z)) ** 2, axis=(1, 2))


def test_estimate_mse_falls_to_the_kept_fraction(ofdm, dev):
    b = benefit_run(8, SIGMA)
    mse = lambda Hc: np.mean(np.abs(np.conj(np.asarray(Hc, np.complex128)) - b["Htrue"]) ** 2) / SIGMA ** 2
    raw, model, gpu = mse(b["H0"]), mse(b["Hm"]), mse(b["H1"])
    print(f"estimate MSE / sigma^2: raw {raw:.4f}, float64 model {model:.5f}, GPU {gpu:.5f}")
    assert 0.9 < raw < 1.1
    assert model < 0.02
    assert abs(gpu - model) <= 1e-3 * model
    assert gpu < 0.02


def test_noise_estimate_no_longer_absorbs_the_ls_error(ofdm, dev):
    b = benefit_run(8, SIGMA)
    m0 = model_noise(ref_mrc(b["iq"], b["cp"], b["H0"], b["P0"]), b["P0"]).mean() / SIGMA ** 2
    m1 = model_noise(ref_mrc(b["iq"], b["cp"], b["Hm"], b["Pm"]), b["Pm"]).mean() / SIGMA ** 2
    g0, g1 = b["nv0"].mean() / SIGMA ** 2, b["nv1"].mean() / SIGMA ** 2
    print(f"noise_var / sigma^2: raw model {m0:.4f} GPU {g0:.4f}; denoised model {m1:.4f} GPU {g1:.4f}")
    assert m0 > 1.9 and m1 < 1.1
    assert abs(g0 - m0) <= 1e-3 * m0 and abs(g1 - m1) <= 1e-3 * m1
    assert g0 > 1.9 and g1 < 1.1


def test_symbol_errors_halve_at_low_snr(ofdm, dev):
    b = benefit_run(4, 1.0)
    errs = lambda Z: int(np.sum(slice_qpsk(Z) != slice_qpsk(b["data"])))
    m0 = errs(ref_mrc(b["iq"], b["cp"], b["H0"], b["P0"]))
    m1 = errs(ref_mrc(b["iq"], b["cp"], b["Hm"], b["Pm"]))
    g0, g1 = errs(b["z0"]), errs(b["z1"])
    n = b["data"].size
    print(f"QPSK symbol errors of {n}: raw model {m0} ({m0 / n:.3f}) GPU {g0}; denoised model {m1} ({m1 / n:.3f}) GPU {g1}")
    assert 2 * m1 <= m0
    assert abs(g0 - m0) <= 1e-3 * m0 and abs(g1 - m1) <= 1e-3 * m1
    assert 2 * g1 <= g0
