"""Soft output on the GPU: ofdm_frame_noise_estimate and ofdm_frame_soft_demap
against a float64 numpy statement of the formulas in include/ofdm_lsmrc.h,
applied to the GPU's own Z and to P from ofdm_frame_export_estimate, so that
both sides see identical inputs.

Frames are built in numpy in the frequency domain: channel CN(0, 1) per
(frame, antenna, subcarrier), QPSK pilots, known random bits through this
file's own 38.211 mapper, complex noise of std 0.05 per antenna bin.  The
shapes whose time-domain estimate is kept in a receiver's lane order (C =
1024, 1536, 2048, 4096) go through torch.fft.ifft + frame_demod, which is the
only way to get such a workspace; the others through frame_demod_freq.

Bounds (none taken from what the kernels return):
  f32   |llr - ref| <= 1e-5 (P/s2) (|Re Z| + |Im Z| + 1): the per-axis function
        is at most 8 f32 operations on magnitudes below |Z| + 1 and the scale a
        reciprocal and a product, ~10 * 2^-24 of that magnitude; 1e-5 is the
        project's RTOL (tests/helpers.py).
  i8    |q - clamp(rint(ref scale))| <= 1 everywhere, equality wherever no
        rounding boundary lies within the f32 bound times scale of ref scale;
        at most 2 % of the elements may be excused that way.
  noise |nv - ref| <= 1e-5 ref: a fixed-order f32 sum of N <= 2^17
        non-negative terms errs by ~(log2 N + 5) 2^-24 = 1.5e-6.
"""
import functools

import numpy as np
import pytest

from soft_cases import A, llr_bound, out_src, ref_llr, ref_noise_var, ref_slice  # the float64 statement

pytestmark = pytest.mark.gpu

NOISE_STD = 0.05

# (F, S, R, C): path
SHAPES = {
    (3, 3, 2, 8): "tiny, K = 7",
    (2, 4, 3, 9): "even K: the three-segment branch of out_src",
    (3, 3, 4, 64): "generic bin-layout workspace",
    (3, 3, 4, 1024): "lane-order workspace; a tile of 1024 elements straddles symbols and frames",
    (2, 2, 4, 2048): "fused receiver, other lane order",
    (1, 2, 4, 4096): "fused receiver, other lane order",
    (2, 3, 4, 1536): "fused non-power-of-two",
}
TIME_DOMAIN_C = (1024, 1536, 2048, 4096)
CASES = [(shape, bps) for shape in SHAPES for bps in ((2, 4, 6, 8) if shape[3] in (64, 1024) else (2, 6))]


def map_38211(bits):
    """bits [..., bps] in {0, 1} -> unit-energy Gray-mapped symbols (3GPP TS 38.211 5.1.3-5.1.6)"""
    bps = bits.shape[-1]
    s = 1 - 2 * bits.astype(np.float64)

    def axis(b):  # the bits of one axis, most significant first
        amp = np.ones(b.shape[:-1])
        for i in range(b.shape[-1] - 1, 0, -1):  # 2^i - s_i (...): 16-QAM 2 - s2; 64-QAM 4 - s2 (2 - s4); ...
            amp = 2.0 ** (b.shape[-1] - i) - b[..., i] * amp
        return b[..., 0] * amp

    return A[bps] * (axis(s[..., 0::2]) + 1j * axis(s[..., 1::2]))


def make_frames(F, S, R, C, bps, seed=0):
    """Frequency-domain frames Y [F, S, R, C], pilots X [K], bits in OUTPUT order [F, S-1, K, bps]"""
    rng = np.random.default_rng([seed, F, S, R, C, bps])
    K = C - 1
    X = map_38211(rng.integers(0, 2, (K, 2)))
    H = (rng.standard_normal((F, 1, R, K)) + 1j * rng.standard_normal((F, 1, R, K))) / np.sqrt(2)
    bits = rng.integers(0, 2, (F, S - 1, K, bps)).astype(np.uint8)
    sym = np.concatenate([np.broadcast_to(X, (F, 1, K)), map_38211(bits)], axis=1)  # [F, S, K] by subcarrier
    Y = np.zeros((F, S, R, C), np.complex128)
    Y[..., 1:] = H * sym[:, :, None, :]
    Y += NOISE_STD / np.sqrt(2) * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    return Y.astype(np.complex64), X.astype(np.complex64), bits[:, :, out_src(K), :]


@functools.lru_cache(maxsize=None)
def run_case(shape, bps):
    """One receiver run and the float64 references, shared by the tests of a case (read only)."""
    import torch
    import ofdm_lsmrc as ofdm
    F, S, R, C = shape
    K = C - 1
    dev = torch.device("cuda:0")
    Yh, Xh, bits = make_frames(F, S, R, C, bps)
    Y, X = torch.from_numpy(Yh).to(dev), torch.from_numpy(Xh).to(dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    if C in TIME_DOMAIN_C:
        z = ofdm.frame_demod(torch.fft.ifft(Y, dim=-1).contiguous(), X, 0, ws=ws)
    else:
        z = ofdm.frame_demod_freq(Y, X, ws=ws)
    nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, bps)
    llr = ofdm.frame_soft_demap(z, ws, F, S, R, C, bps, nv)
    P = torch.stack([ofdm.frame_export_estimate(ws, F, S, R, C, f)[1] for f in range(F)])
    torch.cuda.synchronize()
    Zh, nvh = z.cpu().numpy(), nv.cpu().numpy()
    Pk = P.cpu().numpy().astype(np.float64)[:, out_src(K)][:, None, :]
    scale = Pk / nvh.astype(np.float64)[:, None, None]
    return dict(z=z, ws=ws, nv=nv, llr=llr.cpu().numpy(), Z=Zh, nvh=nvh, Pk=Pk, scale=scale, bits=bits,
                ref=ref_llr(Zh, scale, bps), bound=llr_bound(Zh, scale))


def test_mapper_and_reference_agree():
    """The file's own mapper and LLR reference: unit energy, and noiseless points decode to their bits."""
    for bps in (2, 4, 6, 8):
        n = 1 << bps
        bits = ((np.arange(n)[:, None] >> np.arange(bps)) & 1).astype(np.uint8)
        pts = map_38211(bits)
        assert len(set(np.round(pts, 9))) == n
        assert abs(np.mean(np.abs(pts) ** 2) - 1) < 1e-12
        assert np.array_equal(ref_llr(pts, 1.0, bps) < 0, bits.astype(bool))
        assert np.allclose(ref_slice(pts * (1 + 1e-3), bps), pts)
    # 38.211 table 5.1.4: b = 0000 -> (1 + 1j)/sqrt(10), b = 0011 (b2 = b3 = 1) -> (3 + 3j)/sqrt(10)
    assert np.allclose(map_38211(np.array([[0, 0, 0, 0], [0, 0, 1, 1], [1, 0, 0, 0]])),
                       np.array([1 + 1j, 3 + 3j, -1 + 1j]) / np.sqrt(10))


@pytest.mark.parametrize("shape,bps", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bps{v}")
def test_f32_parity(dev, shape, bps):
    c = run_case(shape, bps)
    F, S, R, C = shape
    assert c["llr"].shape == (F, S - 1, C - 1, bps) and c["llr"].dtype == np.float32
    assert np.all(np.isfinite(c["llr"]))
    err = np.abs(c["llr"].astype(np.float64) - c["ref"])
    worst = np.max(err / c["bound"])
    print(f"{shape} bps={bps}: max |llr - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("shape,bps", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bps{v}")
def test_noise_estimate(dev, ofdm, shape, bps):
    import torch
    c = run_case(shape, bps)
    F, S, R, C = shape
    ref = ref_noise_var(c["Z"], c["Pk"], bps)
    rel = np.max(np.abs(c["nvh"].astype(np.float64) - ref) / ref)
    print(f"{shape} bps={bps}: noise estimate max rel err {rel:.3e}, nv/sigma^2 = {c['nvh'] / NOISE_STD ** 2}")
    assert c["nvh"].dtype == np.float32 and c["nvh"].shape == (F,)
    assert rel <= 1e-5
    again = ofdm.frame_noise_estimate(c["z"], c["ws"], F, S, R, C, bps)
    assert torch.equal(again, c["nv"]), "two calls differ"


@pytest.mark.parametrize("shape,bps", [c for c in CASES if c[1] in (2, 4)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bps{v}")
def test_signs(dev, shape, bps):
    c = run_case(shape, bps)
    sent = c["bits"].astype(bool)
    assert np.count_nonzero((c["ref"] < 0) != sent) == 0, "the reference itself errs on this draw"
    assert np.count_nonzero((c["llr"] < 0) != sent) == 0


@pytest.mark.parametrize("shape,bps", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bps{v}")
def test_i8(dev, ofdm, shape, bps):
    c = run_case(shape, bps)
    F, S, R, C = shape
    qs = 127.0 / np.quantile(np.abs(c["ref"]), 0.95)  # ~5 % of the values saturate
    q = ofdm.frame_soft_demap(c["z"], c["ws"], F, S, R, C, bps, c["nv"], fmt="i8", scale=float(np.float32(qs)))
    q = q.cpu().numpy()
    assert q.dtype == np.int8 and q.shape == c["ref"].shape
    v = c["ref"] * np.float64(np.float32(qs))
    want = np.clip(np.rint(v), -127, 127)
    band = c["bound"] * np.float64(np.float32(qs))
    lo, hi = np.clip(np.rint(v - band), -127, 127), np.clip(np.rint(v + band), -127, 127)
    sure = lo == hi  # no rounding boundary within the f32 bound of ref * scale
    excused = 1 - np.mean(sure)
    sat = np.mean(np.abs(want) == 127)
    print(f"{shape} bps={bps}: scale {qs:.4g}, saturated {sat:.3%}, excused {excused:.3%}, "
          f"max |q - want| {np.max(np.abs(q - want)):.0f}")
    assert excused <= 0.02
    assert 0.02 < sat < 0.10
    assert q.min() >= -127, "-128 produced"
    assert np.all(np.abs(q - want) <= 1)
    assert np.array_equal(q[sure], want[sure].astype(np.int8))
    assert np.all(q[v > 127.5 + band] == 127) and np.all(q[v < -127.5 - band] == -127)


def test_noise_estimate_absorbs_ls_error(dev, ofdm):
    """Without the LS error nv / sigma^2 would be 1; with equal-energy pilots and QPSK data it is near 2."""
    import torch
    F, S, R, C = 8, 8, 8, 1024
    Yh, Xh, _ = make_frames(F, S, R, C, 2, seed=1)
    Y, X = torch.from_numpy(Yh).to(dev), torch.from_numpy(Xh).to(dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.frame_demod_freq(Y, X, ws=ws)
    nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, 2).cpu().numpy()
    ratio = nv / NOISE_STD ** 2
    print(f"nv / sigma^2 per frame: {ratio}, mean {ratio.mean():.4f}")
    assert np.all((0.5 < ratio) & (ratio < 4))


def test_refusals(dev, ofdm):
    import torch
    F, S, R, C = 2, 3, 4, 1024
    Yh, Xh, _ = make_frames(F, S, R, C, 2)
    iq = torch.fft.ifft(torch.from_numpy(Yh).to(dev), dim=-1).contiguous()
    X = torch.from_numpy(Xh).to(dev)
    z = ofdm.c64((F, S - 1, C - 1), dev).zero_()
    nv = torch.ones(F, dtype=torch.float32, device=dev)
    # an antenna-split partial |H|^2
    _, ws = ofdm.frame_ls_partial(iq, X, 0)
    for call in (lambda: ofdm.frame_noise_estimate(z, ws, F, S, R, C, 2),
                 lambda: ofdm.frame_soft_demap(z, ws, F, S, R, C, 2, nv)):
        with pytest.raises(ofdm.OfdmError, match=r"\(-1\).*partial"):
            call()
    # an estimate of another S (same workspace size: the fused C = 1024 workspace does not depend on S)
    ws2 = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(iq, X, 0, ws2)
    assert ofdm.workspace_bytes(F, S + 1, R, C) == ws2.numel()
    z2 = ofdm.c64((F, S, C - 1), dev).zero_()
    for call in (lambda: ofdm.frame_noise_estimate(z2, ws2, F, S + 1, R, C, 2),
                 lambda: ofdm.frame_soft_demap(z2, ws2, F, S + 1, R, C, 2, nv)):
        with pytest.raises(ofdm.OfdmError, match=r"\(-1\).*S=3"):
            call()
    # and the same workspace is accepted for the geometry it was filled for
    out = ofdm.frame_soft_demap(z, ws2, F, S, R, C, 2, nv)
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0  # Z = 0: every QPSK LLR is 0


def test_erasures(dev, ofdm):
    """A frame whose noise_var is 0, negative, inf or NaN gets llr = 0 in both formats."""
    import torch
    c = run_case((3, 3, 4, 64), 4)
    F, S, R, C = 3, 3, 4, 64
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        nv = c["nv"].clone()
        nv[1] = bad
        f32 = ofdm.frame_soft_demap(c["z"], c["ws"], F, S, R, C, 4, nv).cpu().numpy()
        i8 = ofdm.frame_soft_demap(c["z"], c["ws"], F, S, R, C, 4, nv, fmt="i8", scale=3.0).cpu().numpy()
        assert np.all(f32[1] == 0) and np.all(i8[1] == 0), bad
        assert np.array_equal(f32[[0, 2]], c["llr"][[0, 2]])


def test_synthetic_generator_link(dev, ofdm):
    """ofdm_synth_frames' QPSK bit n SET = positive axis = 38.211 bit 0: with count_symbol_errors == 0 the hard
    decisions llr > 0 are the generator's bits."""
    import torch
    F, S, R, C = 4, 5, 4, 1024
    rng = np.random.default_rng(7)
    X = torch.from_numpy(map_38211(rng.integers(0, 2, (C - 1, 2))).astype(np.complex64)).to(dev)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=0, seed=99, noise_std=NOISE_STD)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.frame_demod(iq, X, 0, ws=ws)
    assert int(ofdm.count_symbol_errors(z, S, seed=99).item()) == 0
    nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, 2)
    llr = ofdm.frame_soft_demap(z, ws, F, S, R, C, 2, nv)
    torch.cuda.synchronize()
    # count_symbol_errors == 0: (Re z > 0, Im z > 0) are the generator's bits (0, 1) at every element
    assert torch.equal(llr[..., 0] > 0, z.real > 0) and torch.equal(llr[..., 1] > 0, z.imag > 0)
    assert torch.all(nv > 0)
