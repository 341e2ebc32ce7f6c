"""Pilots of non-unit modulus through every LS estimator on the GPU.

Every other GPU test feeds ls_conj (csrc/common.hpp) |x|^2 = 1 (the two
`boosted` fixtures of tests/golden/ apart), so that its division is never
seen.  Here the estimate itself is compared -- ofdm_frame_export_estimate,
ofdm_ls_estimate, d_P of ofdm_frame_ls_partial -- next to the output, and the
estimate's consumers (noise estimate, LLR scale, denoising) get a reference P
that does not come from the device.

References: pilot_cases.ls128 (complex128 on the same f32 inputs) where the
entry takes frequency-domain symbols, oracle.ls on the complex128 FFT of the
pilot rows where it takes time-domain ones; test_pilot_modulus_cpu.py shows
that both stay below 1e-6 of each other on these pilots and that a dropped or
wrong division misses RTOL by 30x (fill_cpu) to 1e5x.  Bounds: helpers.RTOL
through helpers.parity, or element by element (pilot_cases.elementwise) for
the `wide` family; the consumers keep the bounds of test_soft_demap_gpu.py
and test_denoise_gpu.py.

Shapes are the smallest that reach each kernel: F = 2 frames of S = 3 symbols,
noise 0.02, frames 0 and F - 1 compared.
"""
import functools

import numpy as np
import pytest

import pilot_cases as pc
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

F, S, NOISE = 2, 3, 0.02
TD_FAMILIES = ("fill_gpu", "fill_cpu", "boosted")
A = np.float32(0.70710678)


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def qpsk(rng, shape):
    return (rng.choice([-A, A], shape) + 1j * rng.choice([-A, A], shape)).astype(np.complex64)


def export(ofdm, ws, R, C, f, nframes=F, nsym=S):
    H, P = ofdm.frame_export_estimate(ws, nframes, nsym, R, C, frame=f)
    return host(H), host(P)


def pilot_fft(iq, f, prefix):
    """The pilot symbol of frame f in the frequency domain: complex128 FFT of the f32 samples, rounded to f32."""
    return np.fft.fft(iq[f, 0, :, prefix:].astype(np.complex128), axis=-1).astype(np.complex64)


# ------------------------------------------------------- a. the stage entry

@pytest.mark.parametrize("R,C", pc.STAGE_SHAPES)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_stage_ls_estimate(ofdm, oracle, dev, family, R, C):
    """ofdm_ls_estimate (k_ls_freq) against ls128, against the channel itself at noise 0, then ofdm_mrc_demod"""
    Y, X, Htrue = pc.stage_input(family, R, C)
    Href, Pref = pc.ls128(Y, X)
    Hc, P = ofdm.ls_estimate(to_dev(Y, dev), to_dev(X, dev))
    eh = pc.compare(family, host(Hc), Href)
    ep = pc.compare(family, host(P), Pref)
    print(f"{family} R={R} C={C}: Hconj {eh}, Hsqrd {ep}")

    Y0, _, _ = pc.stage_input(family, R, C, noise=0.0)
    Hc0, _ = ofdm.ls_estimate(to_dev(Y0, dev), to_dev(X, dev))
    pc.elementwise(np.conj(host(Hc0)), Htrue)

    rng = np.random.default_rng([R, C])
    nsym = 3
    Yd = np.zeros((nsym, R, C), np.complex128)
    Yd[..., 1:] = Htrue * qpsk(rng, (nsym, 1, C - 1))
    Yd += 0.01 / np.sqrt(2) * (rng.standard_normal(Yd.shape) + 1j * rng.standard_normal(Yd.shape))
    Yd = Yd.astype(np.complex64)
    out = host(ofdm.mrc_demod(to_dev(Yd, dev), Hc, P))
    Ho, Po = oracle.ls(Y, X)
    parity(out, np.stack([oracle.mrc(Yd[s], Ho, Po) for s in range(nsym)]))


# ------------------------------------- b. frequency-domain frame estimators

@functools.lru_cache(maxsize=None)
def freq_frames(family, R, C, bps=2, noise=NOISE):
    """Y (F, S, R, C) complex64 built on the host, X (K,): Y = H x + noise |x| n on the pilot symbol (so that the
    small bins of `wide` hold a channel, not noise), H x + noise n on the data symbols."""
    rng = np.random.default_rng([R, C, 11])
    K = C - 1
    X = pc.pilots(family, K, seed=R)
    H = (rng.standard_normal((F, 1, R, K)) + 1j * rng.standard_normal((F, 1, R, K))) / np.sqrt(2)
    sym = np.concatenate([np.broadcast_to(X.astype(np.complex128), (F, 1, K)), qpsk(rng, (F, S - 1, K))], axis=1)
    Y = np.zeros((F, S, R, C), np.complex128)
    Y[..., 1:] = H * sym[:, :, None, :]
    n = noise / np.sqrt(2) * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    n[:, 0, :, 1:] *= np.abs(X.astype(np.complex128))
    Y = (Y + n).astype(np.complex64)
    Y.setflags(write=False)
    X.setflags(write=False)
    return Y, X


@pytest.mark.parametrize("R", [3, 9])
@pytest.mark.parametrize("C", [64, 600, 601, 1024])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_freq_frame_estimators(ofdm, oracle, dev, family, C, R):
    """frame_estimate_freq + export, frame_demod_freq, frame_demod_freq_mfma (C a multiple of 64: the entry
    refuses every other C, which is asserted)"""
    Yh, Xh = freq_frames(family, R, C)
    Y, X = to_dev(Yh, dev), to_dev(Xh, dev)
    ref_out = oracle.frames_demod_freq(Yh, Xh)
    refs = {f: pc.ls128(Yh[f, 0], Xh) for f in (0, F - 1)}

    def check_estimate(ws, what):
        for f, (Href, Pref) in refs.items():
            H, P = export(ofdm, ws, R, C, f)
            eh, ep = pc.compare(family, H, Href), pc.compare(family, P, Pref)
            print(f"{family} R={R} C={C} {what} frame {f}: Hconj {eh}, Hsqrd {ep}")

    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_freq(Y, X, ws)
    check_estimate(ws, "estimate_freq")

    entries = [("demod_freq", ofdm.frame_demod_freq)]
    if C % 64 == 0:
        entries.append(("demod_freq_mfma", ofdm.frame_demod_freq_mfma))
    else:
        with pytest.raises(ofdm.OfdmError, match="not a multiple of 64"):
            ofdm.frame_demod_freq_mfma(Y, X)
    for what, entry in entries:
        ws = ofdm.workspace(F, S, R, C, dev)
        out = host(entry(Y, X, ws=ws))
        check_estimate(ws, what)
        print(f"{family} R={R} C={C} {what}: output {parity(out, ref_out)}")


# ------------------------------------------------ c. time-domain estimators

# C -> the estimator kernel that serves it
TD_KERNELS = {
    1024: "C = 1024: one-launch, two-launch, and spin_ticks = 0 (the MRC workgroups re-estimate)",
    2048: "fused 2048", 4096: "fused 4096",
    128: "tdsmall", 256: "tdsmall", 512: "tdsmall",
    1536: "fft512 family", 3072: "fft512 family", 6144: "fft512 family",
    600: "generic, even C", 75: "generic, odd C",
}


def td_flows(ofdm, C):
    if C != 1024:
        return {"default": {}}
    return {"one-launch": dict(flow=ofdm.FLOW_AUTO), "two-launch": dict(flow=ofdm.FLOW_TWO_LAUNCH),
            "spin0": dict(flow=ofdm.FLOW_AUTO, spin_ticks=0)}


@pytest.mark.parametrize("prefix", [0, 3])
@pytest.mark.parametrize("R", [1, 9])
@pytest.mark.parametrize("C", list(TD_KERNELS))
@pytest.mark.parametrize("family", TD_FAMILIES)
def test_time_domain_estimators(ofdm, oracle, dev, family, C, R, prefix):
    """frame_demod of synthetic frames: exported Hconj, Hsqrd against oracle.ls on the complex128 FFT of the
    pilot rows, the output against oracle.frames_demod, no QPSK decision error at R = 9.

    At R = 1 and noise 0.02 a single Rayleigh antenna fades below the noise in a few bins of every frame
    (P(|H| < 0.05) = 0.25 %), and no receiver decides those right: on an MI355X count_symbol_errors gives 0 - 12
    errors among the 296 - 24572 symbols of these cases, the same with |x|^2 = 2 (fill_gpu, an exact division) as
    with any pilot.  So there the count must be the oracle's: the decision errors of oracle.frames_demod's output
    against the generator's bits, computed on the host (reference_decision_errors)."""
    Xh = pc.pilots(family, C - 1, seed=R)
    X = to_dev(Xh, dev)
    seed = 300 + C + R
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=seed, noise_std=NOISE)
    a = host(iq)
    ref_out = oracle.frames_demod(a, Xh, prefix)
    refs = {f: oracle.ls(pilot_fft(a, f, prefix), Xh) for f in (0, F - 1)}
    for name, kw in td_flows(ofdm, C).items():
        ws = ofdm.workspace(F, S, R, C, dev)
        out = ofdm.frame_demod(iq, X, prefix, ws=ws, **kw)
        errs = int(ofdm.count_symbol_errors(out, S, seed=seed).item())
        for f, (Href, Pref) in refs.items():
            H, P = export(ofdm, ws, R, C, f)
            eh, ep = parity(H, Href), parity(P, Pref)
            print(f"{family} C={C} R={R} prefix={prefix} {name} frame {f}: Hconj {eh}, Hsqrd {ep}")
        eo = td_output_parity(host(out), ref_out, a, prefix, R)
        lo, hi = reference_decision_errors(ref_out, seed)
        print(f"{family} C={C} R={R} prefix={prefix} {name}: output {eo}, {errs} decision errors, "
              f"the oracle's output has {lo} to {hi}")
        if R > 1:
            assert errs == 0
        assert lo <= errs <= hi


def td_output_parity(out, ref, iq, prefix, R):
    """helpers.parity at RTOL.  At R = 1 the output is Z = Yd X / Y0, one bin divided by one bin: where the single
    antenna's channel fades, the rounding of the two f32 transforms -- about log2(C) 2^-24 of a row's rms each
    (test_denoise_gpu.py) -- is amplified by rms / |bin|, whatever the receiver does afterwards (the reference's
    own f32 arithmetic is at 1.0e-5 - 1.6e-5 there: test_gpu_parity.py, test_frame_demod_synth_vs_oracle).  So at
    R = 1 the element-wise bound is max(RTOL, log2(C) 2^-24 (rms(Y0) / |Y0[j]| + rms(Yd) / |Yd[j]|)) per element,
    from the complex128 FFT of the input, which leaves RTOL in force wherever the bins are not 10 dB or more below
    their rows; the norm-relative bound stays RTOL.  Measured on an MI355X: plain element-wise error 1.7e-6 - 2.5e-5
    over the R = 1 cases of this file, above RTOL in at most 12 of 24572 elements (as large with |x|^2 = 2, where the
    division is exact, as with any other pilot), at most 0.45 of this bound; norm-relative at most 1.6e-6."""
    if R > 1:
        return parity(out, ref)
    nrel, erel = parity(out, ref, rtol=1.0)
    C = iq.shape[-1] - prefix
    Yf = np.fft.fft(iq[:, :, 0, prefix:].astype(np.complex128), axis=-1)[..., 1:]  # (F, S, K) by subcarrier
    amp = np.sqrt(np.mean(np.abs(Yf) ** 2, axis=-1, keepdims=True)) / np.abs(Yf)
    u = np.log2(C) * 2.0 ** -24
    tol = np.maximum(RTOL, u * (amp[:, :1] + amp[:, 1:]))[..., out_src(C - 1)]
    ref128 = ref.astype(np.complex128)
    rel = np.abs(out - ref128) / np.maximum(np.abs(ref128), np.sqrt(np.mean(np.abs(ref128) ** 2)))
    print(f"R=1: plain parity {nrel:.2e} {erel:.2e}; worst error / single-antenna bound {np.max(rel / tol):.3f}, "
          f"{np.count_nonzero(rel > RTOL)} of {rel.size} elements above RTOL")
    assert nrel <= RTOL
    assert np.all(rel <= tol)
    return nrel, erel


def out_src(K):
    """subcarrier at output position k (shiftOneRow, odd and even K)"""
    k = np.arange(K)
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return np.where(k < n2, k + h, np.where(k < n2 + h, k - n2, k))


# The generator's data bits on the host (csrc/fft_synth.hip synth_bits, csrc/common.hpp hash4): bit 0 set <=> Re > 0,
# bit 1 set <=> Im > 0.  check_counter below holds this port against the generator and the counter themselves.
def splitmix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def synth_bits(seed, fg, s, j):
    a = lambda v: np.asarray(v, np.uint64)
    h = splitmix64(a([seed]) ^ np.uint64(2))
    return splitmix64(splitmix64(h ^ a(fg)) ^ ((a(s) << np.uint64(32)) | a(j))) & np.uint64(3)


def host_decisions_wrong(z, seed, frame0=0):
    """bool (F, S-1, K): the decision on z[f][s-1][k] is not the generator's symbol"""
    nf, nd, K = z.shape
    f, s, j = np.arange(nf)[:, None, None] + frame0, np.arange(1, nd + 1)[None, :, None], out_src(K)[None, None, :]
    bits = synth_bits(seed, f, s, j)
    return ((z.real > 0) != ((bits & np.uint64(1)) != 0)) | ((z.imag > 0) != ((bits & np.uint64(2)) != 0))


def reference_decision_errors(ref, seed, frame0=0):
    """(lo, hi): the decision errors of the oracle's output against the generator's bits, counting an element whose
    real or imaginary part lies within RTOL of zero (in the parity metric's scale) as either."""
    ref = ref.astype(np.complex128)
    scale = RTOL * np.maximum(np.abs(ref), np.sqrt(np.mean(np.abs(ref) ** 2)))
    open_ = (np.abs(ref.real) <= scale) | (np.abs(ref.imag) <= scale)
    wrong = host_decisions_wrong(ref, seed, frame0)
    lo = int(np.count_nonzero(wrong & ~open_))
    return lo, lo + int(np.count_nonzero(open_))


# ------------------------------------------------------------------ d. sc16

@pytest.mark.parametrize("scale", [2.0 ** -15, 1.0 / 32767], ids=["2^-15", "1/32767"])
def test_sc16_estimate_in_the_units_of_x(ofdm, oracle, dev, scale):
    import torch
    R, C, prefix = 5, 1024, 7
    Xh = pc.pilots("boosted", C - 1, seed=16)
    X = to_dev(Xh, dev)
    iq = host(ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=16, noise_std=NOISE))
    v = np.stack([iq.real, iq.imag], -1).astype(np.float64)
    q = np.ascontiguousarray(np.rint(v * (16000.0 / np.abs(v).max())).astype(np.int16))
    xq = np.ascontiguousarray(q.astype(np.float32) * np.float32(scale)).view(np.complex64)[..., 0]  # x = i16 * scale
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_sc16(to_dev(q, dev), X, prefix, ws, scale=float(np.float32(scale)))
    for f in (0, F - 1):
        Href, Pref = oracle.ls(pilot_fft(xq, f, prefix), Xh)
        H, P = export(ofdm, ws, R, C, f)
        print(f"sc16 scale {scale:.6e} frame {f}: Hconj {parity(H, Href)}, Hsqrd {parity(P, Pref)}")
    out = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.frame_combine(to_dev(xq, dev), prefix, ws, out)
    parity(host(out), oracle.frames_demod(xq, Xh, prefix))


# --------------------------------------------------------- e. antenna split

@pytest.mark.parametrize("C", [1024, 2048, 256, 1200])
def test_ls_partial(ofdm, oracle, dev, C):
    """d_P of every shard against ls128 on the shard's rows; two shards sum to the full estimate's Hsqrd"""
    import torch
    R, prefix, seed = 5, 3, 40 + C
    Xh = pc.pilots("boosted", C - 1, seed=5)
    X = to_dev(Xh, dev)
    shards = [ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=seed, noise_std=NOISE, r0=r0) for r0 in (0, R)]
    parts = []
    for iq in shards:
        Pd, ws = ofdm.frame_ls_partial(iq, X, prefix)
        Pd, a = host(Pd), host(iq)
        assert Pd.shape == (F, C - 1)
        for f in (0, F - 1):
            Href, Pref = pc.ls128(pilot_fft(a, f, prefix), Xh)
            H, Pw = export(ofdm, ws, R, C, f)
            print(f"C={C} frame {f}: d_P {parity(Pd[f], Pref)}, exported Hconj {parity(H, Href)}")
            parity(Pw, Pref)
        parts.append(Pd)
    full = torch.cat(shards, dim=2).contiguous()
    ws = ofdm.workspace(F, S, 2 * R, C, dev)
    ofdm.frame_estimate(full, X, prefix, ws)
    for f in (0, F - 1):
        _, Pfull = export(ofdm, ws, 2 * R, C, f)
        parity(parts[0][f].astype(np.float64) + parts[1][f], Pfull)
        parity(Pfull, pc.ls128(pilot_fft(host(full), f, prefix), Xh)[1])


# -------------------------- f. consumers, P computed on the host from ls128

@functools.lru_cache(maxsize=None)
def consumer_case(C, bps):
    """A receiver run on boosted pilots and the float64 noise and LLR models of test_soft_demap_gpu.py fed with
    P = ls128 of the frame's pilot symbol.  C = 1024: time domain (lane-order workspace); C = 600: frequency."""
    import torch
    import ofdm_lsmrc as ofdm
    import test_soft_demap_gpu as sd
    dev = torch.device("cuda:0")
    R, K = 4, C - 1
    rng = np.random.default_rng([C, bps, 13])
    Xh = pc.pilots("boosted", K, seed=bps)
    H = (rng.standard_normal((F, 1, R, K)) + 1j * rng.standard_normal((F, 1, R, K))) / np.sqrt(2)
    bits = rng.integers(0, 2, (F, S - 1, K, bps)).astype(np.uint8)
    sym = np.concatenate([np.broadcast_to(Xh.astype(np.complex128), (F, 1, K)), sd.map_38211(bits)], axis=1)
    Y = np.zeros((F, S, R, C), np.complex128)
    Y[..., 1:] = H * sym[:, :, None, :]
    Y += sd.NOISE_STD / np.sqrt(2) * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    X = to_dev(Xh, dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    if C == 1024:
        iq = np.fft.ifft(Y, axis=-1).astype(np.complex64)
        z = ofdm.frame_demod(to_dev(iq, dev), X, 0, ws=ws)
        Yp = np.stack([pilot_fft(iq, f, 0) for f in range(F)])
    else:
        Yh = Y.astype(np.complex64)
        z = ofdm.frame_demod_freq(to_dev(Yh, dev), X, ws=ws)
        Yp = Yh[:, 0]
    nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, bps)
    llr = ofdm.frame_soft_demap(z, ws, F, S, R, C, bps, nv)
    P = pc.ls128(Yp, Xh)[1]  # (F, K), float64, by subcarrier
    Pk = P[:, sd.out_src(K)][:, None, :]
    Zh, nvh = host(z), host(nv)
    scale = Pk / nvh.astype(np.float64)[:, None, None]
    return dict(Z=Zh, nv=nvh, llr=host(llr), Pk=Pk, noise_ref=sd.ref_noise_var(Zh, Pk, bps),
                llr_ref=sd.ref_llr(Zh, scale, bps), bound=sd.llr_bound(Zh, scale), bits=bits[:, :, sd.out_src(K), :])


@pytest.mark.parametrize("bps", [2, 4], ids=["qpsk", "qam16"])
@pytest.mark.parametrize("C", [1024, 600])
def test_noise_estimate_with_host_P(dev, C, bps):
    c = consumer_case(C, bps)
    rel = np.max(np.abs(c["nv"].astype(np.float64) - c["noise_ref"]) / c["noise_ref"])
    print(f"C={C} bps={bps}: noise estimate max rel err {rel:.3e}")
    assert c["nv"].shape == (F,) and c["nv"].dtype == np.float32
    assert rel <= 1e-5


@pytest.mark.parametrize("bps", [2, 4], ids=["qpsk", "qam16"])
@pytest.mark.parametrize("C", [1024, 600])
def test_soft_demap_with_host_P(dev, C, bps):
    c = consumer_case(C, bps)
    assert c["llr"].shape == (F, S - 1, C - 1, bps) and np.all(np.isfinite(c["llr"]))
    worst = np.max(np.abs(c["llr"].astype(np.float64) - c["llr_ref"]) / c["bound"])
    print(f"C={C} bps={bps}: max |llr - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert np.count_nonzero((c["llr"] < 0) != c["bits"].astype(bool)) == 0


# --------------------------------------------------------------- g. denoise

@pytest.mark.parametrize("keep_all", [False, True], ids=["window", "keep-all"])
@pytest.mark.parametrize("C,L,window", [(1024, 16, (24, 8)), (600, 12, (16, 4))], ids=["c1024-lane-order", "c600-bins"])
def test_denoise_from_host_estimate(ofdm, dev, C, L, window, keep_all):
    """Steps 1-5 of the header in complex128 from ls128 of the pilot rows, not from the device's own export"""
    import test_denoise_gpu as dn
    R, cp, sigma = 3, 5, 0.05
    tp, tq = (C - 5, 5) if keep_all else window
    rng = np.random.default_rng([C, 17])
    K = C - 1
    Xh = pc.pilots("boosted", K, seed=17)
    h = np.zeros((F, R, C), np.complex128)
    h[..., :L] = (rng.standard_normal((F, R, L)) + 1j * rng.standard_normal((F, R, L))) / np.sqrt(2 * L)
    Hf = np.fft.fft(np.roll(h, -3, axis=-1), axis=-1)
    tx = np.zeros((F, S, 1, C), np.complex128)
    tx[:, 0, 0, 1:] = Xh
    tx[:, 1:, 0, 1:] = qpsk(rng, (F, S - 1, K))
    Y = Hf[:, None] * tx
    Y = Y + sigma * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2)
    Y[..., 0] = 0
    x = np.fft.ifft(Y, axis=-1)
    iq = np.ascontiguousarray(np.concatenate([x[..., C - cp:], x], axis=-1).astype(np.complex64))
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(to_dev(iq, dev), to_dev(Xh, dev), cp, ws)
    ofdm.frame_estimate_denoise(ws, F, S, R, C, tp, tq)
    H1, P1 = dn.export_all(ofdm, ws, F, S, R, C)
    H0, P0 = pc.ls128(np.stack([pilot_fft(iq, f, cp) for f in range(F)]), Xh)
    Href, Pref = (H0, P0) if keep_all else dn.ref_denoise(H0, C, tp, tq)
    eh, ep = parity(H1, Href, RTOL), parity(P1, Pref, RTOL)
    print(f"denoise C={C} window=({tp},{tq}): Hconj {eh}, Hsqrd {ep}")


# ------------------------------------------- count_symbol_errors must count

def flip_cases(n, per_frame, rng):
    """flat indices to flip: the first and the last element, both sides of every frame boundary, a few more"""
    idx = {0, n - 1}
    for b in range(per_frame, n, per_frame):
        idx |= {b - 1, b}
    idx |= set(int(i) for i in rng.integers(0, n, 5))
    return np.array(sorted(idx))


def check_counter(ofdm, dev, nframes, nsym, C, frame0, extra=()):
    import torch
    seed = 1000 + C
    K = C - 1
    X = to_dev(pc.pilots("boosted", K, seed=3), dev)
    iq = ofdm.synth_frames(nframes, nsym, 1, C, X, seed=seed, frame0=frame0, noise_std=0.0)
    out = ofdm.frame_demod(iq, X, 0)
    count = lambda t, f0=frame0: int(ofdm.count_symbol_errors(t, nsym, seed=seed, frame0=f0).item())
    assert count(out) == 0
    assert not host_decisions_wrong(host(out), seed, frame0).any(), "the host port of synth_bits is not the generator's"
    n = out.numel()
    idx = np.union1d(flip_cases(n, (nsym - 1) * K, np.random.default_rng(C)), np.array(extra, np.int64))
    m = len(idx)
    assert m >= 3 and idx[0] == 0 and idx[-1] == n - 1
    sel = torch.from_numpy(idx).to(dev)
    for re, im in ((-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)):
        bad = torch.view_as_real(out.clone()).view(-1, 2)
        bad[sel] *= torch.tensor([re, im], device=dev)
        bad = torch.view_as_complex(bad.view(*out.shape, 2))
        assert count(bad) == m, (re, im)
        assert np.array_equal(np.flatnonzero(host_decisions_wrong(host(bad), seed, frame0)), idx)
    assert count(out) == 0
    return out, count, n


@pytest.mark.parametrize("frame0", [0, 5])
@pytest.mark.parametrize("C", [8, 7])
def test_count_symbol_errors_counts(ofdm, dev, C, frame0):
    """exactly m after m flips of the real part, of the imaginary part, of both (symbols, not bits);
    C = 7: K = 6, the three-memmove rotation"""
    check_counter(ofdm, dev, F, S, C, frame0)


def test_count_symbol_errors_second_grid_trip(ofdm, dev):
    """1 049 598 elements: more than the 4096 x 256 threads of one grid pass.  Flips on both sides of that
    boundary; then a frame0 that is not the generator's leaves one decision in four right."""
    nsym, C = 1027, 1024
    one_pass = 4096 * 256
    out, count, n = check_counter(ofdm, dev, 1, nsym, C, 0, extra=(one_pass - 1, one_pass, one_pass + 1))
    assert n == 1049598 and n > one_pass
    wrong = count(out, 1)
    print(f"frame0 off by one: {wrong} of {n} = {wrong / n:.4f}")
    assert 0.70 * n <= wrong <= 0.80 * n
