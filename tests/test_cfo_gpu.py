"""Carrier frequency offset on the GPU (include/ofdm_lsmrc.h, "carrier
frequency offset"): the derotating C = 1024 receiver against the CPU oracle on
x' (numpy float64 applies the definition to the f32 input and rounds to
complex64), the stand-alone derotator and the prefix estimator against numpy
float64, the closed loop estimate -> receiver, and the pipeline's CFO mode.
The tolerance is the project's RTOL throughout (helpers.parity, norm-wise and
element-wise); the estimator's is stated where it is used."""
import numpy as np
import pytest

import cfo_cases as cc
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cached inputs are read-only


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def nan_out(shape, dev):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.complex64, device=dev)


# ------------------------------------------------------- 1. receiver parity

# (F, S, R, cp) at C = 1024, eps: None = the cycle 0.03, -0.2, 0.45, 0, -0.004 over the frames
PARITY = [((2, 9, 16, 0), None),      # every workgroup inside one frame: the shared-Hc loop, even R, no prefix
          ((3, 4, 5, 7), None),       # workgroups straddle frames, tail waves, odd R, rows only 8-byte aligned
          ((1, 2, 1, 0), None),       # R = 1
          ((2, 3, 17, 16), None),     # the 16-wave LS takes a second pass
          ((512, 2, 5, 0), None),     # the 4-wave LS, 21 MB
          ((1, 101, 2, 16), (0.49,))]  # 46 turns by the last symbol: a symbol phase formed in f32 misses RTOL

_refs = {}


def parity_case(oracle, key, eps):
    """(frames, eps passed to the device (one frame's NaN, acting as 0), x', oracle output and estimate of x')"""
    k = (key, eps)
    if k not in _refs:
        F, S, R, cp = key
        c = cc.frames(F, S, R, 1024, cp, eps, seed=F + R)
        e = np.array(c["eps"], np.float32)
        if F > 1:
            e[F - 1] = np.nan
        xp = cc.derotate_ref(c["y"], e, cp)
        ref = oracle.frames_demod(xp, c["X"], cp)
        est = {f: oracle.ls(np.fft.fft(xp[f, 0, :, cp:].astype(np.complex128), axis=-1).astype(np.complex64), c["X"])
               for f in {0, F - 1}}
        for v in (e, xp, ref):
            v.setflags(write=False)
        _refs[k] = (c, e, xp, ref, est)
    return _refs[k]


@pytest.mark.parametrize("key,eps", PARITY)
def test_receiver_parity(ofdm, dev, oracle, key, eps):
    c, e, xp, ref, est = parity_case(oracle, key, eps)
    F, S, R, cp = key
    y, X, ed = to_dev(c["y"], dev), to_dev(c["X"], dev), to_dev(e, dev)
    outs = []
    for _ in range(2):
        out = nan_out(ref.shape, dev)
        ofdm.frame_demod_cfo(y, X, cp, ed, out=out)
        outs.append(host(out))
    assert np.all(np.isfinite(outs[0])), "an output element was not written"
    nrel, erel = parity(outs[0], ref)
    print(f"{key}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    # the rotation matters: the plain receiver on the same frames is far off
    if eps is None and F > 1:
        plain = host(ofdm.frame_demod(y, X, cp))
        assert np.linalg.norm(plain - ref) > 0.1 * np.linalg.norm(ref)


@pytest.mark.parametrize("key,eps", PARITY)
def test_estimate_of_the_derotated_frames(ofdm, dev, oracle, key, eps):
    c, e, xp, ref, est = parity_case(oracle, key, eps)
    F, S, R, cp = key
    y, X, ed = to_dev(c["y"], dev), to_dev(c["X"], dev), to_dev(e, dev)
    ws = ofdm.workspace(F, S, R, 1024, dev)
    ofdm.frame_estimate_cfo(y, X, cp, ws, ed)
    for f, (Href, Pref) in est.items():
        H, P = ofdm.frame_export_estimate(ws, F, S, R, 1024, f)
        eh, ep = parity(host(H), Href), parity(host(P), Pref)
        print(f"{key} frame {f}: Hconj {eh[0]:.2e} / {eh[1]:.2e}, Hsqrd {ep[0]:.2e} / {ep[1]:.2e}")
    # the estimate serves the combine as a stage of its own, bit for bit
    out = nan_out(ref.shape, dev)
    ofdm.frame_combine_cfo(y, cp, ws, out, ed)
    whole = nan_out(ref.shape, dev)
    ofdm.frame_demod_cfo(y, X, cp, ed, out=whole)
    assert np.array_equal(bits(host(out)), bits(host(whole)))


@pytest.mark.parametrize("key,eps", PARITY)
def test_estimate_denoise_combine(ofdm, dev, oracle, key, eps):
    """estimate_cfo -> denoise -> combine_cfo against the same chain of fp32 entries on x'"""
    c, e, xp, ref, est = parity_case(oracle, key, eps)
    F, S, R, cp = key
    y, X, ed, xd = to_dev(c["y"], dev), to_dev(c["X"], dev), to_dev(e, dev), to_dev(xp, dev)
    ws, wr = ofdm.workspace(F, S, R, 1024, dev), ofdm.workspace(F, S, R, 1024, dev)
    got, want = nan_out(ref.shape, dev), nan_out(ref.shape, dev)
    ofdm.frame_estimate_cfo(y, X, cp, ws, ed)
    ofdm.frame_estimate_denoise(ws, F, S, R, 1024, 12, 4)
    ofdm.frame_combine_cfo(y, cp, ws, got, ed)
    ofdm.frame_estimate(xd, X, cp, wr)
    ofdm.frame_estimate_denoise(wr, F, S, R, 1024, 12, 4)
    ofdm.frame_combine(xd, cp, wr, want)
    nrel, erel = parity(host(got), host(want))
    print(f"{key}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    assert not np.array_equal(bits(host(got)), bits(ref))  # the denoising took part


# ------------------------------------------------------------ 2. derotator

@pytest.mark.parametrize("F,S,R,C,cp,eps", [(1, 400, 2, 64, 16, (0.45,)),   # 225 turns by the last symbol
                                            (3, 3, 3, 600, 9, None),        # odd row length: 8-byte aligned rows
                                            (2, 2, 2, 4096, 0, None)])
def test_derotator(ofdm, dev, F, S, R, C, cp, eps):
    import torch
    c = cc.frames(F, S, R, C, cp, eps, seed=C)
    e = np.array(c["eps"], np.float32)
    if F > 1:
        e[F - 1] = np.nan
    want = cc.derotate_ref(c["y"], e, cp)
    n, G = c["y"].size, 4  # guard samples on either side
    ed = to_dev(e, dev)
    guard = np.float32(12345.0) + 1j * np.float32(-54321.0)

    def padded(fill):
        buf = torch.full((n + 2 * G,), complex(guard), dtype=torch.complex64, device=dev)
        if fill is not None:
            buf[G:G + n] = to_dev(fill, dev).reshape(-1)
        return buf

    src, dst = padded(c["y"]), padded(None)
    dst[G:G + n] = float("nan")
    view = lambda b: b[G:G + n].view(F, S, R, C + cp)
    ofdm.frame_cfo_derotate(view(src), cp, ed, out=view(dst))
    got = host(dst)
    nrel, erel = parity(got[G:G + n], want)
    print(f"C={C} out of place: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    assert np.all(got[:G] == guard) and np.all(got[G + n:] == guard)
    assert np.array_equal(bits(host(src)[G:G + n]), bits(c["y"].reshape(-1)))  # the input is left alone
    ofdm.frame_cfo_derotate(view(src), cp, ed, out=view(src))
    inplace = host(src)
    assert np.array_equal(bits(inplace[G:G + n]), bits(got[G:G + n]))
    assert np.all(inplace[:G] == guard) and np.all(inplace[G + n:] == guard)
    # any other overlap is refused
    if n > 16:
        with pytest.raises(ofdm.OfdmError, match="overlaps"):
            ofdm._check(ofdm.lib().ofdm_frame_cfo_derotate(ofdm._P(src.data_ptr()), ofdm._P(src.data_ptr() + 16), F, S,
                                                           R, C, cp, ofdm._dptr(ed), None), "ofdm_frame_cfo_derotate")


# ------------------------------------------------------------ 3. estimator

@pytest.mark.parametrize("F,S,R,C,cp,skip", [(3, 4, 5, 1024, 16, 0), (3, 4, 5, 1024, 7, 3), (3, 3, 3, 600, 9, 0),
                                             (2, 3, 8, 2048, 16, 0),
                                             (2, 101, 16, 1024, 72, 0)])  # the long sum: 116 352 terms per frame
def test_estimator(ofdm, dev, F, S, R, C, cp, skip):
    """gamma within 1e-5 relative of the float64 sum on the same f32 input, eps
    within 1e-5 / 2 pi of the float64 value (which follows from the gamma
    bound); not against the true eps, which the noise moves by ~1e-4."""
    import torch
    c = cc.frames(F, S, R, C, cp, None, seed=cp)
    y = np.array(c["y"])
    y[F - 1] = 0  # an all-zero frame: gamma = 0, eps = 0
    g64, e64 = cc.gamma_ref(y, cp, skip)
    yd = to_dev(y, dev)
    runs = []
    for _ in range(2):
        gamma = nan_out((F,), dev)
        eps = torch.full((F,), float("nan"), dtype=torch.float32, device=dev)
        ofdm.frame_cfo_estimate(yd, cp, skip, eps=eps, gamma=gamma)
        runs.append((host(gamma), host(eps)))
    (g, e), (g2, e2) = runs
    assert np.array_equal(bits(g), bits(g2)) and np.array_equal(e.view(np.uint32), e2.view(np.uint32))
    gerr = np.abs(g - g64) / np.maximum(np.abs(g64), 1e-300)
    eerr = np.abs(e.astype(np.float64) - e64)
    print(f"C={C} cp={cp} skip={skip}: gamma rel {gerr[:F - 1].max():.2e}, eps abs {eerr.max():.2e}; "
          f"eps {e.tolist()} true {c['eps'].tolist()}")
    assert g[F - 1] == 0 and e[F - 1] == 0
    assert np.all(gerr[:F - 1] <= 1e-5)
    assert np.all(eerr <= 1e-5 / (2 * np.pi))
    assert np.all((e > -0.5) & (e <= 0.5))
    # and the estimate is an estimate: within the noise of the offset put in (the shortest sum here, 80 terms
    # at sigma = 0.02 on faded antennas, has a standard deviation of about 1e-3)
    assert np.all(np.abs(e[:F - 1] - c["eps"][:F - 1]) < 5e-3)


# ---------------------------------------------------------- 4. closed loop

def test_closed_loop_c1024(ofdm, dev, oracle):
    F, S, R, C, cp = 3, 4, 5, 1024, 16
    c = cc.frames(F, S, R, C, cp, (0.03, -0.2, 0.45), seed=4)
    truth = oracle.frames_demod(c["clean"], c["X"], cp)
    y, X = to_dev(c["y"], dev), to_dev(c["X"], dev)
    wrong = cc.decision_errors(host(ofdm.frame_demod(y, X, cp)), truth)
    eps = ofdm.frame_cfo_estimate(y, cp)
    fixed = cc.decision_errors(host(ofdm.frame_demod_cfo(y, X, cp, eps)), truth)
    print(f"C={C}: {wrong} of {truth.size} decisions wrong uncorrected, {fixed} corrected; eps {host(eps).tolist()}")
    assert wrong > truth.size // 4
    assert fixed == 0


@pytest.mark.parametrize("F,S,R,C,cp", [(3, 5, 4, 256, 32), (3, 3, 8, 2048, 16)])
def test_closed_loop_derotate_route(ofdm, dev, oracle, F, S, R, C, cp):
    c = cc.frames(F, S, R, C, cp, (0.03, -0.2, 0.45), seed=4)
    truth = oracle.frames_demod(c["clean"], c["X"], cp)
    y, X = to_dev(c["y"], dev), to_dev(c["X"], dev)
    wrong = cc.decision_errors(host(ofdm.frame_demod(y, X, cp)), truth)
    eps = ofdm.frame_cfo_estimate(y, cp)
    ofdm.frame_cfo_derotate(y, cp, eps, out=y)
    fixed = cc.decision_errors(host(ofdm.frame_demod(y, X, cp)), truth)
    print(f"C={C}: {wrong} of {truth.size} decisions wrong uncorrected, {fixed} corrected; eps {host(eps).tolist()}")
    assert wrong > truth.size // 4
    assert fixed == 0
    with pytest.raises(ofdm.OfdmError, match="ofdm_frame_cfo_derotate"):
        ofdm.frame_demod_cfo(y, X, cp, eps)  # no derotating receiver at this C: the derotator is named


# ------------------------------------------------------------- 5. pipeline

CHUNK = 2


def direct(ofdm, dev, c, cp, denoise, sc16_scale=None):
    """What a CFO pipeline of CHUNK-frame chunks enqueues, called directly."""
    import torch
    F, S, R, Cp = c["y"].shape
    C = Cp - cp
    X = to_dev(c["X"], dev)
    out = nan_out((F, S - 1, C - 1), dev)
    for f0 in range(0, F, CHUNK):
        n = min(CHUNK, F - f0)
        if sc16_scale is None:
            y = to_dev(c["y"][f0:f0 + n], dev)
        else:
            y = ofdm.iq_convert_sc16(to_dev(c["q"][f0:f0 + n], dev), sc16_scale)
        ws = ofdm.workspace(n, S, R, C, dev)
        o = out[f0:f0 + n]
        eps = ofdm.frame_cfo_estimate(y, cp, 1)
        if C != 1024:
            ofdm.frame_cfo_derotate(y, cp, eps, out=y)
        if denoise and C == 1024:
            ofdm.frame_estimate_cfo(y, X, cp, ws, eps)
            ofdm.frame_estimate_denoise(ws, n, S, R, C, 12, 4)
            ofdm.frame_combine_cfo(y, cp, ws, o, eps)
        elif denoise:
            ofdm.frame_estimate(y, X, cp, ws)
            ofdm.frame_estimate_denoise(ws, n, S, R, C, 12, 4)
            ofdm.frame_combine(y, cp, ws, o)
        elif C == 1024:
            ofdm.frame_demod_cfo(y, X, cp, eps, ws=ws, out=o)
        else:
            ofdm.frame_demod(y, X, cp, ws=ws, out=o)
    return host(out)


def piped(ofdm, c, cp, configure, **kw):
    F, S, R, Cp = c["y"].shape
    C = Cp - cp
    out = np.full((F, S - 1, C - 1), np.nan, np.complex64)
    with ofdm.Pipeline(S, R, C, c["X"], cp, chunk_frames=CHUNK, depth=2, **kw) as pl:
        configure(pl)
        pl.demod(np.array(c["q"] if kw else c["y"]), out)
        pl.sync()
    return out


@pytest.mark.parametrize("C", [1024, 256])
def test_pipeline_set_cfo(ofdm, dev, oracle, C):
    F, S, R, cp = 5, 4, 4, 16
    c = cc.frames(F, S, R, C, cp, None, seed=C + 1)
    truth = oracle.frames_demod(c["clean"], c["X"], cp)
    on = piped(ofdm, c, cp, lambda pl: pl.set_cfo(True, 1))
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, False)))
    assert cc.decision_errors(on, truth) == 0

    def both(pl):
        pl.set_cfo(True, 1)
        pl.set_denoise(12, 4)

    den = piped(ofdm, c, cp, both)
    assert np.array_equal(bits(den), bits(direct(ofdm, dev, c, cp, True)))
    assert not np.array_equal(bits(den), bits(on))

    def on_then_off(pl):
        pl.set_cfo(True, 1)
        pl.set_cfo(False)

    never = piped(ofdm, c, cp, lambda pl: None)
    assert np.array_equal(bits(piped(ofdm, c, cp, on_then_off)), bits(never))
    assert cc.decision_errors(never, truth) > truth.size // 5  # two of the five frames are lost
    with ofdm.Pipeline(S, R, C, c["X"], cp, chunk_frames=CHUNK, depth=2) as pl:
        for bad in (-1, cp):
            with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_cfo failed \(-1\)"):
                pl.set_cfo(True, bad)
        pl.set_cfo(True, cp - 1)
    with ofdm.Pipeline(S, R, C, c["X"], 0, chunk_frames=CHUNK, depth=2) as pl:
        with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_cfo failed \(-1\)"):
            pl.set_cfo(True, 0)
        pl.set_cfo(False)


def test_pipeline_set_cfo_sc16(ofdm, dev, oracle):
    """an sc16 pipeline at C = 256 estimates and derotates on its converted chunk; at C = 1024 it is refused"""
    F, S, R, C, cp = 5, 4, 4, 256, 16
    c = dict(cc.frames(F, S, R, C, cp, None, seed=C + 1))
    scale = float(np.float32(2.0 ** -12))
    v = np.stack([c["y"].real, c["y"].imag], -1).astype(np.float64)
    assert np.abs(v).max() < 7.9
    c["q"] = np.ascontiguousarray(np.rint(v / scale).astype(np.int16))
    truth = oracle.frames_demod(c["clean"], c["X"], cp)
    on = piped(ofdm, c, cp, lambda pl: pl.set_cfo(True, 1), sample_format="sc16", scale=scale)
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, False, sc16_scale=scale)))
    assert cc.decision_errors(on, truth) == 0
    with ofdm.Pipeline(S, R, 1024, np.ones(1023, np.complex64), cp, chunk_frames=CHUNK, depth=2, sample_format="sc16",
                       scale=scale) as pl:
        with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_cfo failed \(-3\)"):
            pl.set_cfo(True, 0)
        pl.set_cfo(False)
