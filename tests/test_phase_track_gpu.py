"""Phase tracking on the GPU (include/ofdm_lsmrc.h, "phase tracking"):
ofdm_frame_phase_track against the float64 model (phase_cases.track, the
definition) on the same f32 z and the P the device exports, determinism and
buffer discipline, the two robustness rules, the closed loop behind the plain
receiver, the soft chain, and the pipeline's tracking mode.

The workspace of every case is filled by a real frame_estimate on small
cfo_cases frames; z comes from the generator.  Outputs: the project's RTOL
through helpers.parity (norm-wise and element-wise); phases: 1e-5 rad plus one
f32 spacing of the stored value (a phase error delta is a relative output
error delta, hence the same bound).  The slicer is discontinuous: every parity
case asserts the model's margin to the nearest decision threshold."""
import numpy as np
import pytest

import cfo_cases as cc
import phase_cases as pc
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


def nan_phase(F, S, dev):
    import torch
    return torch.full((F, S - 1), float("nan"), dtype=torch.float32, device=dev)


_ws = {}


def estimate(ofdm, dev, F, S, R, C, cp, zero_pilot=None):
    """(workspace filled by frame_estimate on cfo_cases frames without offset,
    P by output position (F, K) as the device exports it)"""
    import torch
    key = (F, S, R, C, cp, zero_pilot)
    if key not in _ws:
        c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
        y = np.array(c["y"])
        if zero_pilot is not None:
            y[zero_pilot, 0] = 0
        ws = ofdm.workspace(F, S, R, C, dev)
        ofdm.frame_estimate(to_dev(y, dev), to_dev(c["X"], dev), cp, ws)
        Pw = np.stack([host(ofdm.frame_export_estimate(ws, F, S, R, C, f)[1]) for f in range(F)])
        Pw = pc.p_by_position(Pw)
        Pw.setflags(write=False)
        _ws[key] = (ws, Pw)
    return _ws[key]


def check(ofdm, dev, ws, Pw, z, geom, bps, label):
    """One out-of-place run with phases against the model; returns (out, phase, model theta)."""
    F, S, R, C = geom
    ref, theta, margin = pc.track(z, Pw, bps)
    assert margin >= pc.MARGIN_MIN, f"{label}: the model's margin {margin:.2e} a says nothing about parity"
    out, phase = nan_out(z.shape, dev), nan_phase(F, S, dev)
    ofdm.frame_phase_track(to_dev(z, dev), ws, F, S, R, C, bps, out=out, phase=phase)
    out, phase = host(out), host(phase)
    ok = np.isfinite(ref)  # a NaN put into z stays one, in both
    assert np.array_equal(np.isfinite(out), ok)
    nrel, erel = parity(out[ok], ref[ok])
    perr = np.abs(phase.astype(np.float64) - theta)
    print(f"{label}: norm-rel {nrel:.2e} elem-rel {erel:.2e}, phase {perr.max():.2e} rad of {np.abs(theta).max():.2f}, "
          f"margin {margin:.3f} a")
    assert np.all(perr <= RTOL + np.spacing(np.abs(phase)))
    return out, phase, theta


# ------------------------------------------------------------- 1. parity

# (F, S, R, C, cp), bps, step, jitter, snr
PARITY = [((3, 13, 4, 1024, 16), 2, 0.03, 0.005, 15),   # K = 1023: the lane-order workspace, four elements per thread
          ((3, 13, 4, 1024, 16), 4, 0.03, 0.005, 25),
          ((3, 13, 4, 1024, 16), 6, 0.03, 0.005, 30),
          ((3, 13, 4, 1024, 16), 8, 0.03, 0.005, 38),
          ((3, 13, 4, 64, 4), 2, 0.03, 0.005, 15),      # K = 63: one wave short of an element
          ((3, 13, 4, 64, 4), 8, 0.03, 0.005, 38),
          ((2, 11, 2, 64, 4), 4, 0.03, 0.005, 25),      # 10 rows: the row loop's three-row trips leave one
          ((3, 13, 4, 8, 2), 4, 0.03, 0.005, 25),       # K = 7: less than a wave
          ((3, 13, 4, 9, 2), 4, 0.03, 0.005, 25),       # K = 8, even: out_src's three segments
          ((2, 3, 1, 2048, 16), 6, 0.03, 0.005, 30),    # K = 2047: the 1024-thread kernel, two elements per thread
          ((3, 13, 4, 256, 16), 2, 0.3, 0.005, 15)]     # theta past pi (4.7 rad): the phase output is unwrapped


@pytest.mark.parametrize("geom,bps,step,jitter,snr", PARITY)
def test_parity(ofdm, dev, geom, bps, step, jitter, snr):
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    assert np.all(Pw > 0)
    c = pc.case(F, S - 1, C - 1, bps, step, jitter, snr)
    out, phase, theta = check(ofdm, dev, ws, Pw, c["z"], (F, S, R, C), bps, f"C={C} bps={bps} step={step}")
    assert pc.symbol_errors(out, c["d"], bps) == 0
    if step > 0.1:
        assert np.abs(phase).max() > np.pi


# ------------------------------------------- 2. determinism and buffers

@pytest.mark.parametrize("geom,bps,snr", [((3, 13, 4, 1024, 16), 8, 38), ((2, 3, 1, 2048, 16), 6, 30),
                                          ((3, 13, 4, 9, 2), 4, 25)])
def test_determinism_and_buffers(ofdm, dev, geom, bps, snr):
    import torch
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    c = pc.case(F, S - 1, C - 1, bps, 0.03, 0.005, snr)
    n, m, G = c["z"].size, F * (S - 1), 3  # G guard words: the buffers start 8-byte, not 16-byte, aligned
    guard = np.float32(12345.0) + 1j * np.float32(-54321.0)

    def padded(fill):
        buf = torch.full((n + 2 * G,), complex(guard), dtype=torch.complex64, device=dev)
        buf[G:G + n] = float("nan") if fill is None else to_dev(fill, dev).reshape(-1)
        return buf

    def padded_phase():
        buf = torch.full((m + 2 * G,), 777.0, dtype=torch.float32, device=dev)
        buf[G:G + m] = float("nan")
        return buf

    view = lambda b: b[G:G + n].view(F, S - 1, C - 1)
    pview = lambda b: b[G:G + m].view(F, S - 1)
    runs = []
    for _ in range(2):
        src, dst, ph = padded(c["z"]), padded(None), padded_phase()
        ofdm.frame_phase_track(view(src), ws, F, S, R, C, bps, out=view(dst), phase=pview(ph))
        got, gph = host(dst), host(ph)
        assert np.all(got[:G] == guard) and np.all(got[G + n:] == guard)
        assert np.all(gph[:G] == 777.0) and np.all(gph[G + m:] == 777.0)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(gph)), "an element was not written"
        assert np.array_equal(bits(host(src)[G:G + n]), bits(c["z"].reshape(-1)))  # the input is left alone
        runs.append((got, gph))
    assert np.array_equal(bits(runs[0][0]), bits(runs[1][0])) and np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    # in place, and without the phases
    src = padded(c["z"])
    ofdm.frame_phase_track(view(src), ws, F, S, R, C, bps, out=view(src))
    inplace = host(src)
    assert np.array_equal(bits(inplace), bits(runs[0][0]))
    # any other overlap, and phases inside a buffer, are refused
    p = src.data_ptr() + 8 * G
    call = lambda out, phase: ofdm._check(ofdm.lib().ofdm_frame_phase_track(
        ofdm._P(p), F, S, R, C, ofdm._dptr(ws), ws.numel(), bps, ofdm._P(out), ofdm._P(phase), None),
        "ofdm_frame_phase_track")
    with pytest.raises(ofdm.OfdmError, match="overlaps"):
        call(p + 8, None)
    with pytest.raises(ofdm.OfdmError, match="d_phase overlaps"):
        call(p, p + 8 * n - 4)


def test_workspace_registry(ofdm, dev):
    """Another geometry, an antenna-split partial estimate and a released workspace are refused."""
    import torch
    F, S, R, C, cp = 3, 13, 4, 64, 4
    ws, _ = estimate(ofdm, dev, F, S, R, C, cp)
    z = nan_out((F, S - 1, C - 1), dev)
    for bad in ((F - 1, S, R, C), (F, S - 1, R, C), (F, S, R + 1, C)):
        with pytest.raises(ofdm.OfdmError, match=r"ofdm_frame_phase_track failed \(-1\).*workspace estimate is for"):
            ofdm.frame_phase_track(nan_out((bad[0], bad[1] - 1, C - 1), dev), ws, *bad, 2)
    c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
    _, wp = ofdm.frame_ls_partial(to_dev(c["y"], dev), to_dev(c["X"], dev), cp)
    with pytest.raises(ofdm.OfdmError, match="partial"):
        ofdm.frame_phase_track(z, wp, F, S, R, C, 2)
    ofdm.workspace_release(wp)
    with pytest.raises(ofdm.OfdmError, match="holds no estimate"):
        ofdm.frame_phase_track(z, wp, F, S, R, C, 2)
    torch.cuda.synchronize()
    assert np.all(np.isnan(host(z)))  # nothing ran


# ---------------------------------------------------------- 3. robustness

def test_one_nan_does_not_poison_the_frame(ofdm, dev):
    geom, bps = (3, 13, 4, 1024, 16), 4
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    z = np.array(pc.case(F, S - 1, C - 1, bps, 0.03, 0.005, 25)["z"])
    z[1, 3, 500] = np.nan
    out, phase, theta = check(ofdm, dev, ws, Pw, z, (F, S, R, C), bps, "NaN in row 3 of frame 1")
    assert theta[1, 3] == theta[1, 2] + (theta[1, 2] - theta[1, 1])  # the model: theta_3 = phi_3
    assert abs(float(phase[1, 3]) - (2.0 * float(phase[1, 2]) - float(phase[1, 1]))) <= 4 * np.spacing(np.float32(1.0))
    assert np.isnan(out[1, 3, 500]) and np.count_nonzero(np.isnan(out)) == 1


def test_frame_without_estimate_passes_through(ofdm, dev):
    geom, bps = (3, 13, 4, 64, 4), 2
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp, zero_pilot=1)
    assert np.all(Pw[1] == 0) and np.all(Pw[0] > 0) and np.all(Pw[2] > 0)
    z = pc.case(F, S - 1, C - 1, bps, 0.03, 0.005, 15)["z"]
    out, phase, theta = check(ofdm, dev, ws, Pw, z, (F, S, R, C), bps, "frame 1 with P = 0")
    assert np.all(phase[1] == 0) and np.array_equal(out[1], z[1])
    assert np.all(phase[0] != 0) and np.all(phase[2] != 0)


# ---------------------------------------------- 4. end to end, soft chain

E2E = ((3, 40, 4, 256, 16), (0.004, -0.006, 0.002))

_e2e = {}


def e2e(ofdm, dev, seed):
    if seed not in _e2e:
        import torch
        (F, S, R, C, cp), eps = E2E
        c = cc.frames(F, S, R, C, cp, eps, seed=seed)
        ws = ofdm.workspace(F, S, R, C, dev)
        z = ofdm.frame_demod(to_dev(c["y"], dev), to_dev(c["X"], dev), cp, ws=ws)
        phase = nan_phase(F, S, dev)
        out = ofdm.frame_phase_track(z, ws, F, S, R, C, 2, phase=phase)
        truth = c["data"][..., pc.out_src(C - 1)]  # the transmitted QPSK by output position
        _e2e[seed] = (c, ws, z, out, phase, truth)
    return _e2e[seed]


# seed 7 is the one the model figures of test_phase_track_cpu.py are for (7 638 wrong, eps within 8.1e-6)
@pytest.mark.parametrize("seed", [0, 7])
def test_end_to_end(ofdm, dev, seed):
    (F, S, R, C, cp), eps = E2E
    c, ws, z, out, phase, truth = e2e(ofdm, dev, seed)
    wrong, fixed = cc.decision_errors(host(z), truth), cc.decision_errors(host(out), truth)
    got = host(ofdm.residual_cfo(phase, C, cp))
    print(f"seed {seed}: {wrong} of {truth.size} decisions wrong untracked, {fixed} tracked; "
          f"residual eps error {np.abs(got - c['eps']).max():.2e}")
    assert wrong > 5000
    assert fixed == 0
    assert np.abs(got - c["eps"]).max() <= 5e-5


@pytest.mark.parametrize("seed", [0, 7])
def test_soft_chain(ofdm, dev, seed):
    """combine -> track -> noise estimate: the rotation no longer books as noise."""
    (F, S, R, C, cp), eps = E2E
    c, ws, z, out, phase, truth = e2e(ofdm, dev, seed)
    raw = host(ofdm.frame_noise_estimate(z, ws, F, S, R, C, 2))
    tracked = host(ofdm.frame_noise_estimate(out, ws, F, S, R, C, 2))
    print(f"seed {seed}: noise estimate untracked {raw.tolist()}, tracked {tracked.tolist()}")
    assert np.all(tracked > 0) and np.all(tracked < raw)


# ------------------------------------------------------------- 5. pipeline

CHUNK = 2


def direct(ofdm, dev, c, cp, cfo, mod, sc16_scale=None):
    """What a tracking pipeline of CHUNK-frame chunks enqueues, called directly."""
    F, S, R, Cp = c["y"].shape
    C = Cp - cp
    X = to_dev(c["X"], dev)
    out = nan_out((F, S - 1, C - 1), dev)
    for f0 in range(0, F, CHUNK):
        n = min(CHUNK, F - f0)
        ws = ofdm.workspace(n, S, R, C, dev)
        o = out[f0:f0 + n]
        if sc16_scale is None:
            y = to_dev(c["y"][f0:f0 + n], dev)
        else:
            y = ofdm.iq_convert_sc16(to_dev(c["q"][f0:f0 + n], dev), sc16_scale)
        if cfo:
            eps = ofdm.frame_cfo_estimate(y, cp, 1)
            ofdm.frame_demod_cfo(y, X, cp, eps, ws=ws, out=o)
        else:
            ofdm.frame_demod(y, X, cp, ws=ws, out=o)
        if mod:
            ofdm.frame_phase_track(o, ws, n, S, R, C, mod, out=o)
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


def test_pipeline_fp32_with_cfo(ofdm, dev):
    F, S, R, C, cp = 5, 6, 4, 1024, 16
    c = cc.frames(F, S, R, C, cp, (0.03, -0.2, 0.45, 0.0, -0.004), seed=3)
    truth = c["data"][..., pc.out_src(C - 1)]

    def both(pl):
        pl.set_cfo(True, 1)
        pl.set_phase_track(2)

    def on_then_off(pl):
        both(pl)
        pl.set_phase_track(0)

    on = piped(ofdm, c, cp, both)
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, True, 2)))
    assert cc.decision_errors(on, truth) == 0
    never = piped(ofdm, c, cp, lambda pl: pl.set_cfo(True, 1))
    assert np.array_equal(bits(piped(ofdm, c, cp, on_then_off)), bits(never))
    assert np.array_equal(bits(never), bits(direct(ofdm, dev, c, cp, True, 0)))
    assert not np.array_equal(bits(on), bits(never))
    with ofdm.Pipeline(S, R, C, c["X"], cp, chunk_frames=CHUNK, depth=2) as pl:
        for bad in (-1, 1, 3, 10):
            with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_phase_track failed \(-1\)"):
                pl.set_phase_track(bad)
        for mod in (2, 4, 6, 8, 0):
            pl.set_phase_track(mod)


def test_pipeline_sc16(ofdm, dev):
    """an sc16 pipeline at C = 256 (converted chunk, the fp32 receiver), small offsets left uncorrected"""
    F, S, R, C, cp = 5, 6, 4, 256, 16
    c = dict(cc.frames(F, S, R, C, cp, (0.004, -0.006, 0.002, 0.0, 0.001), seed=5))
    scale = float(np.float32(2.0 ** -12))
    v = np.stack([c["y"].real, c["y"].imag], -1).astype(np.float64)
    assert np.abs(v).max() < 7.9
    c["q"] = np.ascontiguousarray(np.rint(v / scale).astype(np.int16))
    truth = c["data"][..., pc.out_src(C - 1)]
    kw = dict(sample_format="sc16", scale=scale)
    on = piped(ofdm, c, cp, lambda pl: pl.set_phase_track(2), **kw)
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, False, 2, sc16_scale=scale)))
    assert cc.decision_errors(on, truth) == 0

    def on_then_off(pl):
        pl.set_phase_track(2)
        pl.set_phase_track(0)

    never = piped(ofdm, c, cp, lambda pl: None, **kw)
    assert np.array_equal(bits(piped(ofdm, c, cp, on_then_off, **kw)), bits(never))
    assert not np.array_equal(bits(on), bits(never))
