"""Phase and timing tracking on the GPU (include/ofdm_lsmrc_timing.h):
ofdm_frame_timing_track against the float64 model (timing_cases.track, the
definition) on the same f32 z and the P the device exports, determinism and
buffer discipline, the robustness rules, the closed loop behind the plain
receiver on frames with a sampling clock offset, the pipeline's mode, and
containment.

The workspace of every parity case is filled by a real frame_estimate on small
cfo_cases frames; z comes from the generator.  Outputs: the project's RTOL
through helpers.parity (norm-wise and element-wise); phases: RTOL rad plus one
f32 spacing of the stored value; timing: RTOL / pi samples plus one f32
spacing (a timing error e is a phase error of at most pi e at the band edge,
hence the same bound).  The slicer is discontinuous: every parity case
asserts the model's margin to the nearest decision threshold."""
import numpy as np
import pytest

import cfo_cases as cc
import phase_cases as pc
import timing_cases as tc
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

SNR = {2: 15, 4: 25, 6: 30, 8: 38}  # per constellation, phase_cases' figures
STEP, JITTER = 0.03, 0.005


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


def nan_rows(F, S, dev):
    import torch
    return torch.full((F, S - 1), float("nan"), dtype=torch.float32, device=dev)


_ws = {}


def exported_p(ofdm, ws, F, S, R, C):
    Pw = np.stack([host(ofdm.frame_export_estimate(ws, F, S, R, C, f)[1]) for f in range(F)])
    Pw = pc.p_by_position(Pw)
    Pw.setflags(write=False)
    return Pw


def estimate(ofdm, dev, F, S, R, C, cp, zero_pilot=None, zero_lower=None, scale_log2=None):
    """(workspace filled by frame_estimate on cfo_cases frames without offset,
    P by output position (F, K) as the device exports it).  zero_pilot: that
    frame's pilot symbol is all zero (P = 0); zero_lower: that frame's P is
    set to 0 on every bin of the lower half (C/2 .. C-1) in the workspace;
    scale_log2: every P of the workspace is multiplied by 2^scale_log2."""
    import torch
    key = (F, S, R, C, cp, zero_pilot, zero_lower, scale_log2)
    if key not in _ws:
        c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
        y = np.array(c["y"])
        if zero_pilot is not None:
            y[zero_pilot, 0] = 0
        ws = ofdm.workspace(F, S, R, C, dev)
        ofdm.frame_estimate(to_dev(y, dev), to_dev(c["X"], dev), cp, ws)
        if zero_lower is not None or scale_log2 is not None:
            torch.cuda.synchronize()
            # The workspace's layout as capi.cpp's carve() lays it out (and test_containment_gpu's poke_bin0 and
            # test_denoise_gpu read it): Hc, cf32 [F][R][C], rounded up to 256 bytes, then P, f32 [F][C] by FFT
            # bin.  A change to carve() shows here: every caller asserts the exported P against what it poked.
            nh = (F * R * C * 8 + 255) // 256 * 256
            Pd = ws[nh:nh + F * C * 4].view(torch.float32).view(F, C)
            if zero_lower is not None:
                Pd[zero_lower, (C + 1) // 2:] = 0.0
            if scale_log2 is not None:
                Pd *= 2.0 ** scale_log2
        _ws[key] = (ws, exported_p(ofdm, ws, F, S, R, C))
    return _ws[key]


def check(ofdm, dev, ws, Pw, z, geom, bps, label):
    """One out-of-place run with phases and timing against the model;
    returns (out, phase, timing, model theta, model tau)."""
    F, S, R, C = geom
    ref, theta, tau, margin = tc.track(z, Pw, bps)
    assert margin >= pc.MARGIN_MIN, f"{label}: the model's margin {margin:.2e} a says nothing about parity"
    out, phase, timing = nan_out(z.shape, dev), nan_rows(F, S, dev), nan_rows(F, S, dev)
    ofdm.frame_timing_track(to_dev(z, dev), ws, F, S, R, C, bps, out=out, phase=phase, timing=timing)
    out, phase, timing = host(out), host(phase), host(timing)
    ok = np.isfinite(ref)  # a NaN put into z stays one, in both
    assert np.array_equal(np.isfinite(out), ok)
    perr = np.abs(phase.astype(np.float64) - theta)
    terr = np.abs(timing.astype(np.float64) - tau)
    d = out[ok].astype(np.complex128) - ref[ok]
    print(f"{label}: norm-rel {np.linalg.norm(d) / np.linalg.norm(ref[ok]):.2e}, phase {perr.max():.2e} rad of "
          f"{np.abs(theta).max():.2f}, timing {terr.max():.2e} of {np.abs(tau).max():.3f} samples, margin {margin:.3f} a")
    nrel, erel = parity(out[ok], ref[ok])
    assert np.all(perr <= RTOL + np.spacing(np.abs(phase)))
    assert np.all(terr <= RTOL / np.pi + np.spacing(np.abs(timing)))
    return out, phase, timing, theta, tau


# ------------------------------------------------------------- 1. parity

# (F, S, R, C, cp), bps, dstep, seed (the seeds: margin >= MARGIN_MIN, gone through on the CPU)
PARITY = [((3, 13, 4, 1024, 16), 2, 0.03, 0),   # K = 1023: four elements per thread, DC between the second and third
          ((3, 13, 4, 1024, 16), 4, 0.03, 0),
          ((3, 13, 4, 1024, 16), 6, 0.02, 5),
          ((3, 13, 4, 1024, 16), 8, 0.01, 5),
          ((3, 13, 4, 64, 4), 2, 0.03, 0),      # K = 63: one wave short of an element, DC inside it
          ((3, 13, 4, 64, 4), 8, 0.01, 1),
          ((2, 11, 2, 64, 4), 4, 0.03, 0),      # 10 rows: the row loop's three-row trips leave one
          ((3, 13, 4, 8, 2), 4, 0.03, 0),       # K = 7: less than a wave
          ((3, 13, 4, 9, 2), 4, 0.03, 0),       # K = 8, even: nu is not monotonic in k, the per-element form
          ((2, 3, 1, 2048, 16), 6, 0.02, 1),    # K = 2047: the 1024-thread form, DC inside a thread's second step
          ((2, 5, 2, 601, 8), 4, 0.03, 0),      # odd C, K = 600: the per-element form on three elements and four waves
          ((2, 5, 2, 601, 8), 8, 0.01, 5),
          ((2, 3, 1, 2049, 16), 4, 0.03, 0),    # odd C, K = 2048: the per-element form's 512-thread kernel, eight waves
          ((2, 3, 1, 2049, 16), 6, 0.02, 1)]


@pytest.mark.parametrize("geom,bps,dstep,seed", PARITY)
def test_parity(ofdm, dev, geom, bps, dstep, seed):
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    assert np.all(Pw > 0)
    c = tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], dstep, seed)
    out, phase, timing, theta, tau = check(ofdm, dev, ws, Pw, c["z"], (F, S, R, C), bps, f"C={C} bps={bps}")
    assert pc.symbol_errors(out, c["d"], bps) == 0
    assert np.abs(timing[0]).max() > 0.9 * dstep * (S - 1)  # the drift was followed, not ignored


# ------------------------------------------- 2. determinism and buffers

@pytest.mark.parametrize("geom,bps,dstep,seed", [((3, 13, 4, 1024, 16), 8, 0.01, 5), ((2, 3, 1, 2048, 16), 6, 0.02, 1),
                                                 ((3, 13, 4, 9, 2), 4, 0.03, 0), ((2, 5, 2, 601, 8), 8, 0.01, 5),
                                                 ((2, 3, 1, 2049, 16), 6, 0.02, 1)])
def test_determinism_and_buffers(ofdm, dev, geom, bps, dstep, seed):
    import torch
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    c = tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], dstep, seed)
    n, m, G = c["z"].size, F * (S - 1), 3  # G guard words: the buffers start 8-byte, not 16-byte, aligned
    guard = np.float32(12345.0) + 1j * np.float32(-54321.0)

    def padded(fill):
        buf = torch.full((n + 2 * G,), complex(guard), dtype=torch.complex64, device=dev)
        buf[G:G + n] = float("nan") if fill is None else to_dev(fill, dev).reshape(-1)
        return buf

    def padded_rows():
        buf = torch.full((m + 2 * G,), 777.0, dtype=torch.float32, device=dev)
        buf[G:G + m] = float("nan")
        return buf

    view = lambda b: b[G:G + n].view(F, S - 1, C - 1)
    pview = lambda b: b[G:G + m].view(F, S - 1)
    runs = []
    for _ in range(2):
        src, dst, ph, tm = padded(c["z"]), padded(None), padded_rows(), padded_rows()
        ofdm.frame_timing_track(view(src), ws, F, S, R, C, bps, out=view(dst), phase=pview(ph), timing=pview(tm))
        got, gph, gtm = host(dst), host(ph), host(tm)
        assert np.all(got[:G] == guard) and np.all(got[G + n:] == guard)
        for r in (gph, gtm):
            assert np.all(r[:G] == 777.0) and np.all(r[G + m:] == 777.0)
            assert np.all(np.isfinite(r)), "a row's value was not written"
        assert np.all(np.isfinite(got)), "an element was not written"
        gsrc = host(src)
        assert np.array_equal(bits(gsrc[G:G + n]), bits(c["z"].reshape(-1)))  # the input is left alone
        assert np.all(gsrc[:G] == guard) and np.all(gsrc[G + n:] == guard)   # ... and so is what lies around it
        runs.append((got, gph, gtm))
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))
    # in place, without the phases and the timing; then with only one of them
    src = padded(c["z"])
    ofdm.frame_timing_track(view(src), ws, F, S, R, C, bps, out=view(src))
    assert np.array_equal(bits(host(src)), bits(runs[0][0]))
    src, tm = padded(c["z"]), padded_rows()
    ofdm.frame_timing_track(view(src), ws, F, S, R, C, bps, out=view(src), timing=pview(tm))
    assert np.array_equal(bits(host(src)), bits(runs[0][0])) and np.array_equal(bits(host(tm)), bits(runs[0][2]))
    # any other overlap, and phases or timing inside a buffer or each other, are refused
    p, q = src.data_ptr() + 8 * G, tm.data_ptr() + 4 * G
    call = lambda out, phase, timing: ofdm._check(ofdm.lib().ofdm_frame_timing_track(
        ofdm._P(p), F, S, R, C, ofdm._dptr(ws), ws.numel(), bps, ofdm._P(out), ofdm._P(phase), ofdm._P(timing), None),
        "ofdm_frame_timing_track")
    with pytest.raises(ofdm.OfdmError, match="d_out overlaps"):
        call(p + 8, None, None)
    with pytest.raises(ofdm.OfdmError, match="d_phase overlaps"):
        call(p, p + 8 * n - 4, None)
    with pytest.raises(ofdm.OfdmError, match="d_timing overlaps d_z or d_out"):
        call(p, None, p + 8 * n - 4)
    with pytest.raises(ofdm.OfdmError, match="d_timing overlaps d_phase"):
        call(p, q, q + 4 * m - 4)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host(src)), bits(runs[0][0]))  # nothing ran


def test_workspace_registry(ofdm, dev):
    """Another geometry, an antenna-split partial estimate and a released workspace are refused."""
    import torch
    F, S, R, C, cp = 3, 13, 4, 64, 4
    ws, _ = estimate(ofdm, dev, F, S, R, C, cp)
    z = nan_out((F, S - 1, C - 1), dev)
    for bad in ((F - 1, S, R, C), (F, S - 1, R, C), (F, S, R + 1, C)):
        with pytest.raises(ofdm.OfdmError, match=r"ofdm_frame_timing_track failed \(-1\).*workspace estimate is for"):
            ofdm.frame_timing_track(nan_out((bad[0], bad[1] - 1, C - 1), dev), ws, *bad, 2)
    c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
    _, wp = ofdm.frame_ls_partial(to_dev(c["y"], dev), to_dev(c["X"], dev), cp)
    with pytest.raises(ofdm.OfdmError, match="partial"):
        ofdm.frame_timing_track(z, wp, F, S, R, C, 2)
    ofdm.workspace_release(wp)
    with pytest.raises(ofdm.OfdmError, match="holds no estimate"):
        ofdm.frame_timing_track(z, wp, F, S, R, C, 2)
    torch.cuda.synchronize()
    assert np.all(np.isnan(host(z)))  # nothing ran


# ---------------------------------------------------------- 3. robustness

def test_one_nan_does_not_poison_the_frame(ofdm, dev):
    geom, bps = (3, 13, 4, 1024, 16), 4
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp)
    z = np.array(tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], 0.03, 0)["z"])
    z[1, 3, 500] = np.nan
    out, phase, timing, theta, tau = check(ofdm, dev, ws, Pw, z, (F, S, R, C), bps, "NaN in row 3 of frame 1")
    assert theta[1, 3] == 2 * theta[1, 2] - theta[1, 1] and tau[1, 3] == 2 * tau[1, 2] - tau[1, 1]  # the model
    eps1 = np.spacing(np.float32(1.0))
    assert abs(float(phase[1, 3]) - (2.0 * float(phase[1, 2]) - float(phase[1, 1]))) <= 4 * eps1
    assert abs(float(timing[1, 3]) - (2.0 * float(timing[1, 2]) - float(timing[1, 1]))) <= 4 * eps1
    assert np.isnan(out[1, 3, 500]) and np.count_nonzero(np.isnan(out)) == 1


def test_frame_without_estimate_passes_through(ofdm, dev):
    geom, bps = (3, 13, 4, 64, 4), 2
    F, S, R, C, cp = geom
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp, zero_pilot=1)
    assert np.all(Pw[1] == 0) and np.all(Pw[0] > 0) and np.all(Pw[2] > 0)
    z = tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], 0.03, 0)["z"]
    out, phase, timing, theta, tau = check(ofdm, dev, ws, Pw, z, (F, S, R, C), bps, "frame 1 with P = 0")
    assert np.all(phase[1] == 0) and np.all(timing[1] == 0) and np.array_equal(bits(out[1]), bits(z[1]))
    for f in (0, 2):
        assert np.all(phase[f] != 0) and np.all(timing[f] != 0)


@pytest.mark.parametrize("C,cp", [(64, 4), (9, 2)])
def test_frame_without_lower_half_is_phase_tracked(ofdm, dev, C, cp):
    """P zeroed on the whole lower half: tau is exactly 0, the frame is tracked as the phase tracker tracks it."""
    F, S, R, bps = 3, 13, 4, 2
    ws, Pw = estimate(ofdm, dev, F, S, R, C, cp, zero_lower=1)
    nu = tc.signed_bins(C - 1)
    assert np.all(Pw[1][nu < 0] == 0) and np.all(Pw[1][nu > 0] > 0) and np.all(Pw[0] > 0) and np.all(Pw[2] > 0)
    # frame 1 carries no timing drift the tracker could not follow: a phase-only case there
    z = np.array(tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], 0.03, 0)["z"])
    z[1] = pc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps])["z"][1]
    out, phase, timing, theta, tau = check(ofdm, dev, ws, Pw, z, (F, S, R, C), bps, f"C={C}, frame 1 without a lower half")
    assert np.all(tau[1] == 0) and np.all(timing[1] == 0)
    ref, th_ref, _ = pc.track(z[1:2], Pw[1:2], bps)
    assert np.abs(theta[1] - th_ref[0]).max() <= 1e-12
    parity(out[1], ref[0])
    assert np.all(timing[0] != 0) and np.all(timing[2] != 0) and np.all(phase[1] != 0)


@pytest.mark.parametrize("log2", [70, -80, 114])
def test_estimate_scaled_by_a_power_of_two(ofdm, dev, log2):
    """P times 2^n scales every sum of the recursion exactly, so outputs, phases and timing keep their bits --
    also where the product of the two half sums, taken as it stands, would leave f32's range (2^158, 2^-142),
    and where their sum would: in this case the half sums reach 2^13.53 and g = g_L + g_U 2^14.32 (the float64
    model), so at 2^114 both halves are finite in every row (up to 2^127.53) and g_L + g_U as it stands is not."""
    geom, bps = (3, 13, 4, 64, 4), 4
    F, S, R, C, cp = geom
    ws0, Pw0 = estimate(ofdm, dev, F, S, R, C, cp)
    ws1, Pw1 = estimate(ofdm, dev, F, S, R, C, cp, scale_log2=log2)
    assert np.array_equal(Pw1, Pw0 * np.float32(2.0 ** log2)) and np.all(Pw1 > 0) and np.all(np.isfinite(Pw1))
    z = to_dev(tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], 0.03, 0)["z"], dev)
    got = []
    for ws in (ws0, ws1):
        phase, timing = nan_rows(F, S, dev), nan_rows(F, S, dev)
        out = ofdm.frame_timing_track(z, ws, F, S, R, C, bps, phase=phase, timing=timing)
        got.append((host(out), host(phase), host(timing)))
    assert np.all(got[0][2] != 0)
    for a, b in zip(*got):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------- 4. end to end, soft chain

E2E = ((3, 40, 4, 256, 16), (0.004, -0.006, 0.002), (40e-6, -60e-6, 25e-6))

_e2e = {}


def e2e(ofdm, dev, seed):
    if seed not in _e2e:
        (F, S, R, C, cp), eps, delta = E2E
        c = tc.frames(F, S, R, C, cp, eps, delta, seed=seed)
        ws = ofdm.workspace(F, S, R, C, dev)
        z = ofdm.frame_demod(to_dev(c["y"], dev), to_dev(c["X"], dev), cp, ws=ws)
        phase_only = ofdm.frame_phase_track(z, ws, F, S, R, C, 2)
        phase, timing = nan_rows(F, S, dev), nan_rows(F, S, dev)
        out = ofdm.frame_timing_track(z, ws, F, S, R, C, 2, phase=phase, timing=timing)
        truth = c["data"][..., pc.out_src(C - 1)]  # the transmitted QPSK by output position
        _e2e[seed] = (c, ws, z, phase_only, out, phase, timing, truth)
    return _e2e[seed]


@pytest.mark.parametrize("seed", [0, 7])
def test_end_to_end(ofdm, dev, seed):
    """Frames with a sampling clock offset behind the real receiver: the phase tracker alone leaves more
    than a tenth of the decisions wrong, this tracker none."""
    (F, S, R, C, cp), eps, delta = E2E
    c, ws, z, phase_only, out, phase, timing, truth = e2e(ofdm, dev, seed)
    raw, before, after = (cc.decision_errors(host(v), truth) for v in (z, phase_only, out))
    got_d = host(ofdm.sampling_offset(timing, C, cp))
    got_e = host(ofdm.residual_cfo(phase, C, cp))
    print(f"seed {seed}: {raw} of {truth.size} decisions wrong untracked, {before} phase-tracked, {after} with timing; "
          f"delta within {np.abs(got_d - c['delta']).max() * 1e6:.3f} ppm, eps within {np.abs(got_e - c['eps']).max():.2e}")
    assert before > truth.size / 10
    assert after == 0
    assert np.abs(got_d - c["delta"]).max() <= 1e-6
    assert np.abs(got_e - c["eps"]).max() <= 5e-5


@pytest.mark.parametrize("seed", [0, 7])
def test_soft_chain(ofdm, dev, seed):
    """combine -> track -> noise estimate: neither the rotation nor the slope books as noise any more."""
    (F, S, R, C, cp), eps, delta = E2E
    c, ws, z, phase_only, out, phase, timing, truth = e2e(ofdm, dev, seed)
    raw, mid, tracked = (host(ofdm.frame_noise_estimate(v, ws, F, S, R, C, 2)) for v in (z, phase_only, out))
    print(f"seed {seed}: noise estimate untracked {raw.tolist()}, phase-tracked {mid.tolist()}, with timing {tracked.tolist()}")
    assert np.all(tracked > 0) and np.all(tracked < mid) and np.all(mid < raw)


# ------------------------------------------------------------- 5. pipeline

CHUNK = 2


def direct(ofdm, dev, c, cp, cfo, track, sc16_scale=None):
    """What a pipeline of CHUNK-frame chunks enqueues, called directly; track: None, ("timing", mod) or ("phase", mod)."""
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
        if track:
            (ofdm.frame_timing_track if track[0] == "timing" else ofdm.frame_phase_track)(o, ws, n, S, R, C, track[1], out=o)
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
    c = tc.frames(F, S, R, C, cp, (0.03, -0.2, 0.45, 0.0, -0.004), (100e-6, -150e-6, 60e-6, 0.0, -40e-6), seed=3,
                  sigma=cc.SIGMA)
    truth = c["data"][..., pc.out_src(C - 1)]

    def on(pl):
        pl.set_cfo(True, 1)
        pl.set_timing_track(2)

    def both(pl):
        on(pl)
        pl.set_phase_track(2)

    def on_then_off(pl):
        on(pl)
        pl.set_timing_track(0)

    got = piped(ofdm, c, cp, on)
    assert np.array_equal(bits(got), bits(direct(ofdm, dev, c, cp, True, ("timing", 2))))
    assert cc.decision_errors(got, truth) == 0
    never = piped(ofdm, c, cp, lambda pl: pl.set_cfo(True, 1))
    assert np.array_equal(bits(piped(ofdm, c, cp, on_then_off)), bits(never))
    assert np.array_equal(bits(never), bits(direct(ofdm, dev, c, cp, True, None)))
    assert not np.array_equal(bits(got), bits(never))
    # with both trackers set the timing tracker runs alone; turned off again, the phase tracker is back
    assert np.array_equal(bits(piped(ofdm, c, cp, both)), bits(got))
    phase_only = direct(ofdm, dev, c, cp, True, ("phase", 2))
    assert not np.array_equal(bits(phase_only), bits(got))

    def both_then_off(pl):
        both(pl)
        pl.set_timing_track(0)

    assert np.array_equal(bits(piped(ofdm, c, cp, both_then_off)), bits(phase_only))
    with ofdm.Pipeline(S, R, C, c["X"], cp, chunk_frames=CHUNK, depth=2) as pl:
        for bad in (-1, 1, 3, 10):
            with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_timing_track failed \(-1\)"):
                pl.set_timing_track(bad)
        for mod in (2, 4, 6, 8, 0):
            pl.set_timing_track(mod)


def test_pipeline_sc16(ofdm, dev):
    """an sc16 pipeline at C = 256 (converted chunk, the fp32 receiver), small offsets left uncorrected"""
    F, S, R, C, cp = 5, 6, 4, 256, 16
    c = dict(tc.frames(F, S, R, C, cp, (0.004, -0.006, 0.002, 0.0, 0.001), (300e-6, -400e-6, 200e-6, 0.0, 100e-6),
                       seed=5, sigma=cc.SIGMA))
    scale = float(np.float32(2.0 ** -12))
    v = np.stack([c["y"].real, c["y"].imag], -1).astype(np.float64)
    assert np.abs(v).max() < 7.9
    c["q"] = np.ascontiguousarray(np.rint(v / scale).astype(np.int16))
    truth = c["data"][..., pc.out_src(C - 1)]
    kw = dict(sample_format="sc16", scale=scale)
    on = piped(ofdm, c, cp, lambda pl: pl.set_timing_track(2), **kw)
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, False, ("timing", 2), sc16_scale=scale)))
    assert cc.decision_errors(on, truth) == 0

    def on_then_off(pl):
        pl.set_timing_track(2)
        pl.set_timing_track(0)

    never = piped(ofdm, c, cp, lambda pl: None, **kw)
    assert np.array_equal(bits(piped(ofdm, c, cp, on_then_off, **kw)), bits(never))
    assert not np.array_equal(bits(on), bits(never))


# ---------------------------------------------------------- 6. containment

class TimingRow:
    """A row as test_containment_gpu's table holds them, kept out of that
    table: its rows are the main header's entries."""

    def __init__(self, F, S, R, C, cp, bps, dstep, seed):
        self.id = f"timing_{F}x{S}x{R}x{C}_bps{bps}"
        self.entries = ("ofdm_frame_timing_track",)
        self.prefix, self.aligned = False, True
        self.key = (F, S, R, C, cp, bps, dstep, seed)

    def setup(self, env):
        F, S, R, C, cp, bps, dstep, seed = self.key
        c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
        z = tc.case(F, S - 1, C - 1, bps, STEP, JITTER, SNR[bps], dstep, seed)["z"]
        return dict(iq=np.array(c["y"]), X=np.array(c["X"]), z=np.array(z))

    def run(self, cx, d):
        import test_containment_gpu as tg
        F, S, R, C, cp, bps, dstep, seed = self.key
        K, o = C - 1, cx.ofdm
        ws = cx.ws("ws", F, S, R, C)
        o.frame_estimate(cx.inp("iq", d["iq"], align=16), cx.inp("X", d["X"]), cp, ws)
        cx.freeze("ws")
        Pq = cx.out("Pexp", (F, K), "float32")
        for f in range(F):
            tg.call("ofdm_frame_export_estimate", tg.P(ws), ws.numel(), F, S, R, C, f,
                    tg.P(cx.out(f"H{f}", (R, K), "complex64")), tg.P(Pq[f]))
        z = cx.inp("z", d["z"])  # rows of K elements, K odd: 8-byte aligned
        o.frame_timing_track(z, ws, F, S, R, C, bps, out=cx.out("out", (F, S - 1, K), "complex64"),
                             phase=cx.out("phase", (F, S - 1), "float32"), timing=cx.out("timing", (F, S - 1), "float32"))

    def check(self, env, d, o):
        bps = self.key[5]
        ref, theta, tau, margin = tc.track(d["z"], pc.p_by_position(o["Pexp"]), bps)
        assert margin >= pc.MARGIN_MIN
        parity(o["out"], ref)
        assert np.all(np.abs(o["phase"].astype(np.float64) - theta) <= RTOL + np.spacing(np.abs(o["phase"])))
        assert np.all(np.abs(o["timing"].astype(np.float64) - tau) <= RTOL / np.pi + np.spacing(np.abs(o["timing"])))


ROWS = [TimingRow(3, 13, 4, 1024, 16, 8, 0.01, 5), TimingRow(2, 5, 2, 600, 9, 4, 0.03, 0)]  # K = 1023 and K = 599


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_containment(ofdm, oracle, dev, row):
    """test_containment_gpu.test_containment's sequence on d_z, d_ws, d_out, d_phase and d_timing, each in a
    guarded arena of its own, the workspace at exactly its stated size"""
    import test_containment_gpu as tg
    env = tg.Env(ofdm, dev, oracle)
    _, plain = tg._run(env, row, "plain")
    cx, guarded = tg._run(env, row, "guarded")
    assert {"z", "ws", "out", "phase", "timing"} <= set(cx.bufs)
    tg._contained(cx, row, "guarded")                                       # bands, every word written, inputs
    tg._same(row, "the plain and the guarded run", plain, guarded, cx.never)
    row.check(env, tg._data[row.id], plain)
    ax, at = tg._run(env, row, "aligned")                                   # each buffer at exactly its stated alignment
    tg._contained(ax, row, "aligned")
    row.check(env, tg._data[row.id], at)
    ofdm.device_status()
    tg._data.pop(row.id, None)


def test_rows_cover_the_new_header(ofdm):
    import test_containment_gpu as tg
    header = set(ofdm.header_symbols(ofdm.TIMING_HEADER_PATH))
    covered = {e for r in ROWS for e in r.entries}
    excluded = {s for s in header for n in tg.EXCLUDED if s == n or (n.endswith("*") and s.startswith(n[:-1]))}
    assert covered <= header and not covered & excluded
    assert not header - covered - excluded, sorted(header - covered - excluded)
    assert not any(r.id in {t.id for t in tg.TABLE} for r in ROWS)
