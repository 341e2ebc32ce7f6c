"""Phase and timing tracking (include/ofdm_lsmrc_timing.h) without a device:
the new header declares exactly the two entries and the main header and its
table gain nothing, every refusal answers before any HIP call (fake device
pointers) and names its argument, the library carries k_timing_track for the
four constellations without a private segment, and the float64 model the GPU
tests lean on (timing_cases.track, the definition) equals today's tracker
where slope tracking is off and gives the figures of DESIGN.md 7o's table where
it is on."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import cfo_cases as cc
import phase_cases as pc
import timing_cases as tc
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_frame_timing_track", "ofdm_pipeline_set_timing_track"]
P = ctypes.c_void_p
ARG, UNSUPPORTED = -1, -3


def test_header_and_binding_declare_the_entries(ofdm):
    assert os.path.exists(ofdm.TIMING_HEADER_PATH)
    names = ofdm.header_symbols(ofdm.TIMING_HEADER_PATH)
    assert sorted(names) == sorted(ENTRIES)
    assert set(ofdm._SIGS_TIMING) == set(names), set(ofdm._SIGS_TIMING) ^ set(names)
    # the main header and its table gain nothing
    assert not set(names) & set(ofdm.header_symbols()) and not set(names) & set(ofdm._SIGS)
    assert not set(names) & set(ofdm._SIGS_ACQUIRE)
    L = ofdm.lib()
    for e in ENTRIES:
        assert hasattr(L, e), f"{e} not exported"
        assert getattr(L, e).argtypes == ofdm._SIGS_TIMING[e][1]
        assert e in dict(ofdm._all_sigs())
    assert L.ofdm_version() == 2  # no version step
    assert '#include "ofdm_lsmrc.h"' in open(ofdm.TIMING_HEADER_PATH).read()
    assert callable(ofdm.frame_timing_track) and callable(ofdm.sampling_offset)
    assert callable(ofdm.Pipeline.set_timing_track)
    assert "TIMING_HEADER_PATH" in inspect.getsource(ofdm.build_id)  # the build identity covers the new header


def _track(L, z=4096, F=2, S=5, R=8, C=1024, ws=1 << 20, need=None, mod=2, out=1 << 24, phase=1 << 28,
           timing=1 << 29):
    if need is None:
        need = L.ofdm_frame_workspace_bytes(max(F, 1), max(S, 2), max(R, 1), min(max(C, 2), 8192))
    rc = L.ofdm_frame_timing_track(P(z), F, S, R, C, P(ws), need, mod, P(out), P(phase), P(timing), None)
    return rc, L.ofdm_last_error()


def test_refusals_without_device(ofdm):
    L = ofdm.lib()
    fn = b"ofdm_frame_timing_track"
    for mod in (0, 1, 3, 5, 7, 10, -2):
        rc, e = _track(L, mod=mod)
        assert rc == ARG and fn in e and b"modulation" in e, mod
    for bad, word in ((dict(F=-1), b"nframes"), (dict(S=1), b"S=1"), (dict(R=0), b"R=0"), (dict(z=0), b"d_z"),
                      (dict(out=0), b"d_out"), (dict(ws=0), b"d_ws"), (dict(z=4100), b"d_z"),
                      (dict(out=(1 << 24) + 4), b"d_out"), (dict(phase=(1 << 28) + 2), b"d_phase"),
                      (dict(timing=(1 << 29) + 2), b"d_timing")):
        rc, e = _track(L, **bad)
        assert rc == ARG and fn in e and word in e, (bad, e)
    for C in (1, 8193):
        rc, e = _track(L, C=C)
        assert rc == UNSUPPORTED and fn in e and b"C=" in e
    # overlap: in place is allowed (and would go on to the registry), disjoint too; anything else is refused
    nbytes, pbytes = 2 * 4 * 1023 * 8, 2 * 4 * 4
    for out in (4096 + 8, 4096 + nbytes - 8, 4096 - 8):
        rc, e = _track(L, out=out)
        assert rc == ARG and b"overlaps" in e and b"d_out" in e, out
    for phase in (4096, 4096 + nbytes - 4, (1 << 24) + 8, (1 << 24) - 4):
        rc, e = _track(L, phase=phase)
        assert rc == ARG and b"overlaps" in e and b"d_phase" in e, phase
    for timing in (4096, 4096 + nbytes - 4, (1 << 24) + 8, (1 << 24) - 4):
        rc, e = _track(L, timing=timing)
        assert rc == ARG and b"overlaps" in e and b"d_timing" in e and b"d_out" in e, timing
    for timing in (1 << 28, (1 << 28) + pbytes - 4, (1 << 28) - pbytes + 4):
        rc, e = _track(L, timing=timing)
        assert rc == ARG and b"d_timing overlaps d_phase" in e, timing
    # the registry: a workspace no estimate filled; touching phase and timing arrays are no overlap
    assert L.ofdm_workspace_release(P(1 << 20)) == 0
    for kw in (dict(), dict(out=4096), dict(phase=0), dict(timing=0), dict(phase=0, timing=0), dict(out=4096 + nbytes),
               dict(z=4104, out=4104), dict(timing=(1 << 28) + pbytes), dict(timing=(1 << 28) - pbytes)):
        rc, e = _track(L, **kw)
        assert rc == ARG and fn in e and b"holds no estimate" in e, (kw, e)
    for mod in (2, 0, 3):
        assert L.ofdm_pipeline_set_timing_track(None, mod) == ARG
        assert b"ofdm_pipeline_set_timing_track" in L.ofdm_last_error()


def test_zero_frames_is_a_noop(ofdm):
    L = ofdm.lib()
    for mod in (2, 4, 6, 8):
        assert _track(L, F=0, mod=mod)[0] == 0
    assert L.ofdm_frame_timing_track(None, 0, 5, 8, 1024, None, 0, 4, None, None, None, None) == 0
    # ... but still not with a bad modulation or geometry
    assert L.ofdm_frame_timing_track(None, 0, 5, 8, 1024, None, 0, 3, None, None, None, None) == ARG
    assert L.ofdm_frame_timing_track(None, 0, 1, 8, 1024, None, 0, 2, None, None, None, None) == ARG
    assert L.ofdm_frame_timing_track(None, 0, 5, 8, 8193, None, 0, 2, None, None, None, None) == UNSUPPORTED


def test_does_not_consume_device_status(ofdm):
    """The workspace is only read, no work tickets: a raised sticky status is left for the ticketed entries."""
    L = ofdm.lib()
    assert L.ofdm_device_status() == 0
    assert L.ofdm_device_status_inject(1) == 0
    assert _track(L)[0] == ARG  # its own validation, not OFDM_E_DEVICE
    assert L.ofdm_device_status() == -5
    assert L.ofdm_device_status() == 0


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_timing_track_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    assert not any("k_phase_track" in n for n in seg if "k_timing_track" in n)  # the two are told apart by name
    for bps in (2, 4, 6, 8):
        found = {n: v for n, v in seg.items() if f"k_timing_trackILi{bps}E" in n}
        assert len(found) >= 2, f"k_timing_track<{bps}>: {sorted(found)}"
        assert all(v == 0 for v in found.values()), f"k_timing_track<{bps}>: private segment {found}"


def test_sampling_offset_helper(ofdm):
    """tau = delta (C + cp) n' gives delta back, from numpy and from torch alike; the formula as stated."""
    import torch
    C, cp, delta = 1024, 72, np.array([10e-6, -8e-6])
    n = np.arange(1, 101, dtype=np.float64)
    tau = delta[:, None] * (C + cp) * n[None, :]
    assert np.allclose(ofdm.sampling_offset(tau.astype(np.float32), C, cp), delta, rtol=1e-6, atol=0)
    got = ofdm.sampling_offset(torch.from_numpy(tau.astype(np.float32)), C, cp)
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), delta, rtol=1e-6, atol=0)
    assert np.allclose(tc.sampling_offset(tau, C, cp), delta, rtol=1e-12, atol=0)
    rng = np.random.default_rng(1)
    t = rng.standard_normal((3, 12))
    want = np.array([sum((i + 1) * t[f, i] for i in range(12)) / sum((i + 1) ** 2 for i in range(12)) / (64 + 4)
                     for f in range(3)])
    assert np.allclose(ofdm.sampling_offset(t, 64, 4), want, rtol=1e-13, atol=0)
    assert np.allclose(tc.sampling_offset(t, 64, 4), want, rtol=1e-13, atol=0)


# ------------------------------------------------------------ the model

def test_signed_bins():
    assert tc.signed_bins(7).tolist() == [-4, -3, -2, -1, 1, 2, 3]             # C = 8: Nyquist is -C/2
    assert tc.signed_bins(8).tolist() == [4, -4, -3, -2, 1, 2, 3, -1]           # C = 9, K even: not monotonic
    assert tc.signed_bins(1).tolist() == [-1]                                   # C = 2
    nu = tc.signed_bins(1023)
    assert np.array_equal(nu, np.arange(1023) - 512 + (np.arange(1023) >= 512))


@pytest.mark.parametrize("K,bps,snr_db,zero", [(63, 4, 25, "lower"), (63, 2, 15, "upper"), (8, 4, 25, "lower"),
                                               (1, 2, 15, None), (63, 8, 38, "all")])
def test_model_equals_phase_tracker_with_slope_off(K, bps, snr_db, zero):
    """P zero on one half (or C = 2, or no P at all): tau is exactly 0 and the model is phase_cases.track."""
    F, N = 3, 12
    c = pc.case(F, N, K, bps, 0.03, 0.005, snr_db)
    nu = tc.signed_bins(K)
    Pw = 0.5 + np.random.default_rng(K).random((F, K))
    if zero is not None:
        Pw[:, {"lower": nu < 0, "upper": nu > 0, "all": nu != 0}[zero]] = 0.0
    out, theta, tau, margin = tc.track(c["z"], Pw, bps)
    ref, th_ref, m_ref = pc.track(c["z"], Pw, bps)
    assert np.all(tau == 0)
    assert np.abs(theta - th_ref).max() <= 1e-12 and np.abs(out - ref).max() <= 1e-12
    assert margin == m_ref or abs(margin - m_ref) <= 1e-12
    if zero != "all":
        assert pc.symbol_errors(out, c["d"], bps) == 0


# DESIGN.md 7o's table: time-domain frames with a sampling clock offset, received without any correction
MODEL = [((3, 40, 4, 256, 16), (0.004, -0.006, 0.002), (40e-6, -60e-6, 25e-6)),
         ((2, 101, 2, 1024, 72), (0.002, -0.003), (10e-6, -8e-6))]


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("shape,eps,delta", MODEL)
def test_model_on_drifting_frames(shape, eps, delta, seed):
    F, S, R, C, cp = shape
    c = tc.frames(F, S, R, C, cp, eps, delta, seed=seed)
    z, Pw = tc.receive(c, cp)
    truth = c["data"][..., pc.out_src(C - 1)]
    total = truth.size
    assert total == F * (S - 1) * (C - 1)
    raw = cc.decision_errors(z, truth)
    phase_only = cc.decision_errors(pc.track(z, Pw, 2)[0], truth)
    out, theta, tau, margin = tc.track(z, Pw, 2)
    wrong = cc.decision_errors(out, truth)
    d = tc.sampling_offset(tau, C, cp)
    e = pc.residual_cfo(theta, C, cp)
    derr, eerr = np.abs(d - c["delta"]).max(), np.abs(e - c["eps"]).max()
    print(f"{shape} seed {seed}: {raw} of {total} wrong untracked, {phase_only} phase-tracked, {wrong} with timing; "
          f"margin {margin:.3f} a, delta within {derr * 1e6:.3f} ppm, eps within {eerr:.2e}")
    assert raw > total / 10 and phase_only > total / 10
    assert wrong == 0
    assert margin >= pc.MARGIN_MIN
    assert derr <= 1e-6   # 1 ppm: set for C = 256, where the model was measured at 0.37; C = 1024 is far inside it
    assert eerr <= 5e-5   # the slope of the common phase still gives eps back


# one case per modulation on synthetic z, the seeds the GPU parity cases use
@pytest.mark.parametrize("K,bps,snr_db,dstep,seed", [(1023, 2, 15, 0.03, 0), (1023, 4, 25, 0.03, 0),
                                                     (1023, 6, 30, 0.02, 5), (1023, 8, 38, 0.01, 5),
                                                     (8, 4, 25, 0.03, 0)])
def test_model_per_modulation(K, bps, snr_db, dstep, seed):
    F, N = 3, 12
    c = tc.case(F, N, K, bps, 0.03, 0.005, snr_db, dstep, seed)
    Pw = np.ones((F, K))
    phase_only = pc.symbol_errors(pc.track(c["z"], Pw, bps)[0], c["d"], bps)
    out, theta, tau, margin = tc.track(c["z"], Pw, bps)
    after = pc.symbol_errors(out, c["d"], bps)
    print(f"K {K} bps {bps}: {phase_only} of {c['d'].size} wrong phase-tracked, {after} with timing, "
          f"margin {margin:.3f} a, tau error {np.abs(tau - c['tau_true']).max():.2e} samples")
    assert phase_only > c["d"].size / 20 and after == 0
    assert margin >= pc.MARGIN_MIN
    # a timing error e is a phase error of at most pi e at the band edge: well inside what 256-QAM tolerates
    assert np.abs(tau - c["tau_true"]).max() < (0.02 if K > 100 else 0.06)


def test_model_skips_and_survives():
    """P = 0, negative or not finite takes an element out of both sums; a NaN
    symbol leaves theta and tau at the prediction and the rows after it recover."""
    F, N, K, bps = 1, 8, 63, 4
    c = tc.case(F, N, K, bps, 0.03, 0.0, 30, 0.03)
    Pw = np.ones((F, K))
    ref, th_ref, ta_ref, _ = tc.track(c["z"], Pw, bps)
    z = np.array(c["z"])
    z[0, :, :4] = 5.0 + 5.0j                      # garbage where P says "skip"
    Pw[0, :4] = (0.0, -1.0, np.nan, np.inf)
    out, th, ta, _ = tc.track(z, Pw, bps)
    assert np.abs(th - th_ref).max() < 0.02 and np.abs(ta - ta_ref).max() < 0.02
    nu = tc.signed_bins(K)[:4]
    rot = np.exp(-1j * (th[0][:, None] + 2 * np.pi * nu[None, :] * ta[0][:, None] / (K + 1)))
    assert np.allclose(out[0, :, :4], z[0, :, :4] * rot)   # ... and are still rotated
    z = np.array(c["z"])
    z[0, 3, 10] = np.nan
    out, th, ta, _ = tc.track(z, np.ones((F, K)), bps)
    assert th[0, 3] == 2 * th[0, 2] - th[0, 1] and ta[0, 3] == 2 * ta[0, 2] - ta[0, 1]
    assert np.abs(th[0, 4:] - th_ref[0, 4:]).max() < 0.02 and np.abs(ta[0, 4:] - ta_ref[0, 4:]).max() < 0.02
    assert [v.tolist() for v in tc.track(np.zeros((1, 3, 5), np.complex64), np.zeros((1, 5)), 2)[1:3]] == \
        [[[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]]
