"""Phase tracking (include/ofdm_lsmrc.h, "phase tracking") without a device:
the header and the binding declare the entries, every refusal answers before
any HIP call (fake device pointers) and names its argument, the library
carries k_phase_track for the four constellations without a private segment,
and the float64 model the GPU tests lean on (phase_cases.track, the
definition) does what the issue's figures say."""
import ctypes
import os

import numpy as np
import pytest

import cfo_cases as cc
import phase_cases as pc
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_frame_phase_track", "ofdm_pipeline_set_phase_track"]
P = ctypes.c_void_p
ARG, UNSUPPORTED = -1, -3


def test_header_and_binding_declare_the_entries(ofdm):
    names = ofdm.header_symbols()
    L = ofdm.lib()
    for e in ENTRIES:
        assert e in names, f"{e} not declared in include/ofdm_lsmrc.h"
        assert e in ofdm._SIGS, f"{e} not in the binding's signature table"
        assert hasattr(L, e), f"{e} not exported"
    assert L.ofdm_version() == 2  # no version step
    assert callable(ofdm.frame_phase_track) and callable(ofdm.residual_cfo)
    assert callable(ofdm.Pipeline.set_phase_track)


def _track(L, z=4096, F=2, S=5, R=8, C=1024, ws=1 << 20, need=None, mod=2, out=1 << 24, phase=1 << 28):
    if need is None:
        need = L.ofdm_frame_workspace_bytes(max(F, 1), max(S, 2), max(R, 1), min(max(C, 2), 8192))
    rc = L.ofdm_frame_phase_track(P(z), F, S, R, C, P(ws), need, mod, P(out), P(phase), None)
    return rc, L.ofdm_last_error()


def test_refusals_without_device(ofdm):
    L = ofdm.lib()
    for mod in (0, 1, 3, 5, 7, 10, -2):
        rc, e = _track(L, mod=mod)
        assert rc == ARG and b"ofdm_frame_phase_track" in e and b"modulation" in e, mod
    for bad, word in ((dict(F=-1), b"nframes"), (dict(S=1), b"S=1"), (dict(R=0), b"R=0"), (dict(z=0), b"d_z"),
                      (dict(out=0), b"d_out"), (dict(ws=0), b"d_ws"), (dict(z=4100), b"d_z"),
                      (dict(out=(1 << 24) + 4), b"d_out"), (dict(phase=(1 << 28) + 2), b"d_phase")):
        rc, e = _track(L, **bad)
        assert rc == ARG and b"ofdm_frame_phase_track" in e and word in e, (bad, e)
    for C in (1, 8193):
        rc, e = _track(L, C=C)
        assert rc == UNSUPPORTED and b"C=" in e
    # overlap: in place is allowed (and would go on to the registry), disjoint too; anything else is refused
    nbytes = 2 * 4 * 1023 * 8
    for out in (4096 + 8, 4096 + nbytes - 8, 4096 - 8):
        rc, e = _track(L, out=out)
        assert rc == ARG and b"overlaps" in e and b"d_out" in e, out
    for phase in (4096, 4096 + nbytes - 4, (1 << 24) + 8, (1 << 24) - 4):
        rc, e = _track(L, phase=phase)
        assert rc == ARG and b"overlaps" in e and b"d_phase" in e, phase
    # the registry: a workspace no estimate filled, for in place, out of place and without phases alike
    assert L.ofdm_workspace_release(P(1 << 20)) == 0
    for kw in (dict(), dict(out=4096), dict(phase=0), dict(out=4096 + nbytes), dict(z=4104, out=4104)):
        rc, e = _track(L, **kw)
        assert rc == ARG and b"ofdm_frame_phase_track" in e and b"holds no estimate" in e, (kw, e)
    assert L.ofdm_pipeline_set_phase_track(None, 2) == ARG
    assert L.ofdm_pipeline_set_phase_track(None, 0) == ARG
    assert b"ofdm_pipeline_set_phase_track" in L.ofdm_last_error()


def test_zero_frames_is_a_noop(ofdm):
    L = ofdm.lib()
    for mod in (2, 4, 6, 8):
        assert _track(L, F=0, mod=mod)[0] == 0
    assert L.ofdm_frame_phase_track(None, 0, 5, 8, 1024, None, 0, 4, None, None, None) == 0
    # ... but still not with a bad modulation or geometry
    assert L.ofdm_frame_phase_track(None, 0, 5, 8, 1024, None, 0, 3, None, None, None) == ARG
    assert L.ofdm_frame_phase_track(None, 0, 1, 8, 1024, None, 0, 2, None, None, None) == ARG


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
def test_phase_track_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    for bps in (2, 4, 6, 8):
        found = {n: v for n, v in seg.items() if f"k_phase_trackILi{bps}E" in n}
        assert found, f"k_phase_track<{bps}> not in the library"
        assert all(v == 0 for v in found.values()), f"k_phase_track<{bps}>: private segment {found}"


def test_residual_cfo_helper(ofdm):
    """theta = 2 pi eps (C + cp) / C n' gives eps back, from numpy and from torch alike."""
    import torch
    C, cp, eps = 1024, 72, np.array([3e-4, -2e-3])
    theta = 2 * np.pi * eps[:, None] * (C + cp) / C * np.arange(1, 101)[None, :]
    assert np.allclose(ofdm.residual_cfo(theta.astype(np.float32), C, cp), eps, rtol=1e-6, atol=0)
    got = ofdm.residual_cfo(torch.from_numpy(theta.astype(np.float32)), C, cp)
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), eps, rtol=1e-6, atol=0)
    assert np.allclose(pc.residual_cfo(theta, C, cp), eps, rtol=1e-12, atol=0)


# ------------------------------------------------------------ the model

def receive(c, cp):
    """The float64 LS + MRC receiver on a cfo_cases frame set, by bin (no output rotation): (z, P)."""
    Y = np.fft.fft(c["y"][..., cp:].astype(np.complex128), axis=-1)[..., 1:]
    H = Y[:, 0] / c["X"]
    Pw = (np.abs(H) ** 2).sum(1)
    return (Y[:, 1:] * np.conj(H)[:, None]).sum(2) / Pw[:, None], Pw


# the issue's table: cfo_cases frames (seed 7) received without any correction
@pytest.mark.parametrize("shape,eps,wrong", [((3, 40, 4, 256, 16), (0.004, -0.006, 0.002), 7638),
                                             ((2, 101, 4, 1024, 72), (0.002, -0.003), 106046)])
def test_model_on_uncorrected_frames(shape, eps, wrong):
    F, S, R, C, cp = shape
    c = cc.frames(F, S, R, C, cp, eps, seed=7)
    z, Pw = receive(c, cp)
    assert c["data"].size == F * (S - 1) * (C - 1)
    assert cc.decision_errors(z, c["data"]) == wrong
    out, theta, margin = pc.track(z, Pw, 2)
    e = pc.residual_cfo(theta, C, cp)
    print(f"{shape}: {wrong} -> {cc.decision_errors(out, c['data'])} wrong, margin {margin:.3f} a, "
          f"eps error {np.abs(e - c['eps']).max():.2e}")
    assert cc.decision_errors(out, c["data"]) == 0
    assert margin >= pc.MARGIN_MIN
    assert np.abs(e - c["eps"]).max() <= 8.1e-6


# one case per modulation: 0.03 rad per symbol (times the frame's factor) and 0.005 rad of jitter
@pytest.mark.parametrize("bps,snr_db", [(2, 15), (4, 25), (6, 30), (8, 38)])
def test_model_per_modulation(bps, snr_db):
    F, N, K = 3, 12, 1023
    c = pc.case(F, N, K, bps, 0.03, 0.005, snr_db)
    before = pc.symbol_errors(c["z"], c["d"], bps)
    out, theta, margin = pc.track(c["z"], np.ones((F, K)), bps)
    after = pc.symbol_errors(out, c["d"], bps)
    print(f"bps {bps} at {snr_db} dB: {before} -> {after} of {c['d'].size} wrong, margin {margin:.3f} a, "
          f"theta error {np.abs(theta - c['theta_true']).max():.2e} rad")
    assert before > 0 and after == 0
    assert margin >= pc.MARGIN_MIN
    # the phase is followed to well inside what the densest constellation tolerates
    assert np.abs(theta - c["theta_true"]).max() < 0.02


def test_model_skips_and_survives():
    """P = 0, negative or not finite takes an element out of the sum; a NaN
    symbol leaves theta at the prediction and the rows after it recover."""
    F, N, K, bps = 1, 8, 63, 4
    c = pc.case(F, N, K, bps, 0.03, 0.0, 30)
    Pw = np.ones((F, K))
    ref, th_ref, _ = pc.track(c["z"], Pw, bps)
    z = np.array(c["z"])
    z[0, :, :4] = 5.0 + 5.0j                      # garbage where P says "skip"
    Pw[0, :4] = (0.0, -1.0, np.nan, np.inf)
    out, th, _ = pc.track(z, Pw, bps)
    assert np.abs(th - th_ref).max() < 0.02       # the four garbage columns did not take part
    assert np.allclose(out[0, :, :4], z[0, :, :4] * np.exp(-1j * th[0])[:, None])  # ... and are still rotated
    z = np.array(c["z"])
    z[0, 3, 10] = np.nan
    out, th, _ = pc.track(z, np.ones((F, K)), bps)
    assert th[0, 3] == th[0, 2] + (th[0, 2] - th[0, 1])
    assert np.abs(th[0, 4:] - th_ref[0, 4:]).max() < 0.02
    assert pc.track(np.zeros((1, 3, 5), np.complex64), np.zeros((1, 5)), 2)[1].tolist() == [[0.0, 0.0, 0.0]]
