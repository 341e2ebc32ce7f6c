"""ofdm_frame_estimate_denoise and ofdm_pipeline_set_denoise without a device:
the library exports them, the binding declares them, their argument checks
answer before any device work (never-dereferenced pointers), and the denoising
kernels are in the gfx950 code object with no private segment.

Two refusals need a workspace the registry knows -- an estimate of another
geometry and an antenna-split partial estimate -- and a registry entry is only
made by an estimate that was launched: tests/test_denoise_gpu.py holds them
(test_refusals_that_need_a_registered_workspace), as it holds
set_denoise's taps_post + taps_pre > C, which needs a pipeline to read C from."""
import ctypes
import os

import pytest

import test_kernel_resources as kr

P = ctypes.c_void_p
E_ARG = -1


def _call(L, F=2, S=5, R=8, C=1024, tp=16, tq=0, ws=1 << 20, need=None):
    if need is None:
        need = L.ofdm_frame_workspace_bytes(max(F, 1), max(S, 2), max(R, 1), C if 2 <= C <= 8192 else 1024)
    rc = L.ofdm_frame_estimate_denoise(P(ws), need, F, S, R, C, tp, tq, None)
    return rc, L.ofdm_last_error()


def test_symbols_exported_and_bound(ofdm):
    L = ofdm.lib()
    for n in ("ofdm_frame_estimate_denoise", "ofdm_pipeline_set_denoise"):
        assert hasattr(L, n), f"{n} not exported"
        assert n in ofdm._SIGS and n in ofdm.header_symbols()
    assert callable(ofdm.frame_estimate_denoise) and callable(ofdm.Pipeline.set_denoise)
    assert L.ofdm_version() == 2  # added without a version step


def test_bad_taps(ofdm):
    L = ofdm.lib()
    for tp, tq in ((0, 0), (-1, 0), (0, 4), (16, -1), (1024, 1), (1, 1024), (1025, 0), (600, 600),
                   (2 ** 31 - 1, 2 ** 31 - 1)):
        rc, e = _call(L, tp=tp, tq=tq)
        assert rc == E_ARG and b"ofdm_frame_estimate_denoise" in e and b"taps_post" in e, (tp, tq)
    # the whole window is a valid choice: the call goes on to the workspace check
    for tp, tq in ((1024, 0), (1019, 5), (1, 1023), (1, 0)):
        rc, e = _call(L, tp=tp, tq=tq)
        assert rc == E_ARG and b"holds no estimate" in e, (tp, tq)
    rc, e = _call(L, C=7, tp=4, tq=4)
    assert rc == E_ARG and b"taps_post" in e


def test_bad_geometry(ofdm):
    L = ofdm.lib()
    for kw in (dict(F=-1), dict(S=1), dict(S=0), dict(R=0), dict(R=-3), dict(C=1), dict(C=0), dict(C=8193), dict(C=-5)):
        rc, e = _call(L, **kw)
        assert rc == E_ARG and b"ofdm_frame_estimate_denoise" in e, kw
        assert b"geometry" in e or b"nframes" in e, kw


def test_null_workspace(ofdm):
    L = ofdm.lib()
    rc, e = _call(L, ws=0)
    assert rc == E_ARG and b"null" in e


def test_unknown_workspace(ofdm):
    L = ofdm.lib()
    rc, e = _call(L)
    assert rc == E_ARG and b"ofdm_frame_estimate_denoise" in e and b"holds no estimate" in e
    # a released address is unknown too
    assert L.ofdm_workspace_release(P(1 << 20)) == 0
    rc, e = _call(L)
    assert rc == E_ARG and b"holds no estimate" in e


def test_zero_frames_is_a_noop(ofdm):
    L = ofdm.lib()
    assert _call(L, F=0)[0] == 0
    assert L.ofdm_frame_estimate_denoise(None, 0, 0, 5, 8, 1024, 16, 0, None) == 0
    assert L.ofdm_frame_estimate_denoise(None, 0, 0, 5, 8, 1024, 1024, 0, None) == 0
    # ... but still not with a bad window or geometry
    assert L.ofdm_frame_estimate_denoise(None, 0, 0, 5, 8, 1024, 0, 0, None) == E_ARG
    assert L.ofdm_frame_estimate_denoise(None, 0, 0, 1, 8, 1024, 16, 0, None) == E_ARG


def test_does_not_consume_device_status(ofdm):
    """No work tickets: a raised sticky status is left for the ticketed entry points."""
    L = ofdm.lib()
    assert L.ofdm_device_status() == 0
    assert L.ofdm_device_status_inject(1) == 0
    rc, e = _call(L)
    assert rc == E_ARG and b"holds no estimate" in e  # its own validation, not OFDM_E_DEVICE
    assert L.ofdm_device_status() == -5
    assert L.ofdm_device_status() == 0


def test_pipeline_set_denoise_refusals(ofdm):
    L = ofdm.lib()
    rc = L.ofdm_pipeline_set_denoise(None, 16, 0)
    assert rc == E_ARG and b"ofdm_pipeline_set_denoise" in L.ofdm_last_error() and b"null" in L.ofdm_last_error()
    assert L.ofdm_pipeline_set_denoise(None, 0, 0) == E_ARG
    # negative values and a pre-cursor window without a post-cursor one are refused before the pipeline is read
    for tp, tq in ((-1, 0), (16, -1), (-2, -2), (0, 3)):
        rc = L.ofdm_pipeline_set_denoise(P(1 << 20), tp, tq)
        assert rc == E_ARG and b"ofdm_pipeline_set_denoise" in L.ofdm_last_error(), (tp, tq)


@pytest.mark.skipif(not os.path.exists(kr.LIB) or not all(os.path.exists(t) for t in kr.TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_kernels_present_without_private_segment():
    seg = kr.kernel_private_segments(kr.LIB)
    mine = {n: v for n, v in seg.items() if "k_denoise" in n}
    # the stage kernel in its three LDS capacities and the fused C = 1024 wave kernel
    assert sum("k_denoise_any" in n for n in mine) == 3, sorted(mine)
    assert any("k_denoise1024" in n for n in mine), sorted(mine)
    assert not any(mine.values()), mine
