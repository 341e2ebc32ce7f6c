"""Carrier frequency offset (include/ofdm_lsmrc.h, "carrier frequency offset")
without a device: the header and the binding declare the entries, every
refusal answers before any HIP call (null device pointers), the library
carries the derotating instantiations of the C = 1024 receiver and the two
cfo.hip kernels, none with a private segment, and the float64 model the GPU
tests lean on does what the issue's figures say."""
import ctypes
import os

import numpy as np
import pytest

import cfo_cases as cc
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_frame_cfo_estimate", "ofdm_frame_cfo_derotate", "ofdm_frame_estimate_cfo", "ofdm_frame_combine_cfo",
           "ofdm_frame_demod_cfo", "ofdm_pipeline_set_cfo"]
P = ctypes.c_void_p
ARG, UNSUPPORTED, DEVICE = -1, -3, -5


def test_header_and_binding_declare_the_entries(ofdm):
    names = ofdm.header_symbols()
    L = ofdm.lib()
    for e in ENTRIES:
        assert e in names, f"{e} not declared in include/ofdm_lsmrc.h"
        assert e in ofdm._SIGS, f"{e} not in the binding's signature table"
        assert hasattr(L, e), f"{e} not exported"
    assert L.ofdm_version() == 2  # no version step
    for f in ("frame_cfo_estimate", "frame_cfo_derotate", "frame_estimate_cfo", "frame_combine_cfo",
              "frame_demod_cfo"):
        assert callable(getattr(ofdm, f))
    assert callable(ofdm.Pipeline.set_cfo)


def test_estimator_and_derotator_refusals_without_device(ofdm):
    L = ofdm.lib()
    fake, fake2 = P(4096), P(1 << 24)
    est = lambda iq=fake, F=2, S=4, R=5, C=1024, cp=16, skip=0, gamma=None, eps=fake: L.ofdm_frame_cfo_estimate(
        iq, F, S, R, C, cp, skip, gamma, eps, None)
    for bad in (dict(cp=0), dict(cp=-1), dict(skip=-1), dict(skip=16), dict(skip=99), dict(iq=None), dict(eps=None),
                dict(S=1), dict(R=0), dict(F=-1), dict(cp=2000), dict(iq=P(4104))):
        assert est(**bad) == ARG, bad
    assert b"cp_skip" in (est(skip=16), L.ofdm_last_error())[1]
    assert b"cyclic prefix" in (est(cp=0), L.ofdm_last_error())[1]
    for C in (1, 8193):
        assert est(C=C) == UNSUPPORTED
    assert est(F=0, iq=None, eps=None) == 0  # a no-op
    rot = lambda i=fake, o=fake2, F=2, S=4, R=5, C=600, cp=9, eps=fake: L.ofdm_frame_cfo_derotate(
        i, o, F, S, R, C, cp, eps, None)
    for bad in (dict(i=None), dict(o=None), dict(eps=None), dict(S=1), dict(R=0), dict(F=-1), dict(cp=-1),
                dict(cp=601), dict(i=P(4104)), dict(o=P((1 << 24) + 8))):
        assert rot(**bad) == ARG, bad
    assert rot(C=9000) == UNSUPPORTED
    assert rot(F=0, i=None, o=None, eps=None) == 0
    # overlap: in place is allowed (and would launch, so it is not called here); anything else is refused
    nbytes = 2 * 4 * 5 * 609 * 8
    for o in (4096 + 16, 4096 + nbytes - 16):
        assert rot(o=P(o)) == ARG
        assert b"overlaps" in L.ofdm_last_error()
    assert rot(i=P(4096 + nbytes - 16), o=fake) == ARG
    assert b"overlaps" in L.ofdm_last_error()


def test_receiver_refusals_without_device(ofdm):
    L = ofdm.lib()
    fake, ws = P(4096), P(1 << 20)
    need = L.ofdm_frame_workspace_bytes(2, 5, 8, 1024)
    demod = lambda iq=fake, F=2, S=5, C=1024, X=fake, out=fake, cp=0, eps=fake, n=need: L.ofdm_frame_demod_cfo(
        iq, F, S, 8, C, cp, X, ws, n, out, eps, None)
    est = lambda iq=fake, C=1024, X=fake, eps=fake: L.ofdm_frame_estimate_cfo(iq, 2, 5, 8, C, 0, X, ws, need, eps, None)
    comb = lambda iq=fake, C=1024, out=fake, eps=fake: L.ofdm_frame_combine_cfo(iq, 2, 5, 8, C, 0, ws, need, out, eps,
                                                                                 None)
    for call in (demod, est, comb):
        assert call(eps=None) == ARG
        assert b"d_eps" in L.ofdm_last_error()
        assert call(iq=None) == ARG
        assert call(iq=P(4100)) == ARG
        assert b"aligned" in L.ofdm_last_error()
        # no derotating receiver at this C: the derotator is named
        for C in (2048, 600, 256):
            assert call(C=C) == UNSUPPORTED
            assert b"ofdm_frame_cfo_derotate" in L.ofdm_last_error()
        assert call(C=16384) == UNSUPPORTED
    assert demod(out=None) == ARG and demod(X=None) == ARG and est(X=None) == ARG and comb(out=None) == ARG
    assert demod(cp=2000) == ARG and demod(S=1) == ARG
    assert demod(F=0) == 0
    assert demod(n=need - 1) == ARG
    assert b"workspace" in L.ofdm_last_error()
    # the registry: combine refuses a workspace no estimate filled
    assert L.ofdm_workspace_release(ws) == 0
    assert comb() == ARG
    assert b"holds no estimate" in L.ofdm_last_error()
    assert L.ofdm_pipeline_set_cfo(None, 1, 0) == ARG
    assert L.ofdm_pipeline_set_cfo(None, 0, 0) == ARG


def test_sticky_status_is_consulted_like_the_fp32_entries(ofdm):
    L = ofdm.lib()
    ws = P(1 << 20)
    assert L.ofdm_device_status() == 0
    for call in (lambda: L.ofdm_frame_demod_cfo(None, 1, 1, 4, 1024, 0, None, None, 0, None, None, None),
                 lambda: L.ofdm_frame_combine_cfo(None, 1, 1, 4, 1024, 0, ws, 0, None, None, None)):
        assert L.ofdm_device_status_inject(1) == 0
        assert call() == DEVICE
        assert call() == ARG
    # the estimate, like ofdm_frame_estimate, does not consume it
    assert L.ofdm_device_status_inject(1) == 0
    assert L.ofdm_frame_estimate_cfo(None, 1, 1, 4, 1024, 0, None, None, 0, None, None) == ARG
    assert L.ofdm_device_status() == DEVICE
    assert L.ofdm_device_status() == 0


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_cfo_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    # the C = 1024 kernels' CFO instantiations carry the policy tag (src_cfo) in their symbol
    want = {("k_ls_td1024", "src_cfo"): 2,        # the 4-wave and the 16-wave estimator
            ("k_mrc_td1024_hlds", "src_cfo"): 1, ("k_cfo_estimate",): 1, ("k_cfo_derotate",): 1}
    for k, n in want.items():
        found = {name: v for name, v in seg.items() if all(part in name for part in k)}
        assert len(found) == n, (k, found)
        assert all(v == 0 for v in found.values()), f"{k}: private segment {found}"
    # the one-launch kernel has no CFO form, and there is no sc16 x CFO kernel
    assert not [n for n in seg if "cfo" in n and ("sc16" in n or "k_demod" in n)]


def test_float64_model_uncorrected_and_corrected():
    """The generator and the float64 receiver model: at the issue's shape the
    uncorrected receiver loses more than a quarter of its decisions, the
    prefix estimate plus the definition's derotation none."""
    F, S, R, C, cp = 3, 4, 5, 1024, 16
    c = cc.frames(F, S, R, C, cp, (0.03, -0.2, 0.45), seed=4)

    def receive(y):
        Y = np.fft.fft(y[..., cp:].astype(np.complex128), axis=-1)[..., 1:]
        H = Y[:, 0] / c["X"]
        return (Y[:, 1:] * np.conj(H)[:, None]).sum(2) / (np.abs(H) ** 2).sum(1)[:, None]

    wrong = cc.decision_errors(receive(c["y"]), c["data"])
    g, e = cc.gamma_ref(c["y"], cp)
    assert np.all(np.abs(e - c["eps"]) < 1e-3)
    fixed = cc.decision_errors(receive(cc.derotate_ref(c["y"], e.astype(np.float32), cp)), c["data"])
    assert wrong > c["data"].size // 4 and fixed == 0, (wrong, fixed)
    # rounding x' to f32 does not matter at the project's tolerance
    x64 = c["y"].astype(np.complex128) * cc.rotation(e.astype(np.float32), S, C, cp, -1.0)
    a, b = receive(x64), receive(x64.astype(np.complex64))
    assert np.linalg.norm(a - b) / np.linalg.norm(a) < 1e-6
