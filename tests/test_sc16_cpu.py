"""sc16 IQ (include/ofdm_lsmrc.h, "sc16 IQ") without a device: the header and
the binding declare the seven entries, the sample is 4 bytes, argument
validation answers before any HIP call, and the library carries sc16
instantiations of the C = 1024 receiver and the converter, none with a
private segment."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_iq_convert_sc16", "ofdm_frame_demod_sc16", "ofdm_frame_estimate_sc16", "ofdm_frame_combine_sc16",
           "ofdm_pipeline_create_sc16", "ofdm_pipeline_acquire_sc16", "ofdm_pipeline_demod_sc16"]
P = ctypes.c_void_p
F32 = ctypes.c_float
SCALE = F32(2.0 ** -15)


class ofdm_sc16(ctypes.Structure):
    _fields_ = [("re", ctypes.c_int16), ("im", ctypes.c_int16)]


def test_header_and_binding_declare_the_entries(ofdm):
    names = ofdm.header_symbols()
    L = ofdm.lib()
    for e in ENTRIES:
        assert e in names, f"{e} not declared in include/ofdm_lsmrc.h"
        assert e in ofdm._SIGS, f"{e} not in the binding's signature table"
        assert hasattr(L, e), f"{e} not exported"
    txt = open(ofdm.HEADER_PATH).read()
    assert re.search(r"typedef struct ofdm_sc16 \{ int16_t re, im; \} ofdm_sc16;", txt)
    assert ctypes.sizeof(ofdm_sc16) == 4
    assert L.ofdm_version() == 2
    for f in ("iq_convert_sc16", "frame_demod_sc16", "frame_estimate_sc16", "frame_combine_sc16"):
        assert callable(getattr(ofdm, f))


def test_argument_validation_without_device(ofdm):
    L = ofdm.lib()
    fake, ws = P(4096), P(1 << 20)
    need = L.ofdm_frame_workspace_bytes(2, 5, 8, 1024)
    demod = lambda iq=fake, F=2, C=1024, scale=SCALE, X=fake, out=fake, cp=0: L.ofdm_frame_demod_sc16(
        iq, F, 5, 8, C, cp, scale, X, ws, need, out, None)
    est = lambda iq=fake, C=1024, scale=SCALE, X=fake: L.ofdm_frame_estimate_sc16(
        iq, 2, 5, 8, C, 0, scale, X, ws, need, None)
    comb = lambda iq=fake, C=1024, scale=SCALE, out=fake: L.ofdm_frame_combine_sc16(
        iq, 2, 5, 8, C, 0, scale, ws, need, out, None)
    # a scale that is not positive and finite
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for call in (demod, est, comb):
            assert call(scale=F32(bad)) == -1
            assert b"scale" in L.ofdm_last_error()
        assert L.ofdm_iq_convert_sc16(fake, 16, F32(bad), fake, None) == -1
        assert b"scale" in L.ofdm_last_error()
    # null pointers
    assert demod(iq=None) == -1 and demod(out=None) == -1 and demod(X=None) == -1
    assert est(iq=None) == -1 and est(X=None) == -1
    assert comb(iq=None) == -1 and comb(out=None) == -1
    assert L.ofdm_iq_convert_sc16(None, 16, SCALE, fake, None) == -1
    assert L.ofdm_iq_convert_sc16(fake, 16, SCALE, None, None) == -1
    assert L.ofdm_iq_convert_sc16(fake, -1, SCALE, fake, None) == -1
    # misaligned input: the base is 16-byte aligned (rows need 4 bytes only)
    for call in (demod, est, comb):
        assert call(iq=P(4100)) == -1
        assert b"aligned" in L.ofdm_last_error()
    assert L.ofdm_iq_convert_sc16(P(4100), 16, SCALE, fake, None) == -1
    assert b"aligned" in L.ofdm_last_error()
    assert L.ofdm_iq_convert_sc16(fake, 16, SCALE, P(4104), None) == -1
    # geometry, as the fp32 entries
    assert demod(cp=2000) == -1
    assert L.ofdm_frame_demod_sc16(fake, 2, 1, 8, 1024, 0, SCALE, fake, ws, need, fake, None) == -1
    assert demod(C=16384) == -3
    # no sc16 receiver at this C: the converter is the route
    for C in (2048, 600):
        for call in (demod, est, comb):
            assert call(C=C) == -3
            assert b"ofdm_iq_convert_sc16" in L.ofdm_last_error()
    # zero frames / samples: nothing launched
    assert demod(F=0) == 0
    assert L.ofdm_iq_convert_sc16(None, 0, SCALE, None, None) == 0
    # the registry: combine refuses a workspace no estimate filled
    assert L.ofdm_workspace_release(ws) == 0
    assert comb() == -1
    assert b"holds no estimate" in L.ofdm_last_error()
    # workspace too small
    assert L.ofdm_frame_demod_sc16(fake, 2, 5, 8, 1024, 0, SCALE, fake, ws, need - 1, fake, None) == -1
    assert b"workspace" in L.ofdm_last_error()


def test_sticky_status_is_consulted_like_the_fp32_entries(ofdm):
    L = ofdm.lib()
    fake, ws = P(4096), P(1 << 20)
    assert L.ofdm_device_status() == 0
    for call in (lambda: L.ofdm_frame_demod_sc16(None, 1, 1, 4, 1024, 0, SCALE, None, None, 0, None, None),
                 lambda: L.ofdm_frame_combine_sc16(None, 1, 1, 4, 1024, 0, SCALE, ws, 0, None, None)):
        assert L.ofdm_device_status_inject(1) == 0
        assert call() == -5
        assert call() == -1
    # the estimate, like ofdm_frame_estimate, does not consume it
    assert L.ofdm_device_status_inject(1) == 0
    assert L.ofdm_frame_estimate_sc16(None, 1, 1, 4, 1024, 0, SCALE, None, None, 0, None) == -1
    assert L.ofdm_device_status() == -5
    assert L.ofdm_device_status() == 0


def test_pipeline_argument_validation_without_device(ofdm):
    """ofdm_pipeline_*_sc16 reject bad geometry / scale / null handles before any HIP call."""
    L = ofdm.lib()
    X = np.ones(1023, np.complex64)
    Xp = X.ctypes.data_as(P)
    h = P()
    create = L.ofdm_pipeline_create_sc16
    assert create(101, 64, 1024, 0, SCALE, None, 4, 3, ctypes.byref(h)) == -1
    assert create(101, 64, 1024, 0, SCALE, Xp, 0, 3, ctypes.byref(h)) == -1
    assert create(101, 64, 1024, 0, SCALE, Xp, 4, 0, ctypes.byref(h)) == -1
    assert create(101, 64, 9000, 0, SCALE, Xp, 4, 3, ctypes.byref(h)) == -3
    assert create(1, 64, 1024, 0, SCALE, Xp, 4, 3, ctypes.byref(h)) == -3
    assert create(101, 64, 1024, 2000, SCALE, Xp, 4, 3, ctypes.byref(h)) == -1
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert create(101, 64, 1024, 0, F32(bad), Xp, 4, 3, ctypes.byref(h)) == -1
        assert b"scale" in L.ofdm_last_error()
    assert h.value is None
    d, s = P(), P()
    assert L.ofdm_pipeline_acquire_sc16(None, ctypes.byref(d), ctypes.byref(s)) == -1
    assert L.ofdm_pipeline_demod_sc16(None, None, 1, None) == -1


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_sc16_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    found = {}
    for k in ("k_ls_td1024", "k_mrc_td1024_hlds"):
        found[k] = {n: v for n, v in seg.items() if k in n and "sc16" in n}
    found["k_iq_sc16_to_cf32"] = {n: v for n, v in seg.items() if "k_iq_sc16_to_cf32" in n}
    assert len(found["k_ls_td1024"]) == 2, found  # the 4-wave and the 16-wave estimator
    assert len(found["k_mrc_td1024_hlds"]) == 1, found
    assert len(found["k_iq_sc16_to_cf32"]) == 1, found
    for k, d in found.items():
        assert all(v == 0 for v in d.values()), f"{k}: private segment {d}"
