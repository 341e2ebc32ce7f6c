"""Integer carrier offset (include/ofdm_lsmrc_acquire.h) without a device:
the new header declares both entries, the binding's second signature table is
that header's symbol set and the library exports it, every refusal answers
before any HIP call (fake device pointers) in the order the header states and
names the offending argument, the kernel is in the library with no private
segment, and the float64 model the GPU tests lean on recovers the offsets of
the issue's cases with the margins it was measured at."""
import ctypes
import os

import numpy as np
import pytest

import acquire_cases as ac
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_frame_cfo_acquire", "ofdm_pipeline_set_cfo_search"]
P = ctypes.c_void_p
ARG, UNSUPPORTED = -1, -3


def test_header_and_binding_declare_the_entries(ofdm):
    assert os.path.exists(ofdm.ACQUIRE_HEADER_PATH)
    names = ofdm.header_symbols(ofdm.ACQUIRE_HEADER_PATH)
    assert sorted(names) == sorted(ENTRIES)
    assert set(ofdm._SIGS_ACQUIRE) == set(names), set(ofdm._SIGS_ACQUIRE) ^ set(names)
    # the main header and its table gain nothing
    assert not set(names) & set(ofdm.header_symbols()) and not set(names) & set(ofdm._SIGS)
    L = ofdm.lib()
    for e in ENTRIES:
        assert hasattr(L, e), f"{e} not exported"
        assert getattr(L, e).argtypes == ofdm._SIGS_ACQUIRE[e][1]
    assert L.ofdm_version() == 2  # no version step
    txt = open(ofdm.ACQUIRE_HEADER_PATH).read()
    assert '#include "ofdm_lsmrc.h"' in txt and "#define OFDM_ACQ_MAX_SHIFT 64" in txt
    assert ofdm.ACQ_MAX_SHIFT == 64
    assert callable(ofdm.frame_cfo_acquire) and callable(ofdm.Pipeline.set_cfo_search)
    # the build identity covers the new header
    import inspect
    assert "ACQUIRE_HEADER_PATH" in inspect.getsource(ofdm.build_id)


def test_refusals_without_device(ofdm):
    L = ofdm.lib()
    iq, X, eo, sh, me = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20)

    def acq(iq=iq, F=2, S=3, R=4, C=1024, cp=16, X=X, D=16, ratio=2.0, ein=None, eout=eo, shift=sh, metric=me):
        return L.ofdm_frame_cfo_acquire(iq, F, S, R, C, cp, X, D, ratio, ein, eout, shift, metric, None)

    def refused(code, word, **kw):
        assert acq(**kw) == code, kw
        assert word in L.ofdm_last_error(), (kw, L.ofdm_last_error())

    refused(ARG, b"nframes", F=-1)
    refused(ARG, b"S=", S=1)
    refused(ARG, b"R=", R=0)
    refused(ARG, b"cp_len", cp=-1)
    refused(ARG, b"cp_len", cp=1025)
    refused(ARG, b"d_iq", iq=None)
    refused(ARG, b"d_X", X=None)
    refused(ARG, b"d_eps_out", eout=None)
    refused(ARG, b"d_iq", iq=P((1 << 20) + 8))
    assert b"aligned" in L.ofdm_last_error()
    for D in (0, -1, 65):
        refused(ARG, b"max_shift", D=D)
    for r in (0.5, 0.999, float("nan"), float("inf"), -2.0):
        refused(ARG, b"min_ratio", ratio=r)
    # d_eps_out inside d_metric (2 x 33 floats) or d_shift (2 ints); touching ends are disjoint
    refused(ARG, b"d_metric", eout=P((5 << 20) + 4 * 65))
    refused(ARG, b"d_metric", metric=P((3 << 20) + 4))
    refused(ARG, b"d_shift", eout=P((4 << 20) + 4))
    refused(ARG, b"d_shift", shift=eo)
    for C in (6, 7, 8193, 16384):
        refused(UNSUPPORTED, b"C=", C=C, cp=0, D=1)
    refused(ARG, b"max_shift", C=8, cp=0, D=3)
    refused(ARG, b"max_shift", C=63, cp=9, D=16)
    refused(ARG, b"max_shift", C=255, cp=0, D=64)
    # the order: the argument checks, then the C range, then 4 max_shift <= C
    refused(ARG, b"S=", S=1, C=6, cp=0)
    refused(ARG, b"min_ratio", ratio=0.0, C=6, cp=0)
    refused(ARG, b"d_shift", shift=eo, C=6, cp=0)
    refused(UNSUPPORTED, b"C=", C=6, cp=0, D=16)
    # nframes == 0 is a no-op, null pointers and all; its other arguments are still checked
    assert acq(F=0, iq=None, X=None, eout=None, shift=None, metric=None) == 0
    assert acq(F=0, iq=None, X=None, eout=None, shift=None, metric=None, cp=0) == 0
    refused(ARG, b"max_shift", F=0, D=0)
    refused(UNSUPPORTED, b"C=", F=0, C=4, cp=0, D=1)
    # the sticky device status is neither consulted nor cleared
    assert L.ofdm_device_status() == 0
    assert L.ofdm_device_status_inject(1) == 0
    assert acq(F=0) == 0 and acq(S=1) == ARG
    assert L.ofdm_device_status() == -5
    assert L.ofdm_device_status() == 0
    # the pipeline setter refuses a null pipeline before it looks at anything else
    for D, r in ((16, 2.0), (0, 2.0), (-1, 2.0), (16, 0.5)):
        assert L.ofdm_pipeline_set_cfo_search(None, D, r) == ARG
        assert b"null pipeline" in L.ofdm_last_error()


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_acquire_kernel_has_no_private_segment():
    seg = kernel_private_segments(LIB)
    found = {n: v for n, v in seg.items() if "k_acquire_any" in n}
    assert len(found) == 3, found  # one per LDS capacity: 2048, 4096, 8192
    assert all(v == 0 for v in found.values()), f"private segment {found}"


EPS = lambda D: (2.03, -3.2, 0.45, 7.0, -0.496, D - 0.45)
MODEL_SHAPES = [(1024, 4, 16, 16), (600, 3, 9, 16), (256, 2, 16, 8)]  # C, R, cp, D


@pytest.mark.parametrize("C,R,cp,D", MODEL_SHAPES)
def test_model_recovers_the_offsets(C, R, cp, D):
    eps = np.array(EPS(D), np.float32)
    F = len(eps)
    c = ac.frames(F, 2, R, C, cp, eps, ac.random_pilots(C - 1, seed=C), seed=1)
    _, est = ac.cc.gamma_ref(c["y"], cp)
    want = np.rint(eps.astype(np.float64) - est).astype(np.int32)
    assert np.all(np.abs(eps - est - want) < 5e-3)  # the estimator sees eps modulo one spacing
    shift, eps_out, M, ratio = ac.acquire(c["y"], c["X"], cp, D, est.astype(np.float32), 2.0)
    print(f"C={C}: shifts {shift.tolist()} ratios {np.round(ratio, 1).tolist()} eps_out {eps_out.tolist()}")
    assert np.array_equal(shift, want)
    assert np.all(ratio >= 3.0)
    assert np.all(np.abs(eps_out.astype(np.float64) - eps) < 5e-3)
    # D - 0.45 resolves the +-0.5 wrap: the estimator sees about -0.45 and the search adds D
    assert est[-1] < 0 and shift[-1] == D
    # a null eps_in on integer offsets, and the ungated M whatever the gate
    ci = ac.frames(3, 2, R, C, cp, (3.0, -5.0, 0.0), c["X"], seed=2)
    s0, e0, M0, r0 = ac.acquire(ci["y"], ci["X"], cp, D, None, 1.0)
    s1, e1, M1, r1 = ac.acquire(ci["y"], ci["X"], cp, D, None, 1e6)
    assert s0.tolist() == [3, -5, 0] and np.all(r0 >= 3.0) and e0.tolist() == [3.0, -5.0, 0.0]
    assert s1.tolist() == [0, 0, 0] and np.array_equal(M0, M1) and np.array_equal(r0, r1)


@pytest.mark.parametrize("C,R,cp,D", MODEL_SHAPES)
def test_model_gate_cases(C, R, cp, D):
    """constant pilots (the reference's fallback fill) and noise-only frames: no shift stands out"""
    eps = np.array([2.0, -3.0, 0.0], np.float32)
    const = ac.frames(3, 2, R, C, cp, eps, ac.constant_pilots(C - 1), seed=3)
    noise = ac.frames(3, 2, R, C, cp, eps, ac.random_pilots(C - 1, seed=C), seed=4, noise_only=True)
    for name, c in (("constant pilots", const), ("noise only", noise)):
        shift, eps_out, M, ratio = ac.acquire(c["y"], c["X"], cp, D, np.zeros(3, np.float32), 2.0)
        print(f"C={C} {name}: ratios {np.round(ratio, 3).tolist()}")
        assert np.all(ratio <= 1.5) and np.all(ratio > 0)
        assert shift.tolist() == [0, 0, 0] and eps_out.tolist() == [0.0, 0.0, 0.0]


def test_model_ties_zero_and_non_finite():
    C, R, cp, D = 64, 1, 8, 4
    c = ac.frames(3, 2, R, C, cp, (1.0, 0.0, -2.0), ac.random_pilots(C - 1, seed=9), seed=5)
    y = np.array(c["y"])
    y[1] = 0                                  # M = 0 everywhere: no M is positive
    y[2, 0, 0, cp + 3] = np.nan               # every M of frame 2 is NaN: never chosen
    ein = np.array([np.nan, 0.25, np.inf], np.float32)
    shift, eps_out, M, ratio = ac.acquire(y, c["X"], cp, D, ein, 1.0)
    assert shift.tolist() == [1, 0, 0] and eps_out.tolist() == [1.0, 0.25, 0.0]
    assert np.all(M[1] == 0) and np.all(np.isnan(M[2])) and ratio[1] == 0 and ratio[2] == 0
    assert ac.priority(2) == [0, -1, 1, -2, 2]
