"""CPU-side checks of the C ABI library: it loads, exports every symbol that
include/ofdm_lsmrc.h declares, its host functions match the oracle, and its
argument validation fails loudly before touching any device."""
import ctypes
import os

import numpy as np
import pytest

from helpers import GOLDEN


def test_library_exports_header(ofdm):
    names = ofdm.header_symbols()
    assert len(names) >= 16, names
    L = ofdm.lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/ofdm_lsmrc.h but not exported"
    # and the binding's signature table covers the header exactly
    assert set(names) == set(ofdm._SIGS), set(names) ^ set(ofdm._SIGS)
    assert L.ofdm_version() == 2


def test_product_library_reads_no_environment(ofdm):
    """The shipped library has no experiment switches: it does not even import
    getenv."""
    import subprocess
    path = ofdm.LIB_PATH
    if os.environ.get("OFDM_LSMRC_LIB"):
        pytest.skip("OFDM_LSMRC_LIB selects an experiment build")
    syms = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms, "the product library must not read environment variables"


def test_pilot_rotate_matches_oracle(ofdm, oracle):
    for K in (3, 255, 1023, 4095):
        raw = (np.arange(K) - 1j * np.arange(K)).astype(np.complex64)
        assert np.array_equal(ofdm.pilot_rotate(raw), oracle.pilot_rotate(raw))


def test_read_pilots_file_and_missing(ofdm, tmp_path):
    X, fill = ofdm.read_pilots(os.path.join(GOLDEN, "Pilots.dat"), 1023)
    assert not fill
    assert np.array_equal(X, np.load(os.path.join(GOLDEN, "pilots_rotated_k1023.npy")))
    # missing file: reference fills 0.707+0.707i on the CPU path (cpuLS.hpp:84-90)
    # and 1+1i on the GPU path (gpuLS.cu:57-63)
    X, fill = ofdm.read_pilots(str(tmp_path / "nope.dat"), 7, 0.707)
    assert fill and np.all(X == np.complex64(0.707 + 0.707j))
    X, fill = ofdm.read_pilots(str(tmp_path / "nope.dat"), 7, 1.0)
    assert fill and np.all(X == np.complex64(1 + 1j))


def test_argument_validation_without_device(ofdm):
    L = ofdm.lib()
    P = ctypes.c_void_p
    fake = P(4096)  # never dereferenced: validation rejects first
    # unsupported FFT size
    assert L.ofdm_fft_rows(fake, fake, 1, 8193, 0, None) == -3
    assert b"out of [2, 8192]" in L.ofdm_last_error()
    assert L.ofdm_fft_rows(fake, fake, 1, 1, 0, None) == -3
    assert L.ofdm_frame_demod(fake, 1, 2, 4, 16384, 0, fake, fake, 1 << 30, fake, None) == -3
    # null pointers
    assert L.ofdm_ls_estimate(None, fake, 4, 1024, fake, fake, None) == -1
    # frame shape errors
    assert L.ofdm_frame_demod(fake, 1, 1, 4, 1024, 0, fake, fake, 1 << 30, fake, None) == -1
    assert L.ofdm_frame_demod(fake, 1, 2, 0, 1024, 0, fake, fake, 1 << 30, fake, None) == -1
    assert L.ofdm_frame_demod(fake, 1, 2, 4, 1024, 2000, fake, fake, 1 << 30, fake, None) == -1
    # misaligned input
    assert L.ofdm_frame_demod(P(4104), 1, 2, 4, 1024, 0, fake, fake, 1 << 30, fake, None) == -1
    assert b"aligned" in L.ofdm_last_error()
    # workspace too small
    need = L.ofdm_frame_workspace_bytes(10, 11, 64, 1024)
    assert need >= 10 * 64 * 1024 * 8
    assert L.ofdm_frame_demod(fake, 10, 11, 64, 1024, 0, fake, fake, need - 1, fake, None) == -1
    assert b"workspace" in L.ofdm_last_error()
    # zero frames is a no-op success (nothing launched)
    assert L.ofdm_frame_demod(fake, 0, 11, 64, 1024, 0, fake, fake, need, fake, None) == 0


def test_stated_alignments_are_refused_without_device(ofdm):
    """The header's alignment paragraph: the sample input of the frame, symbol
    and MRC entries 16 bytes, the workspace 256 -- refused with OFDM_E_ARG
    before any device work when only the element's natural 8 bytes hold (the
    containment tests run every pointer at exactly its stated alignment and
    none below it)."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    ok, off8 = P(4096), P(4096 + 8)
    need = L.ofdm_frame_workspace_bytes(2, 5, 8, 1024)
    calls = [
        lambda: L.ofdm_mrc_demod(off8, 3, ok, ok, 4, 1024, ok, None),
        lambda: L.ofdm_mrc_numerator(off8, 3, ok, 4, 1024, ok, None),
        lambda: L.ofdm_frame_estimate(off8, 2, 5, 8, 1024, 0, ok, ok, need, None),
        lambda: L.ofdm_frame_combine(off8, 2, 5, 8, 1024, 0, ok, need, ok, None),
        lambda: L.ofdm_frame_demod_freq(off8, 2, 5, 8, 1024, ok, ok, need, ok, None),
        lambda: L.ofdm_frame_demod_freq_mfma(off8, 2, 5, 8, 1024, ok, ok, need, ok, None),
        lambda: L.ofdm_frame_ls_partial(off8, 2, 5, 8, 1024, 0, ok, ok, need, ok, None),
        lambda: L.ofdm_frame_cfo_estimate(off8, 2, 5, 8, 1024, 16, 0, None, ok, None),
        lambda: L.ofdm_symbols_demod(off8, 3, 8, 1024, 0, ok, need, 0, ok, None),
        lambda: L.ofdm_frame_demod(ok, 2, 5, 8, 1024, 0, ok, P(4096 + 128), need, ok, None),  # the workspace
    ]
    for i, call in enumerate(calls):
        assert call() == -1, i
        assert b"aligned" in L.ofdm_last_error(), (i, L.ofdm_last_error())
    # the natural alignment is enough for every other pointer: these get past the alignment checks
    assert L.ofdm_mrc_demod(ok, 3, off8, P(4096 + 4), 4, 8193, off8, None) == -3  # (refused for C alone)
    assert L.ofdm_frame_combine(ok, 2, 5, 8, 1024, 0, ok, need, off8, None) == -1
    assert b"holds no estimate" in L.ofdm_last_error()


def test_zf_argument_validation_without_device(ofdm):
    """ofdm_zf_* reject unsupported geometry and null pointers before any launch."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    fake = P(4096)
    assert L.ofdm_zf_precoder(fake, 33, 64, 1023, fake, None, None) == -3  # > OFDM_ZF_MAX_USERS
    assert b"users" in L.ofdm_last_error()
    assert L.ofdm_zf_precoder(fake, 16, 513, 1023, fake, None, None) == -3  # users*rows > 8192
    assert L.ofdm_zf_precoder(fake, 0, 64, 1023, fake, None, None) == -3
    assert L.ofdm_zf_precoder(fake, 4, 0, 1023, fake, None, None) == -1
    assert L.ofdm_zf_precoder(fake, 4, 8, 1023, None, None, None) == -1  # no output at all
    assert L.ofdm_zf_precoder(None, 4, 8, 0, None, None, None) == 0  # K = 0: nothing to do
    assert L.ofdm_zf_transpose(fake, 4, 8, 16, fake, None) == -1  # aliased
    assert L.ofdm_zf_apply(fake, fake, 4, 8, 16, -1, fake, None) == -1
    assert L.ofdm_zf_apply(None, None, 4, 8, 16, 0, None, None) == 0  # no symbols
    assert L.ofdm_zf_detect(fake, None, 4, 8, 16, 3, fake, None) == -1


def test_workspace_registry_without_device(ofdm):
    """The consumers of a workspace refuse one that no estimate call filled
    (host registry, checked before any launch); releasing an unknown or null
    workspace is a no-op."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    fake, ws = P(4096), P(1 << 20)
    need = L.ofdm_frame_workspace_bytes(2, 5, 8, 1024)
    assert L.ofdm_workspace_release(ws) == 0
    assert L.ofdm_workspace_release(None) == 0
    assert L.ofdm_frame_combine(fake, 2, 5, 8, 1024, 0, ws, need, fake, None) == -1
    assert b"holds no estimate" in L.ofdm_last_error()
    assert L.ofdm_frame_mrc_partial(fake, 2, 5, 8, 1024, 0, ws, need, fake, None) == -1
    assert L.ofdm_frame_combine_freq(fake, 2, 5, 8, 1024, ws, need, fake, None) == -1
    assert L.ofdm_frame_export_estimate(ws, need, 2, 5, 8, 1024, 0, fake, None, None) == -1
    assert b"holds no estimate" in L.ofdm_last_error()
    # the range entry: its range is checked first, then the same registry
    assert L.ofdm_frame_mrc_partial_range(fake, 2, 1, 2, 5, 8, 1024, 0, ws, need, fake, None) == -1
    assert b"outside" in L.ofdm_last_error()
    assert L.ofdm_frame_mrc_partial_range(fake, 2, -1, 1, 5, 8, 1024, 0, ws, need, fake, None) == -1
    assert L.ofdm_frame_mrc_partial_range(None, 2, 2, 0, 5, 8, 1024, 0, ws, need, None, None) == 0  # empty range
    assert L.ofdm_frame_mrc_partial_range(fake, 2, 0, 2, 5, 8, 1024, 0, ws, need, fake, None) == -1
    assert b"holds no estimate" in L.ofdm_last_error()


def test_product_library_dispatches_only_product_kernels(ofdm):
    """Measured-and-dropped candidates live in scripts/experiments, not in the
    shipped library or its sources: no wave-quad C = 4096 receiver, no
    register-FFT test kernel, no one-launch C = 2048 /
    4096 demod, no A/B-only ZF GEMMs and no experiment-switch build at all
    (VERDICT r3 item 7)."""
    import glob
    import subprocess
    path = ofdm.LIB_PATH
    if os.environ.get("OFDM_LSMRC_LIB"):
        pytest.skip("OFDM_LSMRC_LIB selects an experiment build")
    syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                          check=True).stdout
    for bad in ("td4096r", "rfft", "k_demod_td2048", "k_demod_td4096", "k_zf_gemm_dma", "k_zf_mfmaILi",
                "k_zf_mfma_ldsILi"):
        assert bad not in syms, f"{bad} kernel in the product library"
    pkg = os.path.dirname(os.path.dirname(path))
    mk = open(os.path.join(pkg, "Makefile")).read()
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS_HIP")][0]
    assert "td4096r" not in srcs and "rfft" not in srcs
    assert "OFDM_AB_KNOBS" not in mk
    for src in glob.glob(os.path.join(pkg, "csrc", "*")):
        text = open(src).read()
        assert "OFDM_AB_KNOBS" not in text and "ab_knob(" not in text, src


def test_workspace_sizes(ofdm):
    # fused C=1024: Hc [F][R][C] + P [F][C] + one flag word per frame + the
    # 4-KiB ticket area (8 work-ticket counters, one 128-B line each), no staging
    F, S, R, C = 100, 101, 16, 1024
    b = ofdm.workspace_bytes(F, S, R, C)
    assert b == F * R * C * 8 + F * C * 4 + (F * 8 + 255) // 256 * 256 + 4 * 8 * 128
    # non-fused C carries a bounded staging buffer (<= 256 MiB or one frame)
    b2 = ofdm.workspace_bytes(F, S, 64, 2048)
    assert b2 - (F * 64 * 2048 * 8 + F * 2048 * 4) <= max(256 << 20, S * 64 * 2048 * 8) + 512 + 2048
    # any other C in [2, 8192] runs the staged path (mixed-radix row FFT)
    for c in (2, 7, 1000, 1536, 8192):
        assert ofdm.workspace_bytes(F, S, R, c) >= F * R * c * 8 + F * c * 4 + S * R * c * 8
    assert ofdm.workspace_bytes(F, S, R, 1) == 0 and ofdm.workspace_bytes(F, S, R, 8193) == 0


def test_pipeline_argument_validation_without_device(ofdm):
    """ofdm_pipeline_* reject bad geometry / null handles before any HIP call."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    X = np.ones(1023, np.complex64)
    h = P()
    assert L.ofdm_pipeline_create(101, 64, 1024, 0, None, 4, 3, ctypes.byref(h)) == -1
    assert L.ofdm_pipeline_create(101, 64, 1024, 0, X.ctypes.data_as(P), 0, 3, ctypes.byref(h)) == -1
    assert L.ofdm_pipeline_create(101, 64, 1024, 0, X.ctypes.data_as(P), 4, 0, ctypes.byref(h)) == -1
    assert L.ofdm_pipeline_create(101, 64, 9000, 0, X.ctypes.data_as(P), 4, 3, ctypes.byref(h)) == -3
    assert L.ofdm_pipeline_create(1, 64, 1024, 0, X.ctypes.data_as(P), 4, 3, ctypes.byref(h)) == -3
    assert L.ofdm_pipeline_create(101, 64, 1024, 2000, X.ctypes.data_as(P), 4, 3,
                                  ctypes.byref(h)) == -1
    assert h.value is None
    assert L.ofdm_pipeline_submit(None, 1, None) == -1
    assert L.ofdm_pipeline_demod(None, None, 1, None) == -1
    assert L.ofdm_pipeline_sync(None) == -1
    assert L.ofdm_pipeline_destroy(None) == 0
    assert L.ofdm_host_register(None, 10) == -1


def test_device_status_reporting_without_device(ofdm):
    """The sticky device status (include/ofdm_lsmrc.h): once raised, the next
    work-ticketed entry returns OFDM_E_DEVICE (-5) before validating or
    launching anything and clears it; entries without tickets ignore it;
    ofdm_device_status() reports and clears it on demand."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    fake, ws = P(4096), P(1 << 20)
    assert L.ofdm_device_status() == 0
    need = L.ofdm_frame_workspace_bytes(2, 5, 8, 4096)
    ticketed = [
        lambda: L.ofdm_frame_demod(None, 1, 1, 4, 1024, 0, None, None, 0, None, None),
        lambda: L.ofdm_frame_demod_ex(None, 1, 1, 4, 1024, 0, None, None, 0, None, 0, -1, None),
        lambda: L.ofdm_frame_combine(fake, 2, 5, 8, 4096, 0, ws, need, fake, None),
        lambda: L.ofdm_frame_mrc_partial(fake, 2, 5, 8, 4096, 0, ws, need, fake, None),
        lambda: L.ofdm_frame_mrc_partial_range(fake, 2, 0, 2, 5, 8, 4096, 0, ws, need, fake, None),
        lambda: L.ofdm_symbols_demod(fake, 1, 8, 4096, 0, ws, need, 0, fake, None),
    ]
    for call in ticketed:
        assert L.ofdm_device_status_inject(1) == 0
        assert L.ofdm_fft_rows(fake, fake, 1, 8193, 0, None) == -3  # no tickets: not consumed here
        assert call() == -5
        assert b"work-ticket" in L.ofdm_last_error() and b"foreign count" in L.ofdm_last_error()
        assert call() == -1  # cleared: the call's own validation speaks again
    assert L.ofdm_device_status_inject(2 | 4) == 0
    assert L.ofdm_device_status() == -5
    assert b"count out of range" in L.ofdm_last_error() and b"contended" in L.ofdm_last_error()
    assert L.ofdm_device_status() == 0


def test_hbm_probe_refuses_small_destination(ofdm):
    """ofdm_hbm_probe checks d_dst's size before launching."""
    L = ofdm.lib()
    P = ctypes.c_void_p
    fake = P(4096)
    assert L.ofdm_hbm_probe(0, fake, fake, 1 << 20, (1 << 20) - 16, None) == -1
    assert b"d_dst holds" in L.ofdm_last_error()
    assert L.ofdm_hbm_probe(1, fake, fake, 1 << 20, (1 << 20) - 16, None) == -1
    assert L.ofdm_hbm_probe(2, fake, fake, 1 << 20, 1 << 20, None) == -1


def test_zf_pitched_validation_without_device(ofdm):
    L = ofdm.lib()
    fake = ctypes.c_void_p(4096)
    assert L.ofdm_zf_detect_ex(fake, fake, 1022, 16, 64, 1023, 4, fake, 1024, None) == -1  # ldy < K
    assert b"below K" in L.ofdm_last_error()
    assert L.ofdm_zf_detect_ex(fake, fake, 1024, 16, 64, 1023, 4, fake, 1000, None) == -1  # ldx < K
    assert L.ofdm_zf_detect_ex(fake, fake, 1024, 16, 100, 1023, 4, fake, 1024, None) == -3  # pitched, R > 72
    assert L.ofdm_zf_detect_ex(fake, fake, 1024, 33, 64, 1023, 4, fake, 1024, None) == -3  # users > 32
    assert L.ofdm_zf_detect_ex(None, None, 1024, 16, 64, 1023, 0, None, 1024, None) == 0  # no symbols
    assert L.ofdm_zf_apply_ex(fake, fake, 1000, 16, 64, 1023, 4, fake, 1024, None) == -1  # ldx < K
    assert b"below K" in L.ofdm_last_error()
    assert L.ofdm_zf_apply_ex(fake, fake, 1024, 16, 4, 1023, 4, fake, 1024, None) == -3  # pitched, rows < 8
    assert L.ofdm_zf_apply_ex(fake, fake, 1024, 41, 64, 1023, 4, fake, 1024, None) == -3  # pitched, users > 40
    assert L.ofdm_zf_apply_ex(None, None, 1024, 16, 64, 1023, 0, None, 1024, None) == 0
