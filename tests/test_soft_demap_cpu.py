"""Soft-output entry points (ofdm_frame_noise_estimate, ofdm_frame_soft_demap):
the library exports them, the binding declares them, and their argument
checks answer before any device work -- no GPU is touched here."""
import ctypes

P = ctypes.c_void_p
E_ARG, E_UNSUPPORTED = -1, -3
F32, I8 = 0, 1


def _calls(L, F=2, S=5, R=8, C=1024, mod=2, fmt=F32, scale=1.0, z=4096, ws=1 << 20, nv=8192, llr=1 << 16,
           need=None):
    """(noise_estimate rc, soft_demap rc, last error of the soft_demap call) on never-dereferenced pointers."""
    if need is None:
        need = L.ofdm_frame_workspace_bytes(max(F, 1), S, R, C)
    a = L.ofdm_frame_noise_estimate(P(z), F, S, R, C, P(ws), need, mod, P(nv), None)
    ea = L.ofdm_last_error()
    b = L.ofdm_frame_soft_demap(P(z), F, S, R, C, P(ws), need, mod, P(nv), fmt, scale, P(llr), None)
    return a, ea, b, L.ofdm_last_error()


def test_symbols_exported_and_bound(ofdm):
    L = ofdm.lib()
    for n in ("ofdm_frame_noise_estimate", "ofdm_frame_soft_demap"):
        assert hasattr(L, n), f"{n} not exported"
        assert n in ofdm._SIGS and n in ofdm.header_symbols()
    assert callable(ofdm.frame_noise_estimate) and callable(ofdm.frame_soft_demap)
    assert (ofdm.MOD_QPSK, ofdm.MOD_QAM16, ofdm.MOD_QAM64, ofdm.MOD_QAM256) == (2, 4, 6, 8)
    assert L.ofdm_version() == 2  # added without a version step


def test_bad_modulation(ofdm):
    L = ofdm.lib()
    for mod in (0, 1, 3, 5, 7, 10, -2):
        a, ea, b, eb = _calls(L, mod=mod)
        assert a == E_ARG and b == E_ARG, mod
        assert b"ofdm_frame_noise_estimate" in ea and b"modulation" in ea
        assert b"ofdm_frame_soft_demap" in eb and b"modulation" in eb


def test_bad_format(ofdm):
    L = ofdm.lib()
    for fmt in (-1, 2, 8):
        _, _, b, eb = _calls(L, fmt=fmt)
        assert b == E_ARG and b"ofdm_frame_soft_demap" in eb and b"llr_format" in eb


def test_i8_scale_must_be_positive_and_finite(ofdm):
    L = ofdm.lib()
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        _, _, b, eb = _calls(L, fmt=I8, scale=scale)
        assert b == E_ARG and b"ofdm_frame_soft_demap" in eb and b"llr_scale" in eb, scale
    # the float format ignores the scale: the call goes on to the workspace check
    _, _, b, eb = _calls(L, fmt=F32, scale=0.0)
    assert b == E_ARG and b"holds no estimate" in eb


def test_unknown_workspace(ofdm):
    L = ofdm.lib()
    for fmt in (F32, I8):
        a, ea, b, eb = _calls(L, fmt=fmt, scale=4.0)
        assert a == E_ARG and b"ofdm_frame_noise_estimate" in ea and b"holds no estimate" in ea
        assert b == E_ARG and b"ofdm_frame_soft_demap" in eb and b"holds no estimate" in eb


def test_geometry_and_pointers(ofdm):
    L = ofdm.lib()
    a, _, b, _ = _calls(L, S=1)
    assert a == E_ARG and b == E_ARG
    a, _, b, _ = _calls(L, R=0)
    assert a == E_ARG and b == E_ARG
    a, _, b, _ = _calls(L, C=8193, need=1 << 20)
    assert a == E_UNSUPPORTED and b == E_UNSUPPORTED
    a, _, b, _ = _calls(L, F=-1)
    assert a == E_ARG and b == E_ARG
    a, ea, b, eb = _calls(L, z=0)
    assert a == E_ARG and b == E_ARG and b"null" in ea and b"null" in eb
    a, _, b, _ = _calls(L, nv=0)
    assert a == E_ARG and b == E_ARG
    a, ea, b, eb = _calls(L, z=4104)
    assert a == E_ARG and b == E_ARG and b"aligned" in ea and b"aligned" in eb


def test_zero_frames_is_a_noop(ofdm):
    L = ofdm.lib()
    for mod in (2, 4, 6, 8):
        a, _, b, _ = _calls(L, F=0, mod=mod, fmt=I8, scale=2.0)
        assert a == 0 and b == 0
    # ... with null pointers too, but still not with a bad modulation
    assert L.ofdm_frame_noise_estimate(None, 0, 5, 8, 1024, None, 0, 4, None, None) == 0
    assert L.ofdm_frame_soft_demap(None, 0, 5, 8, 1024, None, 0, 4, None, F32, 1.0, None, None) == 0
    assert L.ofdm_frame_soft_demap(None, 0, 5, 8, 1024, None, 0, 3, None, F32, 1.0, None, None) == E_ARG


def test_does_not_consume_device_status(ofdm):
    """No work tickets: a raised sticky status is left for the ticketed entry points."""
    L = ofdm.lib()
    assert L.ofdm_device_status() == 0
    assert L.ofdm_device_status_inject(1) == 0
    a, _, b, _ = _calls(L)
    assert a == E_ARG and b == E_ARG  # their own validation, not OFDM_E_DEVICE
    assert L.ofdm_device_status() == -5
    assert L.ofdm_device_status() == 0
