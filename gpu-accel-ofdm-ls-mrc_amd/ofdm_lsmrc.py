"""Python binding of the C ABI in include/ofdm_lsmrc.h (libofdm_lsmrc.so).

Plumbing for tests and bench.py: device memory and streams come from PyTorch
(ROCm build), the compute is the HIP library.  There is no CPU fallback:
every compute call goes through libofdm_lsmrc.so and raises if it fails.

Mirrors the reference's operator surface:
  gpuLS::batchedFFT / cufft        -> fft_rows
  findHs + findDistSqrd            -> ls_estimate
  multiplyWithChannelConj + combineForMRC + shiftOneRow -> mrc_demod
  demodOneFrameCUDA (batched)      -> frame_demod / frame_demod_freq
  matrix_readX                     -> read_pilots / pilot_rotate
  modOneSymbol / modRefSymbol      -> tx_modulate
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# OFDM_LSMRC_LIB=<v> loads lib/libofdm_lsmrc_<v>.so instead, a build of
# experiment sources for scripts/ comparisons (scripts/libab.py); the product
# library has no switches.
_LIBSEL = os.environ.get("OFDM_LSMRC_LIB", "")
LIB_PATH = os.path.join(HERE, "lib", f"libofdm_lsmrc_{_LIBSEL}.so" if _LIBSEL else "libofdm_lsmrc.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ofdm_lsmrc.h")
ACQUIRE_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ofdm_lsmrc_acquire.h")
TIMING_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ofdm_lsmrc_timing.h")
DECODE_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ofdm_lsmrc_decode.h")
LDPC_HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "ofdm_lsmrc_ldpc.h")

_c = ctypes
_P = _c.c_void_p
_LL = _c.c_longlong
_I = _c.c_int

# name -> (restype, argtypes)
_SIGS = {
    "ofdm_version": (_I, []),
    "ofdm_last_error": (_c.c_char_p, []),
    "ofdm_pilot_rotate": (_I, [_P, _I, _P]),
    "ofdm_read_pilots": (_I, [_c.c_char_p, _I, _c.c_float, _P]),
    "ofdm_fft_rows": (_I, [_P, _P, _LL, _I, _I, _P]),
    "ofdm_ls_estimate": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "ofdm_mrc_demod": (_I, [_P, _LL, _P, _P, _I, _I, _P, _P]),
    "ofdm_mrc_numerator": (_I, [_P, _LL, _P, _I, _I, _P, _P]),
    "ofdm_mrc_finalize": (_I, [_P, _LL, _LL, _I, _I, _P, _P, _P]),
    "ofdm_channel_conj_product": (_I, [_P, _LL, _P, _I, _I, _P, _P]),
    "ofdm_combine_products": (_I, [_P, _LL, _P, _I, _I, _I, _P, _P]),
    "ofdm_shift_rows": (_I, [_P, _LL, _I, _P, _P]),
    "ofdm_dist_sqrd": (_I, [_P, _I, _I, _P, _P]),
    "ofdm_frame_workspace_bytes": (_c.c_size_t, [_LL, _I, _I, _I]),
    "ofdm_workspace_release": (_I, [_P]),
    "ofdm_frame_demod": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_demod_ex": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P, _I, _LL, _P]),
    "ofdm_frame_estimate": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P]),
    "ofdm_frame_combine": (_I, [_P, _LL, _I, _I, _I, _I, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_demod_freq": (_I, [_P, _LL, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_estimate_freq": (_I, [_P, _LL, _I, _I, _I, _P, _P, _c.c_size_t, _P]),
    "ofdm_frame_combine_freq": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_demod_freq_mfma": (_I, [_P, _LL, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_ls_partial": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_mrc_partial": (_I, [_P, _LL, _I, _I, _I, _I, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_mrc_partial_range": (_I, [_P, _LL, _LL, _LL, _I, _I, _I, _I, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_export_estimate": (_I, [_P, _c.c_size_t, _LL, _I, _I, _I, _LL, _P, _P, _P]),
    "ofdm_frame_estimate_denoise": (_I, [_P, _c.c_size_t, _LL, _I, _I, _I, _I, _I, _P]),
    "ofdm_frame_noise_estimate": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _I, _P, _P]),
    "ofdm_frame_soft_demap": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _I, _P, _I, _c.c_float, _P, _P]),
    "ofdm_symbols_demod": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _LL, _P, _P]),
    "ofdm_synth_frames": (_I, [_P, _LL, _I, _I, _I, _I, _P, _c.c_ulonglong, _LL, _c.c_float,
                               _I, _I, _P]),
    "ofdm_count_symbol_errors": (_I, [_P, _LL, _I, _I, _c.c_ulonglong, _LL, _P, _P]),
    "ofdm_pipeline_create": (_I, [_I, _I, _I, _I, _P, _I, _I, _c.POINTER(_P)]),
    "ofdm_pipeline_destroy": (_I, [_P]),
    "ofdm_pipeline_acquire": (_I, [_P, _c.POINTER(_P), _c.POINTER(_P)]),
    "ofdm_pipeline_submit": (_I, [_P, _LL, _P]),
    "ofdm_pipeline_demod": (_I, [_P, _P, _LL, _P]),
    "ofdm_pipeline_sync": (_I, [_P]),
    "ofdm_pipeline_set_denoise": (_I, [_P, _I, _I]),
    "ofdm_iq_convert_sc16": (_I, [_P, _LL, _c.c_float, _P, _P]),
    "ofdm_frame_demod_sc16": (_I, [_P, _LL, _I, _I, _I, _I, _c.c_float, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_estimate_sc16": (_I, [_P, _LL, _I, _I, _I, _I, _c.c_float, _P, _P, _c.c_size_t, _P]),
    "ofdm_frame_combine_sc16": (_I, [_P, _LL, _I, _I, _I, _I, _c.c_float, _P, _c.c_size_t, _P, _P]),
    "ofdm_pipeline_create_sc16": (_I, [_I, _I, _I, _I, _c.c_float, _P, _I, _I, _c.POINTER(_P)]),
    "ofdm_pipeline_acquire_sc16": (_I, [_P, _c.POINTER(_P), _c.POINTER(_P)]),
    "ofdm_pipeline_demod_sc16": (_I, [_P, _P, _LL, _P]),
    "ofdm_frame_cfo_estimate": (_I, [_P, _LL, _I, _I, _I, _I, _I, _P, _P, _P]),
    "ofdm_frame_cfo_derotate": (_I, [_P, _P, _LL, _I, _I, _I, _I, _P, _P]),
    "ofdm_frame_estimate_cfo": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P]),
    "ofdm_frame_combine_cfo": (_I, [_P, _LL, _I, _I, _I, _I, _P, _c.c_size_t, _P, _P, _P]),
    "ofdm_frame_demod_cfo": (_I, [_P, _LL, _I, _I, _I, _I, _P, _P, _c.c_size_t, _P, _P, _P]),
    "ofdm_pipeline_set_cfo": (_I, [_P, _I, _I]),
    "ofdm_frame_phase_track": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _I, _P, _P, _P]),
    "ofdm_pipeline_set_phase_track": (_I, [_P, _I]),
    "ofdm_host_register": (_I, [_P, _c.c_size_t]),
    "ofdm_host_unregister": (_I, [_P]),
    "ofdm_pn_correlate": (_I, [_P, _I, _LL, _P, _I, _c.c_float, _P, _P, _P]),
    "ofdm_pn_extract": (_I, [_P, _P, _I, _LL, _I, _P, _I, _I, _I, _P, _P]),
    "ofdm_zf_precoder": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "ofdm_zf_transpose": (_I, [_P, _I, _I, _I, _P, _P]),
    "ofdm_zf_apply": (_I, [_P, _P, _I, _I, _I, _LL, _P, _P]),
    "ofdm_zf_detect": (_I, [_P, _P, _I, _I, _I, _LL, _P, _P]),
    "ofdm_zf_detect_ex": (_I, [_P, _P, _LL, _I, _I, _I, _LL, _P, _LL, _P]),
    "ofdm_zf_apply_ex": (_I, [_P, _P, _LL, _I, _I, _I, _LL, _P, _LL, _P]),
    "ofdm_tx_modulate": (_I, [_P, _LL, _LL, _I, _I, _I, _I, _c.c_float, _P, _P, _P]),
    "ofdm_hbm_probe": (_I, [_I, _P, _P, _c.c_size_t, _c.c_size_t, _P]),
    "ofdm_device_status": (_I, []),
    "ofdm_device_status_inject": (_I, [_c.c_uint]),
    "ofdm_buffer_hash": (_I, [_P, _c.c_size_t, _P, _P]),
}

# include/ofdm_lsmrc_acquire.h (the same library; a table of its own, as the
# header is a header of its own until it is folded into the main one)
_SIGS_ACQUIRE = {
    "ofdm_frame_cfo_acquire": (_I, [_P, _LL, _I, _I, _I, _I, _P, _I, _c.c_float, _P, _P, _P, _P, _P]),
    "ofdm_pipeline_set_cfo_search": (_I, [_P, _I, _c.c_float]),
}
ACQ_MAX_SHIFT = 64  # OFDM_ACQ_MAX_SHIFT

# include/ofdm_lsmrc_timing.h (likewise)
_SIGS_TIMING = {
    "ofdm_frame_timing_track": (_I, [_P, _LL, _I, _I, _I, _P, _c.c_size_t, _I, _P, _P, _P, _P]),
    "ofdm_pipeline_set_timing_track": (_I, [_P, _I]),
}

# include/ofdm_lsmrc_decode.h (likewise)
_SIGS_DECODE = {
    "ofdm_conv_coded_len": (_I, [_P, _I, _c.POINTER(_LL)]),
    "ofdm_viterbi_workspace_bytes": (_I, [_P, _I, _LL, _c.POINTER(_c.c_size_t)]),
    "ofdm_viterbi_decode": (_I, [_P, _I, _c.c_float, _LL, _LL, _I, _P, _P, _LL, _P, _P, _c.c_size_t, _P]),
}

# include/ofdm_lsmrc_ldpc.h (likewise)
_SIGS_LDPC = {
    "ofdm_ldpc_code_create": (_I, [_P, _c.POINTER(_P)]),
    "ofdm_ldpc_code_destroy": (_I, [_P]),
    "ofdm_ldpc_workspace_bytes": (_I, [_P, _LL, _c.POINTER(_c.c_size_t)]),
    "ofdm_ldpc_decode": (_I, [_P, _I, _c.c_float, _LL, _LL, _P, _I, _I, _I, _I, _I, _I, _I, _P, _LL, _P, _P,
                              _c.c_size_t, _P]),
}


def _all_sigs():
    return (list(_SIGS.items()) + list(_SIGS_ACQUIRE.items()) + list(_SIGS_TIMING.items())
            + list(_SIGS_DECODE.items()) + list(_SIGS_LDPC.items()))

_lib = None


def build_id():
    """Identity of the product library's build: the first 16 hex digits of
    a SHA-256 over its sources (csrc/, the Makefile, include/ofdm_lsmrc.h,
    include/ofdm_lsmrc_acquire.h, include/ofdm_lsmrc_timing.h,
    include/ofdm_lsmrc_decode.h, include/ofdm_lsmrc_ldpc.h), in sorted order.
    PMC profiles record it
    (scripts/pmc_summary.py) and bench.py attaches a profile's traffic only to
    the build it measured."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(HERE, "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc))] + [os.path.join(HERE, "Makefile"), HEADER_PATH,
                                                                         ACQUIRE_HEADER_PATH, TIMING_HEADER_PATH,
                                                                         DECODE_HEADER_PATH, LDPC_HEADER_PATH]
    for f in files:
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode() + b"\0")
            with open(f, "rb") as fp:
                h.update(fp.read())
    return h.hexdigest()[:16]


class OfdmError(RuntimeError):
    pass


def lib():
    """Load libofdm_lsmrc.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OfdmError(f"{LIB_PATH} not built: run `make -C gpu-accel-ofdm-ls-mrc_amd` "
                            "(or __graft_entry__.build())")
        # One HIP runtime per process: torch's wheel bundles libamdhip64
        # (SONAME libamdhip64.so.7).  Loading torch first lets our NEEDED
        # libamdhip64.so.7 bind to that copy; loading ours first would pull
        # in /opt/rocm's and torch would then load a second runtime.
        import torch  # noqa: F401
        L = _c.CDLL(LIB_PATH)
        for name, (res, args) in _all_sigs():
            if _LIBSEL and not hasattr(L, name):
                continue  # an older variant build (OFDM_LSMRC_LIB): its missing entries fail when called
            fn = getattr(L, name)  # the product library: every entry, or AttributeError here
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def load_library(path):
    """Another build of this library (the diagnostic build, lib/
    libofdm_lsmrc_diag.so, or an A/B variant) loaded beside the product one,
    with the same signatures; call it through `using(L)`.  Its device state
    (workspace registry, flag epochs, twiddle tables) is its own."""
    import torch  # noqa: F401  (same HIP runtime as torch, see lib())
    L = _c.CDLL(path)
    for name, (res, args) in _all_sigs():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
    return L


class using:
    """with using(L): ... -- the binding's calls go to library L."""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        global _lib
        lib()
        self.prev, _lib = _lib, self.L
        return self.L

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def hbm_probe(mode, src, dst, stream=None):
    """Box probe: mode 0 copies src -> dst (float4), mode 1 reads src (dst:
    >= 1 MiB of partial sums).  Byte tensors on the device, 16-B multiples."""
    nbytes = src.numel() * src.element_size()
    _check(lib().ofdm_hbm_probe(mode, _dptr(src, "src"), _dptr(dst, "dst"), nbytes, dst.numel() * dst.element_size(),
                                _stream(stream)),
           "ofdm_hbm_probe")


def device_status():
    """Raises OfdmError (OFDM_E_DEVICE) if a ticketed launch reported a fault
    since the last check, and clears it (include/ofdm_lsmrc.h)."""
    _check(lib().ofdm_device_status(), "ofdm_device_status")


def _check(rc, fn):
    if rc < 0:
        msg = lib().ofdm_last_error().decode(errors="replace")
        raise OfdmError(f"{fn} failed ({rc}): {msg}")
    return rc


def _dptr(t, name="tensor"):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise OfdmError(f"{name} must be a device tensor")
    if not t.is_contiguous():
        raise OfdmError(f"{name} must be contiguous")
    return _P(t.data_ptr())


def _stream(stream):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    return _P(stream.cuda_stream)


def c64(shape, device="cuda"):
    import torch
    return torch.empty(shape, dtype=torch.complex64, device=device)


# ---------------------------------------------------------------- host side

def pilot_rotate(raw):
    raw = np.ascontiguousarray(raw, np.complex64)
    X = np.empty_like(raw)
    _check(lib().ofdm_pilot_rotate(raw.ctypes.data_as(_P), raw.size, X.ctypes.data_as(_P)),
           "ofdm_pilot_rotate")
    return X


def read_pilots(path, K, fill=0.707):
    """matrix_readX: returns (X, used_fill)."""
    X = np.empty(K, np.complex64)
    rc = _check(lib().ofdm_read_pilots(None if path is None else path.encode(), K, fill,
                                       X.ctypes.data_as(_P)), "ofdm_read_pilots")
    return X, rc == 1


# -------------------------------------------------------------- device side

def fft_rows(x, out=None, inverse=False, stream=None):
    C = x.shape[-1]
    nrows = x.numel() // C
    if out is None:
        out = x
    _check(lib().ofdm_fft_rows(_dptr(x, "x"), _dptr(out, "out"), nrows, C, int(inverse),
                               _stream(stream)), "ofdm_fft_rows")
    return out


def ls_estimate(Y, X, stream=None):
    """Y: (R, C) freq-domain pilot symbol, X: (K,) rotated pilots -> (Hconj (R,K), Hsqrd (K,))."""
    import torch
    R, C = Y.shape
    H = c64((R, C - 1), Y.device)
    P = torch.empty(C - 1, dtype=torch.float32, device=Y.device)
    _check(lib().ofdm_ls_estimate(_dptr(Y), _dptr(X), R, C, _dptr(H), _dptr(P), _stream(stream)),
           "ofdm_ls_estimate")
    return H, P


def mrc_demod(Y, H, P, stream=None):
    """Y: (nsyms, R, C) freq-domain data symbols -> (nsyms, K)."""
    n, R, C = Y.shape
    out = c64((n, C - 1), Y.device)
    _check(lib().ofdm_mrc_demod(_dptr(Y), n, _dptr(H), _dptr(P), R, C, _dptr(out),
                                _stream(stream)), "ofdm_mrc_demod")
    return out


def mrc_numerator(Y, H, stream=None):
    n, R, C = Y.shape
    out = c64((n, C - 1), Y.device)
    _check(lib().ofdm_mrc_numerator(_dptr(Y), n, _dptr(H), R, C, _dptr(out), _stream(stream)),
           "ofdm_mrc_numerator")
    return out


def mrc_finalize(num_chunk, e0, nsym, K, P, out, stream=None):
    _check(lib().ofdm_mrc_finalize(_dptr(num_chunk), e0, num_chunk.numel(), nsym, K, _dptr(P),
                                   _dptr(out), _stream(stream)), "ofdm_mrc_finalize")
    return out


def channel_conj_product(Y, H, stream=None):
    """multiplyWithChannelConj: Y (nsyms, R, C), H (R, K) -> (nsyms, R, K)."""
    n, R, C = Y.shape
    out = c64((n, R, C - 1), Y.device)
    _check(lib().ofdm_channel_conj_product(_dptr(Y), n, _dptr(H), R, C, _dptr(out),
                                           _stream(stream)), "ofdm_channel_conj_product")
    return out


def combine_products(prod, P, rotate=True, stream=None):
    """combineForMRC [+ shiftOneRow]: prod (nsyms, R, K) -> (nsyms, K)."""
    n, R, K = prod.shape
    out = c64((n, K), prod.device)
    _check(lib().ofdm_combine_products(_dptr(prod), n, _dptr(P), R, K, int(rotate), _dptr(out),
                                       _stream(stream)), "ofdm_combine_products")
    return out


def shift_rows(x, stream=None):
    K = x.shape[-1]
    out = c64(x.shape, x.device)
    _check(lib().ofdm_shift_rows(_dptr(x), x.numel() // K, K, _dptr(out), _stream(stream)),
           "ofdm_shift_rows")
    return out


def dist_sqrd(H, stream=None):
    import torch
    R, K = H.shape
    P = torch.empty(K, dtype=torch.float32, device=H.device)
    _check(lib().ofdm_dist_sqrd(_dptr(H), R, K, _dptr(P), _stream(stream)), "ofdm_dist_sqrd")
    return P


def workspace_bytes(nframes, S, R, C):
    return int(lib().ofdm_frame_workspace_bytes(nframes, S, R, C))


def workspace(nframes, S, R, C, device="cuda"):
    """A frame workspace.  When the tensor is collected its estimate tag is
    dropped from the library's registry (ofdm_workspace_release), so that a
    workspace the caching allocator later hands out at the same address is
    refused by combine / mrc_partial / export until an estimate fills it."""
    import torch
    import weakref
    ws = torch.empty(max(workspace_bytes(nframes, S, R, C), 256), dtype=torch.uint8, device=device)
    weakref.finalize(ws, lib().ofdm_workspace_release, _c.c_void_p(ws.data_ptr()))
    return ws


def workspace_release(ws):
    """Forget the estimate held in `ws` (a tensor or a raw device address)."""
    ptr = ws if isinstance(ws, int) else ws.data_ptr()
    lib().ofdm_workspace_release(_c.c_void_p(ptr))


FLOW_AUTO, FLOW_TWO_LAUNCH = 0, 1  # OFDM_FLOW_* of ofdm_frame_demod_ex


def frame_demod(iq, X, prefix=0, ws=None, out=None, stream=None, flow=None, spin_ticks=None):
    """iq: (F, S, R, C+prefix) time domain -> (F, S-1, K).  flow / spin_ticks:
    ofdm_frame_demod_ex's scheduling choices (default: ofdm_frame_demod's)."""
    F, S, R, Cp = iq.shape
    C = Cp - prefix
    if ws is None:
        ws = workspace(F, S, R, C, iq.device)
    if out is None:
        out = c64((F, S - 1, C - 1), iq.device)
    if flow is None and spin_ticks is None:
        _check(lib().ofdm_frame_demod(_dptr(iq), F, S, R, C, prefix, _dptr(X), _dptr(ws), ws.numel(),
                                      _dptr(out), _stream(stream)), "ofdm_frame_demod")
    else:
        _check(lib().ofdm_frame_demod_ex(_dptr(iq), F, S, R, C, prefix, _dptr(X), _dptr(ws), ws.numel(),
                                         _dptr(out), FLOW_AUTO if flow is None else flow,
                                         -1 if spin_ticks is None else spin_ticks, _stream(stream)),
               "ofdm_frame_demod_ex")
    return out


def frame_estimate(iq, X, prefix, ws, stream=None):
    """LS stage of frame_demod: estimates of every frame into the workspace."""
    F, S, R, Cp = iq.shape
    _check(lib().ofdm_frame_estimate(_dptr(iq), F, S, R, Cp - prefix, prefix, _dptr(X), _dptr(ws),
                                     ws.numel(), _stream(stream)), "ofdm_frame_estimate")
    return ws


def frame_combine(iq, prefix, ws, out, stream=None):
    """MRC stage of frame_demod against the estimates in the workspace."""
    F, S, R, Cp = iq.shape
    _check(lib().ofdm_frame_combine(_dptr(iq), F, S, R, Cp - prefix, prefix, _dptr(ws),
                                    ws.numel(), _dptr(out), _stream(stream)),
           "ofdm_frame_combine")
    return out


SC16_SCALE = 2.0 ** -15  # the power-of-two scale; UHD's own convention is 1 / 32767


def _sc16(t, name, ndim=None):
    """The device pointer of a torch.int16 tensor of sc16 samples (..., 2)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int16 or t.shape[-1] != 2:
        raise OfdmError(f"{name} must be a torch.int16 tensor whose last dimension is (re, im)")
    if ndim is not None and t.dim() != ndim:
        raise OfdmError(f"{name} must have {ndim} dimensions, not {t.dim()}")
    return _dptr(t, name)


def iq_convert_sc16(iq, scale=SC16_SCALE, out=None, stream=None):
    """sc16 samples (..., 2) torch.int16 -> complex64 (...): x = i16 * scale per
    component, one rounding (bit-exact).  The route to every fp32 entry for
    the FFT lengths without an sc16 receiver."""
    p = _sc16(iq, "iq")
    n = iq.numel() // 2
    if out is None:
        out = c64(tuple(iq.shape[:-1]), iq.device)
    _check(lib().ofdm_iq_convert_sc16(p if n else None, n, scale, _dptr(out, "out") if n else None, _stream(stream)),
           "ofdm_iq_convert_sc16")
    return out


def frame_demod_sc16(iq, X, prefix=0, scale=SC16_SCALE, ws=None, out=None, stream=None):
    """frame_demod on sc16 frames: iq (F, S, R, C+prefix, 2) torch.int16,
    x = i16 * scale -> (F, S-1, K).  C = 1024 (else convert, then frame_demod)."""
    p = _sc16(iq, "iq", 5)
    F, S, R, Cp, _ = iq.shape
    C = Cp - prefix
    if ws is None:
        ws = workspace(F, S, R, C, iq.device)
    if out is None:
        out = c64((F, S - 1, C - 1), iq.device)
    _check(lib().ofdm_frame_demod_sc16(p, F, S, R, C, prefix, scale, _dptr(X), _dptr(ws), ws.numel(), _dptr(out),
                                       _stream(stream)), "ofdm_frame_demod_sc16")
    return out


def frame_estimate_sc16(iq, X, prefix, ws, scale=SC16_SCALE, stream=None):
    """LS stage of frame_demod_sc16; the estimate in ws is in the units of
    x = i16 * scale and serves the fp32 consumers too."""
    p = _sc16(iq, "iq", 5)
    F, S, R, Cp, _ = iq.shape
    _check(lib().ofdm_frame_estimate_sc16(p, F, S, R, Cp - prefix, prefix, scale, _dptr(X), _dptr(ws), ws.numel(),
                                          _stream(stream)), "ofdm_frame_estimate_sc16")
    return ws


def frame_combine_sc16(iq, prefix, ws, out, scale=SC16_SCALE, stream=None):
    """MRC stage of frame_demod_sc16 against the estimate in ws (made by
    frame_estimate_sc16 or by the fp32 frame_estimate)."""
    p = _sc16(iq, "iq", 5)
    F, S, R, Cp, _ = iq.shape
    _check(lib().ofdm_frame_combine_sc16(p, F, S, R, Cp - prefix, prefix, scale, _dptr(ws), ws.numel(), _dptr(out),
                                         _stream(stream)), "ofdm_frame_combine_sc16")
    return out


def _eps(eps, F, name="eps"):
    """The device pointer of the per-frame offsets, float32 (F,)."""
    import torch
    if not isinstance(eps, torch.Tensor) or eps.dtype != torch.float32 or tuple(eps.shape) != (F,):
        raise OfdmError(f"{name} must be a torch.float32 tensor of shape ({F},)")
    return _dptr(eps, name) if F else None


def frame_cfo_estimate(iq, prefix, cp_skip=0, eps=None, gamma=None, stream=None):
    """Carrier frequency offset of every frame from its cyclic prefixes: iq
    (F, S, R, C+prefix) -> eps (F,) float32 in subcarrier spacings, in
    (-0.5, 0.5].  cp_skip: prefix samples left out at each symbol's head.
    gamma (F,) complex64, when given, receives the prefix correlations."""
    import torch
    F, S, R, Cp = iq.shape
    if eps is None:
        eps = torch.empty(F, dtype=torch.float32, device=iq.device)
    _check(lib().ofdm_frame_cfo_estimate(_dptr(iq, "iq") if F else None, F, S, R, Cp - prefix, prefix, cp_skip,
                                         None if gamma is None else _dptr(gamma, "gamma"), _eps(eps, F),
                                         _stream(stream)), "ofdm_frame_cfo_estimate")
    return eps


def frame_cfo_acquire(iq, X, prefix, max_shift, eps=None, min_ratio=2.0, out=None, shift=None, metric=None,
                      stream=None):
    """The integer part of every frame's carrier frequency offset from its
    pilot symbol (include/ofdm_lsmrc_acquire.h): iq (F, S, R, C+prefix), X the
    K rotated pilots, eps (F,) float32 the fractional estimate (None: 0) ->
    out (F,) float32 = eps + the shift in [-max_shift, max_shift] whose pilot
    differential correlation is largest, 0 where it is less than min_ratio
    times the runner-up.  out=eps works in place.  shift (F,) int32 and metric
    (F, 2 max_shift + 1) float32, when given, receive the shifts and the
    ungated correlation magnitudes."""
    import torch
    F, S, R, Cp = iq.shape
    if out is None:
        out = torch.empty(F, dtype=torch.float32, device=iq.device)
    if shift is not None and (shift.dtype != torch.int32 or tuple(shift.shape) != (F,)):
        raise OfdmError(f"shift must be a torch.int32 tensor of shape ({F},)")
    if metric is not None and (metric.dtype != torch.float32 or tuple(metric.shape) != (F, 2 * max_shift + 1)):
        raise OfdmError(f"metric must be a torch.float32 tensor of shape ({F}, {2 * max_shift + 1})")
    opt = lambda t, name: None if t is None or not F else _dptr(t, name)
    _check(lib().ofdm_frame_cfo_acquire(_dptr(iq, "iq") if F else None, F, S, R, Cp - prefix, prefix, _dptr(X, "X"),
                                        max_shift, min_ratio, None if eps is None else _eps(eps, F),
                                        _eps(out, F, "out"), opt(shift, "shift"), opt(metric, "metric"),
                                        _stream(stream)), "ofdm_frame_cfo_acquire")
    return out


def frame_cfo_derotate(iq, prefix, eps, out=None, stream=None):
    """x' = iq e^{-2 pi i eps_f m / C} over whole frames (m: the sample's index
    in its frame and antenna row, prefix included); out=iq works in place.
    The route to the fp32 entries for every C but 1024 (frame_demod_cfo)."""
    F, S, R, Cp = iq.shape
    if out is None:
        out = c64(tuple(iq.shape), iq.device)
    _check(lib().ofdm_frame_cfo_derotate(_dptr(iq, "iq") if F else None, _dptr(out, "out") if F else None, F, S, R,
                                         Cp - prefix, prefix, _eps(eps, F), _stream(stream)),
           "ofdm_frame_cfo_derotate")
    return out


def frame_demod_cfo(iq, X, prefix, eps, ws=None, out=None, stream=None):
    """frame_demod (two launches) on the frames derotated by eps (F,) float32,
    the rotation applied as each row is loaded.  C = 1024 (else
    frame_cfo_derotate, then frame_demod)."""
    F, S, R, Cp = iq.shape
    C = Cp - prefix
    if ws is None:
        ws = workspace(F, S, R, C, iq.device)
    if out is None:
        out = c64((F, S - 1, C - 1), iq.device)
    _check(lib().ofdm_frame_demod_cfo(_dptr(iq), F, S, R, C, prefix, _dptr(X), _dptr(ws), ws.numel(), _dptr(out),
                                      _eps(eps, F), _stream(stream)), "ofdm_frame_demod_cfo")
    return out


def frame_estimate_cfo(iq, X, prefix, ws, eps, stream=None):
    """LS stage of frame_demod_cfo: the estimate of the derotated frames, for
    every consumer of a workspace estimate."""
    F, S, R, Cp = iq.shape
    _check(lib().ofdm_frame_estimate_cfo(_dptr(iq), F, S, R, Cp - prefix, prefix, _dptr(X), _dptr(ws), ws.numel(),
                                         _eps(eps, F), _stream(stream)), "ofdm_frame_estimate_cfo")
    return ws


def frame_combine_cfo(iq, prefix, ws, out, eps, stream=None):
    """MRC stage of frame_demod_cfo against the estimate in ws."""
    F, S, R, Cp = iq.shape
    _check(lib().ofdm_frame_combine_cfo(_dptr(iq), F, S, R, Cp - prefix, prefix, _dptr(ws), ws.numel(), _dptr(out),
                                        _eps(eps, F), _stream(stream)), "ofdm_frame_combine_cfo")
    return out


def symbols_demod(sym, ws, prefix=0, frame=0, out=None, stream=None):
    """sym: (nsym, R, C+prefix) time-domain data symbols -> (nsym, K), against
    frame `frame`'s estimate in ws (filled by frame_estimate)."""
    n, R, Cp = sym.shape
    C = Cp - prefix
    if out is None:
        out = c64((n, C - 1), sym.device)
    _check(lib().ofdm_symbols_demod(_dptr(sym), n, R, C, prefix, _dptr(ws), ws.numel(), frame, _dptr(out),
                                    _stream(stream)), "ofdm_symbols_demod")
    return out


def frame_demod_freq(Y, X, ws=None, out=None, stream=None):
    """Y: (F, S, R, C) frequency domain -> (F, S-1, K)."""
    F, S, R, C = Y.shape
    if ws is None:
        ws = workspace(F, S, R, C, Y.device)
    if out is None:
        out = c64((F, S - 1, C - 1), Y.device)
    _check(lib().ofdm_frame_demod_freq(_dptr(Y), F, S, R, C, _dptr(X), _dptr(ws), ws.numel(),
                                       _dptr(out), _stream(stream)), "ofdm_frame_demod_freq")
    return out


def frame_estimate_freq(Y, X, ws, stream=None):
    """LS stage of frame_demod_freq: estimates of every frame into the workspace."""
    F, S, R, C = Y.shape
    _check(lib().ofdm_frame_estimate_freq(_dptr(Y), F, S, R, C, _dptr(X), _dptr(ws), ws.numel(),
                                          _stream(stream)), "ofdm_frame_estimate_freq")
    return ws


def frame_combine_freq(Y, ws, out, stream=None):
    """MRC stage of frame_demod_freq against the estimates in the workspace."""
    F, S, R, C = Y.shape
    _check(lib().ofdm_frame_combine_freq(_dptr(Y), F, S, R, C, _dptr(ws), ws.numel(), _dptr(out),
                                         _stream(stream)), "ofdm_frame_combine_freq")
    return out


def frame_demod_freq_mfma(Y, X, ws=None, out=None, stream=None):
    """frame_demod_freq with the antenna combine on the matrix cores."""
    F, S, R, C = Y.shape
    if ws is None:
        ws = workspace(F, S, R, C, Y.device)
    if out is None:
        out = c64((F, S - 1, C - 1), Y.device)
    _check(lib().ofdm_frame_demod_freq_mfma(_dptr(Y), F, S, R, C, _dptr(X), _dptr(ws), ws.numel(),
                                            _dptr(out), _stream(stream)), "ofdm_frame_demod_freq_mfma")
    return out


def frame_ls_partial(iq, X, prefix=0, ws=None, P=None, stream=None):
    import torch
    F, S, R, Cp = iq.shape
    C = Cp - prefix
    if ws is None:
        ws = workspace(F, S, R, C, iq.device)
    if P is None:
        P = torch.empty((F, C - 1), dtype=torch.float32, device=iq.device)
    _check(lib().ofdm_frame_ls_partial(_dptr(iq), F, S, R, C, prefix, _dptr(X), _dptr(ws),
                                       ws.numel(), _dptr(P), _stream(stream)),
           "ofdm_frame_ls_partial")
    return P, ws


def frame_mrc_partial(iq, ws, prefix=0, num=None, stream=None):
    F, S, R, Cp = iq.shape
    C = Cp - prefix
    if num is None:
        num = c64((F, S - 1, C - 1), iq.device)
    _check(lib().ofdm_frame_mrc_partial(_dptr(iq), F, S, R, C, prefix, _dptr(ws), ws.numel(),
                                        _dptr(num), _stream(stream)), "ofdm_frame_mrc_partial")
    return num


def frame_mrc_partial_range(iq, ws, prefix, f0, count, num=None, stream=None):
    """Partial MRC numerators of frames [f0, f0 + count) of the batch `iq`
    whose estimate one frame_ls_partial call left in `ws`."""
    F, S, R, Cp = iq.shape
    C = Cp - prefix
    if num is None:
        num = c64((count, S - 1, C - 1), iq.device)
    _check(lib().ofdm_frame_mrc_partial_range(_dptr(iq), F, f0, count, S, R, C, prefix, _dptr(ws), ws.numel(),
                                              _dptr(num), _stream(stream)), "ofdm_frame_mrc_partial_range")
    return num


def frame_export_estimate(ws, F, S, R, C, frame=0, stream=None):
    """Frame `frame`'s estimate in the reference layout: (Hconj (R, K), Hsqrd (K,))."""
    import torch
    H = c64((R, C - 1), ws.device)
    P = torch.empty(C - 1, dtype=torch.float32, device=ws.device)
    _check(lib().ofdm_frame_export_estimate(_dptr(ws), ws.numel(), F, S, R, C, frame, _dptr(H), _dptr(P),
                                            _stream(stream)), "ofdm_frame_export_estimate")
    return H, P


def frame_estimate_denoise(ws, F, S, R, C, taps_post, taps_pre=0, stream=None):
    """Delay-domain denoising of the estimate in ws (any full estimate of this
    F, S, R, C), in place: the taps [0, taps_post) and [C - taps_pre, C) of
    every antenna's channel are kept, the rest zeroed (include/ofdm_lsmrc.h)."""
    _check(lib().ofdm_frame_estimate_denoise(_dptr(ws, "ws") if F else None, ws.numel() if F else 0, F, S, R, C,
                                             taps_post, taps_pre, _stream(stream)), "ofdm_frame_estimate_denoise")
    return ws


MOD_QPSK, MOD_QAM16, MOD_QAM64, MOD_QAM256 = 2, 4, 6, 8  # OFDM_MOD_*: bits per symbol
_LLR_FORMATS = {"f32": 0, "i8": 1}  # OFDM_LLR_*


def frame_noise_estimate(z, ws, F, S, R, C, modulation, out=None, stream=None):
    """Decision-directed noise variance of every frame, (F,) float32: the mean
    of P |Z - slice(Z)|^2 over the frame's demodulated symbols z (F, S-1, K),
    P from the estimate in ws (any full estimate of this F, S, R, C)."""
    import torch
    if out is None:
        out = torch.empty(F, dtype=torch.float32, device=z.device)
    _check(lib().ofdm_frame_noise_estimate(_dptr(z, "z"), F, S, R, C, _dptr(ws, "ws"), ws.numel(), modulation,
                                           _dptr(out, "out"), _stream(stream)), "ofdm_frame_noise_estimate")
    return out


def frame_soft_demap(z, ws, F, S, R, C, modulation, noise_var, fmt="f32", scale=1.0, out=None, stream=None):
    """Max-log LLRs of the demodulated symbols z (F, S-1, K) -> (F, S-1, K, bps),
    float32 (fmt "f32") or int8 clamp(rint(llr * scale), -127, 127) (fmt "i8");
    llr > 0 <=> bit 0.  noise_var: (F,) float32 on the device."""
    import torch
    if fmt not in _LLR_FORMATS:
        raise OfdmError(f"fmt must be 'f32' or 'i8', not {fmt!r}")
    if out is None:
        out = torch.empty((F, S - 1, C - 1, modulation), dtype=torch.float32 if fmt == "f32" else torch.int8,
                          device=z.device)
    _check(lib().ofdm_frame_soft_demap(_dptr(z, "z"), F, S, R, C, _dptr(ws, "ws"), ws.numel(), modulation,
                                       _dptr(noise_var, "noise_var"), _LLR_FORMATS[fmt], scale, _dptr(out, "out"),
                                       _stream(stream)), "ofdm_frame_soft_demap")
    return out


def frame_phase_track(z, ws, F, S, R, C, modulation, out=None, phase=None, stream=None):
    """Decision-directed phase tracking of the demodulated symbols z
    (F, S-1, K) -> the derotated (F, S-1, K); out=z works in place.  P comes
    from the estimate in ws (any full estimate of this F, S, R, C).  phase
    (F, S-1) float32, when given, receives the tracked phase of every data
    symbol in radians, unwrapped (include/ofdm_lsmrc.h, "phase tracking")."""
    return _track("ofdm_frame_phase_track", z, ws, F, S, R, C, modulation, out, stream, phase=phase)


def _track(entry, z, ws, F, S, R, C, modulation, out, stream, **per_symbol):
    """frame_phase_track and frame_timing_track: the entry's optional (F, S-1)
    float32 outputs by name, in the entry's order."""
    import torch
    if out is None:
        out = c64((F, S - 1, C - 1), z.device)
    for name, t in per_symbol.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32
                              or tuple(t.shape) != (F, S - 1)):
            raise OfdmError(f"{name} must be a torch.float32 tensor of shape ({F}, {S - 1})")
    outs = [_dptr(t, name) if F and t is not None else None for name, t in per_symbol.items()]
    _check(getattr(lib(), entry)(_dptr(z, "z") if F else None, F, S, R, C, _dptr(ws, "ws") if F else None,
                                 ws.numel() if F else 0, modulation, _dptr(out, "out") if F else None, *outs,
                                 _stream(stream)), entry)
    return out


def residual_cfo(phase, C, prefix):
    """The carrier frequency offset a frame's tracked phases show, per frame, in
    subcarrier spacings: the least-squares slope through the origin of
    theta over n' = 1 .. S-1 (the pilot is phase 0), sum n' theta / sum n'^2,
    times C / (2 pi (C + prefix)).  phase: (F, S-1) torch tensor or numpy
    array, as frame_phase_track wrote it; the result is of the same kind,
    float64.  No kernel."""
    k = C / (2.0 * np.pi * (C + prefix))
    if isinstance(phase, np.ndarray):
        n = np.arange(1, phase.shape[-1] + 1, dtype=np.float64)
        return (phase.astype(np.float64) * n).sum(-1) / (n * n).sum() * k
    import torch
    n = torch.arange(1, phase.shape[-1] + 1, dtype=torch.float64, device=phase.device)
    return (phase.to(torch.float64) * n).sum(-1) / (n * n).sum() * k


def frame_timing_track(z, ws, F, S, R, C, modulation, out=None, phase=None, timing=None, stream=None):
    """Decision-directed tracking of the common phase and the timing drift of
    the demodulated symbols z (F, S-1, K) -> the corrected (F, S-1, K); out=z
    works in place.  P comes from the estimate in ws, as for
    frame_phase_track.  phase and timing (F, S-1) float32, when given, receive
    every data symbol's tracked phase (radians, unwrapped) and window offset
    against the pilot's (samples) (include/ofdm_lsmrc_timing.h)."""
    return _track("ofdm_frame_timing_track", z, ws, F, S, R, C, modulation, out, stream, phase=phase, timing=timing)


def sampling_offset(timing, C, prefix):
    """The sampling clock offset a frame's tracked timing shows, per frame, as
    a fraction (1e-6 is one ppm): the least-squares slope through the origin
    of tau over n' = 1 .. S-1 (the pilot is offset 0), sum n' tau / sum n'^2,
    in samples per symbol, over the C + prefix samples of a symbol.  timing:
    (F, S-1) torch tensor or numpy array, as frame_timing_track wrote it; the
    result is of the same kind, float64.  The twin of residual_cfo.  No kernel."""
    if isinstance(timing, np.ndarray):
        n = np.arange(1, timing.shape[-1] + 1, dtype=np.float64)
        return (timing.astype(np.float64) * n).sum(-1) / (n * n).sum() / (C + prefix)
    import torch
    n = torch.arange(1, timing.shape[-1] + 1, dtype=torch.float64, device=timing.device)
    return (timing.to(torch.float64) * n).sum(-1) / (n * n).sum() / (C + prefix)


class ConvCode(_c.Structure):
    """ofdm_conv_code (include/ofdm_lsmrc_decode.h): a constraint-length-7
    convolutional code, its termination and its puncturing."""
    _fields_ = [("n_out", _I), ("g", _I * 3), ("terminated", _I), ("punct_period", _I), ("punct_mask", _c.c_uint)]

    def __init__(self, n_out, g, terminated=True, punct_period=0, punct_mask=0):
        g = list(g) + [0] * (3 - len(g))
        super().__init__(n_out, (_I * 3)(*g), int(bool(terminated)), punct_period, punct_mask)

    @classmethod
    def k7_rate_half(cls, terminated=True):
        """0133 / 0171 (octal): the 802.11 / DVB / CCSDS code."""
        return cls(2, (0o133, 0o171), terminated)

    @classmethod
    def k7_rate_third(cls, terminated=True):
        return cls(3, (0o133, 0o171, 0o165), terminated)

    @classmethod
    def wifi_2_3(cls, terminated=True):
        """802.11 rate 2/3: of every two steps' four coded bits the last is not sent."""
        return cls(2, (0o133, 0o171), terminated, 2, 0x7)

    @classmethod
    def wifi_3_4(cls, terminated=True):
        """802.11 rate 3/4: of every three steps' six coded bits, bits 3 and 4 are not sent."""
        return cls(2, (0o133, 0o171), terminated, 3, 0x27)


def conv_coded_len(code, L):
    """n_rx: the LLRs a codeword of L information bits has (host arithmetic)."""
    n = _LL(0)
    _check(lib().ofdm_conv_coded_len(_c.byref(code), L, _c.byref(n)), "ofdm_conv_coded_len")
    return n.value


def viterbi_workspace_bytes(code, L, ncw):
    n = _c.c_size_t(0)
    _check(lib().ofdm_viterbi_workspace_bytes(_c.byref(code), L, ncw, _c.byref(n)), "ofdm_viterbi_workspace_bytes")
    return n.value


def viterbi_decode(llr, code, L, ncw=None, stride=None, scale=1.0, out=None, out_stride=None, metric=None, ws=None,
                   stream=None):
    """Viterbi decoding of ncw codewords of L information bits each
    (include/ofdm_lsmrc_decode.h) -> (bits uint8 [ncw, out_stride], packed,
    bit t of a codeword in bit t & 7 of byte t >> 3; metric int32 [ncw]).
    llr: a device tensor, int8 (OFDM_LLR_I8) or float32 (OFDM_LLR_F32,
    quantised with `scale`); 2-D (ncw, stride), or flat with ncw and stride
    (default: n_rx) given: codeword c begins at element c * stride.  ws: a byte
    tensor of viterbi_workspace_bytes (made here if absent and needed)."""
    import torch
    if not isinstance(llr, torch.Tensor) or llr.dtype not in (torch.int8, torch.float32):
        raise OfdmError("llr must be a torch.int8 or torch.float32 device tensor")
    n_rx = conv_coded_len(code, L)
    if llr.dim() == 2 and ncw is None and stride is None:
        ncw, stride = llr.shape
    if stride is None:
        stride = n_rx
    if ncw is None:
        ncw = 0 if llr.numel() < n_rx else (llr.numel() - n_rx) // stride + 1
    if ncw > 0 and llr.numel() < (ncw - 1) * stride + n_rx:
        raise OfdmError(f"llr holds {llr.numel()} elements, {ncw} codewords at stride {stride} need "
                        f"{(ncw - 1) * stride + n_rx}")
    nbytes = (L + 7) // 8
    if out_stride is None:
        out_stride = out.shape[-1] if out is not None and out.dim() == 2 else nbytes
    if out is None:
        out = torch.empty((ncw, out_stride), dtype=torch.uint8, device=llr.device)
    elif out.dtype != torch.uint8 or (ncw > 0 and out.numel() < (ncw - 1) * out_stride + min(nbytes, out_stride)):
        raise OfdmError(f"out must be a torch.uint8 tensor of {ncw} rows of {out_stride} bytes")
    if metric is None:
        metric = torch.empty(ncw, dtype=torch.int32, device=llr.device)
    elif metric.dtype != torch.int32 or metric.numel() < ncw:
        raise OfdmError(f"metric must be a torch.int32 tensor of {ncw} elements")
    need = viterbi_workspace_bytes(code, L, ncw)
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device=llr.device)
    live = ncw > 0
    _check(lib().ofdm_viterbi_decode(_dptr(llr, "llr") if live else None, 1 if llr.dtype == torch.int8 else 0, scale,
                                     stride, ncw, L, _c.byref(code), _dptr(out, "out") if live else None, out_stride,
                                     _dptr(metric, "metric") if live else None,
                                     _dptr(ws, "ws") if ws is not None and ws.numel() else None,
                                     ws.numel() if ws is not None else 0, _stream(stream)), "ofdm_viterbi_decode")
    return out, metric


class QcLdpcDesc(_c.Structure):
    """ofdm_qc_ldpc (include/ofdm_lsmrc_ldpc.h): the base matrix as the C entry takes it."""
    _fields_ = [("mb", _I), ("nb", _I), ("Z", _I), ("row_ptr", _c.POINTER(_I)), ("col", _c.POINTER(_I)),
                ("shift", _c.POINTER(_I))]


class QcLdpc:
    """A quasi-cyclic LDPC code and the owner of its ofdm_ldpc_code_t handle.
    rows: one list per base row of (column, shift) pairs, columns strictly
    increasing; entry (c, s) of row r connects check r Z + i to variable
    c Z + (i + s) mod Z.  The handle is destroyed with the object (close())."""

    def __init__(self, mb, nb, Z, rows):
        rows = [list(r) for r in rows]
        if len(rows) != mb:
            raise OfdmError(f"{len(rows)} rows given for mb={mb}")
        self.mb, self.nb, self.Z, self.rows = mb, nb, Z, rows
        self.N, self.M = nb * Z, mb * Z
        ptr = [0]
        for r in rows:
            ptr.append(ptr[-1] + len(r))
        self.nnz = ptr[-1]
        self._arrays = ((_I * (mb + 1))(*ptr), (_I * max(self.nnz, 1))(*[c for r in rows for c, _ in r]),
                        (_I * max(self.nnz, 1))(*[s for r in rows for _, s in r]))
        self.desc = QcLdpcDesc(mb, nb, Z, *[_c.cast(a, _c.POINTER(_I)) for a in self._arrays])
        self.handle = _P(None)
        _check(lib().ofdm_ldpc_code_create(_c.byref(self.desc), _c.byref(self.handle)), "ofdm_ldpc_code_create")

    def close(self):
        if self.handle is not None and self.handle.value:
            lib().ofdm_ldpc_code_destroy(self.handle)
            self.handle = _P(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ldpc_workspace_bytes(code, ncw):
    n = _c.c_size_t(0)
    _check(lib().ofdm_ldpc_workspace_bytes(code.handle, ncw, _c.byref(n)), "ofdm_ldpc_workspace_bytes")
    return n.value


def ldpc_decode(llr, code, ncw=None, stride=None, scale=1.0, pos0=0, n_rx=None, max_iter=20, norm16=12, offset=0,
                early_stop=True, n_bits=None, out=None, out_stride=None, iters=None, ws=None, stream=None):
    """Layered min-sum decoding of ncw codewords of the QcLdpc `code`
    (include/ofdm_lsmrc_ldpc.h) -> (bits uint8 [ncw, out_stride], packed, bit t
    of a codeword in bit t & 7 of byte t >> 3; iters int32 [ncw], +k: zero
    syndrome after k iterations, -k: not).  llr: a device tensor, int8
    (OFDM_LLR_I8) or float32 (OFDM_LLR_F32, quantised with `scale`); 2-D
    (ncw, stride), or flat with ncw and stride (default: n_rx) given: codeword
    c begins at element c * stride and holds positions pos0 .. pos0 + n_rx - 1
    (n_rx defaults to the rest of the codeword, or to a 2-D llr's row where that
    is shorter).  n_bits defaults to N.  ws: a byte tensor of
    ldpc_workspace_bytes (made here if absent and needed)."""
    import torch
    if not isinstance(llr, torch.Tensor) or llr.dtype not in (torch.int8, torch.float32):
        raise OfdmError("llr must be a torch.int8 or torch.float32 device tensor")
    two_d = llr.dim() == 2 and ncw is None and stride is None
    if two_d:
        ncw, stride = llr.shape
    if n_rx is None:
        n_rx = code.N - pos0
        if two_d:
            n_rx = min(n_rx, stride)
    if stride is None:
        stride = n_rx
    if ncw is None:
        ncw = 0 if llr.numel() < n_rx else (llr.numel() - n_rx) // stride + 1
    if ncw > 0 and llr.numel() < (ncw - 1) * stride + n_rx:
        raise OfdmError(f"llr holds {llr.numel()} elements, {ncw} codewords at stride {stride} need "
                        f"{(ncw - 1) * stride + n_rx}")
    if n_bits is None:
        n_bits = code.N
    nbytes = (n_bits + 7) // 8
    if out_stride is None:
        out_stride = out.shape[-1] if out is not None and out.dim() == 2 else nbytes
    if out is None:
        out = torch.empty((ncw, out_stride), dtype=torch.uint8, device=llr.device)
    elif out.dtype != torch.uint8 or (ncw > 0 and out.numel() < (ncw - 1) * out_stride + min(nbytes, out_stride)):
        raise OfdmError(f"out must be a torch.uint8 tensor of {ncw} rows of {out_stride} bytes")
    if iters is None:
        iters = torch.empty(ncw, dtype=torch.int32, device=llr.device)
    elif iters.dtype != torch.int32 or iters.numel() < ncw:
        raise OfdmError(f"iters must be a torch.int32 tensor of {ncw} elements")
    need = ldpc_workspace_bytes(code, ncw)
    if ws is None and need:
        ws = torch.empty(need, dtype=torch.uint8, device=llr.device)
    live = ncw > 0
    _check(lib().ofdm_ldpc_decode(_dptr(llr, "llr") if live else None, 1 if llr.dtype == torch.int8 else 0, scale, stride,
                                  ncw, code.handle, pos0, n_rx, max_iter, norm16, offset, int(bool(early_stop)), n_bits,
                                  _dptr(out, "out") if live else None, out_stride,
                                  _dptr(iters, "iters") if live else None,
                                  _dptr(ws, "ws") if ws is not None and ws.numel() else None,
                                  ws.numel() if ws is not None else 0, _stream(stream)), "ofdm_ldpc_decode")
    return out, iters


def synth_frames(F, S, R, C, X, prefix=0, seed=1234, frame0=0, noise_std=0.01,
                 freq_domain=False, r0=0, out=None, stream=None):
    Cp = C if freq_domain else C + prefix
    if out is None:
        out = c64((F, S, R, Cp), X.device)
    _check(lib().ofdm_synth_frames(_dptr(out), F, S, R, C, prefix, _dptr(X), seed, frame0,
                                   noise_std, int(freq_domain), r0, _stream(stream)),
           "ofdm_synth_frames")
    return out


def count_symbol_errors(out, S, seed=1234, frame0=0, stream=None):
    import torch
    F = out.shape[0]
    K = out.shape[-1]
    err = torch.zeros(1, dtype=torch.int64, device=out.device)
    _check(lib().ofdm_count_symbol_errors(_dptr(out), F, S, K + 1, seed, frame0, _dptr(err),
                                          _stream(stream)), "ofdm_count_symbol_errors")
    return err


def pn_correlate(buf, pn, thres, mag=False, stream=None):
    """PN frame sync (rx_and_corr.cpp:332-360): buf (R, N), pn (L,) device
    complex64 -> (pos, mag): pos = device int64 tensor [ch*(N-L+1) + lag] or
    [-1]; mag = (R, N-L+1) float32 |corr|/L for every lag if requested."""
    import torch
    R, N = buf.shape
    L = pn.shape[0]
    pos = torch.empty(1, dtype=torch.int64, device=buf.device)
    m = torch.empty((R, max(N - L + 1, 0)), dtype=torch.float32, device=buf.device) if mag else None
    _check(lib().ofdm_pn_correlate(_dptr(buf), R, N, _dptr(pn), L, thres, _dptr(pos),
                                   _dptr(m) if mag else None, _stream(stream)),
           "ofdm_pn_correlate")
    return pos, m


def pn_extract(buf1, buf2, L, pos, C, cp, nsym, out=None, stream=None):
    """Frame after the PN (rx_and_corr.cpp:370-392 + copy_to_shared_mem):
    -> (nsym, R, C) symbols, cyclic prefix dropped."""
    R, N = buf1.shape
    if out is None:
        out = c64((nsym, R, C), buf1.device)
    _check(lib().ofdm_pn_extract(_dptr(buf1), _dptr(buf2), R, N, L, _dptr(pos), C, cp, nsym,
                                 _dptr(out), _stream(stream)), "ofdm_pn_extract")
    return out


def _opt_ptr(t, name):
    return None if t is None else _dptr(t, name)


def zf_precoder(H, W=True, Wt=True, stream=None):
    """createZeroForcingMatrix (cpuLS.hpp:415-447): H (U, R, K) device
    complex64 -> (W (K, U, R) reference layout or None, Wt (U, R, K) or None)."""
    U, R, K = H.shape
    W = c64((K, U, R), H.device) if W is True else (None if W is False else W)
    Wt = c64((U, R, K), H.device) if Wt is True else (None if Wt is False else Wt)
    _check(lib().ofdm_zf_precoder(_dptr(H, "H"), U, R, K, _opt_ptr(W, "W"), _opt_ptr(Wt, "Wt"),
                                  _stream(stream)), "ofdm_zf_precoder")
    return W, Wt


def zf_transpose(W, stream=None):
    """(K, U, R) reference layout -> (U, R, K)."""
    K, U, R = W.shape
    Wt = c64((U, R, K), W.device)
    _check(lib().ofdm_zf_transpose(_dptr(W, "W"), U, R, K, _dptr(Wt, "Wt"), _stream(stream)),
           "ofdm_zf_transpose")
    return Wt


def zf_apply(Wt, X, out=None, stream=None):
    """multiplyWithChannelInv (cpuLS.hpp:449-463) over symbols: X (nsym, U, K) -> (nsym, R, K)."""
    U, R, K = Wt.shape
    n = X.shape[0]
    assert tuple(X.shape) == (n, U, K), X.shape
    if out is None:
        out = c64((n, R, K), X.device)
    _check(lib().ofdm_zf_apply(_dptr(Wt, "Wt"), _dptr(X, "X"), U, R, K, n, _dptr(out, "out"),
                               _stream(stream)), "ofdm_zf_apply")
    return out


def zf_detect(Wt, Y, out=None, stream=None):
    """ZF detection with the same matrix: Y (nsym, R, K) -> (nsym, U, K)."""
    U, R, K = Wt.shape
    n = Y.shape[0]
    assert tuple(Y.shape) == (n, R, K), Y.shape
    if out is None:
        out = c64((n, U, K), Y.device)
    _check(lib().ofdm_zf_detect(_dptr(Wt, "Wt"), _dptr(Y, "Y"), U, R, K, n, _dptr(out, "out"),
                                _stream(stream)), "ofdm_zf_detect")
    return out


def zf_apply_pitched(Wt, X, out=None, ldy=None, stream=None):
    """ofdm_zf_apply_ex: X (nsym, U, ldx) with rows padded to ldx >= K -> out
    (nsym, R, ldy), first K columns written (ldy default: ldx)."""
    U, R, K = Wt.shape
    n, u, ldx = X.shape
    assert u == U and ldx >= K, X.shape
    if out is None:
        out = c64((n, R, ldy or ldx), X.device)
    assert out.shape[0] == n and out.shape[1] == R and out.shape[2] >= K, out.shape
    _check(lib().ofdm_zf_apply_ex(_dptr(Wt, "Wt"), _dptr(X, "X"), ldx, U, R, K, n, _dptr(out, "out"),
                                  out.shape[2], _stream(stream)), "ofdm_zf_apply_ex")
    return out


def zf_detect_pitched(Wt, Y, out=None, ldx=None, stream=None):
    """ofdm_zf_detect_ex: Y (nsym, R, ldy) with rows padded to ldy >= K (only
    the first K columns read) -> out (nsym, U, ldx), first K columns written
    (ldx default: ldy)."""
    U, R, K = Wt.shape
    n, r, ldy = Y.shape
    assert r == R and ldy >= K, Y.shape
    if out is None:
        out = c64((n, U, ldx or ldy), Y.device)
    assert out.shape[0] == n and out.shape[1] == U and out.shape[2] >= K, out.shape
    _check(lib().ofdm_zf_detect_ex(_dptr(Wt, "Wt"), _dptr(Y, "Y"), ldy, U, R, K, n, _dptr(out, "out"),
                                   out.shape[2], _stream(stream)), "ofdm_zf_detect_ex")
    return out


TX_MAPS = {"reference": 0, "rx": 1}  # OFDM_TX_MAP_*
TX_NORMS = {"peak": 0, "scale": 1}  # OFDM_TX_NORM_*


def tx_modulate(X, C, cp=0, map="rx", norm="scale", scale=1.0, ldx=None, return_peak=False, out=None, stream=None):
    """OFDM modulator (modOneSymbol / modRefSymbol, cpuLS.hpp:466-529, one pass
    per row): X (..., ldx) device complex64, the first K = C - 1 values of
    every row used (ldx default: X's last dimension) -> iq (..., C + cp), each
    row's cyclic prefix first.  map "reference" (modOneSymbol's bin placement)
    or "rx" (the placement the receivers undo); norm "peak" (row / max|row|)
    or "scale" (row * scale).  return_peak: also the (...,) float32 peaks
    max_n |x[n]| before scaling."""
    import torch
    if map not in TX_MAPS or norm not in TX_NORMS:
        raise OfdmError(f"map must be one of {sorted(TX_MAPS)} and norm one of {sorted(TX_NORMS)}")
    if ldx is None:
        ldx = X.shape[-1]
    if X.shape[-1] != ldx:
        raise OfdmError(f"X's last dimension is {X.shape[-1]}, not ldx={ldx}")
    lead = tuple(X.shape[:-1])
    nrows = X.numel() // ldx if ldx else 0
    if out is None:
        out = c64(lead + (C + cp,), X.device)
    peak = torch.empty(lead, dtype=torch.float32, device=X.device) if return_peak else None
    _check(lib().ofdm_tx_modulate(_dptr(X, "X") if nrows else None, ldx, nrows, C, cp, TX_MAPS[map], TX_NORMS[norm],
                                  scale, _dptr(out, "out") if nrows else None, _opt_ptr(peak, "peak") if nrows else None,
                                  _stream(stream)), "ofdm_tx_modulate")
    return (out, peak) if return_peak else out


class Pipeline:
    """Streaming receiver over host-resident frames (ofdm_pipeline_*):
    `depth` device slots of `chunk_frames` frames, copy-in / compute /
    copy-out on three HIP streams.  demod() is asynchronous: keep `iq` and
    `out` alive until sync().  sample_format "sc16": the frames are int16
    (..., 2) arrays, x = i16 * scale, and the slots hold 4-byte samples
    (ofdm_pipeline_create_sc16: half the bytes over the host link)."""

    def __init__(self, S, R, C, X, prefix=0, chunk_frames=4, depth=3, sample_format="fc32", scale=SC16_SCALE):
        if sample_format not in ("fc32", "sc16"):
            raise OfdmError(f"sample_format must be 'fc32' or 'sc16', not {sample_format!r}")
        self.S, self.R, self.C, self.prefix = S, R, C, prefix
        self.sc16 = sample_format == "sc16"
        Xp = X.data_ptr() if hasattr(X, "data_ptr") else np.ascontiguousarray(
            X, np.complex64).ctypes.data
        h = _P()
        if self.sc16:
            _check(lib().ofdm_pipeline_create_sc16(S, R, C, prefix, scale, _P(Xp), chunk_frames, depth,
                                                   _c.byref(h)), "ofdm_pipeline_create_sc16")
        else:
            _check(lib().ofdm_pipeline_create(S, R, C, prefix, _P(Xp), chunk_frames, depth,
                                              _c.byref(h)), "ofdm_pipeline_create")
        self._h = h

    @staticmethod
    def _ptr(a):
        return _P(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)

    def demod(self, iq, out):
        """iq: (F, S, R, C+prefix) complex64 -- for an sc16 pipeline
        (F, S, R, C+prefix, 2) int16 --, out: (F, S-1, K) complex64: numpy
        arrays or tensors (host or device), contiguous."""
        F = iq.shape[0]
        assert tuple(out.shape) == (F, self.S - 1, self.C - 1), out.shape
        if self.sc16:
            assert tuple(iq.shape[1:]) == (self.S, self.R, self.C + self.prefix, 2), iq.shape
            assert str(iq.dtype).endswith("int16"), iq.dtype
            _check(lib().ofdm_pipeline_demod_sc16(self._h, self._ptr(iq), F, self._ptr(out)),
                   "ofdm_pipeline_demod_sc16")
            return out
        assert tuple(iq.shape[1:]) == (self.S, self.R, self.C + self.prefix), iq.shape
        _check(lib().ofdm_pipeline_demod(self._h, self._ptr(iq), F, self._ptr(out)),
               "ofdm_pipeline_demod")
        return out

    def acquire(self):
        d, s = _P(), _P()
        _check(lib().ofdm_pipeline_acquire(self._h, _c.byref(d), _c.byref(s)),
               "ofdm_pipeline_acquire")
        return d.value, s.value

    def acquire_sc16(self):
        d, s = _P(), _P()
        _check(lib().ofdm_pipeline_acquire_sc16(self._h, _c.byref(d), _c.byref(s)),
               "ofdm_pipeline_acquire_sc16")
        return d.value, s.value

    def submit(self, nframes, out=None):
        _check(lib().ofdm_pipeline_submit(self._h, nframes,
                                          None if out is None else self._ptr(out)),
               "ofdm_pipeline_submit")

    def sync(self):
        _check(lib().ofdm_pipeline_sync(self._h), "ofdm_pipeline_sync")

    def set_denoise(self, taps_post, taps_pre=0):
        """Later submits run estimate -> frame_estimate_denoise -> combine;
        taps_post = 0 turns it off again (the default)."""
        _check(lib().ofdm_pipeline_set_denoise(self._h, taps_post, taps_pre), "ofdm_pipeline_set_denoise")

    def set_cfo(self, on=True, cp_skip=0):
        """Later submits estimate each frame's carrier frequency offset from
        its cyclic prefixes (frame_cfo_estimate) and remove it: the derotating
        receiver at C = 1024, frame_cfo_derotate on the slot at any other C.
        on=False turns it off again (the default)."""
        _check(lib().ofdm_pipeline_set_cfo(self._h, int(bool(on)), cp_skip), "ofdm_pipeline_set_cfo")

    def set_cfo_search(self, max_shift, min_ratio=2.0):
        """Later submits that run with set_cfo on also search the integer
        part of each frame's offset (frame_cfo_acquire, in place on the
        chunk's estimates) within +-max_shift subcarrier spacings;
        max_shift = 0 turns it off again (the default)."""
        _check(lib().ofdm_pipeline_set_cfo_search(self._h, max_shift, min_ratio), "ofdm_pipeline_set_cfo_search")

    def set_phase_track(self, modulation):
        """Later submits run frame_phase_track in place on the slot's output
        (modulation 2, 4, 6 or 8), after whichever receiver form the submit
        used and before the copy-out; 0 turns it off again (the default)."""
        _check(lib().ofdm_pipeline_set_phase_track(self._h, modulation), "ofdm_pipeline_set_phase_track")

    def set_timing_track(self, modulation):
        """Later submits run frame_timing_track in place on the slot's output
        (modulation 2, 4, 6 or 8), instead of the phase tracker when both are
        set; 0 turns it off (include/ofdm_lsmrc_timing.h)."""
        _check(lib().ofdm_pipeline_set_timing_track(self._h, modulation), "ofdm_pipeline_set_timing_track")

    def close(self):
        if getattr(self, "_h", None):
            h, self._h = self._h, None
            _check(lib().ofdm_pipeline_destroy(h), "ofdm_pipeline_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_register(a):
    """Page-lock a host numpy array / CPU tensor for asynchronous DMA."""
    p = a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    n = a.numel() * a.element_size() if hasattr(a, "numel") else a.nbytes
    _check(lib().ofdm_host_register(_P(p), n), "ofdm_host_register")


def host_unregister(a):
    p = a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    _check(lib().ofdm_host_unregister(_P(p)), "ofdm_host_unregister")


def header_symbols(path=HEADER_PATH):
    """Function names declared in include/ofdm_lsmrc.h."""
    import re
    txt = open(path).read()
    return sorted(set(re.findall(r"^\s*(?:int|size_t|const char \*)\s*(ofdm_\w+)\s*\(", txt,
                                 re.M)))
