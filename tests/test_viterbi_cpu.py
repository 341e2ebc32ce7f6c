"""The Viterbi decoder (include/ofdm_lsmrc_decode.h) without a device: the new
header declares exactly the three entries and the other headers and tables
gain nothing, every refusal answers before any HIP call (fake device pointers)
with ofdm_last_error text, the helper entries give the stated lengths and a
workspace within the stated bound, the library carries the four kernels
without a private segment, and the integer model the GPU tests lean on
(viterbi_cases.decode, the definition) checks out against its own encoder."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import viterbi_cases as vc
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_conv_coded_len", "ofdm_viterbi_decode", "ofdm_viterbi_workspace_bytes"]
P = ctypes.c_void_p
ARG, UNSUPPORTED = -1, -3
I8, F32 = 1, 0
KINDS = sorted(vc.KINDS)


def test_header_and_binding_declare_the_entries(ofdm):
    assert os.path.exists(ofdm.DECODE_HEADER_PATH)
    names = ofdm.header_symbols(ofdm.DECODE_HEADER_PATH)
    assert sorted(names) == sorted(ENTRIES)
    assert set(ofdm._SIGS_DECODE) == set(names), set(ofdm._SIGS_DECODE) ^ set(names)
    # the other three headers and their tables gain nothing
    for path in (ofdm.HEADER_PATH, ofdm.ACQUIRE_HEADER_PATH, ofdm.TIMING_HEADER_PATH):
        assert not set(names) & set(ofdm.header_symbols(path))
    for table in (ofdm._SIGS, ofdm._SIGS_ACQUIRE, ofdm._SIGS_TIMING):
        assert not set(names) & set(table)
    L = ofdm.lib()
    for e in ENTRIES:
        assert hasattr(L, e), f"{e} not exported"
        assert getattr(L, e).argtypes == ofdm._SIGS_DECODE[e][1]
        assert e in dict(ofdm._all_sigs())
    assert L.ofdm_version() == 2  # no version step
    assert '#include "ofdm_lsmrc.h"' in open(ofdm.DECODE_HEADER_PATH).read()
    for f in (ofdm.conv_coded_len, ofdm.viterbi_workspace_bytes, ofdm.viterbi_decode, ofdm.ConvCode.k7_rate_half,
              ofdm.ConvCode.k7_rate_third, ofdm.ConvCode.wifi_2_3, ofdm.ConvCode.wifi_3_4):
        assert callable(f)
    assert "DECODE_HEADER_PATH" in inspect.getsource(ofdm.build_id)  # the build identity covers the new header


def test_presets_are_the_stated_codes(ofdm):
    for preset, kind in ((ofdm.ConvCode.k7_rate_half, "half"), (ofdm.ConvCode.k7_rate_third, "third"),
                         (ofdm.ConvCode.wifi_2_3, "r23"), (ofdm.ConvCode.wifi_3_4, "r34")):
        for term in (True, False):
            c, m = preset(terminated=term), vc.code(kind, term)
            assert (c.n_out, tuple(c.g)[:c.n_out], c.terminated, c.punct_period, c.punct_mask) == \
                (m.n_out, m.g, m.terminated, m.p, m.mask)
    assert ofdm.ConvCode.k7_rate_half().terminated == 1


def _decode(L_, ofdm, code="half", llr=4096, fmt=I8, scale=1.0, stride=None, ncw=3, L=40, bits=1 << 24, out_stride=None,
            metric=1 << 28, scratch=1 << 29, scratch_bytes=None, term=True):
    c = code if code is None or isinstance(code, ofdm.ConvCode) else vc.to_c(ofdm, vc.code(code, term))
    n_rx = ofdm.conv_coded_len(c, L) if c is not None and 1 <= L <= 65530 and _valid(c) else 100
    if stride is None:
        stride = n_rx
    if out_stride is None:
        out_stride = (max(L, 1) + 7) // 8
    if scratch_bytes is None:
        scratch_bytes = 1 << 27
    rc = L_.ofdm_viterbi_decode(P(llr), fmt, scale, stride, ncw, L, None if c is None else ctypes.byref(c), P(bits),
                                out_stride, P(metric), P(scratch), scratch_bytes, None)
    return rc, L_.ofdm_last_error()


def _valid(c):
    n, p = c.n_out, c.punct_period
    return (n in (2, 3) and all(1 <= c.g[i] <= 127 for i in range(n)) and 0 <= p and p * n <= 32
            and not (c.punct_mask >> (p * n)) and (p == 0 or c.punct_mask))


def _bad_codes(ofdm):
    C = ofdm.ConvCode
    return [(C(1, (0o133,)), b"n_out"), (C(4, (1, 2, 3)), b"n_out"), (C(2, (0, 0o171)), b"g[0]"),
            (C(2, (0o133, 128)), b"g[1]"), (C(3, (0o133, 0o171, -1)), b"g[2]"), (C(2, (0o133, 0o171), 1, -1, 0), b"punct_period"),
            (C(2, (0o133, 0o171), 1, 17, 0x7), b"punct_period"), (C(3, (0o133, 0o171, 0o165), 1, 11, 0x7), b"punct_period"),
            (C(2, (0o133, 0o171), 1, 2, 0x17), b"punct_mask"), (C(2, (0o133, 0o171), 1, 0, 0x1), b"punct_mask"),
            (C(2, (0o133, 0o171), 1, 3, 0), b"punct_mask")]


def test_refusals_without_device(ofdm):
    L_ = ofdm.lib()
    fn = b"ofdm_viterbi_decode"
    rc, e = _decode(L_, ofdm, code=None)
    assert rc == ARG and fn in e and b"null code" in e
    for c, word in _bad_codes(ofdm):
        rc, e = _decode(L_, ofdm, code=c)
        assert rc == ARG and fn in e and word in e, (word, e)
        n = ctypes.c_longlong(-7)
        assert L_.ofdm_conv_coded_len(ctypes.byref(c), 40, ctypes.byref(n)) == ARG and n.value == -7
        assert b"ofdm_conv_coded_len" in L_.ofdm_last_error() and word in L_.ofdm_last_error()
        b = ctypes.c_size_t(77)
        assert L_.ofdm_viterbi_workspace_bytes(ctypes.byref(c), 40, 3, ctypes.byref(b)) == ARG and b.value == 77
        assert b"ofdm_viterbi_workspace_bytes" in L_.ofdm_last_error()
    # a full-width mask (p * n_out == 32) is a code like any other
    wide = ofdm.ConvCode(2, (0o133, 0o171), 1, 16, 0xFFFF0001)
    assert ofdm.conv_coded_len(wide, 26) == 17 * 2
    n_rx = ofdm.conv_coded_len(ofdm.ConvCode.k7_rate_half(), 40)
    for bad, word in ((dict(L=0), b"L=0"), (dict(L=-3), b"L=-3"), (dict(ncw=-1), b"ncw=-1"), (dict(fmt=2), b"llr_format"),
                      (dict(fmt=-1), b"llr_format"), (dict(fmt=F32, scale=0.0), b"llr_scale"),
                      (dict(fmt=F32, scale=-1.0), b"llr_scale"), (dict(fmt=F32, scale=float("inf")), b"llr_scale"),
                      (dict(fmt=F32, scale=float("nan")), b"llr_scale"), (dict(stride=n_rx - 1), b"cw_stride"),
                      (dict(out_stride=4), b"out_stride"), (dict(llr=0), b"null d_llr"), (dict(bits=0), b"null d_bits"),
                      (dict(fmt=F32, llr=4098), b"d_llr"), (dict(fmt=F32, llr=4097), b"d_llr"),
                      (dict(metric=(1 << 28) + 2), b"d_metric")):
        rc, e = _decode(L_, ofdm, **bad)
        assert rc == ARG and fn in e and word in e, (bad, e)
    rc, e = _decode(L_, ofdm, L=65531)
    assert rc == UNSUPPORTED and fn in e and b"65531" in e
    rc, e = _decode(L_, ofdm, L=65531, ncw=-1)  # the header's order: ncw < 0 comes first
    assert rc == ARG and b"ncw" in e
    # the scale is not consulted for int8; an odd int8 address is aligned
    assert _decode(L_, ofdm, scale=float("nan"), ncw=0)[0] == 0
    assert _decode(L_, ofdm, fmt=F32, scale=float("nan"), ncw=0)[0] == ARG
    # the workspace: beyond 4096 steps a scratch buffer of the stated size, 8-byte aligned
    half = ofdm.ConvCode.k7_rate_half()
    need = ofdm.viterbi_workspace_bytes(half, 5000, 3)
    assert need == 8 * 5006 * 3
    rc, e = _decode(L_, ofdm, L=5000, scratch_bytes=need - 1)
    assert rc == ARG and fn in e and b"scratch_bytes" in e
    rc, e = _decode(L_, ofdm, L=5000, scratch=0, scratch_bytes=need)
    assert rc == ARG and b"null d_scratch" in e
    rc, e = _decode(L_, ofdm, L=5000, scratch=(1 << 29) + 4, scratch_bytes=need)
    assert rc == ARG and b"d_scratch" in e and b"aligned" in e
    # overlaps: the LLR range (gaps included), the bits, the metrics, the scratch bytes in use
    lb, bb, mb = 2 * n_rx + n_rx, 3 * 5, 12
    for kw, word in ((dict(bits=4096 + lb - 1), b"d_bits overlaps d_llr"), (dict(bits=4096 - bb + 1), b"d_bits overlaps d_llr"),
                     (dict(metric=4096 + lb - 4), b"d_metric overlaps"), (dict(metric=(1 << 24) + 12), b"d_metric overlaps"),
                     (dict(metric=(1 << 24) - 8), b"d_metric overlaps")):
        rc, e = _decode(L_, ofdm, **kw)
        assert rc == ARG and fn in e and word in e, (kw, e)
    n5 = ofdm.conv_coded_len(half, 5000)
    for kw in (dict(scratch=4096 + 3 * n5 - 4), dict(scratch=(1 << 24) + 8), dict(scratch=(1 << 28) + 8),
               dict(scratch=(1 << 28) - need + 8)):
        rc, e = _decode(L_, ofdm, L=5000, scratch_bytes=need, **kw)
        assert rc == ARG and fn in e and b"d_scratch overlaps" in e, (kw, e)


def test_zero_codewords_is_a_noop(ofdm):
    L_ = ofdm.lib()
    for kind in KINDS:
        assert _decode(L_, ofdm, code=kind, ncw=0)[0] == 0
    c = ofdm.ConvCode.k7_rate_half()
    assert L_.ofdm_viterbi_decode(None, I8, 1.0, 100, 0, 40, ctypes.byref(c), None, 5, None, None, 0, None) == 0
    # ... but still not with a bad code, length or format
    assert L_.ofdm_viterbi_decode(None, I8, 1.0, 100, 0, 0, ctypes.byref(c), None, 5, None, None, 0, None) == ARG
    assert L_.ofdm_viterbi_decode(None, 3, 1.0, 100, 0, 40, ctypes.byref(c), None, 5, None, None, 0, None) == ARG
    assert L_.ofdm_viterbi_decode(None, I8, 1.0, 100, 0, 65531, ctypes.byref(c), None, 8192, None, None, 0, None) == UNSUPPORTED
    assert L_.ofdm_viterbi_decode(None, I8, 1.0, 100, 0, 40, None, None, 5, None, None, 0, None) == ARG


def test_does_not_consume_device_status(ofdm):
    """No work tickets: a raised sticky status is left for the ticketed entries."""
    L_ = ofdm.lib()
    assert L_.ofdm_device_status() == 0
    assert L_.ofdm_device_status_inject(1) == 0
    assert _decode(L_, ofdm, L=0)[0] == ARG  # its own validation, not OFDM_E_DEVICE
    assert _decode(L_, ofdm, ncw=0)[0] == 0
    assert L_.ofdm_device_status() == -5
    assert L_.ofdm_device_status() == 0


def test_coded_len(ofdm):
    C = ofdm.ConvCode
    assert ofdm.conv_coded_len(C.k7_rate_half(), 1017) == (1017 + 6) * 2 == 2046
    assert ofdm.conv_coded_len(C.wifi_3_4(), 999) == 1340
    assert ofdm.conv_coded_len(C.wifi_2_3(), 1000) == 1509
    assert ofdm.conv_coded_len(C.k7_rate_third(terminated=False), 1) == 3
    for kind in KINDS:
        for term in (True, False):
            for L in (1, 2, 3, 5, 6, 7, 64, 1000, 65530):
                m = vc.code(kind, term)
                assert ofdm.conv_coded_len(vc.to_c(ofdm, m), L) == vc.coded_len(m, L), (kind, term, L)


def test_workspace_within_the_stated_bound(ofdm):
    for kind in ("half", "third", "r34"):
        for term in (True, False):
            c = vc.to_c(ofdm, vc.code(kind, term))
            for L in (1, 40, 1017, 4090, 4096, 4097, 20000, 65530):
                T = L + 6 if term else L
                for ncw in (0, 1, 2, 1024, 1025, 4096, 4097, 125000, 1 << 40):
                    b = ofdm.viterbi_workspace_bytes(c, L, ncw)
                    assert b <= 8 * T * min(ncw, 4096) + 4096, (kind, term, L, ncw, b)
                    assert b == (0 if T <= 4096 else 8 * T * min(ncw, 1024)), (kind, term, L, ncw, b)  # as the header states


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_viterbi_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    for n_out in (2, 3):
        for punct in (0, 1):
            found = {n: v for n, v in seg.items() if f"k_viterbiILi{n_out}ELb{punct}E" in n}
            assert len(found) == 1, f"k_viterbi<{n_out}, {punct}>: {sorted(found)}"
            assert all(v == 0 for v in found.values()), f"k_viterbi<{n_out}, {punct}>: private segment {found}"


# ---- the model's own checks

def test_impulse_response():
    c = vc.code("half", terminated=True)
    out = vc.encode(c, [[1]], punctured=False)[0]  # T = 7 steps
    assert "".join(map(str, out[:, 0])) == "1011011" and "".join(map(str, out[:, 1])) == "1111001"
    c3 = vc.code("third", terminated=True)
    assert "".join(map(str, vc.encode(c3, [[1]], punctured=False)[0][:, 2])) == "1110101"  # 0165


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("term", (True, False), ids=("terminated", "truncated"))
def test_noiseless_round_trip(kind, term):
    c = vc.code(kind, term)
    rng = np.random.default_rng(5)
    for L in (1, 5, 6, 7, 64, 1000):
        bits = rng.integers(0, 2, (3, L)).astype(np.uint8)
        cb = vc.encode(c, bits)
        assert cb.shape == (3, vc.coded_len(c, L))
        q = (100 * (1 - 2 * cb.astype(np.int64))).astype(np.int8)
        u, metric = vc.decode_bits(c, q, L)
        # every generator taps u_t and every step of these codes sends a bit: no other word matches all sent bits
        assert np.array_equal(u, bits), (kind, term, L)
        assert np.all(metric == 100 * cb.shape[1]) and np.array_equal(metric, vc.correlation(c, u, q, L))


@pytest.mark.parametrize("term", (True, False), ids=("terminated", "truncated"))
def test_all_zero_llrs_decode_to_zero(term):
    for kind in KINDS:
        c = vc.code(kind, term)
        for L in (1, 9, 200):
            u, metric = vc.decode_bits(c, np.zeros((2, vc.coded_len(c, L)), np.int8), L)
            assert not u.any() and not metric.any()


def test_metric_is_the_reencoded_correlation():
    rng = np.random.default_rng(9)
    for kind in KINDS:
        for term in (True, False):
            c = vc.code(kind, term)
            for L in (3, 70, 500):
                q = rng.integers(-1, 2, (4, vc.coded_len(c, L))).astype(np.int8)
                u, metric = vc.decode_bits(c, q, L)
                assert np.array_equal(metric, vc.correlation(c, u, q, L)), (kind, term, L)


def test_wrong_decodes_still_beat_the_transmitted_word():
    """sigma = 1.2: the model errs, and its path scores at least the transmitted codeword's correlation."""
    k = vc.noisy_case("half", True, 1000, 3, sigma=1.2)
    u, metric = vc.decode_bits(k["code"], k["q"], 1000)
    wrong = int((u != k["bits"]).sum())
    sent = vc.correlation(k["code"], k["bits"], k["q"], 1000)
    print(f"sigma 1.2: {wrong} wrong bits of 3000, metric {metric} against the transmitted word's {sent}")
    assert wrong > 0 and np.all(metric >= sent) and np.any(metric > sent)
    assert np.array_equal(metric, vc.correlation(k["code"], u, k["q"], 1000))
    assert np.array_equal(vc.pack(u), k["packed"])


def test_design_sigmas_are_in_the_working_range():
    """The GPU grid's noise levels: many wrong raw signs, of which the decoder leaves (next to) none, so that
    the grid compares decodes that correct errors.  (Rate 1/3 at 2.2 dB Eb/N0 is near a bit error rate of
    1e-3: a handful of wrong bits in 3000 is the code, not the model.)"""
    for kind in KINDS:
        k = vc.noisy_case(kind, True, 1000, 3)
        raw = int(((k["q"] < 0) != vc.encode(k["code"], k["bits"]).astype(bool)).sum())
        u, _ = vc.decode_bits(k["code"], k["q"], 1000)
        wrong = int((u != k["bits"]).sum())
        print(f"{kind}: {raw} wrong raw signs of {k['q'].size}, {wrong} wrong decoded bits of {u.size}")
        assert raw > 40 and wrong * 100 < raw


def test_quantisers():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, 126.5, 127.5, -127.5, 1e30, -1e30, np.inf, -np.inf, np.nan,
                  0.0, -0.0, 1e-45, 3e38, -3e38], np.float32)
    assert list(vc.quant_f32(x, 1.0)) == [0, 2, 2, 0, -2, 0, 126, 127, -127, 127, -127, 127, -127, 0, 0, 0, 0, 127, -127]
    assert list(vc.quant_f32(x[:5], 2.0)) == [1, 3, 5, -1, -3]
    assert list(vc.quant_i8(np.array([-128, -127, 127, 0], np.int8))) == [-127, -127, 127, 0]
