"""The QC-LDPC decoder (include/ofdm_lsmrc_ldpc.h) without a device: the new
header declares exactly its four entries and the other headers and tables gain
nothing, every refusal of every entry answers before any HIP call (fake device
pointers) with ofdm_last_error text and in the header's order, the workspace
is within the stated bound, the library carries the two kernels without a
private segment, and the integer model the GPU tests lean on (ldpc_cases.decode,
the definition) checks out against its encoder and against a second, naive
model."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import ldpc_cases as lc
from test_kernel_resources import LIB, TOOLS, kernel_private_segments

ENTRIES = ["ofdm_ldpc_code_create", "ofdm_ldpc_code_destroy", "ofdm_ldpc_decode", "ofdm_ldpc_workspace_bytes"]
P = ctypes.c_void_p
I = ctypes.c_int
ARG, UNSUPPORTED = -1, -3
I8, F32 = 1, 0


def to_c(ofdm, c):
    return ofdm.QcLdpc(c.mb, c.nb, c.Z, c.rows)


def test_header_and_binding_declare_the_entries(ofdm):
    assert os.path.exists(ofdm.LDPC_HEADER_PATH)
    names = ofdm.header_symbols(ofdm.LDPC_HEADER_PATH)
    assert sorted(names) == sorted(ENTRIES)
    assert set(ofdm._SIGS_LDPC) == set(names), set(ofdm._SIGS_LDPC) ^ set(names)
    # the other four headers and their tables gain nothing
    for path in (ofdm.HEADER_PATH, ofdm.ACQUIRE_HEADER_PATH, ofdm.TIMING_HEADER_PATH, ofdm.DECODE_HEADER_PATH):
        assert not set(names) & set(ofdm.header_symbols(path))
    for table in (ofdm._SIGS, ofdm._SIGS_ACQUIRE, ofdm._SIGS_TIMING, ofdm._SIGS_DECODE):
        assert not set(names) & set(table)
    L = ofdm.lib()
    for e in ENTRIES:
        assert hasattr(L, e), f"{e} not exported"
        assert getattr(L, e).argtypes == ofdm._SIGS_LDPC[e][1]
        assert e in dict(ofdm._all_sigs())
    assert L.ofdm_version() == 2  # no version step
    assert '#include "ofdm_lsmrc.h"' in open(ofdm.LDPC_HEADER_PATH).read()
    for f in (ofdm.QcLdpc, ofdm.ldpc_workspace_bytes, ofdm.ldpc_decode):
        assert callable(f)
    assert "LDPC_HEADER_PATH" in inspect.getsource(ofdm.build_id)  # the build identity covers the new header


# ---- the handle

def _create(ofdm, mb, nb, Z, row_ptr, col, shift, null=()):
    a = [(I * len(v))(*v) for v in (row_ptr, col, shift)]
    ptr = [None if k in null else ctypes.cast(a[k], ctypes.POINTER(I)) for k in range(3)]
    d = ofdm.QcLdpcDesc(mb, nb, Z, *ptr)
    h = P(77)
    rc = ofdm.lib().ofdm_ldpc_code_create(ctypes.byref(d), ctypes.byref(h))
    e = ofdm.lib().ofdm_last_error()
    if rc == 0:
        assert ofdm.lib().ofdm_ldpc_code_destroy(h) == 0
    else:
        assert h.value == 77 and b"ofdm_ldpc_code_create" in e
    return rc, e


GOOD = dict(mb=2, nb=4, Z=5, row_ptr=[0, 3, 5], col=[0, 1, 2, 1, 3], shift=[0, 4, 1, 2, 0])


def test_create_refusals(ofdm):
    L_ = ofdm.lib()
    assert _create(ofdm, **GOOD)[0] == 0
    assert L_.ofdm_ldpc_code_create(None, ctypes.byref(P())) == ARG and b"null code" in L_.ofdm_last_error()
    d = ofdm.QcLdpcDesc(2, 4, 5, None, None, None)
    assert L_.ofdm_ldpc_code_create(ctypes.byref(d), None) == ARG and b"null handle" in L_.ofdm_last_error()
    for k in range(3):
        rc, e = _create(ofdm, **GOOD, null=(k,))
        assert rc == ARG and b"null row_ptr, col or shift" in e
    for kw, word in ((dict(mb=0), b"mb=0"), (dict(nb=2), b"nb=2"), (dict(nb=1), b"nb=1"), (dict(Z=1), b"Z=1"),
                     (dict(row_ptr=[1, 3, 5]), b"row_ptr[0]"), (dict(row_ptr=[0, 1, 5]), b"row 0 has degree 1"),
                     (dict(row_ptr=[0, 4, 5], col=[0, 1, 2, 3, 3]), b"row 1 has degree 1"), (dict(row_ptr=[0, 3, 2]), b"row 1 has degree -1"),
                     (dict(col=[0, 1, 4, 1, 3]), b"col=4 outside"), (dict(col=[-1, 1, 2, 1, 3]), b"col=-1 outside"),
                     (dict(col=[0, 1, 1, 1, 3]), b"col=1 not above"), (dict(col=[0, 2, 1, 1, 3]), b"col=1 not above"),
                     (dict(shift=[0, 5, 1, 2, 0]), b"shift=5 outside"), (dict(shift=[0, 4, 1, 2, -1]), b"shift=-1 outside")):
        rc, e = _create(ofdm, **{**GOOD, **kw})
        assert rc == ARG and word in e, (kw, e)
    # a new row may begin at a lower column than the last row ended with
    assert _create(ofdm, 2, 4, 5, [0, 2, 4], [2, 3, 0, 1], [0, 0, 0, 0])[0] == 0
    # the size limits: a code that is valid otherwise
    rc, e = _create(ofdm, **{**GOOD, "Z": 385})
    assert rc == UNSUPPORTED and b"Z=385" in e
    assert _create(ofdm, **{**GOOD, "Z": 384})[0] == 0
    deg = lambda d, nb, Z: dict(mb=1, nb=nb, Z=Z, row_ptr=[0, d], col=list(range(d)), shift=[0] * d)
    rc, e = _create(ofdm, **deg(33, 40, 4))
    assert rc == UNSUPPORTED and b"degree 33" in e
    assert _create(ofdm, **deg(32, 40, 4))[0] == 0
    rc, e = _create(ofdm, **deg(2, 16385, 2))
    assert rc == UNSUPPORTED and b"N=32770" in e
    assert _create(ofdm, **deg(2, 16384, 2))[0] == 0
    # two faults: every OFDM_E_ARG fault answers before a size limit
    rc, e = _create(ofdm, **{**GOOD, "Z": 385, "shift": [0, 385, 1, 2, 0]})
    assert rc == ARG and b"shift=385" in e
    rc, e = _create(ofdm, **{**deg(33, 40, 4), "shift": [0] * 32 + [4]})
    assert rc == ARG and b"shift=4" in e
    rc, e = _create(ofdm, **{**GOOD, "mb": 0, "Z": 1})
    assert rc == ARG and b"mb=0" in e


def test_destroyed_and_null_handles(ofdm):
    L_ = ofdm.lib()
    code = to_c(ofdm, lc.gen_code(2, 4, 5))
    h = P(code.handle.value)
    assert ofdm.ldpc_workspace_bytes(code, 3) == 0
    code.close()
    code.close()  # idempotent in the binding
    b = ctypes.c_size_t(9)
    for handle in (h, P(None)):
        assert L_.ofdm_ldpc_code_destroy(handle) == ARG and b"ofdm_ldpc_code_destroy" in L_.ofdm_last_error()
        assert L_.ofdm_ldpc_workspace_bytes(handle, 3, ctypes.byref(b)) == ARG and b.value == 9
        assert b"ofdm_ldpc_workspace_bytes: null or destroyed handle" in L_.ofdm_last_error()
        rc = L_.ofdm_ldpc_decode(P(4096), I8, 1.0, 20, 3, handle, 0, 20, 5, 12, 0, 1, 20, P(1 << 24), 3, None, None, 0, None)
        assert rc == ARG and b"ofdm_ldpc_decode: null or destroyed handle" in L_.ofdm_last_error()
        # ... before everything else, a bad format and ncw = 0 included
        assert L_.ofdm_ldpc_decode(None, 7, 1.0, 20, 0, handle, 0, 20, 5, 12, 0, 1, 20, None, 3, None, None, 0, None) == ARG
        assert b"handle" in L_.ofdm_last_error()


# ---- ofdm_ldpc_decode's refusals

@pytest.fixture(scope="module")
def small(ofdm):
    c = lc.gen_code(2, 4, 5)  # N = 20
    code = to_c(ofdm, c)
    yield code
    code.close()


@pytest.fixture(scope="module")
def big(ofdm):
    c = lc.special_codes()["scratch_first"]
    code = to_c(ofdm, c)
    yield code
    code.close()


def _decode(L_, code, llr=4096, fmt=I8, scale=1.0, stride=None, ncw=3, pos0=0, n_rx=None, max_iter=5, norm16=12, offset=0,
            early_stop=1, n_bits=None, bits=1 << 24, out_stride=None, iters=1 << 28, scratch=1 << 29, scratch_bytes=1 << 27):
    n_rx = code.N - pos0 if n_rx is None else n_rx
    n_bits = code.N if n_bits is None else n_bits
    stride = n_rx if stride is None else stride
    out_stride = (max(n_bits, 1) + 7) // 8 if out_stride is None else out_stride
    rc = L_.ofdm_ldpc_decode(P(llr), fmt, scale, stride, ncw, code.handle, pos0, n_rx, max_iter, norm16, offset, early_stop,
                             n_bits, P(bits), out_stride, P(iters), P(scratch), scratch_bytes, None)
    return rc, L_.ofdm_last_error()


def test_refusals_without_device(ofdm, small, big):
    L_ = ofdm.lib()
    fn = b"ofdm_ldpc_decode"
    for bad, word in ((dict(fmt=2), b"llr_format"), (dict(fmt=-1), b"llr_format"), (dict(fmt=F32, scale=0.0), b"llr_scale"),
                      (dict(fmt=F32, scale=-1.0), b"llr_scale"), (dict(fmt=F32, scale=float("inf")), b"llr_scale"),
                      (dict(fmt=F32, scale=float("nan")), b"llr_scale"), (dict(pos0=-1, n_rx=5), b"window pos0=-1"),
                      (dict(n_rx=0), b"n_rx=0"), (dict(n_rx=-2), b"n_rx=-2"), (dict(pos0=1, n_rx=20), b"window pos0=1 n_rx=20"),
                      (dict(pos0=20, n_rx=1), b"window"), (dict(n_rx=21), b"window"),
                      (dict(pos0=2 ** 31 - 1, n_rx=2 ** 31 - 1), b"window"), (dict(stride=19), b"cw_stride=19"),
                      (dict(n_bits=0), b"n_bits=0"), (dict(n_bits=21), b"n_bits=21"), (dict(n_bits=-1), b"n_bits=-1"),
                      (dict(out_stride=2), b"out_stride=2"), (dict(n_bits=9, out_stride=1), b"out_stride=1"),
                      (dict(max_iter=0), b"max_iter=0"), (dict(max_iter=1001), b"max_iter=1001"), (dict(norm16=0), b"norm16=0"),
                      (dict(norm16=17), b"norm16=17"), (dict(offset=-1), b"offset=-1"), (dict(offset=128), b"offset=128"),
                      (dict(early_stop=2), b"early_stop=2"), (dict(early_stop=-1), b"early_stop=-1"), (dict(ncw=-1), b"ncw=-1"),
                      (dict(llr=0), b"null d_llr"), (dict(bits=0), b"null d_bits"), (dict(fmt=F32, llr=4098), b"d_llr"),
                      (dict(fmt=F32, llr=4097), b"d_llr"), (dict(iters=(1 << 28) + 2), b"d_iters")):
        rc, e = _decode(L_, small, **bad)
        assert rc == ARG and fn in e and word in e, (bad, e)
    # the limits themselves serve (ncw = 0: nothing is launched)
    for ok in (dict(max_iter=1000), dict(max_iter=1), dict(norm16=1), dict(norm16=16), dict(offset=127), dict(n_bits=1, out_stride=1),
               dict(pos0=19, n_rx=1), dict(early_stop=0)):
        assert _decode(L_, small, ncw=0, **ok)[0] == 0, ok
    # two faults: the header's order
    for bad, word in ((dict(fmt=2, n_rx=0), b"llr_format"), (dict(n_rx=0, stride=-1), b"window"), (dict(stride=19, n_bits=0), b"cw_stride"),
                      (dict(n_bits=0, max_iter=0), b"n_bits"), (dict(out_stride=2, max_iter=0), b"out_stride"),
                      (dict(max_iter=0, norm16=0), b"max_iter"), (dict(norm16=0, offset=-1), b"norm16"),
                      (dict(offset=200, early_stop=3), b"offset"), (dict(early_stop=3, ncw=-1), b"early_stop"),
                      (dict(ncw=-1, llr=0), b"ncw"), (dict(llr=0, bits=0), b"null d_llr"),
                      (dict(bits=0, iters=(1 << 28) + 1), b"null d_bits")):
        rc, e = _decode(L_, small, **bad)
        assert rc == ARG and fn in e and word in e, (bad, e)
    # the scale is not consulted for int8; an odd int8 address is aligned
    assert _decode(L_, small, scale=float("nan"), ncw=0)[0] == 0
    assert _decode(L_, small, fmt=F32, scale=float("nan"), ncw=0)[0] == ARG
    # the workspace: a scratch buffer of the stated size where the messages do not fit in LDS
    c = lc.special_codes()["scratch_first"]
    need = ofdm.ldpc_workspace_bytes(big, 3)
    assert need == lc.nnz(c) * c.Z * 3 > 0
    rc, e = _decode(L_, big, scratch_bytes=need - 1)
    assert rc == ARG and fn in e and b"scratch_bytes" in e
    rc, e = _decode(L_, big, scratch=0, scratch_bytes=need)
    assert rc == ARG and b"null d_scratch" in e
    rc, e = _decode(L_, big, scratch_bytes=need - 1, fmt=F32, llr=4097)  # the size before the alignments
    assert rc == ARG and b"scratch_bytes" in e
    # overlaps: the LLR range (gaps included), the bits, the iteration counts, the scratch bytes in use
    lb, bb = 2 * 25 + 20, 3 * 3
    for kw, word in ((dict(bits=4096 + lb - 1), b"d_bits overlaps d_llr"), (dict(bits=4096 - bb + 1), b"d_bits overlaps d_llr"),
                     (dict(iters=4096 + lb - 2), b"d_iters overlaps"), (dict(iters=(1 << 24) + 8), b"d_iters overlaps"),
                     (dict(iters=(1 << 24) - 8), b"d_iters overlaps")):
        rc, e = _decode(L_, small, stride=25, **kw)
        assert rc == ARG and fn in e and word in e, (kw, e)
    assert _decode(L_, small, stride=25, bits=4096 + lb, ncw=0)[0] == 0
    nB = big.N
    for kw in (dict(scratch=4096 + 3 * nB - 4), dict(scratch=(1 << 24) + 8), dict(scratch=(1 << 28) + 8),
               dict(scratch=(1 << 28) - need + 8)):
        rc, e = _decode(L_, big, scratch_bytes=need, **kw)
        assert rc == ARG and fn in e and b"d_scratch overlaps" in e, (kw, e)
    # scratch that a code does not use may lie anywhere
    rc, e = _decode(L_, small, scratch=4096, ncw=-1)
    assert rc == ARG and b"ncw" in e


def test_zero_codewords_is_a_noop(ofdm, small, big):
    L_ = ofdm.lib()
    assert _decode(L_, small, ncw=0)[0] == 0 and _decode(L_, big, ncw=0)[0] == 0
    args = (20, 0, small.handle, 0, 20, 5, 12, 0, 1, 20, None, 3, None, None, 0, None)
    assert L_.ofdm_ldpc_decode(None, I8, 1.0, *args) == 0
    # ... but still not with a bad format, window or control
    assert L_.ofdm_ldpc_decode(None, 3, 1.0, *args) == ARG
    assert _decode(L_, small, ncw=0, n_rx=21)[0] == ARG and _decode(L_, small, ncw=0, max_iter=0)[0] == ARG


def test_does_not_consume_device_status(ofdm, small):
    """No work tickets: a raised sticky status is left for the ticketed entries."""
    L_ = ofdm.lib()
    assert L_.ofdm_device_status() == 0
    assert L_.ofdm_device_status_inject(1) == 0
    assert _decode(L_, small, max_iter=0)[0] == ARG  # its own validation, not OFDM_E_DEVICE
    assert _decode(L_, small, ncw=0)[0] == 0
    assert ofdm.ldpc_workspace_bytes(small, 5) == 0
    assert L_.ofdm_device_status() == -5
    assert L_.ofdm_device_status() == 0


def test_workspace_within_the_stated_bound(ofdm):
    codes = [lc.gen_code(2, 4, 2), lc.gen_code(12, 24, 384), lc.code_1944(), lc.saturation_case()[0]]
    codes += list(lc.special_codes().values())
    seen = set()
    for c in codes:
        code = to_c(ofdm, c)
        fits = 2 * lc.N(c) + lc.nnz(c) * c.Z <= 65536
        seen.add(fits)
        for ncw in (0, 1, 2, 1023, 1024, 1025, 125000, 1 << 40):
            b = ofdm.ldpc_workspace_bytes(code, ncw)
            assert b <= 32 * c.mb * c.Z * min(ncw, 1024), (c[:3], ncw, b)
            assert b == (0 if fits else lc.nnz(c) * c.Z * min(ncw, 1024)), (c[:3], ncw, b)  # as the header states
        with pytest.raises(ofdm.OfdmError, match="ncw=-1"):
            ofdm.ldpc_workspace_bytes(code, -1)
        assert ofdm.lib().ofdm_ldpc_workspace_bytes(code.handle, 1, None) == ARG
        code.close()
    assert seen == {True, False}


@pytest.mark.skipif(not os.path.exists(LIB) or not all(os.path.exists(t) for t in TOOLS),
                    reason="product library or ROCm LLVM tools absent")
def test_ldpc_kernels_have_no_private_segment():
    seg = kernel_private_segments(LIB)
    for msg_lds in (0, 1):
        found = {n: v for n, v in seg.items() if f"k_ldpcILb{msg_lds}E" in n}
        assert len(found) == 1, f"k_ldpc<{msg_lds}>: {sorted(found)}"
        assert all(v == 0 for v in found.values()), f"k_ldpc<{msg_lds}>: private segment {found}"


# ---- the model's own checks

def test_encoder_output_satisfies_every_check():
    rng = np.random.default_rng(1)
    for c in (lc.gen_code(3, 6, 5), lc.gen_code(2, 4, 2), lc.code_1944(), lc.special_codes()["deg2_and_32"],
              lc.special_codes()["shift_ends"], lc.saturation_case()[0]):
        x = lc.encode(c, rng.integers(0, 2, (5, lc.K(c))))
        assert x.shape == (5, lc.N(c)) and x.any() and not lc.syndrome(c, x).any()
        assert lc.syndrome(c, x ^ np.eye(1, lc.N(c), 3, dtype=np.uint8)).any()  # and one wrong bit does not
    c = lc.special_codes()["shift_ends"]
    assert all({0, c.Z - 1} <= {s for _, s in row} for row in c.rows)
    first, last = lc.layer_order_code().rows[0], lc.layer_order_code().rows[-1]
    assert [col for col, _ in first] == [col for col, _ in last]
    degs = lambda c: [len(r) for r in c.rows]
    assert degs(lc.special_codes()["deg2_and_32"]) == [2, 32, 32] and degs(lc.special_codes()["deg19"]) == [19] * 3


def test_noiseless_codeword_stops_after_one_iteration():
    rng = np.random.default_rng(2)
    for c in (lc.gen_code(3, 6, 5), lc.code_1944()):
        x = lc.encode(c, rng.integers(0, 2, (4, lc.K(c))))
        for ctl in lc.CONTROLS:
            xd, it = lc.decode(c, 100 * (1 - 2 * x.astype(np.int64)), 20, *ctl)
            assert np.array_equal(xd, x) and np.all(it == 1), ctl
        xd, it = lc.decode(c, 100 * (1 - 2 * x.astype(np.int64)), 7, early_stop=False)
        assert np.array_equal(xd, x) and np.all(it == 7)


def test_all_zero_llrs_decode_to_zero():
    for c in (lc.gen_code(3, 6, 5), lc.code_1944(), lc.layer_order_code()):
        xd, it = lc.decode(c, np.zeros((2, lc.N(c)), np.int64))
        assert not xd.any() and np.all(it == 1)


def test_vectorised_model_equals_the_naive_one():
    """mb 3, nb 6, Z 5: 200 random inputs, every (norm16, offset) used elsewhere, both stopping rules; small
    values among them, so that equal minima and zeros (ties, the first-minimum rule) occur."""
    c = lc.gen_code(3, 6, 5)
    rng = np.random.default_rng(4)
    q = rng.integers(-127, 128, (200, lc.N(c)))
    q[:60] = rng.integers(-3, 4, (60, lc.N(c)))
    q[60:80] = rng.choice([-127, 127], (20, lc.N(c)))
    differ = set()
    for ctl in lc.CONTROLS:
        for es, mi in ((True, 6), (False, 3), (True, 1)):
            a, b = lc.decode(c, q, mi, *ctl, es), lc.decode_naive(c, q, mi, *ctl, es)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (ctl, es, mi)
            differ.add(a[0].tobytes())
    assert len(differ) > len(lc.CONTROLS)  # the controls matter
    lo = lc.layer_order_code(5)
    ql = rng.integers(-20, 21, (40, lc.N(lo)))
    a, b = lc.decode(lo, ql, 4), lc.decode_naive(lo, ql, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # ... and the layer order matters to it: the first and last rows exchanged decode otherwise
    swapped = lc.Code(lo.mb, lo.nb, lo.Z, (lo.rows[2], lo.rows[1], lo.rows[0]))
    assert not np.array_equal(lc.decode(swapped, ql, 1, early_stop=False)[0], lc.decode(lo, ql, 1, early_stop=False)[0])


def test_saturation_input_reaches_the_clamp():
    c, q, ctl = lc.saturation_case()
    stats = {}
    x, it = lc.decode(c, lc.full_q(c, q), stats=stats, **ctl)
    print(f"saturation: {stats['clamp_hits']} posterior updates met the clamp, d_iters {it}")
    assert stats["clamp_hits"] > 0 and it[0] == 3 and np.any(it < 0)
    assert all(len(r) == 32 for r in c.rows)


@pytest.mark.parametrize("name", sorted(lc.NOISY))
def test_noise_levels_are_in_the_working_range(name):
    """Of every noisy GPU case: some hard decisions are wrong before decoding, and the model alone recovers
    every codeword in fewer than MAX_ITER iterations."""
    k, (x, it) = lc.case(name)
    raw = int(((k["q"] < 0) != k["x"].astype(bool)).sum())
    print(f"{name}: {raw} wrong hard decisions of {k['q'].size}, iterations {it.min()} .. {it.max()}")
    assert raw > 0
    assert np.array_equal(x, k["x"]) and np.all(it >= 1) and np.all(it < lc.MAX_ITER)


def test_quantisers_are_the_viterbi_decoders():
    import viterbi_cases as vc
    assert lc.quant_f32 is vc.quant_f32 and lc.quant_i8 is vc.quant_i8 and lc.pack is vc.pack
