"""ofdm_tx_modulate on the GPU (the C = 1024 wave kernel and the any-C
workgroup kernel) against
  * tests/golden/tx/*.npz: what the reference's own modOneSymbol /
    modRefSymbol made of the seeded rows (recorded by
    tests/golden/make_tx_golden.py, pinned by test_tx_ref_cpu.py), and
  * the float64 numpy statement of include/ofdm_lsmrc.h (tx_cases.tx_numpy),
both at helpers.parity with the project's RTOL = 1e-5 (norm-wise and
element-wise with the row RMS as floor), d_peak within 1e-5 relative.
Structure (prefix, pads, guards, repeatability, zero rows, the store paths)
is checked bit for bit.  The loop-back builds frames from CHOSEN payloads on
the device and gets them back from ofdm_frame_demod and, bit by bit, from
ofdm_frame_soft_demap -- what the library could not do before.

Bounds set here, with their reasons:
  * zero-forcing chain through the drop-in modOneSymbol(chanMultiply = true):
    2 * RTOL, two operations (apply, modulate) each held to RTOL elsewhere.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tx_cases
from any_c_cases import CALLER_LENGTHS
from helpers import RTOL, parity
from tx_cases import REF_SHAPES, tx_numpy

pytestmark = pytest.mark.gpu

MAPS, NORMS = ("reference", "rx"), ("peak", "scale")


def dev_t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def check(got, peak, X, C, cp, map, norm, scale):
    want, wpeak = tx_numpy(X, C, cp, map, norm, scale)
    parity(got.cpu().numpy(), want, RTOL)
    assert np.allclose(peak.cpu().numpy(), wpeak, rtol=1e-5, atol=0)


# ------------------------------------------------------------------ parity

@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_reference_fixtures(ofdm, dev, rows, C, prefix):
    """MAP_REFERENCE + NORM_PEAK is modOneSymbol / modRefSymbol: the reference's recorded outputs."""
    z = tx_cases.load_fixture(rows, C, prefix)
    got, peak = ofdm.tx_modulate(dev_t(z["X"], dev), C, prefix, "reference", "peak", return_peak=True)
    nrel, erel = parity(got.cpu().numpy(), z["iq"], RTOL)
    print(f"C={C} prefix={prefix}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    check(got, peak, z["X"], C, prefix, "reference", "peak", 1.0)
    got = ofdm.tx_modulate(dev_t(z["ref_X"][None], dev), C, prefix, "reference", "peak")
    parity(got.cpu().numpy()[0], z["ref_iq"], RTOL)


@pytest.mark.parametrize("nrows", [1, 3, 9])  # 9: a second, partial workgroup of 8 waves
@pytest.mark.parametrize("cp", [0, 1, 7, 16, 1024])  # 1, 7: rows not 16-B aligned, the 8-B store path
def test_c1024_against_statement(ofdm, dev, nrows, cp):
    import torch
    C, K = 1024, 1023
    X = tx_cases.rows_of(100 * nrows + cp, nrows, K)
    for ldx in (1023, 1024):
        Xd = torch.full((nrows, ldx), float("nan"), dtype=torch.complex64, device=dev)
        Xd[:, :K] = dev_t(X, dev)
        for map in MAPS:
            for norm in NORMS:
                got, peak = ofdm.tx_modulate(Xd, C, cp, map, norm, scale=0.25, return_peak=True)
                assert got.shape == (nrows, C + cp)
                check(got, peak, X, C, cp, map, norm, 0.25)


# every path of the stage machinery: radix 2 alone, powers of 8, odd C (even
# K), mixed radices (600 = 8 * 3 * 5^2, 1536 = 2^9 * 3), the three LDS
# capacities (<= 2048, 4096, 8192).  cp = 5 is beyond C = 2's limit
# (cp_len <= C): there the largest legal prefix, cp = C, is used.
# CALLER_LENGTHS: a prime above 8, a 7 and a 5 in one plan per capacity, and 7 * 7.
@pytest.mark.parametrize("C", [2, 8, 9, 64, 600, 1536, 2048, 4096, 8192] + CALLER_LENGTHS)
@pytest.mark.parametrize("cp", [0, 5])
def test_any_c_against_statement(ofdm, dev, C, cp):
    cp = min(cp, C)
    X = tx_cases.rows_of(C + cp, 2, C - 1)
    for map in MAPS:
        for norm in NORMS:
            got, peak = ofdm.tx_modulate(dev_t(X, dev), C, cp, map, norm, scale=2.0, return_peak=True)
            check(got, peak, X, C, cp, map, norm, 2.0)


def test_bare_ifft_equals_fft_rows_inverse(ofdm, dev):
    """NORM_SCALE, scale = 1 is ofdm_fft_rows(inverse) of the placed bins -- the unfused route's middle step."""
    for C in (1024, 1536):
        X = tx_cases.rows_of(3, 2, C - 1)
        bins = tx_cases.tx_bins(X, C, "rx").astype(np.complex64)
        want = ofdm.fft_rows(dev_t(bins, dev), inverse=True).cpu().numpy()
        got = ofdm.tx_modulate(dev_t(X, dev), C, 0, "rx", "scale", 1.0).cpu().numpy()
        parity(got, want, RTOL)


# --------------------------------------------------------------- structure

@pytest.mark.parametrize("C,cp,nrows", [(1024, 16, 9), (1024, 7, 3), (1024, 1024, 2), (600, 5, 3), (9, 9, 2)])
def test_structure_is_exact(ofdm, dev, C, cp, nrows):
    import torch
    K, Cp = C - 1, C + cp
    X = dev_t(tx_cases.rows_of(C + nrows, nrows, K), dev)
    nan = float("nan")
    buf = torch.full((nrows + 2, Cp), nan, dtype=torch.complex64, device=dev)
    peaks = torch.full((nrows + 2,), nan, dtype=torch.float32, device=dev)
    L = ofdm.lib()
    rc = L.ofdm_tx_modulate(X.data_ptr(), K, nrows, C, cp, 0, 0, 1.0, buf[1:].data_ptr(), peaks[1:].data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.ofdm_last_error()
    got = buf.cpu().numpy()
    # nothing outside the nrows rows and peaks was written
    assert np.isnan(got[0]).all() and np.isnan(got[nrows + 1]).all() and np.isfinite(got[1:nrows + 1]).all()
    pk = peaks.cpu().numpy()
    assert np.isnan(pk[0]) and np.isnan(pk[nrows + 1]) and np.isfinite(pk[1:nrows + 1]).all()
    iq = got[1:nrows + 1]
    assert np.array_equal(iq[:, :cp].view(np.uint64), iq[:, C:C + cp].view(np.uint64))  # the prefix is the tail
    # the binding's own allocation, twice: the same bytes
    a = ofdm.tx_modulate(X, C, cp, "reference", "peak").cpu().numpy()
    b = ofdm.tx_modulate(X, C, cp, "reference", "peak").cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a.view(np.uint64), iq.view(np.uint64))
    # a NaN-filled pad of ldx = K + 1 rows changes nothing
    Xp = torch.full((nrows, K + 1), nan, dtype=torch.complex64, device=dev)
    Xp[:, :K] = X
    c = ofdm.tx_modulate(Xp, C, cp, "reference", "peak").cpu().numpy()
    assert np.array_equal(c.view(np.uint64), a.view(np.uint64))
    # a destination 8 B off a 16-B boundary (the 8-B store path at even cp): the same bytes
    flat = torch.full((nrows * Cp + 3,), nan, dtype=torch.complex64, device=dev)
    off = 1 if flat.data_ptr() % 16 == 0 else 2
    d = flat[off:off + nrows * Cp].view(nrows, Cp)
    assert d.data_ptr() % 16 == 8
    ofdm.tx_modulate(X, C, cp, "reference", "peak", out=d)
    f = flat.cpu().numpy()
    assert np.isnan(f[:off]).all() and np.isnan(f[off + nrows * Cp:]).all()
    assert np.array_equal(f[off:off + nrows * Cp].view(np.uint64), a.ravel().view(np.uint64))


@pytest.mark.parametrize("C,cp", [(1024, 16), (1024, 3), (64, 4), (9, 0)])
def test_zero_row_gives_zeros_and_peak_zero(ofdm, dev, C, cp):
    X = tx_cases.rows_of(C, 3, C - 1)
    X[1] = 0
    for norm in NORMS:
        got, peak = ofdm.tx_modulate(dev_t(X, dev), C, cp, "rx", norm, return_peak=True)
        got, peak = got.cpu().numpy(), peak.cpu().numpy()
        assert np.all(got[1] == 0) and peak[1] == 0 and np.isfinite(got).all()
        assert peak[0] > 0 and peak[2] > 0
        if norm == "peak":
            assert np.allclose(np.abs(got[[0, 2]]).max(axis=1), 1.0, atol=1e-6)


def test_binding_refuses_bad_arguments(ofdm, dev):
    import torch
    X = torch.zeros((2, 1023), dtype=torch.complex64, device=dev)
    with pytest.raises(ofdm.OfdmError, match="cp_len"):
        ofdm.tx_modulate(X, 1024, 1025)
    with pytest.raises(ofdm.OfdmError, match="ldx"):
        ofdm.tx_modulate(X[:, :1000].contiguous(), 1024)
    with pytest.raises(ofdm.OfdmError, match="map"):
        ofdm.tx_modulate(X, 1024, map="shifted")
    assert ofdm.tx_modulate(X[:0], 1024, 8).shape == (0, 1032)


# --------------------------------------------------------------- loop-back

def qam16_rows(seed, shape_bits):
    from test_soft_demap_gpu import map_38211
    bits = np.random.default_rng(seed).integers(0, 2, shape_bits + (4,)).astype(np.uint8)
    return bits, map_38211(bits).astype(np.complex64)


# (2, 3, 4, 1024, 16): the fused C = 1024 receiver; (1, 3, 3, 64, 4): the staged
# any-C receiver; (2, 3, 2, 9, 2): even K = 8, shiftOneRow's three-segment rotation
@pytest.mark.parametrize("F,S,R,C,cp", [(2, 3, 4, 1024, 16), (1, 3, 3, 64, 4), (2, 3, 2, 9, 2)])
def test_loop_back_through_the_receiver(ofdm, dev, F, S, R, C, cp):
    """Frames from given data: symbol 0 the raw pilots, symbols 1..S-1 seeded
    16-QAM rows, MAP_RX + NORM_SCALE, every antenna's copy times its own
    complex gain -> ofdm_frame_demod returns the data rows, and
    ofdm_frame_soft_demap every transmitted bit."""
    import torch
    K = C - 1
    raw = np.fromfile(tx_cases.PILOTS, np.complex64, K)
    assert raw.size == K and np.all(np.abs(raw) > 0.1)
    bits, data = qam16_rows(C + cp, (F, S - 1, K))
    rng = np.random.default_rng(R)
    gain = (rng.uniform(0.5, 2.0, R) * np.exp(2j * np.pi * rng.uniform(0, 1, R))).astype(np.complex64)
    sym = torch.cat([dev_t(raw, dev).expand(F, 1, K), dev_t(data, dev)], dim=1)  # [F, S, K]
    Xin = (sym[:, :, None, :] * dev_t(gain, dev)[None, None, :, None]).contiguous()  # [F, S, R, K]
    iq = ofdm.tx_modulate(Xin, C, cp, "rx", "scale", 1.0)
    assert iq.shape == (F, S, R, C + cp)
    Xrot = dev_t(ofdm.pilot_rotate(raw), dev)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.frame_demod(iq, Xrot, cp, ws=ws)
    nrel, erel = parity(z.cpu().numpy(), data, RTOL)
    print(f"loop-back C={C}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    nv = torch.full((F,), 0.01, dtype=torch.float32, device=dev)
    llr = ofdm.frame_soft_demap(z, ws, F, S, R, C, ofdm.MOD_QAM16, nv).cpu().numpy()
    assert np.array_equal((llr < 0).astype(np.uint8), bits)


# ------------------------------------------------------------------- chain

def test_zf_precoded_rows_chain_bit_for_bit(ofdm, oracle, dev):
    """ofdm_zf_apply_ex(ldy = 1024) -> ofdm_tx_modulate(ldx = 1024) equals
    ofdm_zf_apply -> ofdm_tx_modulate(ldx = K): the downlink from the users'
    symbols to the IQ of every antenna, with or without the row padding."""
    import torch
    from zf_cases import channel, qpsk
    U, R, K, n, cp = 4, 16, 1023, 3, 16
    W = oracle.zf_precoder(channel(U, R, K, seed=77))
    Wt = ofdm.zf_transpose(dev_t(W, dev))
    X = dev_t(qpsk(n, U, K, seed=78), dev)
    Xp = torch.full((n, U, 1024), float("nan"), dtype=torch.complex64, device=dev)
    Xp[:, :, :K] = X
    Yp = torch.full((n, R, 1024), float("nan"), dtype=torch.complex64, device=dev)
    ofdm.zf_apply_pitched(Wt, Xp, out=Yp)
    a, pa = ofdm.tx_modulate(Yp, 1024, cp, "reference", "peak", ldx=1024, return_peak=True)
    b, pb = ofdm.tx_modulate(ofdm.zf_apply(Wt, X), 1024, cp, "reference", "peak", return_peak=True)
    assert a.shape == b.shape == (n, R, 1024 + cp)
    assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
    assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy())
    assert np.isfinite(a.cpu().numpy()).all()


# ----------------------------------------------------------------- drop-in

@pytest.mark.parametrize("rows,C,prefix", [(2, 1024, 16), (2, 9, 2)])
def test_cpuls_tx_call_sequence(oracle, dev, tmp_path, rows, C, prefix):
    """modRefSymbol and modOneSymbol of the drop-in cpuLS.hpp (a C++ driver,
    tests/cpp/tx_driver.cpp, built with the fixture's prefix) against the
    reference's recorded outputs; chanMultiply = true against the oracle's
    multiplyWithChannelInv followed by the statement."""
    from zf_cases import channel
    z = tx_cases.load_fixture(rows, C, prefix)
    K, Cp = C - 1, C + prefix
    shutil.copy(tx_cases.PILOTS, tmp_path / "Pilots.dat")
    z["X"].tofile(tmp_path / "X.bin")
    R = 8
    W = oracle.zf_precoder(channel(rows, R, K, seed=C))
    W.tofile(tmp_path / "W.bin")
    exe = tx_cases.build_tx_driver(tmp_path, prefix)
    subprocess.run([exe, str(C), str(rows), str(R)], cwd=tmp_path, check=True, timeout=120)
    assert np.array_equal(np.fromfile(tmp_path / "REFX.bin", np.complex64), z["ref_X"])
    parity(np.fromfile(tmp_path / "REF.bin", np.complex64), z["ref_iq"], RTOL)
    parity(np.fromfile(tmp_path / "ONE.bin", np.complex64).reshape(rows, Cp), z["iq"], RTOL)
    want, _ = tx_numpy(oracle.zf_apply(W, z["X"][None])[0], C, prefix, "reference", "peak")
    parity(np.fromfile(tmp_path / "ZF.bin", np.complex64).reshape(R, Cp), want, 2 * RTOL)
