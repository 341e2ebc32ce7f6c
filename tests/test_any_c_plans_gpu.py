"""Every radix plan class of the any-length FFT (fft_any.hip) on the device.

The lengths come from tests/any_c_cases.py; tests/test_any_c_plan_cpu.py
proves that they reach every (variant, radix, position) stage class, every
(variant, last radix) of k_mrc_any at its fewest and its most accumulator
slots, a ragged row group per last radix, and the tails of the pure powers
of two.  The checks and bounds are those of test_any_c_gpu.py: fft_rows against numpy in float64 at
2e-6 * max(log2 C, 1) * max|ref|, frame_demod against the oracle at
helpers.RTOL norm- and element-wise.  k_tx_any, k_denoise_any and
k_acquire_any take any_c_cases.CALLER_LENGTHS through the parameter lists of
their own test files."""
import numpy as np
import pytest

import any_c_cases as ac
from helpers import parity
from test_any_c_gpu import check_export_and_antenna_partials, host, qpsk, to_dev

pytestmark = pytest.mark.gpu


# ------------------------------------------------- (a) k_fft_any, every stage class

@pytest.mark.parametrize("C", ac.STAGE_LENGTHS)
def test_fft_rows_stage_classes_vs_numpy(ofdm, dev, C):
    """test_fft_rows_any_c_vs_numpy's assertions on max(37, 2 G + 1) rows (a
    full row group and a ragged one at every length); rows 0, 1, 2 are a unit
    impulse at sample 1, one at sample C - 1 and a constant row, whose
    transforms (W_C^k, W_C^-k, C at bin 0) are also held to the bound row by row."""
    G = ac.cap_of(C) // C
    n = max(37, 2 * G + 1)
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((n, C)) + 1j * rng.standard_normal((n, C))).astype(np.complex64)
    x[:3] = 0
    x[0, 1] = 1
    x[1, C - 1] = 1
    x[2] = 1
    d = to_dev(x, dev)
    out = ofdm.c64(x.shape, dev)
    tol = 2e-6 * max(np.log2(C), 1.0)
    got = host(ofdm.fft_rows(d, out))
    inv = host(ofdm.fft_rows(d, out, inverse=True))
    ref = np.fft.fft(x.astype(np.complex128), axis=-1)
    refi = np.fft.ifft(x.astype(np.complex128), axis=-1) * C
    k = np.arange(C)
    assert np.abs(ref[0] - np.exp(-2j * np.pi * k / C)).max() < 1e-12 and np.abs(ref[2, 1:]).max() < 1e-9
    err = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    print(f"C={C} rows={n}: forward {err(got, ref):.2e} inverse {err(inv, refi):.2e} of max|ref|, bound {tol:.2e}; "
          f"structured rows {max(err(g[r], f[r]) for g, f in ((got, ref), (inv, refi)) for r in range(3)):.2e}")
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max()
    assert np.abs(inv - refi).max() <= tol * np.abs(refi).max()
    for r in range(3):
        assert np.abs(got[r] - ref[r]).max() <= tol * np.abs(ref[r]).max(), r
        assert np.abs(inv[r] - refi[r]).max() <= tol * np.abs(refi[r]).max(), r
    assert np.array_equal(host(ofdm.fft_rows(d)), got)  # in place


# --------------------------- (b) k_mrc_any, every last-stage class and ragged groups

# an odd prefix (rows that are only 8-byte aligned at even C), none once per variant; prefix <= C: 1 at C = 2
DEMOD = [(C, 4, 0 if C in ac.NO_PREFIX else 3 if C > 2 else 1)
         for C in sorted(set(ac.LAST_LENGTHS + ac.ONLY_LENGTHS + ac.POW2_TAIL_LENGTHS))] + \
        [(C, R, 3) for C, R in ac.GROUP_CASES]


@pytest.mark.parametrize("C,R,prefix", DEMOD)
def test_frame_demod_last_stage_classes_vs_oracle(ofdm, oracle, dev, C, R, prefix):
    F, S = 2, 3
    X = to_dev(qpsk(C - 1), dev)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=C + R)
    out = host(ofdm.frame_demod(iq, X, prefix))
    ref = oracle.frames_demod(host(iq), host(X), prefix)
    nrel, erel = parity(out, ref)
    print(f"C={C} R={R} prefix={prefix}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    assert int(ofdm.count_symbol_errors(to_dev(out, dev), S, seed=C + R).item()) == 0
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(iq, X, prefix, ws)
    out2 = ofdm.c64(out.shape, dev)
    ofdm.frame_combine(iq, prefix, ws, out2)
    assert np.array_equal(host(out2), out)


# ------------------------------------------ (c) the numerator store of every last radix

@pytest.mark.parametrize("C", ac.NUMERATOR_LENGTHS)
def test_antenna_partials_every_last_radix(ofdm, oracle, dev, C):
    """R = 5 in shards of 2 and 3 rows at G = 3: a partial group and a full one"""
    check_export_and_antenna_partials(ofdm, oracle, dev, C, 5, 3)
