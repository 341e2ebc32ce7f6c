"""The reference's own transmit helpers (ifftShiftOneRow, ifftOneRow,
addPrefix, matrix_readX, modRefSymbol, modOneSymbol; cpuLS.hpp:80-132,
152-162, 391-398, 466-529), compiled at test time from the reference tree,
pin the OFDM_TX_MAP_REFERENCE + OFDM_TX_NORM_PEAK semantics of
ofdm_tx_modulate as include/ofdm_lsmrc.h states them.

Nothing of the reference is in the repository: its functions are read where
they lie (tx_cases.build_ref_harness), behind the project's stand-ins for the
libraries the image lacks (tests/cpp/tx_ref_standins.hpp: a float64 DFT for
FFTW, clange_ 'M', cblas_csscal).  Checked against the float64 numpy
statement (tx_cases.tx_numpy):
  * bin placement, exact: ifftShiftOneRow on index-coded rows, and every unit
    impulse through modOneSymbol (which bin of the output's spectrum it lit);
  * the prefix, exact;
  * the samples within helpers.parity at RTOL = 1e-5.  The stand-in DFT
    rounds once from float64, the peak and the scale are float32 operations:
    a few 1e-7 in all.
Odd C (the (2, 9, 2) shape): the reference's ifftShiftOneRow moves two halves
of C / 2 and leaves the last element in place; nothing reads or writes out of
bounds, and the placement test below confirms the statement for it.
The committed fixtures tests/golden/tx/*.npz (tests/golden/make_tx_golden.py)
must equal what the harness produces now; this test writes nothing."""
import os

import numpy as np
import pytest

import tx_cases
from helpers import RTOL, parity
from tx_cases import REF_SHAPES, bin_of, tx_bins, tx_numpy

pytestmark = pytest.mark.skipif(not tx_cases.reference_present(), reason="no reference tree to compile")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tx_ref")
    return {p: tx_cases.RefTx(tmp, p) for p in sorted({s[2] for s in REF_SHAPES})}


@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_shift_places_bins_as_stated(refs, rows, C, prefix):
    d = np.zeros(C, np.complex64)
    d[1:] = np.arange(1, C) + 1j * np.arange(1, C)  # d[k + 1] = X[k], coded by index
    got = refs[prefix].ifftshift(d)
    assert np.array_equal(got, tx_bins(d[1:], C, "reference").astype(np.complex64))
    if C % 2 == 0:  # the header's closed form, and its two consequences
        assert all(bin_of(k, C, "reference") == (k + 1 + C // 2) % C for k in range(C - 1))
        assert got[C // 2] == 0 and got[0] == d[C // 2]


@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_unit_impulses_light_the_stated_bins(refs, rows, C, prefix):
    K = C - 1
    out = refs[prefix].mod_one_symbol(np.eye(K, dtype=np.complex64), C)
    spec = np.fft.fft(out[:, prefix:].astype(np.complex128), axis=-1) / C
    lit = np.argmax(np.abs(spec), axis=-1)
    assert np.array_equal(lit, [bin_of(k, C, "reference") for k in range(K)])
    # one bin each, of unit peak after the normalisation
    assert np.allclose(np.abs(spec[np.arange(K), lit]), 1.0, atol=1e-6)
    assert np.abs(spec).sum(axis=-1).max() < 1.0 + 1e-4


@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_prefix_is_the_rows_tail(refs, rows, C, prefix):
    X = tx_cases.rows_of(tx_cases.seed_of(rows, C, prefix), rows, C - 1)
    out = refs[prefix].mod_one_symbol(X, C)
    assert out.shape == (rows, C + prefix)
    assert np.array_equal(out[:, :prefix], out[:, C:C + prefix])
    dY = tx_cases.rows_of(5, rows, C)
    Y = refs[prefix].add_prefix(dY)
    assert np.array_equal(Y, np.concatenate([dY[:, C - prefix:], dY], axis=1))


@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_samples_match_the_statement(refs, rows, C, prefix):
    X = tx_cases.rows_of(tx_cases.seed_of(rows, C, prefix), rows, C - 1)
    want, _ = tx_numpy(X, C, prefix, "reference", "peak")
    nrel, erel = parity(refs[prefix].mod_one_symbol(X, C), want, RTOL)
    print(f"modOneSymbol C={C} prefix={prefix}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    # modRefSymbol: matrix_readX's rotated pilots as the one row
    iq, Xr = refs[prefix].mod_ref_symbol(C)
    raw = np.fromfile(tx_cases.PILOTS, np.complex64, C - 1)
    K = C - 1
    assert np.array_equal(Xr, raw[[tx_cases.out_pos_any(j, K) for j in range(K)]])
    want, _ = tx_numpy(Xr, C, prefix, "reference", "peak")
    parity(iq, want, RTOL)
    assert np.isclose(np.abs(iq).max(), 1.0, atol=1e-6)


@pytest.mark.parametrize("rows,C,prefix", REF_SHAPES)
def test_committed_fixtures_equal_a_fresh_run(tmp_path, rows, C, prefix):
    path = tx_cases.fixture_path(rows, C, prefix)
    assert os.path.exists(path), f"{path} missing: run tests/golden/make_tx_golden.py"
    assert os.path.getsize(path) < (1 << 20)
    have = tx_cases.load_fixture(rows, C, prefix)
    now = tx_cases.reference_record(tmp_path, rows, C, prefix)
    assert sorted(have.files) == sorted(now)
    for key, v in now.items():
        assert np.array_equal(have[key], v), key
