"""Pilots of non-unit modulus on the CPU: what tests/pilot_cases.py promises,
the oracle's LS against the plain complex128 reference on those pilots, and
that the two metrics used by test_pilot_modulus_gpu.py catch a wrong division.

The GPU file compares the kernels with pilot_cases.ls128 and with oracle.ls;
this file shows that on the same inputs the two agree far inside RTOL (so a
GPU failure is the kernel's) and that a missing or wrong division by |x|^2
is far outside it (so a GPU pass means something)."""
import numpy as np
import pytest

import pilot_cases as pc
from helpers import RTOL, parity
from oracle_bindings import Reference, reference_available


@pytest.mark.parametrize("K", [3, 6, 63, 1023, 6143])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_family_properties(family, K):
    X = pc.pilots(family, K, seed=K)
    assert X.dtype == np.complex64 and X.shape == (K,)
    assert np.array_equal(X, pc.pilots(family, K, seed=K)), "not a function of (family, K, seed)"
    m2 = np.abs(X.astype(np.complex128)) ** 2
    off = np.abs(m2 - 1) >= 3e-4
    den = X.real * X.real + X.imag * X.imag  # the f32 denominator of ls_conj
    assert np.all(np.isfinite(den)) and np.all(den >= np.finfo(np.float32).tiny), "|x|^2 is not a normal float"
    if family in pc.FILL_FAMILIES:
        assert np.all(off)
        assert np.all(X == X[0])
    else:
        assert np.mean(off) >= 0.99
        if K >= 63:
            assert np.mean(np.abs(np.abs(X.real) - np.abs(X.imag)) > 1e-3 * np.abs(X)) > 0.9, "phases on the diagonals only"
            assert np.mean(X.real < 0) > 0.3 and np.mean(X.imag < 0) > 0.3
    if family == "fill_gpu":
        assert X[0] == np.complex64(1 + 1j)
    if family == "fill_cpu":
        assert abs(m2[0] - 0.999698) < 1e-6
    if family == "boosted":
        assert 0.5 <= np.abs(X).min() and np.abs(X).max() <= 2.0
        if K >= 1023:
            assert np.abs(X).min() < 0.55 and np.abs(X).max() > 1.8
    if family == "wide":
        e = np.log2(np.abs(X.astype(np.complex128)))
        assert np.all(np.abs(e - np.rint(e)) < 1e-6) and e.min() >= -20 - 1e-6 and e.max() <= 20 + 1e-6
        if K >= 1023:
            assert e.min() < -19.5 and e.max() > 19.5


def test_seeds_and_sizes_differ():
    for family in ("boosted", "wide"):
        assert not np.array_equal(pc.pilots(family, 63, 0), pc.pilots(family, 63, 1))
        assert not np.array_equal(pc.pilots(family, 63, 0), pc.pilots(family, 64, 0)[:63])


def test_elementwise_metric():
    ref = np.array([1e-12 + 0j, 1.0, 1e12j])
    assert pc.elementwise(ref * (1 + 5e-6), ref) == pytest.approx(5e-6, rel=1e-3)
    for bad in (ref * np.array([1 + 2e-5, 1, 1]),       # the small bin alone: parity's rms floor would excuse it
                ref + np.array([0, 0, np.nan]), ref[:2]):
        with pytest.raises(AssertionError):
            pc.elementwise(bad, ref)
    parity(ref * np.array([1 + 2e-5, 1, 1]), ref)  # which is why `wide` does not use parity
    with pytest.raises(AssertionError):
        pc.elementwise(np.array([1e-30]), np.array([0.0]))
    assert pc.elementwise(np.zeros(2), np.zeros(2)) == 0.0


@pytest.mark.parametrize("R,C", pc.STAGE_SHAPES + [(64, 1024)])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_oracle_ls_vs_plain_reference(oracle, family, R, C):
    """oracle.ls (pinned to the reference's divideOneRow by test_oracle.py) against ls128 under both metrics."""
    Y, X, _ = pc.stage_input(family, R, C)
    H, P = oracle.ls(Y, X)
    Href, Pref = pc.ls128(Y, X)
    eh, ep = pc.elementwise(H, Href), pc.elementwise(P, Pref)
    nh, np_ = parity(H, Href), parity(P, Pref)
    print(f"{family} R={R} C={C}: element-wise H {eh:.2e} P {ep:.2e}; parity H {nh[1]:.2e} P {np_[1]:.2e}")
    assert eh <= 1e-6 and ep <= 2e-6, "the reference itself leaves less than a fifth of RTOL to the kernels"
    if reference_available():
        Hr, Pr = Reference().ls(Y, X)
        assert np.array_equal(Hr.view(np.uint32), H.view(np.uint32))
        assert np.array_equal(Pr.view(np.uint32), P.view(np.uint32))


def test_truth_without_noise():
    """noise 0: conj(Hconj) of the plain reference is the channel the input was built from"""
    for family in pc.FAMILIES:
        Y, X, Htrue = pc.stage_input(family, 5, 64, noise=0.0)
        pc.elementwise(np.conj(pc.ls128(Y, X)[0]), Htrue)


def mutants(Y, X):
    """name -> (H, P) of a wrong estimator, in complex128 from the plain reference"""
    H, P = pc.ls128(Y, X)
    m = np.abs(X.astype(np.complex128))
    Xn = np.roll(X, 1)
    return {
        "division dropped": (H * m ** 2, None),
        "divided by the modulus": (H * m, None),
        "P of the undivided estimate": (None, P * m ** 4),
        "pilot of the neighbouring bin": (pc.ls128(Y, Xn)[0], None),
    }


@pytest.mark.parametrize("R,C", pc.STAGE_SHAPES)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_metrics_catch_the_mutants(family, R, C):
    Y, X, _ = pc.stage_input(family, R, C)
    Href, Pref = pc.ls128(Y, X)
    pc.elementwise(Href, Href), parity(Pref, Pref)
    for name, (H, P) in mutants(Y, X).items():
        if name == "pilot of the neighbouring bin" and family in pc.FILL_FAMILIES:
            continue  # every bin holds the same pilot: the neighbour's is the right one
        got, ref = (H, Href) if H is not None else (P, Pref)
        for metric in (pc.elementwise, parity):
            with pytest.raises(AssertionError):
                metric(got, ref)
            # and on the f32 rounding of the mutant, which is what a kernel would hand back
            with pytest.raises(AssertionError):
                metric(got.astype(np.complex64 if H is not None else np.float32), ref)
