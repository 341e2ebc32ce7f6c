"""The C = 1024 receivers' fused-FMA row transform and combine (fft16_fma,
common.hpp; mac, frame_td.hip) against the float64 oracle, through both
flows: the one-launch ofdm_frame_demod and ofdm_frame_estimate +
ofdm_frame_combine.

Cases (F, S, R, prefix):
  2 x 3 x 1, prefix 0     one antenna: nothing averages the FFT error.  Bounds
                          of test_many_small_frames' R = 1 case: element-wise
                          2e-4 against the oracle, 2e-3 between the flows.
  3 x 7 x 5, prefix 8     straddling blocks, tail waves, the non-shared loop
  1 x 2 x 64, prefix 0    the full antenna chain of the MAC
  60 x 101 x 9, prefix 8  ticketed half units of 5 + 4 rows per wave; frames
                          0 and 59 against the oracle
Everything else: helpers.RTOL = 1e-5, norm-relative and element-wise.  Every
figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest

from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

C = 1024
# (F, S, R, prefix, frames checked against the oracle, element-wise bound vs oracle, vs the other flow)
CASES = [(2, 3, 1, 0, (0, 1), 2e-4, 2e-3),
         (3, 7, 5, 8, (0, 1, 2), RTOL, RTOL),
         (1, 2, 64, 0, (0,), RTOL, RTOL),
         (60, 101, 9, 8, (0, 59), RTOL, RTOL)]


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def pilots(dev, K, seed=5):
    import torch
    rng = np.random.default_rng(seed)
    a = np.float32(0.70710678)
    X = (rng.choice([-a, a], K) + 1j * rng.choice([-a, a], K)).astype(np.complex64)
    return torch.from_numpy(X).to(dev)


def errors(got, ref):
    """(norm-relative, element-wise) error in helpers.parity's metric, not asserted"""
    got = np.asarray(got, np.complex128).ravel()
    ref = np.asarray(ref, np.complex128).ravel()
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    return (np.linalg.norm(got - ref) / np.linalg.norm(ref),
            np.max(np.abs(got - ref) / np.maximum(np.abs(ref), rms)))


@pytest.mark.parametrize("F,S,R,prefix,frames,etol,etol_flows", CASES)
def test_fma_rows_vs_oracle(ofdm, oracle, dev, F, S, R, prefix, frames, etol, etol_flows):
    X = pilots(dev, C - 1, seed=11)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=F * 1000 + S * 10 + R, noise_std=0.01)
    one = ofdm.c64((F, S - 1, C - 1), dev)
    one.fill_(float("nan"))
    ofdm.frame_demod(iq, X, prefix, out=one)
    one = host(one)
    ws = ofdm.workspace(F, S, R, C, dev)
    two = ofdm.c64((F, S - 1, C - 1), dev)
    two.fill_(float("nan"))
    ofdm.frame_estimate(iq, X, prefix, ws)
    ofdm.frame_combine(iq, prefix, ws, two)
    two = host(two)
    xs = host(X)
    refs = {f: oracle.frame_demod(host(iq[f]), xs, prefix)[0] for f in frames}
    for f, ref in refs.items():
        for name, got in (("one-launch", one), ("two-launch", two)):
            n, e = errors(got[f], ref)
            print(f"F={F} S={S} R={R} prefix={prefix} frame {f} {name} vs oracle: norm-rel {n:.3e} elem {e:.3e}")
    n, e = errors(one, two)
    print(f"F={F} S={S} R={R} prefix={prefix} one-launch vs two-launch: norm-rel {n:.3e} elem {e:.3e}")
    for f, ref in refs.items():
        parity(one[f], ref, erel_tol=etol)
        parity(two[f], ref, erel_tol=etol)
    parity(one, two, erel_tol=etol_flows)
