"""The shared-Hc row loop of the C = 1024 receivers with its rows alternating
between two register buffers (hlds_row_pp / hlds_rows<SHARED>, frame_td.hip)
against the float64 oracle, through both flows: the one-launch
ofdm_frame_demod and ofdm_frame_estimate + ofdm_frame_combine.

The loop's forms, by the number of antenna rows R: an even R peels row 0 in
front (into the second buffer), then come the pairs, then the final row
without a prefetch.

Cases (F, S, R, prefix):
  2 x 9 x R, prefix 0     every block inside one frame (8 data symbols per
                          frame = one workgroup): the shared loop alone.
                          R = 1 the final row only; 2 peeled row + final row;
                          3 one pair + final row; 4 peeled row, one pair,
                          final row; 5 two pairs; 8 peeled row, three pairs.
                          R = 1 has the bounds of test_fma_fft1024_gpu's
                          one-antenna case: element-wise 2e-4 against the
                          oracle, 2e-3 between the flows.
  1 x 5 x 3, prefix 8     one block of 4 real symbols and 4 tail waves that
                          duplicate the last one and take part in the barriers
  3 x 12 x 4, prefix 8    blocks inside a frame and blocks straddling two, in
                          one launch
  sc16                    (its rows keep the one-buffer loop, hlds_row_pf, next
                          to the fp32 rows' code in hlds_rows)
                          the 2 x 9 x R shapes, R = 2, 3, 4, through
                          frame_demod_sc16 and frame_estimate_sc16 +
                          frame_combine_sc16, as test_sc16_gpu checks them:
                          helpers.parity against the oracle on the dequantised
                          input, the two flows bit for bit.
Everything else: helpers.RTOL = 1e-5, norm-relative and element-wise.  Outputs
start NaN-filled; every figure is printed before it is asserted."""
import numpy as np
import pytest

from helpers import RTOL, parity
from test_fma_fft1024_gpu import C, errors, host, pilots
from test_sc16_gpu import S15, dequantise, quantise

pytestmark = pytest.mark.gpu

# (F, S, R, prefix, element-wise bound vs oracle, vs the other flow)
CASES = [(2, 9, 1, 0, 2e-4, 2e-3)] + [(2, 9, R, 0, RTOL, RTOL) for R in (2, 3, 4, 5, 8)] + [
    (1, 5, 3, 8, RTOL, RTOL),
    (3, 12, 4, 8, RTOL, RTOL)]


def nan_out(ofdm, dev, F, S):
    out = ofdm.c64((F, S - 1, C - 1), dev)
    out.fill_(float("nan"))
    return out


@pytest.mark.parametrize("F,S,R,prefix,etol,etol_flows", CASES)
def test_rows_vs_oracle(ofdm, oracle, dev, F, S, R, prefix, etol, etol_flows):
    X = pilots(dev, C - 1, seed=13)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=F * 1000 + S * 10 + R, noise_std=0.01)
    one = host(ofdm.frame_demod(iq, X, prefix, out=nan_out(ofdm, dev, F, S)))
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(iq, X, prefix, ws)
    two = host(ofdm.frame_combine(iq, prefix, ws, nan_out(ofdm, dev, F, S)))
    xs = host(X)
    refs = [oracle.frame_demod(host(iq[f]), xs, prefix)[0] for f in range(F)]
    for f, ref in enumerate(refs):
        for name, got in (("one-launch", one), ("two-launch", two)):
            n, e = errors(got[f], ref)
            print(f"F={F} S={S} R={R} prefix={prefix} frame {f} {name} vs oracle: norm-rel {n:.3e} elem {e:.3e}")
    n, e = errors(one, two)
    print(f"F={F} S={S} R={R} prefix={prefix} one-launch vs two-launch: norm-rel {n:.3e} elem {e:.3e}")
    for f, ref in enumerate(refs):
        parity(one[f], ref, erel_tol=etol)
        parity(two[f], ref, erel_tol=etol)
    parity(one, two, erel_tol=etol_flows)


@pytest.mark.parametrize("R", [2, 3, 4])
def test_sc16_rows_vs_oracle(ofdm, oracle, dev, R):
    import torch
    F, S, prefix = 2, 9, 0
    X = pilots(dev, C - 1, seed=17)
    q = quantise(host(ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=40 + R, noise_std=0.02)))
    ref = oracle.frames_demod(dequantise(q, S15), host(X), prefix)
    qd = torch.from_numpy(q).to(dev)
    whole = host(ofdm.frame_demod_sc16(qd, X, prefix, float(S15), out=nan_out(ofdm, dev, F, S)))
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_sc16(qd, X, prefix, ws, float(S15))
    two = host(ofdm.frame_combine_sc16(qd, prefix, ws, nan_out(ofdm, dev, F, S), float(S15)))
    for name, got in (("frame_demod_sc16", whole), ("estimate + combine", two)):
        n, e = errors(got, ref)
        print(f"sc16 F={F} S={S} R={R} {name} vs oracle: norm-rel {n:.3e} elem {e:.3e}")
    parity(whole, ref)
    parity(two, ref)
    assert np.array_equal(two.view(np.uint32), whole.view(np.uint32))
