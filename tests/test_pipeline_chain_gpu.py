"""ofdm_pipeline_submit is one chain of steps (pipeline_chain_cases.py spells
it out): for every sample format, receiver family and option set the pipeline's
output is, bit for bit, what the public entries give when called in that order
on the pipeline's chunks.  The entries themselves are held to the oracle by
their own suites; here only the chaining is at stake, so the comparison is of
the uint32 views, over NaN-prefilled outputs of which no NaN may remain.

C: 1024 (the fused receiver, every source), 2048 (the ticketed fused one), 256
(the FFT512 family), 600 (the any-length FFT).  An sc16 pipeline at C = 1024 has
no derotating receiver: set_cfo must refuse it, and its carrier-on sets are not
run."""
import numpy as np
import pytest

import pipeline_chain_cases as pc
from pipeline_chain_cases import bits

pytestmark = pytest.mark.gpu

CASES = [(C, fmt) for C in (1024, 2048, 256, 600) for fmt in ("fc32", "sc16")]


def assert_same(got, want, what):
    assert not np.isnan(got).any(), f"{what}: the pipeline left an output element unwritten"
    assert not np.isnan(want).any(), f"{what}: the direct calls left an output element unwritten"
    assert np.array_equal(bits(got), bits(want)), f"{what}: the pipeline differs from the direct calls"


@pytest.mark.parametrize("C,fmt", CASES)
def test_pipeline_equals_direct_calls(ofdm, dev, C, fmt):
    sc16 = fmt == "sc16"
    no_cfo = sc16 and C == 1024
    if no_cfo:
        with pc.pipeline(ofdm, C, sc16) as pl:
            with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_cfo failed \(-3\)"):
                pl.set_cfo(True, pc.CP_SKIP)
    outs, ran = {}, 0
    for opt in pc.OPTION_SETS:
        if no_cfo and opt.carrier:
            continue
        outs[opt] = pc.piped(ofdm, C, sc16, lambda pl: pc.configure(pl, opt))
        assert_same(outs[opt], pc.direct(ofdm, dev, C, sc16, opt), f"C={C} {fmt} {opt}")
        ran += 1
    assert ran == (8 if no_cfo else 24)  # 2 x 4 carrier-off sets; all 2 x 3 x 4 otherwise
    for opt, got in outs.items():
        # with both trackers set the timing tracker runs alone
        if opt.tracker == "both":
            assert np.array_equal(bits(got), bits(outs[opt._replace(tracker="timing")])), opt
    # every step takes part: the frames carry offsets, so each option moves the output
    plain = outs[pc.NONE]
    assert not np.array_equal(bits(outs[pc.NONE._replace(denoise=pc.DENOISE)]), bits(plain))
    assert not np.array_equal(bits(outs[pc.NONE._replace(tracker="phase")]), bits(plain))
    assert not np.array_equal(bits(outs[pc.NONE._replace(tracker="timing")]),
                              bits(outs[pc.NONE._replace(tracker="phase")]))
    if not no_cfo:
        assert not np.array_equal(bits(outs[pc.NONE._replace(carrier="cfo")]), bits(plain))


@pytest.mark.parametrize("C,fmt", CASES)
def test_options_on_then_off(ofdm, dev, C, fmt):
    """every option switched on, then off again: the never-configured pipeline, bit for bit"""
    sc16 = fmt == "sc16"
    everything = pc.Options(pc.DENOISE, None if sc16 and C == 1024 else "search", "both")

    def on_then_off(pl):
        pc.configure(pl, everything)
        pc.unconfigure(pl)

    never = pc.piped(ofdm, C, sc16, lambda pl: None)
    assert_same(pc.piped(ofdm, C, sc16, on_then_off), never, f"C={C} {fmt}")
    assert_same(never, pc.direct(ofdm, dev, C, sc16, pc.NONE), f"C={C} {fmt} never configured")
