"""What ofdm_pipeline_submit enqueues for a given option set, spelled out with
the public entries (`direct`), beside the pipeline run itself (`piped`), for
test_pipeline_chain_gpu.py.  One chain, each step once:

  convert (sc16 at C != 1024) -> cfo estimate [-> integer search]
  [-> derotate in place (C != 1024)] -> demod, or estimate -> denoise ->
  combine, on the chunk's source -> timing tracker, else phase tracker

`direct` takes the pipeline's chunking and a fresh workspace per chunk, so its
output is the pipeline's bit for bit (test_pipeline_gpu.py's header says why
another chunking is not)."""
import itertools
from collections import namedtuple

import numpy as np

import cfo_cases as cc

F, S, R, CP = 5, 4, 4, 16
CHUNK, DEPTH = 2, 2          # three submits, slot 0 used twice, one frame in the tail
SC16_SCALE = float(np.float32(2.0 ** -12))
CP_SKIP = 1
DENOISE = (12, 4)
SEARCH = (4, 2.0)
MOD = 2

# denoise: None or (taps_post, taps_pre); carrier: None, "cfo" or "search";
# tracker: None, "phase", "timing" or "both" (the timing tracker alone runs)
Options = namedtuple("Options", "denoise carrier tracker")
NONE = Options(None, None, None)
OPTION_SETS = [Options(*o) for o in itertools.product((None, DENOISE), (None, "cfo", "search"),
                                                      (None, "phase", "timing", "both"))]
assert len(OPTION_SETS) == 24

_cache = {}


def case(C):
    """cfo_cases.frames at the EPS_CYCLE offsets plus q: the frames as sc16, int16 (F, S, R, C + cp, 2)."""
    if C not in _cache:
        c = dict(cc.frames(F, S, R, C, CP, None, seed=C + 1))
        v = np.stack([c["y"].real, c["y"].imag], -1).astype(np.float64)
        assert np.abs(v).max() < 7.9
        c["q"] = np.ascontiguousarray(np.rint(v / SC16_SCALE).astype(np.int16))
        c["q"].setflags(write=False)
        _cache[C] = c
    return _cache[C]


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cached inputs are read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def configure(pl, opt):
    if opt.denoise:
        pl.set_denoise(*opt.denoise)
    if opt.carrier:
        pl.set_cfo(True, CP_SKIP)
    if opt.carrier == "search":
        pl.set_cfo_search(*SEARCH)
    if opt.tracker in ("phase", "both"):
        pl.set_phase_track(MOD)
    if opt.tracker in ("timing", "both"):
        pl.set_timing_track(MOD)


def unconfigure(pl):
    pl.set_denoise(0)
    pl.set_cfo_search(0)
    pl.set_cfo(False)
    pl.set_phase_track(0)
    pl.set_timing_track(0)


def pipeline(ofdm, C, sc16):
    kw = dict(sample_format="sc16", scale=SC16_SCALE) if sc16 else {}
    return ofdm.Pipeline(S, R, C, case(C)["X"], CP, chunk_frames=CHUNK, depth=DEPTH, **kw)


def piped(ofdm, C, sc16, setup):
    """The F frames through a new pipeline that setup(pl) configured; NaN where nothing was written."""
    c = case(C)
    out = np.full((F, S - 1, C - 1), np.nan, np.complex64)
    with pipeline(ofdm, C, sc16) as pl:
        setup(pl)
        pl.demod(np.array(c["q"] if sc16 else c["y"]), out)
        pl.sync()
    return out


def direct(ofdm, dev, C, sc16, opt):
    import torch
    assert not (sc16 and C == 1024 and opt.carrier), "ofdm_pipeline_set_cfo refuses this pipeline"
    c = case(C)
    X = to_dev(c["X"], dev)
    out = torch.full((F, S - 1, C - 1), float("nan"), dtype=torch.complex64, device=dev)
    for f0 in range(0, F, CHUNK):
        n = min(CHUNK, F - f0)
        ws = ofdm.workspace(n, S, R, C, dev)
        o = out[f0:f0 + n]
        y = to_dev((c["q"] if sc16 else c["y"])[f0:f0 + n], dev)
        if sc16 and C != 1024:
            y = ofdm.iq_convert_sc16(y, SC16_SCALE)
        if opt.carrier:
            eps = ofdm.frame_cfo_estimate(y, CP, CP_SKIP)
            if opt.carrier == "search":
                ofdm.frame_cfo_acquire(y, X, CP, SEARCH[0], eps=eps, min_ratio=SEARCH[1], out=eps)
            if C != 1024:
                ofdm.frame_cfo_derotate(y, CP, eps, out=y)
        # the source's three entries
        if sc16 and C == 1024:
            estimate = lambda: ofdm.frame_estimate_sc16(y, X, CP, ws, SC16_SCALE)
            combine = lambda: ofdm.frame_combine_sc16(y, CP, ws, o, SC16_SCALE)
            demod = lambda: ofdm.frame_demod_sc16(y, X, CP, SC16_SCALE, ws=ws, out=o)
        elif opt.carrier and C == 1024:
            estimate = lambda: ofdm.frame_estimate_cfo(y, X, CP, ws, eps)
            combine = lambda: ofdm.frame_combine_cfo(y, CP, ws, o, eps)
            demod = lambda: ofdm.frame_demod_cfo(y, X, CP, eps, ws=ws, out=o)
        else:
            estimate = lambda: ofdm.frame_estimate(y, X, CP, ws)
            combine = lambda: ofdm.frame_combine(y, CP, ws, o)
            demod = lambda: ofdm.frame_demod(y, X, CP, ws=ws, out=o)
        if opt.denoise:
            estimate()
            ofdm.frame_estimate_denoise(ws, n, S, R, C, *opt.denoise)
            combine()
        else:
            demod()
        if opt.tracker in ("timing", "both"):
            ofdm.frame_timing_track(o, ws, n, S, R, C, MOD, out=o)
        elif opt.tracker == "phase":
            ofdm.frame_phase_track(o, ws, n, S, R, C, MOD, out=o)
    torch.cuda.synchronize()
    return out.cpu().numpy()
