"""Integer carrier offset on the GPU (include/ofdm_lsmrc_acquire.h):
ofdm_frame_cfo_acquire against the float64 model of acquire_cases.py (which
is the definition), its gate, the closed loop estimate -> acquire -> receiver
on offsets of several subcarrier spacings, the pipeline's search mode, and the
entry between guard bands (guard_cases.py, as test_containment_gpu.py treats
the main header's entries).

Bounds: the shift and the bits of eps_out are exact wherever the model's
best-to-runner-up ratio is >= 3 (asserted for every non-zero frame);
|M_gpu(d) - M_model(d)| <= RTOL * max_d M_model(d) for every d -- normalised to
the peak because the off-peak sums cancel."""
import numpy as np
import pytest

import acquire_cases as ac
import cfo_cases as cc
from helpers import RTOL
from test_cfo_gpu import CHUNK, bits, host, nan_out, piped, to_dev

pytestmark = pytest.mark.gpu


def i32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_acquire(ofdm, dev, y, X, cp, D, eps, min_ratio=2.0, in_place=False):
    """(eps_out, shift, metric) on the host; outputs prefilled with NaN / a sentinel"""
    import torch
    F = y.shape[0]
    shift = torch.full((F,), -99, dtype=torch.int32, device=dev)
    metric = torch.full((F, 2 * D + 1), float("nan"), dtype=torch.float32, device=dev)
    if in_place:
        out = eps.clone()
        ofdm.frame_cfo_acquire(y, X, cp, D, eps=out, min_ratio=min_ratio, out=out, shift=shift, metric=metric)
    else:
        out = torch.full((F,), float("nan"), dtype=torch.float32, device=dev)
        ofdm.frame_cfo_acquire(y, X, cp, D, eps=eps, min_ratio=min_ratio, out=out, shift=shift, metric=metric)
    return host(out), host(shift), host(metric)


def check_against_model(got, model, zero=None):
    eo, sh, me = got
    shift, eps_out, M, ratio = model
    F = len(shift)
    peak = M.max(axis=1)
    for f in range(F):
        if f == zero:
            continue
        assert ratio[f] >= 3.0, f"frame {f}: the model's margin {ratio[f]:.2f} says nothing about a parity"
        assert sh[f] == shift[f], (f, sh[f], shift[f])
        assert i32(eo)[f] == i32(eps_out)[f], (f, eo[f], eps_out[f])
        assert np.all(np.isfinite(me[f]))
        err = np.abs(me[f].astype(np.float64) - M[f]).max()
        assert err <= RTOL * peak[f], f"frame {f}: |M - model| {err:.3e} > {RTOL:g} * peak {peak[f]:.3e}"
    worst = max(np.abs(me[f].astype(np.float64) - M[f]).max() / peak[f] for f in range(F) if f != zero)
    return worst


# ----------------------------------------------------- (a) parity with the model

# (F, S, R, C, cp, D)
PARITY = [(6, 3, 4, 1024, 16, 16),
          (6, 3, 3, 600, 9, 16),      # mixed radix, odd row length: rows only 8-byte aligned
          (6, 2, 2, 256, 16, 8),
          (3, 2, 17, 1024, 16, 4),    # more rows than one LDS group holds
          (3, 2, 5, 2048, 0, 8),      # cp = 0, d_eps_in null, integer offsets only
          (2, 2, 2, 8192, 16, 32),
          (2, 2, 1, 64, 8, 4),
          # any_c_cases.CALLER_LENGTHS: 7 * 7, and a prime above 8, a 7 and a 5 in one plan per capacity
          # (48 bins at C = 49: eight antennas for the model's margin of 3)
          (4, 2, 8, 49, 5, 8), (4, 2, 3, 770, 9, 16), (3, 2, 2, 2310, 16, 16), (2, 2, 2, 8190, 16, 32)]
NAN_FRAME = 0  # its offset is an integer: with eps_in acting as 0 nothing fractional is left in the frame

_cases = {}


def parity_case(key):
    """frames whose last one is zeroed; frame NAN_FRAME carries an integer offset"""
    if key not in _cases:
        F, S, R, C, cp, D = key
        pool = [-3.0, 2.03, 0.45, D - 0.45, -0.496] if cp else [-3.0, 5.0]
        eps = np.array((pool + [0.0])[:F - 1] + [0.0], np.float32)
        c = ac.frames(F, S, R, C, cp, eps, ac.random_pilots(C - 1, seed=C + R), seed=F + R)
        y = np.array(c["y"])
        y[F - 1] = 0
        y.setflags(write=False)
        _cases[key] = (y, c["X"], eps)
    return _cases[key]


@pytest.mark.parametrize("key", PARITY, ids=lambda k: "x".join(map(str, k)))
def test_parity_with_the_model(ofdm, dev, key):
    import torch
    F, S, R, C, cp, D = key
    y, X, eps = parity_case(key)
    yd, Xd = to_dev(y, dev), to_dev(X, dev)
    if cp:
        ein = host(ofdm.frame_cfo_estimate(yd, cp)).copy()
        assert ein[F - 1] == 0
        ein[NAN_FRAME] = np.nan
        ed = to_dev(ein, dev)
    else:
        ein, ed = None, None
    model = ac.acquire(y, X, cp, D, ein, 2.0)
    want = np.rint(eps.astype(np.float64) - (0 if ein is None else np.nan_to_num(ein.astype(np.float64))))
    assert np.array_equal(model[0][:F - 1], want[:F - 1].astype(np.int32)), (model[0], want)
    a = run_acquire(ofdm, dev, yd, Xd, cp, D, ed)
    b = run_acquire(ofdm, dev, yd, Xd, cp, D, ed)
    worst = check_against_model(a, model, zero=F - 1)
    print(f"{key}: shifts {a[1].tolist()} ratios {np.round(model[3], 1).tolist()} worst |dM| / peak {worst:.2e}")
    for u, v in zip(a, b):  # two runs: the same bits
        assert np.array_equal(i32(u), i32(v))
    # the zero frame: no M is positive
    z = F - 1
    ein_z = np.float32(0 if ein is None else ein[z])
    assert a[1][z] == 0 and np.all(i32(a[2][z]) == 0) and a[0][z].view(np.uint32) == ein_z.view(np.uint32)
    if ed is not None:  # in place: the same bits as out of place
        for u, v in zip(a, run_acquire(ofdm, dev, yd, Xd, cp, D, ed, in_place=True)):
            assert np.array_equal(i32(u), i32(v))
        # the nullable outputs left out change nothing
        out = torch.full((F,), float("nan"), dtype=torch.float32, device=dev)
        ofdm.frame_cfo_acquire(yd, Xd, cp, D, eps=ed, out=out)
        assert np.array_equal(i32(host(out)), i32(a[0]))
    assert np.array_equal(bits(host(yd)), bits(y))  # the frames are only read


# ------------------------------------------------------------------ (b) the gate

def test_gate(ofdm, dev):
    F, S, R, C, cp, D = 3, 2, 2, 256, 16, 8
    eps = np.array([2.0, 2.0, 2.0], np.float32)
    Xr = ac.random_pilots(C - 1, seed=C)
    cases = {"constant": ac.frames(F, S, R, C, cp, eps, ac.constant_pilots(C - 1), seed=3),
             "noise": ac.frames(F, S, R, C, cp, eps, Xr, seed=4, noise_only=True),
             "random": ac.frames(F, S, R, C, cp, eps, Xr, seed=5)}
    for name, c in cases.items():
        yd, Xd = to_dev(c["y"], dev), to_dev(c["X"], dev)
        ed = ofdm.frame_cfo_estimate(yd, cp)
        ein = host(ed)
        shift, eps_out, M, ratio = ac.acquire(c["y"], c["X"], cp, D, ein, 2.0)
        eo, sh, me = run_acquire(ofdm, dev, yd, Xd, cp, D, ed, min_ratio=2.0)
        top = np.sort(me.astype(np.float64), axis=1)
        print(f"{name}: shifts {sh.tolist()} best / runner-up {np.round(top[:, -1] / top[:, -2], 3).tolist()} "
              f"model {np.round(ratio, 3).tolist()}")
        if name == "random":
            assert np.all(ratio >= 3.0)
            assert sh.tolist() == [2, 2, 2] and np.array_equal(i32(eo), i32(eps_out))
        else:
            assert np.all(ratio <= 1.5)
            assert sh.tolist() == [0, 0, 0] and np.array_equal(i32(eo), i32(ein))
            # the metric is stored ungated, and min_ratio = 1 always accepts: some shift wins
            assert np.all(np.abs(me - M) <= RTOL * M.max(axis=1, keepdims=True))
            _, sh1, me1 = run_acquire(ofdm, dev, yd, Xd, cp, D, ed, min_ratio=1.0)
            assert np.array_equal(i32(me1), i32(me))
            assert np.array_equal(sh1, me.astype(np.float64).argmax(axis=1) - D) or name == "constant"


# ------------------------------------------------------------ (c) closed loop

LOOP_EPS = (2.03, -3.2, 0.45, 7.0, -0.496, 15.55)


@pytest.mark.parametrize("S,R,C,cp", [(4, 5, 1024, 16), (4, 4, 256, 16), (3, 3, 600, 9)])
def test_closed_loop(ofdm, dev, oracle, S, R, C, cp):
    """estimate -> receiver on the fractional part alone loses the frames whose
    offset has an integer part; with acquire in between none is lost.  C = 1024
    runs the derotating receiver, the others the derotator and the fp32 one."""
    F, D = len(LOOP_EPS), 16
    c = cc.frames(F, S, R, C, cp, LOOP_EPS, seed=4)
    truth = oracle.frames_demod(c["clean"], c["X"], cp)
    y, X = to_dev(c["y"], dev), to_dev(c["X"], dev)

    def receive(eps):
        if C == 1024:
            return host(ofdm.frame_demod_cfo(y, X, cp, eps))
        return host(ofdm.frame_demod(ofdm.frame_cfo_derotate(y, cp, eps), X, cp))

    frac = ofdm.frame_cfo_estimate(y, cp)
    wrong = cc.decision_errors(receive(frac), truth)
    import torch
    shift = torch.full((F,), -99, dtype=torch.int32, device=dev)
    full = ofdm.frame_cfo_acquire(y, X, cp, D, eps=frac, shift=shift)
    fixed = cc.decision_errors(receive(full), truth)
    print(f"C={C}: {wrong} of {truth.size} decisions wrong on the fractional estimate, {fixed} after the search; "
          f"eps {host(frac).tolist()} -> {host(full).tolist()}")
    want = np.rint(np.array(LOOP_EPS) - host(frac).astype(np.float64))  # -0.496 may reach the receiver as 0.504 - 1
    assert np.array_equal(host(shift), want.astype(np.int32)) and np.count_nonzero(want) >= 4
    assert np.all(np.abs(host(full).astype(np.float64) - np.array(LOOP_EPS)) < 5e-3)
    assert wrong > truth.size // 4
    assert fixed == 0


# --------------------------------------------------------------- (d) pipeline

PIPE_EPS = (2.03, -3.2, 0.45, 7.0, -0.496)
PIPE_D = 16


def direct(ofdm, dev, c, cp, sc16_scale=None):
    """What a CFO pipeline with the search on enqueues per CHUNK-frame chunk, called directly."""
    F, S, R, Cp = c["y"].shape
    C = Cp - cp
    X = to_dev(c["X"], dev)
    out = nan_out((F, S - 1, C - 1), dev)
    for f0 in range(0, F, CHUNK):
        n = min(CHUNK, F - f0)
        if sc16_scale is None:
            y = to_dev(c["y"][f0:f0 + n], dev)
        else:
            y = ofdm.iq_convert_sc16(to_dev(c["q"][f0:f0 + n], dev), sc16_scale)
        ws = ofdm.workspace(n, S, R, C, dev)
        eps = ofdm.frame_cfo_estimate(y, cp, 1)
        ofdm.frame_cfo_acquire(y, X, cp, PIPE_D, eps=eps, out=eps)
        if C == 1024:
            ofdm.frame_demod_cfo(y, X, cp, eps, ws=ws, out=out[f0:f0 + n])
        else:
            ofdm.frame_cfo_derotate(y, cp, eps, out=y)
            ofdm.frame_demod(y, X, cp, ws=ws, out=out[f0:f0 + n])
    return host(out)


def pipeline_checks(ofdm, dev, oracle, c, cp, **kw):
    truth = oracle.frames_demod(c["clean"], c["X"], cp)

    def cfo_and_search(pl):
        pl.set_cfo(True, 1)
        pl.set_cfo_search(PIPE_D)

    def search_then_off(pl):
        pl.set_cfo(True, 1)
        pl.set_cfo_search(PIPE_D, 3.0)
        pl.set_cfo_search(0)

    on = piped(ofdm, c, cp, cfo_and_search, **kw)
    assert np.array_equal(bits(on), bits(direct(ofdm, dev, c, cp, sc16_scale=kw.get("scale"))))
    assert cc.decision_errors(on, truth) == 0
    cfo_only = piped(ofdm, c, cp, lambda pl: pl.set_cfo(True, 1), **kw)
    assert np.array_equal(bits(piped(ofdm, c, cp, search_then_off, **kw)), bits(cfo_only))
    assert cc.decision_errors(cfo_only, truth) > truth.size // 4  # three of the five frames are lost without it
    plain = piped(ofdm, c, cp, lambda pl: None, **kw)
    assert np.array_equal(bits(piped(ofdm, c, cp, lambda pl: pl.set_cfo_search(PIPE_D), **kw)), bits(plain))


@pytest.mark.parametrize("C", [1024, 256])
def test_pipeline_set_cfo_search(ofdm, dev, oracle, C):
    F, S, R, cp = 5, 4, 4, 16
    c = cc.frames(F, S, R, C, cp, PIPE_EPS, seed=C + 1)
    pipeline_checks(ofdm, dev, oracle, c, cp)
    with ofdm.Pipeline(S, R, C, c["X"], cp, chunk_frames=CHUNK, depth=2) as pl:
        for bad in ((-1, 2.0), (65, 2.0), (C // 4 + 1, 2.0), (4, 0.5), (4, float("nan")), (0, float("inf"))):
            with pytest.raises(ofdm.OfdmError, match=r"ofdm_pipeline_set_cfo_search failed \(-1\)"):
                pl.set_cfo_search(*bad)
        pl.set_cfo_search(min(64, C // 4), 1.0)
        pl.set_cfo_search(0)


def test_pipeline_set_cfo_search_sc16(ofdm, dev, oracle):
    """an sc16 pipeline at C = 256 searches on its converted chunk"""
    F, S, R, C, cp = 5, 4, 4, 256, 16
    c = dict(cc.frames(F, S, R, C, cp, PIPE_EPS, seed=C + 1))
    scale = float(np.float32(2.0 ** -12))
    v = np.stack([c["y"].real, c["y"].imag], -1).astype(np.float64)
    assert np.abs(v).max() < 7.9
    c["q"] = np.ascontiguousarray(np.rint(v / scale).astype(np.int16))
    pipeline_checks(ofdm, dev, oracle, c, cp, sample_format="sc16", scale=scale)


# ------------------------------------------------------------ (e) containment

class AcquireRow:
    """A row as test_containment_gpu's table holds them, kept out of that
    table: its rows are the main header's entries."""

    def __init__(self, F, S, R, C, cp, D):
        self.id = f"cfo_acquire_{F}x{S}x{R}x{C}cp{cp}D{D}"
        self.entries = ("ofdm_frame_cfo_acquire",)
        self.prefix, self.aligned = True, True
        self.key = (F, S, R, C, cp, D)

    def setup(self, env):
        F, S, R, C, cp, D = self.key
        eps = np.array([2.03, -3.2, 0.45, D - 0.45, 7.0][:F], np.float32)
        c = ac.frames(F, S, R, C, cp, eps, ac.random_pilots(C - 1, seed=C), seed=F + C)
        ein = cc.gamma_ref(c["y"], cp)[1].astype(np.float32)
        return dict(iq=np.array(c["y"]), X=np.array(c["X"]), eps_in=ein, model=ac.acquire(c["y"], c["X"], cp, D, ein, 2.0))

    def run(self, cx, d):
        F, S, R, C, cp, D = self.key
        iq, X = cx.inp("iq", d["iq"], prefix=cp, align=16), cx.inp("X", d["X"])
        ein = cx.inp("eps_in", d["eps_in"])
        cx.ofdm.frame_cfo_acquire(iq, X, cp, D, eps=ein, out=cx.out("eps_out", (F,), "float32"),
                                  shift=cx.out("shift", (F,), "int32"),
                                  metric=cx.out("metric", (F, 2 * D + 1), "float32"))

    def check(self, env, d, o):
        check_against_model((o["eps_out"], o["shift"], o["metric"]), d["model"])


ROWS = [AcquireRow(4, 2, 3, 1024, 7, 16), AcquireRow(4, 2, 3, 600, 9, 16)]  # rows of 1031 and 609 samples: 8-byte aligned


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_containment(ofdm, oracle, dev, row):
    """test_containment_gpu.test_containment's sequence on d_iq, d_X, d_eps_in,
    d_eps_out, d_shift and d_metric, each in a guarded arena of its own"""
    import test_containment_gpu as tc
    env = tc.Env(ofdm, dev, oracle)
    _, plain = tc._run(env, row, "plain")
    cx, guarded = tc._run(env, row, "guarded")
    assert set(cx.bufs) == {"iq", "X", "eps_in", "eps_out", "shift", "metric"}
    tc._contained(cx, row, "guarded")                                       # bands, every word written, inputs
    tc._same(row, "the plain and the guarded run", plain, guarded, cx.never)
    px, poisoned = tc._run(env, row, "poisoned")                            # the prefix is never read
    tc._contained(px, row, "poisoned")
    tc._same(row, "the guarded run and the run with a poisoned prefix", guarded, poisoned, px.never)
    for n, v in poisoned.items():
        assert np.isfinite(v).all(), f"{row.id}: {n} is not finite with a poisoned prefix"
    row.check(env, tc._data[row.id], plain)
    ax, at = tc._run(env, row, "aligned")                                   # each buffer at exactly its stated alignment
    tc._contained(ax, row, "aligned")
    row.check(env, tc._data[row.id], at)
    ofdm.device_status()
    tc._data.pop(row.id, None)


def test_rows_cover_the_new_header(ofdm):
    import test_containment_gpu as tc
    header = set(ofdm.header_symbols(ofdm.ACQUIRE_HEADER_PATH))
    covered = {e for r in ROWS for e in r.entries}
    excluded = {s for s in header for n in tc.EXCLUDED if s == n or (n.endswith("*") and s.startswith(n[:-1]))}
    assert covered <= header and not covered & excluded
    assert not header - covered - excluded, sorted(header - covered - excluded)
    assert not any(r.id in {t.id for t in tc.TABLE} for r in ROWS)
