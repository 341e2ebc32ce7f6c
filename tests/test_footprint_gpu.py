"""A bad sample spoils only the outputs that depend on it, and a power-of-two
scaling of the input changes no receiver output bit.

Every case runs its entry twice, clean and spoiled, on the same shape with a
workspace of the same size and freshly NaN-filled outputs, and asserts
  (a) outside the footprint (footprint_cases.py: geometry and a written
      dependency rule, never an output) every cell is finite and bit-identical
      to the clean run, compared as integer views;
  (b) inside it, every cell the CPU reference makes non-finite is non-finite
      (NaN against Inf is not compared);
  (c) the clean run passes helpers.parity against the reference at
      helpers.RTOL, so that (a) cannot be met by two equally wrong runs.
test_footprint_cpu.py pins the same footprints to the references.  Where the
header states the treatment of bad elements (soft demap, noise estimate, phase
tracker, the CFO estimators) the test asserts what the header says.

The scale tests run the clean input times 2^k: k = +-40 where an entry forms at
most second powers of its input, +-20 where it forms fourth powers (stated at
each case); P and 1 / P stay normal floats (the header's amplitude range).

Shapes are the smallest that reach each code path; the first lines of a test
assert the path from the launchers' own constants."""
import numpy as np
import pytest

import acquire_cases as ac
import cfo_cases as cc
import footprint_cases as fc
import phase_cases as pc
import soft_cases as sc
import tx_cases
from denoise_cases import ref_denoise
from footprint_cases import NAN, INF, bits, nonfinite
from helpers import parity  # its default bound is helpers.RTOL

pytestmark = pytest.mark.gpu

LS_WAVES = 4          # frame_td.hip: the LS runs 4-wave workgroups unless nframes * LS_WAVES < 2048 and R > LS_WAVES
MRC_SYMS = {1024: 8, 2048: 4}  # data symbols per MRC workgroup (hlds::WAVES, td2048::MRC_WAVES): consecutive, across frames
SC16 = 2.0 ** -15


# ------------------------------------------------------------------ helpers

def cus(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the cached inputs are read-only


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nans(shape, dev, dtype=None):
    import torch
    return torch.full(tuple(shape), float("nan"), dtype=dtype or torch.complex64, device=dev)


def ibits(t):
    import torch
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(
        {4: torch.int32, 1: torch.int8, 2: torch.int16}[(torch.view_as_real(t) if t.is_complex() else t).element_size()])


def outside_identical(got, clean, mask, label):
    """(a) on the device: got, clean tensors, mask a numpy bool array over their elements."""
    import torch
    assert tuple(got.shape) == tuple(clean.shape) == mask.shape, (label, got.shape, clean.shape, mask.shape)
    keep = ~torch.from_numpy(mask).to(got.device)
    g, c = ibits(got), ibits(clean)
    if got.is_complex():
        keep = keep.unsqueeze(-1)
    fin = torch.isfinite(torch.view_as_real(got) if got.is_complex() else got.to(torch.float32))
    ok = bool((~keep | (fin & (g == c))).all().item())
    if not ok:  # the message comes from the host statement of the same check
        fc.assert_outside_identical(host(got), host(clean), mask, label)
        raise AssertionError(label)


def all_finite(t):
    import torch
    return bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t.to(torch.float32)).all().item())


def export_all(ofdm, ws, F, S, R, C):
    import torch
    hp = [ofdm.frame_export_estimate(ws, F, S, R, C, f) for f in range(F)]
    return torch.stack([h for h, _ in hp]), torch.stack([p for _, p in hp])


# ------------------------------------------------- the receivers' entries
# an entry: (ofdm, dev, y, X, eps, shape) -> dict of device tensors; `kind` says what its input is

def e_auto(ofdm, dev, y, X, eps, shape, **kw):
    F, S, R, C, cp = shape
    return dict(out=ofdm.frame_demod(y, X, cp, out=nans((F, S - 1, C - 1), dev), **kw))


def e_two_launch(ofdm, dev, y, X, eps, shape):
    return e_auto(ofdm, dev, y, X, eps, shape, flow=ofdm.FLOW_TWO_LAUNCH)


def _with_estimate(ofdm, dev, shape, ws, res):
    F, S, R, C, cp = shape
    if F <= 8:  # the exported estimate of every frame
        res["H"], res["P"] = export_all(ofdm, ws, F, S, R, C)
    return res


def e_est_comb(ofdm, dev, y, X, eps, shape):
    F, S, R, C, cp = shape
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(y, X, cp, ws)
    out = ofdm.frame_combine(y, cp, ws, nans((F, S - 1, C - 1), dev))
    return _with_estimate(ofdm, dev, shape, ws, dict(out=out))


def e_partial(ofdm, dev, y, X, eps, shape):
    """frame_ls_partial + frame_mrc_partial + mrc_finalize over all antennas."""
    import torch
    F, S, R, C, cp = shape
    K = C - 1
    P, ws = ofdm.frame_ls_partial(y, X, cp, P=nans((F, K), dev, torch.float32))
    num = ofdm.frame_mrc_partial(y, ws, cp, num=nans((F, S - 1, K), dev))
    out = ofdm.mrc_finalize(num.view(-1), 0, S - 1, K, P, nans((F, S - 1, K), dev))
    return dict(out=out, P=P)


def e_symbols(ofdm, dev, y, X, eps, shape):
    """frame_estimate, then ofdm_symbols_demod of every frame's data symbols against its estimate."""
    import torch
    F, S, R, C, cp = shape
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(y, X, cp, ws)
    # a clone: its own 16-byte aligned allocation (a frame's symbols inside y need not be, with an odd prefix)
    return dict(out=torch.stack([ofdm.symbols_demod(y[f, 1:].clone(), ws, cp, frame=f, out=nans((S - 1, C - 1), dev))
                                 for f in range(F)]))


def e_sc16(ofdm, dev, y, X, eps, shape, scale=SC16):
    F, S, R, C, cp = shape
    return dict(out=ofdm.frame_demod_sc16(y, X, cp, scale, out=nans((F, S - 1, C - 1), dev)))


def e_sc16_est_comb(ofdm, dev, y, X, eps, shape, scale=SC16):
    F, S, R, C, cp = shape
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_sc16(y, X, cp, ws, scale)
    out = ofdm.frame_combine_sc16(y, cp, ws, nans((F, S - 1, C - 1), dev), scale)
    return _with_estimate(ofdm, dev, shape, ws, dict(out=out))


def e_cfo(ofdm, dev, y, X, eps, shape):
    F, S, R, C, cp = shape
    return dict(out=ofdm.frame_demod_cfo(y, X, cp, eps, out=nans((F, S - 1, C - 1), dev)))


def e_cfo_est_comb(ofdm, dev, y, X, eps, shape):
    F, S, R, C, cp = shape
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_cfo(y, X, cp, ws, eps)
    out = ofdm.frame_combine_cfo(y, cp, ws, nans((F, S - 1, C - 1), dev), eps)
    return _with_estimate(ofdm, dev, shape, ws, dict(out=out))


ENTRIES = {"auto": (e_auto, "f32"), "two_launch": (e_two_launch, "f32"), "est_comb": (e_est_comb, "f32"),
           "partial": (e_partial, "f32"), "symbols": (e_symbols, "f32"), "sc16": (e_sc16, "sc16"),
           "sc16_est_comb": (e_sc16_est_comb, "sc16"), "cfo": (e_cfo, "cfo"), "cfo_est_comb": (e_cfo_est_comb, "cfo")}

_inputs, _refs = {}, {}


def rx_inputs(shape, kind):
    """The clean host inputs of a receiver case: (y, X, eps); y int16 for kind sc16, eps non-zero per frame for cfo."""
    key = (shape, kind)
    if key not in _inputs:
        F, S, R, C, cp = shape
        eps = [cc.EPS_CYCLE[f % 3] for f in range(F)] if kind == "cfo" else None  # 0.03, -0.2, 0.45: never 0
        c = fc.rx_frames(F, S, R, C, cp, eps, seed=C + R)
        y = fc.to_sc16(c["y"]) if kind == "sc16" else c["y"]
        y.setflags(write=False)
        _inputs[key] = (y, c["X"], c["eps"])
    return _inputs[key]


def rx_reference(oracle, kind, y, X, eps, cp, sel=None):
    """What the entry is defined as: the oracle on the fp32 frames (sc16: on
    i16 * scale; cfo: on the frames derotated in float64), frames `sel`."""
    if sel is not None:
        y, eps = y[sel], (None if eps is None else eps[sel])
    if kind == "sc16":
        y = fc.from_sc16(y, SC16)
    elif kind == "cfo":
        y = cc.derotate_ref(y, eps, cp)
    return oracle.frames_demod(y, X, cp, nthreads=8)


def clean_reference(oracle, shape, kind):
    key = (shape, kind)
    if key not in _refs:
        y, X, eps = rx_inputs(shape, kind)
        _refs[key] = rx_reference(oracle, kind, y, X, eps, shape[4])
        _refs[key].setflags(write=False)
    return _refs[key]


def rx_case(ofdm, oracle, dev, shape, entry, fb, short=False, extra=()):
    """Clean run (c), then every placement's spoiled run (a), (b)."""
    F, S, R, C, cp = shape
    fn, kind = ENTRIES[entry]
    yh, Xh, eh = rx_inputs(shape, kind)
    y, X, eps = to_dev(yh, dev), to_dev(Xh, dev), to_dev(eh, dev)
    clean = fn(ofdm, dev, y, X, eps, shape)
    assert all(all_finite(v) for v in clean.values()), "the clean run left an element unwritten or non-finite"
    nrel, erel = parity(host(clean["out"]), clean_reference(oracle, shape, kind))
    print(f"{entry} {shape}: clean norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    spoils = list(fc.rx_placements(F, S, R, C, cp, fb, short)) + list(extra)
    if kind == "sc16":
        spoils = [sp for sp in spoils if sp["kind"] != "sample"]
    for sp in spoils:
        lab = f"{entry} {shape} {fc.label(sp)}"
        ys, Xs, es = fc.spoil_rx(y, X, eps, sp)
        got = fn(ofdm, dev, ys, Xs, es, shape)
        fp = fc.rx_footprint(sp, F, S, R, C, cp)
        for name in got:
            outside_identical(got[name], clean[name], fp[name], f"{lab} {name}")
        sel = np.flatnonzero(fp["frame"])
        if sp["kind"] == "eps":  # finite, and frame f did move
            assert all_finite(got["out"]) and not np.array_equal(host(got["out"][sp["f"]]), host(clean["out"][sp["f"]]))
        elif sel.size:
            hy, hX, he = fc.spoil_rx(yh, Xh, eh, sp)
            with np.errstate(all="ignore"):
                ref = rx_reference(oracle, kind, hy, hX, he, cp, sel)
            fc.assert_inside_nonfinite(host(got["out"])[sel], ref, fp["out"][sel], lab)
            if "H" in got and sp["kind"] != "silent":  # the estimate's footprint turns non-finite whole
                assert nonfinite(host(got["H"]))[fp["H"]].all() and nonfinite(host(got["P"]))[fp["P"]].all(), lab
            if "P" in got and sp["kind"] == "silent":
                assert not host(got["P"])[sp["f"]].any(), lab


def eps_spoils(F, fb):
    """eps_change on the frames a straddling workgroup shares, the first and the last."""
    return [fc.eps_change(f, v) for f, v in ((fb, 0.11), (fb + 1, -0.3), (0, 0.25), (F - 1, 0.0))]


# ------------------------------------------------------------ C = 1024

C1024_ENTRIES = ["auto", "two_launch", "est_comb", "partial", "symbols", "sc16", "sc16_est_comb", "cfo", "cfo_est_comb"]


@pytest.mark.parametrize("entry", C1024_ENTRIES)
@pytest.mark.parametrize("R", [5, 17])
def test_c1024_straddling_workgroups(ofdm, oracle, dev, entry, R):
    """(F, S, R, cp) = (5, 6, R, 8): S - 1 = 5 data symbols against 8 per MRC
    workgroup, so workgroups straddle frames and take the per-wave Hc path; the
    16-wave LS (R = 17: more antenna rows than waves, a second pass)."""
    shape = (5, 6, R, 1024, 8)
    F, S = shape[:2]
    fb = fc.straddle_frame(F, S, MRC_SYMS[1024])
    assert (S - 1) % MRC_SYMS[1024] and fb == 0 and F * LS_WAVES < 2048 and R > LS_WAVES and (R == 5 or R > 16)
    extra = eps_spoils(F, fb) if entry.startswith("cfo") else ()
    rx_case(ofdm, oracle, dev, shape, entry, fb, extra=extra)


@pytest.mark.parametrize("entry", ["auto", "two_launch", "est_comb", "sc16", "cfo"])
@pytest.mark.parametrize("R", [2, 5])
def test_c1024_four_wave_ls(ofdm, oracle, dev, entry, R):
    """The other side of the LS launcher's choice: 4-wave workgroups, by the
    batch size (R = 5 > LS_WAVES, the smallest F with F * LS_WAVES >= 2048) and
    by the row count (R = 2 <= LS_WAVES at the same F); S = 3."""
    F = 2048 // LS_WAVES
    shape = (F, 3, R, 1024, 8)
    assert not (F * LS_WAVES < 2048 and R > LS_WAVES) and (F - 1) * LS_WAVES < 2048
    fb = fc.straddle_frame(F, 3, MRC_SYMS[1024])
    assert fb == 0
    extra = eps_spoils(F, fb)[:2] if entry == "cfo" else ()
    rx_case(ofdm, oracle, dev, shape, entry, fb, short=True, extra=extra)


def ticketed_frames(dev, nsym):
    """The smallest F whose one-launch demod deals whole-block tickets AND
    half units (launch_demod_td1024: k1 = ticket_k0(2) = 2 * CUs / 8 static
    blocks per XCD range per round, k0 = 2 k1 static, the last k1 of a range in
    half units): blocks per range > k0 + k1."""
    k1 = 2 * cus(dev) // 8
    nb = 8 * (3 * k1) + 1
    return -(-nb * MRC_SYMS[1024] // nsym), k1


@pytest.mark.parametrize("entry", ["auto", "two_launch", "est_comb", "sc16", "cfo"])
def test_c1024_past_the_ticket_threshold(ofdm, oracle, dev, entry):
    """100 data symbols a frame, R = 2, as test_pipeline_ticketed_chunks_with_
    short_tail; the frame count from the launcher's constants (48 frames are
    600 blocks, which two static rounds of 4 x CUs blocks absorb on a 256-CU
    device: no ticket would be taken)."""
    S, R = 101, 2
    F, k1 = ticketed_frames(dev, S - 1)
    nb = -(-F * (S - 1) // MRC_SYMS[1024])
    per = (nb + 7) // 8
    assert per > 2 * k1 + k1, "tickets and half units are dealt"
    fb = fc.straddle_frame(F, S, MRC_SYMS[1024])
    assert fb == 0  # 100 symbols are 12.5 workgroups
    extra = eps_spoils(F, fb)[:2] if entry == "cfo" else ()
    rx_case(ofdm, oracle, dev, (F, S, R, 1024, 0), entry, fb, short=True, extra=extra)


# -------------------------------------------------------- the other sizes

H_PAIRS = 4  # frame_td4096.hip: data symbols per MRC block; ceil((S - 1) / H_PAIRS) blocks PER FRAME, none spans two


@pytest.mark.parametrize("entry", ["auto", "est_comb", "partial", "symbols"])
@pytest.mark.parametrize("C", [2048, 4096])
def test_c2048_c4096(ofdm, oracle, dev, C, entry):
    """C = 2048: 4 consecutive data symbols per MRC workgroup against 5 per
    frame, so workgroups straddle frames.  C = 4096: blocks are dealt per frame
    and never straddle; S - 1 = 5 leaves a ragged second block (one symbol of
    H_PAIRS), which the last-element placements hit; the frame 0 | 1 placements
    stay as plain neighbours."""
    F, S = 4, 6
    if C == 2048:
        assert fc.straddle_frame(F, S, MRC_SYMS[2048]) == 0
    else:
        assert (S - 1) % H_PAIRS == 1
    rx_case(ofdm, oracle, dev, (F, S, 3, C, 7), entry, 0)


# frame_td_fft512.hip, kLane512.per_wg: the data symbols a workgroup owns at a time (consecutive, across frames)
LANE_SYMS = {128: 4, 256: 4, 512: 4, 1536: 4, 3072: 1, 6144: 1}


@pytest.mark.parametrize("entry", ["auto", "est_comb", "partial"])
@pytest.mark.parametrize("C", list(LANE_SYMS))
def test_lane_order_sizes(ofdm, oracle, dev, C, entry):
    """k_mrc_td128 ... k_mrc_td6144: q += nw and the prefetch of the next
    symbol's rows.  Up to C = 1536 a workgroup's 4 waves take 4 consecutive data
    symbols against 7 per frame: the second workgroup spans frames 0 | 1.  At
    C = 3072 and 6144 a workgroup owns one symbol at a time: no workgroup
    straddles, the frame 0 | 1 placements sit on the symbols one workgroup's
    loop takes one after the other (the prefetched next rows)."""
    F, S = 5, 8
    if LANE_SYMS[C] > 1:
        assert fc.straddle_frame(F, S, LANE_SYMS[C]) == 0
    rx_case(ofdm, oracle, dev, (F, S, 3, C, 5), entry, 0)


def any_cap(C):
    return 2048 if C <= 2048 else 4096 if C <= 4096 else 8192


@pytest.mark.parametrize("entry", ["auto", "est_comb", "partial"])
@pytest.mark.parametrize("C", [600, 3000, 5000, 6])
def test_any_c(ofdm, oracle, dev, C, entry):
    """k_fft_any over the pilot rows (G = cap / C rows per group, fft_any.hip)
    and k_mrc_any (one data symbol per workgroup at a time: no straddling
    there).  C = 600: G = 3 = R, the pilot rows of a frame ARE a group; the
    frame 1 | 2 placements put the spoil in its middle row (r = 1) and the
    exported estimate's footprint H[f, 1] leaves its two neighbours to (a).
    C = 6: G = 341, one group holds the pilot rows of all five frames.
    C = 3000, 5000: one row per group."""
    F, S, R = 5, 6, 3
    G = any_cap(C) // C
    assert G == {600: 3, 3000: 1, 5000: 1, 6: 341}[C]
    if C == 600:
        assert G == R and fc.rx_placements(F, S, R, C, 5, 1)[1]["r"] == 1
    if C == 6:
        assert G >= F * R
    rx_case(ofdm, oracle, dev, (F, S, R, C, 5), entry, 1)


# ------------------------------------------------- frequency-domain entries

def f_demod(ofdm, dev, Y, X, shape):
    F, S, R, C = shape
    return dict(out=ofdm.frame_demod_freq(Y, X, out=nans((F, S - 1, C - 1), dev)))


def f_mfma(ofdm, dev, Y, X, shape):
    F, S, R, C = shape
    return dict(out=ofdm.frame_demod_freq_mfma(Y, X, out=nans((F, S - 1, C - 1), dev)))


def f_est_comb(ofdm, dev, Y, X, shape):
    F, S, R, C = shape
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_freq(Y, X, ws)
    out = ofdm.frame_combine_freq(Y, ws, nans((F, S - 1, C - 1), dev))
    H, P = export_all(ofdm, ws, F, S, R, C)
    return dict(out=out, H=H, P=P)


FREQ_ENTRIES = {"demod": f_demod, "est_comb": f_est_comb, "mfma": f_mfma}


# frame_demod_freq_mfma takes multiples of 64 only (OFDM_E_UNSUPPORTED otherwise)
FREQ_CASES = [(C, R, e) for C in (64, 600, 1024) for R in (3, 16) for e in FREQ_ENTRIES if not (e == "mfma" and C % 64)]


@pytest.mark.parametrize("C,R,entry", FREQ_CASES)
def test_frequency_domain(ofdm, oracle, dev, C, R, entry):
    F, S = 4, 4
    shape = (F, S, R, C)
    c = fc.rx_frames(F, S, R, C, 0, seed=C + R)
    Yh = np.fft.fft(c["y"].astype(np.complex128), axis=-1).astype(np.complex64)
    Y, X = to_dev(Yh, dev), to_dev(c["X"], dev)
    fn = FREQ_ENTRIES[entry]
    clean = fn(ofdm, dev, Y, X, shape)
    assert all(all_finite(v) for v in clean.values())
    parity(host(clean["out"]), oracle.frames_demod_freq(Yh, c["X"]))
    for sp in fc.freq_placements(F, S, R, C, 1):
        lab = f"freq {entry} {shape} {fc.label(sp)}"
        Ys, Xs = fc.spoil_freq(Y, X, sp)
        got = fn(ofdm, dev, Ys, Xs, shape)
        fp = fc.rx_footprint(sp, F, S, R, C, freq=True)
        for name in got:
            outside_identical(got[name], clean[name], fp[name], f"{lab} {name}")
        hY, hX = fc.spoil_freq(Yh, c["X"], sp)
        with np.errstate(all="ignore"):
            fc.assert_inside_nonfinite(host(got["out"]), oracle.frames_demod_freq(hY, hX), fp["out"], lab)


def stage_run(ofdm, dev, entry, d):
    if entry == "ls":
        H, P = ofdm.ls_estimate(d["Yp"], d["X"])
        return dict(H=H, P=P)
    if entry == "mrc":
        return dict(out=ofdm.mrc_demod(d["Yd"], d["H"], d["P"]))
    if entry == "numerator":
        return dict(num=ofdm.mrc_numerator(d["Yd"], d["H"]))
    if entry == "conj_product":
        return dict(prod=ofdm.channel_conj_product(d["Yd"], d["H"]))
    if entry == "combine":
        return dict(out=ofdm.combine_products(d["prod"], d["P"]))
    return dict(P=ofdm.dist_sqrd(d["H"]))


@pytest.mark.parametrize("R", [3, 16])
@pytest.mark.parametrize("C", [64, 600, 1024])
def test_stage_entries(ofdm, dev, C, R):
    """ls_estimate, mrc_demod, mrc_numerator, channel_conj_product,
    combine_products, dist_sqrd against their float64 statements."""
    n = 5
    h = fc.stage_inputs(n, R, C, seed=C + R)
    h = dict(h, prod=fc.ref_conj_product(h["Yd"], h["H"]))
    d = {k: to_dev(v, dev) for k, v in h.items()}
    clean = {}
    for entry in ("ls", "mrc", "numerator", "conj_product", "combine", "dist"):
        clean[entry] = stage_run(ofdm, dev, entry, d)
        ref = fc.stage_reference(entry, h)
        for name, v in clean[entry].items():
            assert all_finite(v)
            parity(host(v), ref[name])
    for entry, name, idx, masks in fc.stage_cases(n, R, C):
        for value in (NAN,) if name in ("X", "P") else (NAN, INF):  # dividing by Inf gives a finite 0
            lab = f"{entry} {name}{idx} C={C} R={R}"
            x, xh = d[name].clone(), np.array(h[name])
            x[idx] = value if x.is_complex() else value.real
            xh[idx] = value if np.iscomplexobj(xh) else value.real
            got = stage_run(ofdm, dev, entry, dict(d, **{name: x}))
            ref = fc.stage_reference(entry, dict(h, **{name: xh}))
            for out, mask in masks.items():
                outside_identical(got[out], clean[entry][out], mask, f"{lab} {out}")
                fc.assert_inside_nonfinite(host(got[out]), ref[out], mask, f"{lab} {out}")


# ------------------------------------------------------------ FFT, modulator

@pytest.mark.parametrize("C", [1024, 600, 5000])
def test_fft_rows_and_modulator(ofdm, dev, C):
    """Nine rows (C = 600: three groups of three; row 4 is the middle row of
    its group), the spoil in row 4 and in the last row."""
    import torch
    nrows, cp = 9, 5
    xh, Xh = fc.rows_input(nrows, C), fc.rows_input(nrows, C - 1, seed=1)
    x, X = to_dev(xh, dev), to_dev(Xh, dev)
    fwd = lambda t, inv: ofdm.fft_rows(t, nans((nrows, C), dev), inverse=inv)
    modes = (("rx", "scale"), ("reference", "peak"))
    tx = lambda t, m: ofdm.tx_modulate(t, C, cp, m[0], m[1], 0.25, return_peak=True, out=nans((nrows, C + cp), dev))
    c_f, c_i, c_tx = fwd(x, False), fwd(x, True), {m: tx(X, m) for m in modes}
    tol = 2e-6 * np.log2(C)  # test_fft_rows_any_c_vs_numpy's bound
    for got, inv in ((c_f, False), (c_i, True)):
        ref = fc.ref_fft_rows(xh, inv).astype(np.complex128)
        assert all_finite(got) and np.abs(host(got) - ref).max() <= tol * np.abs(ref).max()
    for m in modes:
        want, wpeak = tx_cases.tx_numpy(Xh, C, cp, m[0], m[1], 0.25)
        parity(host(c_tx[m][0]), want)
        assert np.allclose(host(c_tx[m][1]), wpeak, rtol=1e-5, atol=0)
    for row, col, value in fc.row_placements(nrows, C - 1):
        xs, Xs = x.clone(), X.clone()
        xs[row, col] = value
        Xs[row, col] = value
        lab = f"C={C} row {row} col {col}"
        for inv, clean in ((False, c_f), (True, c_i)):
            got = fwd(xs, inv)
            outside_identical(got, clean, fc.row_footprint(nrows, C, row), f"fft_rows inverse={inv} {lab}")
            assert nonfinite(host(got[row])).all(), lab  # the reference: the whole row (test_footprint_cpu)
        for m in modes:
            got, peak = tx(Xs, m)
            outside_identical(got, c_tx[m][0], fc.row_footprint(nrows, C + cp, row), f"tx_modulate {m} {lab}")
            outside_identical(peak, c_tx[m][1], fc.row_footprint(nrows, 1, row)[:, 0], f"tx_modulate {m} peak {lab}")
            # the header: non-finite inputs propagate (the float64 statement: the whole row and its peak)
            assert nonfinite(host(got[row])).all() and nonfinite(host(peak[row:row + 1])).all(), f"{m} {lab}"


# ------------------------------------------------------------ zero forcing

def test_zf_shapes_reach_every_kernel():
    """The dispatch of zf.hip restated (footprint_cases.zf_detect_kernel /
    zf_apply_kernel): the shapes of test_zf_apply_detect select every detect and
    apply kernel -- the 2-, 4- and 8-row wave tiles with 1, 2 and 4 row groups,
    k_zf_wstat, both MFMA tiles, k_zf_gemm_lds and both k_zf_apply_ws16 tiles."""
    shapes = fc.ZF_SHAPES + fc.ZF_DEGENERATE
    assert {fc.zf_detect_kernel(U, R, K) for U, R, K, _ in shapes} == fc.ZF_DETECT_KERNELS
    assert {fc.zf_apply_kernel(U, R, K) for U, R, K, _ in shapes} == fc.ZF_APPLY_KERNELS


@pytest.mark.parametrize("U,R,K,n", fc.ZF_SHAPES + fc.ZF_DEGENERATE)
def test_zf_apply_detect(ofdm, oracle, dev, U, R, K, n):
    d = fc.zf_inputs(U, R, K, n, precoder=(U, R, K, n) in fc.ZF_SHAPES)
    Wt = ofdm.zf_transpose(to_dev(d["W"], dev))
    X, Y = to_dev(d["X"], dev), to_dev(d["Y"], dev)
    run = {"detect": lambda w, x, y: ofdm.zf_detect(w, y, out=nans((n, U, K), dev)),
           "apply": lambda w, x, y: ofdm.zf_apply(w, x, out=nans((n, R, K), dev))}
    ref = {"detect": lambda W, x, y: oracle.zf_detect(W, y), "apply": lambda W, x, y: oracle.zf_apply(W, x)}
    clean = {e: run[e](Wt, X, Y) for e in run}
    for e in run:
        assert all_finite(clean[e])
        parity(host(clean[e]), ref[e](d["W"], d["X"], d["Y"]))
    for entry, name, idx, mask in fc.zf_cases_of(U, R, K, n):
        for value in (NAN, INF):
            lab = f"zf_{entry} {(U, R, K, n)} {name}{idx}"
            w, x, y = Wt, X, Y
            Wh, xh, yh = d["W"], d["X"], d["Y"]
            if name == "Wt":
                w, Wh = Wt.clone(), d["W"].copy()
                w[idx] = value
                Wh[idx[2], idx[0], idx[1]] = value
            elif name == "Y":
                y, yh = Y.clone(), d["Y"].copy()
                y[idx], yh[idx] = value, value
            else:
                x, xh = X.clone(), d["X"].copy()
                x[idx], xh[idx] = value, value
            got = run[entry](w, x, y)
            outside_identical(got, clean[entry], mask, lab)
            fc.assert_inside_nonfinite(host(got), ref[entry](Wh, xh, yh), mask, lab)


# (U, R, K, n, ld of the input, ld of the output): test_zf_detect_pitched's and test_zf_apply_pitched's, n <= 9
@pytest.mark.parametrize("entry,U,R,K,n,ld_in,ld_out", [
    ("detect", 16, 64, 1023, 9, 1024, 1024), ("detect", 16, 64, 1023, 9, 1023, 1024), ("detect", 16, 64, 1023, 9, 1030, 1023),
    ("detect", 4, 16, 1023, 9, 1024, 1040), ("detect", 24, 40, 200, 9, 208, 201), ("detect", 9, 72, 65, 9, 80, 72),
    ("apply", 16, 64, 1023, 9, 1024, 1024), ("apply", 16, 64, 1023, 9, 1023, 1024), ("apply", 24, 16, 130, 9, 144, 131),
    ("apply", 4, 8, 2, 5, 16, 3)])
def test_zf_pitched(ofdm, oracle, dev, entry, U, R, K, n, ld_in, ld_out):
    """ofdm_zf_detect_ex / ofdm_zf_apply_ex on row-padded layouts: the same
    footprints over the first K columns; the input's pads hold NaN throughout
    (they are never read) and the output's pads keep their sentinel."""
    import torch
    d = fc.zf_inputs(U, R, K, n, precoder=R >= U)  # fewer antennas than users: no precoder exists, a seeded W
    Wt = ofdm.zf_transpose(to_dev(d["W"], dev))
    rows_in, rows_out = (R, U) if entry == "detect" else (U, R)
    src = d["Y"] if entry == "detect" else d["X"]
    call = ofdm.zf_detect_pitched if entry == "detect" else ofdm.zf_apply_pitched
    ref = (lambda W, a: oracle.zf_detect(W, a)) if entry == "detect" else (lambda W, a: oracle.zf_apply(W, a))

    def run(w, a):
        padded = nans((n, rows_in, ld_in), dev)
        padded[:, :, :K] = a
        out = call(w, padded, out=torch.full((n, rows_out, ld_out), 7.0, dtype=torch.complex64, device=dev))
        assert bool((out[:, :, K:] == 7.0).all()), "a pad of the output was written"
        return out[:, :, :K].contiguous()

    A = to_dev(src, dev)
    clean = run(Wt, A)
    assert all_finite(clean)
    parity(host(clean), ref(d["W"], src))
    for e, name, idx, mask in fc.zf_cases_of(U, R, K, n):
        if e != entry:
            continue
        for value in (NAN, INF):
            lab = f"zf_{entry}_ex {(U, R, K, n, ld_in, ld_out)} {name}{idx}"
            w, a, Wh, ah = Wt, A, d["W"], src
            if name == "Wt":
                w, Wh = Wt.clone(), d["W"].copy()
                w[idx] = value
                Wh[idx[2], idx[0], idx[1]] = value
            else:
                a, ah = A.clone(), src.copy()
                a[idx], ah[idx] = value, value
            got = run(w, a)
            outside_identical(got, clean, mask, lab)
            fc.assert_inside_nonfinite(host(got), ref(Wh, ah), mask, lab)


@pytest.mark.parametrize("U,R,K", [(1, 1, 5), (4, 16, 1023), (16, 64, 255), (3, 7, 100), (2, 2, 1)])
def test_zf_precoder(ofdm, oracle, dev, U, R, K):
    """H[u, r, k] reaches subcarrier k's matrix alone, in both layouts."""
    import zf_cases
    Hh = zf_cases.channel(U, R, K, seed=U * 7 + R + K)
    H = to_dev(Hh, dev)
    run = lambda h: ofdm.zf_precoder(h, W=nans((K, U, R), dev), Wt=nans((U, R, K), dev))
    W0, Wt0 = run(H)
    assert all_finite(W0) and all_finite(Wt0)
    assert np.array_equal(host(W0), oracle.zf_precoder(Hh))  # test_zf_precoder_parity's bound: the oracle's bits
    for u, r, k in ((0, 0, 0), (U - 1, R - 1, K - 1), (U // 2, R // 2, K // 2)):
        for value in (NAN, INF):
            Hs, Hr = H.clone(), Hh.copy()
            Hs[u, r, k], Hr[u, r, k] = value, value
            W, Wt = run(Hs)
            fp = fc.zf_precoder_footprint(U, R, K, k)
            lab = f"zf_precoder {(U, R, K)} H{(u, r, k)}"
            outside_identical(W, W0, fp["W"], lab + " W")
            outside_identical(Wt, Wt0, fp["Wt"], lab + " Wt")
            with np.errstate(all="ignore"):
                ref = oracle.zf_precoder(Hr)
            fc.assert_inside_nonfinite(host(W), ref, fp["W"], lab + " W")
            fc.assert_inside_nonfinite(host(Wt), np.ascontiguousarray(ref.transpose(1, 2, 0)), fp["Wt"], lab + " Wt")


# ------------------------------- soft output, phase tracker, CFO, denoiser

def soft_setup(ofdm, dev, shape, seed=0):
    F, S, R, C, cp = shape
    c = fc.rx_frames(F, S, R, C, cp, seed=seed + C)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.frame_demod(to_dev(c["y"], dev), to_dev(c["X"], dev), cp, ws=ws)
    return ws, z


def z_placements(F, N, K):
    return [(0, 0, 0), (F - 1, N - 1, K - 1), (1, N - 1, K // 2), (2, 0, 0)]


@pytest.mark.parametrize("shape,bps", [((5, 6, 3, 1024, 8), 2), ((5, 6, 3, 64, 4), 6), ((4, 3, 2, 600, 5), 4)])
def test_soft_output_chain(ofdm, dev, shape, bps):
    """frame_noise_estimate and frame_soft_demap on z with one bad element
    (f, s, k).  The header: a non-finite z makes noise_var[f] non-finite, the
    demapper then zeroes frame f's LLRs (noise_var not positive and finite);
    with a good noise_var the element's own LLRs are non-finite (f32; in int8
    a NaN is stored as 0, an Inf clamps); every other frame, and element, is
    bit-identical."""
    import torch
    F, S, R, C, cp = shape
    N, K = S - 1, C - 1
    ws, z = soft_setup(ofdm, dev, shape)
    nv0 = ofdm.frame_noise_estimate(z, ws, F, S, R, C, bps, out=nans((F,), dev, torch.float32))
    demap = lambda zz, nv, fmt: ofdm.frame_soft_demap(
        zz, ws, F, S, R, C, bps, nv, fmt, 8.0,
        out=torch.full((F, N, K, bps), -128 if fmt == "i8" else float("nan"), device=dev,
                       dtype=torch.int8 if fmt == "i8" else torch.float32))
    l0, q0 = demap(z, nv0, "f32"), demap(z, nv0, "i8")
    assert all_finite(nv0) and all_finite(l0) and bool((nv0 > 0).all()) and bool((q0 != -128).all())
    # (c): the float64 statement on the device's own z and P, at test_soft_demap_gpu's bounds
    Zh, nvh = host(z), host(nv0).astype(np.float64)
    Pk = host(export_all(ofdm, ws, F, S, R, C)[1]).astype(np.float64)[:, sc.out_src(K)][:, None, :]
    assert np.all(np.abs(nvh - sc.ref_noise_var(Zh, Pk, bps)) <= 1e-5 * sc.ref_noise_var(Zh, Pk, bps))
    scale = Pk / nvh[:, None, None]
    ref, bound = sc.ref_llr(Zh, scale, bps), sc.llr_bound(Zh, scale)
    assert np.all(np.abs(host(l0).astype(np.float64) - ref) <= bound)
    assert np.all(np.abs(host(q0) - np.clip(np.rint(ref * 8.0), -127, 127)) <= 1)
    for f, s, k in z_placements(F, N, K):
        for value in (NAN, INF):
            lab = f"soft {shape} z[{f},{s},{k}]={value}"
            zs = z.clone()
            zs[f, s, k] = value
            fm = np.zeros(F, bool)
            fm[f] = True
            em = np.zeros((F, N, K, bps), bool)
            em[f, s, k] = True
            nv = ofdm.frame_noise_estimate(zs, ws, F, S, R, C, bps, out=nans((F,), dev, torch.float32))
            outside_identical(nv, nv0, fm, lab + " noise_var")
            assert not np.isfinite(host(nv)[f]), lab
            lf, lq = demap(zs, nv0, "f32"), demap(zs, nv0, "i8")
            outside_identical(lf, l0, em, lab + " llr f32")
            outside_identical(lq, q0, em, lab + " llr i8")
            assert nonfinite(host(lf)[f, s, k]).any(), lab
            if value is NAN:  # an Inf z has LLRs of +-Inf and 0, which the int8 format clamps as the header says
                assert not host(lq)[f, s, k].any(), lab + ": a NaN LLR is stored as 0"
            whole = np.zeros((F, N, K, bps), bool)
            whole[f] = True
            for fmt, base in (("f32", l0), ("i8", q0)):
                got = demap(zs, nv, fmt)
                outside_identical(got, base, whole, lab + f" llr {fmt}, noise_var from the spoiled z")
                assert not host(got)[f].any(), lab + ": the header's llr = 0"


@pytest.mark.parametrize("shape,bps", [((5, 6, 3, 1024, 8), 2), ((5, 6, 3, 64, 4), 4)])
def test_phase_tracker_other_frames(ofdm, dev, shape, bps):
    """One bad element of z: non-finite in that element alone (the header's
    step 4), later rows of ITS frame may move, every other frame is bit-identical."""
    import torch
    F, S, R, C, cp = shape
    N, K = S - 1, C - 1
    ws, _ = soft_setup(ofdm, dev, shape)
    z = to_dev(pc.case(F, N, K, bps, 0.03, 0.005, 25)["z"], dev)

    def run(zz):
        ph = nans((F, N), dev, torch.float32)
        return ofdm.frame_phase_track(zz, ws, F, S, R, C, bps, out=nans((F, N, K), dev), phase=ph), ph

    o0, p0 = run(z)
    assert all_finite(o0) and all_finite(p0)
    # (c): the model of phase_cases on the same z and the device's P, at test_phase_track_gpu's bounds
    from test_phase_track_gpu import check as check_model
    Pw = pc.p_by_position(host(export_all(ofdm, ws, F, S, R, C)[1]))
    m_out, m_phase, _ = check_model(ofdm, dev, ws, Pw, host(z), (F, S, R, C), bps, f"phase_track {shape}")
    assert np.array_equal(bits(m_out), bits(host(o0))) and np.array_equal(bits(m_phase), bits(host(p0)))
    for f, s, k in z_placements(F, N, K):
        zs = z.clone()
        zs[f, s, k] = NAN
        o, p = run(zs)
        om = np.zeros((F, N, K), bool)
        om[f, s:] = True
        pm = np.zeros((F, N), bool)
        pm[f, s:] = True
        outside_identical(o, o0, om, f"phase_track {shape} z[{f},{s},{k}] out")
        outside_identical(p, p0, pm, f"phase_track {shape} z[{f},{s},{k}] phase")
        bad = nonfinite(host(o))
        assert bad[f, s, k] and bad.sum() == 1 and all_finite(p)


@pytest.mark.parametrize("C,cp", [(1024, 8), (600, 5)])
def test_cfo_estimators(ofdm, dev, C, cp):
    """frame_cfo_estimate reads the first and last cp samples of a row: a NaN
    there makes gamma[f] and eps[f] NaN (the header); frame_cfo_acquire reads
    the pilot symbol past its prefix: no finite metric, shift 0, eps passed
    through (ofdm_lsmrc_acquire.h's model).  A sample neither reads changes
    nothing; every other frame is bit-identical."""
    import torch
    F, S, R, D = 5, 4, 3, 3
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004, 0.1], seed=C)
    y, X, eps = to_dev(c["y"], dev), to_dev(c["X"], dev), to_dev(c["eps"], dev)

    def run(yy):
        g, e = nans((F,), dev), nans((F,), dev, torch.float32)
        ofdm.frame_cfo_estimate(yy, cp, eps=e, gamma=g)
        o = nans((F,), dev, torch.float32)
        sh = torch.full((F,), -99, dtype=torch.int32, device=dev)
        m = nans((F, 2 * D + 1), dev, torch.float32)
        ofdm.frame_cfo_acquire(yy, X, cp, D, eps=eps, out=o, shift=sh, metric=m)
        return dict(gamma=g, eps=e, out=o, shift=sh, metric=m)

    clean = run(y)
    assert all(all_finite(v) for v in clean.values())
    # (c): test_estimator's bounds (gamma 1e-5 relative, eps 1e-5 / 2 pi) and test_cfo_acquire_gpu's
    # check_against_model (shift and eps_out equal, metric within RTOL of the peak, the model's margin >= 3)
    from test_cfo_acquire_gpu import check_against_model
    g_ref, e_ref = cc.gamma_ref(c["y"], cp)
    assert np.all(np.abs(host(clean["gamma"]) - g_ref) <= 1e-5 * np.abs(g_ref))
    assert np.all(np.abs(host(clean["eps"]).astype(np.float64) - e_ref) <= 1e-5 / (2 * np.pi))
    check_against_model((host(clean["out"]), host(clean["shift"]), host(clean["metric"])),
                        ac.acquire(c["y"], c["X"], cp, D, c["eps"]))
    for f, s, r, i, by_cp, by_acq in ((0, 0, 0, 0, True, False), (F - 1, S - 1, R - 1, C + cp - 1, True, False),
                                      (1, 0, 1, cp + C // 2, False, True), (2, S - 1, R - 1, cp - 1, True, False),
                                      (2, 1, 1, cp + 3, False, False), (F - 1, 0, R - 1, C - 1, False, True)):
        ys = y.clone()
        ys[f, s, r, i] = NAN
        got = run(ys)
        fm = np.zeros(F, bool)
        fm[f] = True
        lab = f"cfo C={C} y[{f},{s},{r},{i}]"
        for name in ("gamma", "eps"):
            outside_identical(got[name], clean[name], fm & by_cp, f"{lab} {name}")
        for name in ("out", "shift"):
            outside_identical(got[name], clean[name], fm & by_acq, f"{lab} {name}")
        outside_identical(got["metric"], clean["metric"], np.repeat(fm[:, None] & by_acq, 2 * D + 1, axis=1), f"{lab} metric")
        if by_cp:
            assert np.isnan(host(got["eps"])[f]) and nonfinite(host(got["gamma"])[f])
        if by_acq:
            assert nonfinite(host(got["metric"])[f]).all() and host(got["shift"])[f] == 0
            assert np.array_equal(bits(host(got["out"])[f:f + 1]), bits(c["eps"][f:f + 1]))


@pytest.mark.parametrize("C", [1024, 600])
def test_cfo_derotate_eps_change(ofdm, dev, C):
    F, S, R, cp = 5, 4, 3, 5
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004, 0.1], seed=C)
    y, eps = to_dev(c["y"], dev), to_dev(c["eps"], dev)
    clean = ofdm.frame_cfo_derotate(y, cp, eps, out=nans((F, S, R, C + cp), dev))
    parity(host(clean), cc.derotate_ref(c["y"], c["eps"], cp))
    for f in (0, 2, F - 1):
        e = eps.clone()
        e[f] = 0.11
        got = ofdm.frame_cfo_derotate(y, cp, e, out=nans((F, S, R, C + cp), dev))
        m = np.zeros((F, S, R, C + cp), bool)
        m[f] = True
        outside_identical(got, clean, m, f"derotate C={C} eps[{f}]")
        assert all_finite(got) and not np.array_equal(host(got[f]), host(clean[f]))


@pytest.mark.parametrize("C", [1024, 600])
def test_denoise_rows(ofdm, dev, C):
    """frame_estimate_denoise keeps 8 rows in flight per workgroup: a NaN pilot
    sample of (f, 0, r) reaches the estimate rows of (f, r) and P[f] alone."""
    F, S, R, cp, taps = 5, 3, 3, 5, 16
    shape = (F, S, R, C, cp)
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    X = to_dev(c["X"], dev)

    def run(yy, before=None):
        ws = ofdm.workspace(F, S, R, C, dev)
        ofdm.frame_estimate(yy, X, cp, ws)
        if before is not None:
            before.append(host(export_all(ofdm, ws, F, S, R, C)[0]))
        ofdm.frame_estimate_denoise(ws, F, S, R, C, taps, 4)
        return export_all(ofdm, ws, F, S, R, C)

    y = to_dev(c["y"], dev)
    raw = []
    H0, P0 = run(y, raw)
    assert all_finite(H0) and all_finite(P0)
    # (c): the float64 statement on the estimate as it was before, as test_denoise_gpu.check_denoise
    Href, Pref = ref_denoise(raw[0], C, taps, 4)
    parity(host(H0), Href)
    parity(host(P0), Pref)
    for f, r, i in ((0, 0, cp), (F - 1, R - 1, C + cp - 1), (2, 1, cp + C // 2), (1, 2, cp + 1)):
        ys = y.clone()
        ys[f, 0, r, i] = NAN
        H, P = run(ys)
        fp = fc.rx_footprint(fc.sample(f, 0, r, i), *shape)
        outside_identical(H, H0, fp["H"], f"denoise C={C} y[{f},0,{r},{i}] H")
        outside_identical(P, P0, fp["P"], f"denoise C={C} y[{f},0,{r},{i}] P")
        assert nonfinite(host(H))[fp["H"]].all() and nonfinite(host(P))[fp["P"]].all()


# ------------------------------------------------------------ the pipeline

PIPE = {"plain": lambda p: None, "denoise": lambda p: p.set_denoise(16, 4), "cfo": lambda p: p.set_cfo(True),
        "phase_track": lambda p: p.set_phase_track(2)}


@pytest.mark.parametrize("configure", list(PIPE))
@pytest.mark.parametrize("C", [1024, 600])
def pipeline_reference(ofdm, oracle, dev, c, cp, configure):
    """What a pass is defined as, from the oracle and the float64 statements:
    plain: the oracle; denoise (16, 4): the oracle's estimate through
    ref_denoise, then the float64 MRC; cfo: the oracle on the frames derotated in
    float64 by the device's own prefix estimates (each taken exactly, as the
    header defines the *_cfo entries; the estimates themselves are
    test_cfo_estimators'); phase_track: the tracker's model on the oracle's output."""
    y, X = c["y"], c["X"]
    C = y.shape[-1] - cp
    if configure == "plain":
        return oracle.frames_demod(y, X, cp)
    if configure == "denoise":
        from test_denoise_gpu import ref_mrc
        Hd, Pd = ref_denoise(fc.oracle_estimates(oracle, y, X, cp)[0], C, 16, 4)
        return ref_mrc(y, cp, Hd, Pd)
    if configure == "cfo":
        eps = host(ofdm.frame_cfo_estimate(to_dev(y, dev), cp))
        return oracle.frames_demod(cc.derotate_ref(y, eps, cp), X, cp)
    Pw = pc.p_by_position(fc.oracle_estimates(oracle, y, X, cp)[1])
    out, _, margin = pc.track(oracle.frames_demod(y, X, cp), Pw, 2)
    assert margin >= pc.MARGIN_MIN
    return out


@pytest.mark.parametrize("configure", list(PIPE))
@pytest.mark.parametrize("C", [1024, 600])
def test_pipeline_slots(ofdm, oracle, dev, C, configure):
    """chunk_frames = 2, depth = 2, 7 frames: a NaN pilot sample of frame f
    reaches frame f alone -- not the other frame of its chunk, nor the later
    chunks that reuse the slot's workspace --, against a clean pass through
    the same pipeline object."""
    F, S, R, cp = 7, 4, 3, 8
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.01 * (f - 3) for f in range(F)] if configure == "cfo" else None, seed=C)
    with ofdm.Pipeline(S, R, C, np.array(c["X"]), cp, chunk_frames=2, depth=2) as p:
        PIPE[configure](p)

        def run(y):
            out = np.full((F, S - 1, C - 1), np.nan, np.complex64)
            p.demod(np.ascontiguousarray(y), out)
            p.sync()
            return out

        clean = run(c["y"])
        assert np.all(np.isfinite(clean))
        parity(clean, pipeline_reference(ofdm, oracle, dev, c, cp, configure))  # (c)
        for f in (2, 3, 6):
            y = np.array(c["y"])
            y[f, 0, 1, cp + 3] = NAN  # not among the row's last cp samples: the prefix estimator does not read it
            got = run(y)
            m = np.zeros(clean.shape, bool)
            m[f] = True
            fc.assert_outside_identical(got, clean, m, f"pipeline {configure} C={C} frame {f}")
            assert nonfinite(got[f]).all()
        assert np.array_equal(bits(run(c["y"])), bits(clean))  # and nothing of the spoiled passes stayed behind


# ------------------------------------------------------ the scale property

# the footprint tests' shapes, every C family (the F = 512 and ticketed C = 1024 batches run the same kernels as
# (5, 6, 5, 1024, 8) on more workgroups; the sc16 receivers exist at C = 1024 only, the header's limit)
SCALE_SHAPES = [(5, 6, 5, 1024, 8), (5, 6, 17, 1024, 8), (4, 6, 3, 2048, 7), (4, 6, 3, 4096, 7)] + \
               [(5, 8, 3, C, 5) for C in (128, 256, 512, 1536, 3072, 6144)] + [(5, 6, 3, C, 5) for C in (600, 3000, 5000, 6)]


@pytest.mark.parametrize("k", [40, -40])  # the receivers form at most second powers of the IQ (|H|^2, Y conj(H))
@pytest.mark.parametrize("shape", SCALE_SHAPES)
def test_receivers_are_scale_exact(ofdm, dev, shape, k):
    """IQ x 2^k: out bit-identical, the exported estimate x 2^k and P x 2^2k exactly."""
    F, S, R, C, cp = shape
    names = ["auto", "two_launch", "est_comb", "partial"] + (["symbols"] if C in (1024, 2048, 4096) else []) + \
            (["cfo", "cfo_est_comb"] if C == 1024 else [])
    for entry in names:
        fn, kind = ENTRIES[entry]
        yh, Xh, eh = rx_inputs(shape, kind)
        X, eps = to_dev(Xh, dev), to_dev(eh, dev)
        base = fn(ofdm, dev, to_dev(yh, dev), X, eps, shape)
        got = fn(ofdm, dev, to_dev(fc.scaled(yh, k), dev), X, eps, shape)
        assert all(all_finite(v) for v in got.values()), entry
        assert np.array_equal(bits(host(got["out"])), bits(host(base["out"]))), f"{entry} {shape} 2^{k}: out"
        if "H" in got:
            assert np.array_equal(bits(host(got["H"])), bits(fc.scaled(host(base["H"]), k))), f"{entry} {shape} 2^{k}: H"
        if "P" in got:
            assert np.array_equal(bits(host(got["P"])), bits(fc.scaled(host(base["P"]), 2 * k))), f"{entry} {shape} 2^{k}: P"
    if C == 1024:  # sc16: the scale argument carries 2^k
        for fn in (e_sc16, e_sc16_est_comb):
            yh, Xh, eh = rx_inputs(shape, "sc16")
            y, X = to_dev(yh, dev), to_dev(Xh, dev)
            base, got = fn(ofdm, dev, y, X, None, shape), fn(ofdm, dev, y, X, None, shape, scale=2.0 ** (k - 15))
            assert np.array_equal(bits(host(got["out"])), bits(host(base["out"]))), f"{fn.__name__} 2^{k}: out"
            if "H" in got:
                assert np.array_equal(bits(host(got["H"])), bits(fc.scaled(host(base["H"]), k)))
                assert np.array_equal(bits(host(got["P"])), bits(fc.scaled(host(base["P"]), 2 * k)))


@pytest.mark.parametrize("k", [40, -40])
@pytest.mark.parametrize("R,C", [(3, 64), (16, 600), (16, 1024)])
def test_frequency_domain_is_scale_exact(ofdm, dev, R, C, k):
    F, S = 4, 4
    c = fc.rx_frames(F, S, R, C, 0, seed=C + R)
    Yh = np.fft.fft(c["y"].astype(np.complex128), axis=-1).astype(np.complex64)
    X = to_dev(c["X"], dev)
    for entry, fn in FREQ_ENTRIES.items():
        if entry == "mfma" and C % 64:
            continue
        base, got = fn(ofdm, dev, to_dev(Yh, dev), X, (F, S, R, C)), fn(ofdm, dev, to_dev(fc.scaled(Yh, k), dev), X, (F, S, R, C))
        assert np.array_equal(bits(host(got["out"])), bits(host(base["out"]))), f"freq {entry} C={C} R={R} 2^{k}"
        if "H" in got:
            assert np.array_equal(bits(host(got["H"])), bits(fc.scaled(host(base["H"]), k)))
            assert np.array_equal(bits(host(got["P"])), bits(fc.scaled(host(base["P"]), 2 * k)))


@pytest.mark.parametrize("k", [40, -40])
def test_soft_output_is_scale_exact(ofdm, dev, k):
    """noise_var from frame_noise_estimate on the scaled data: P / noise_var, and so every LLR, is unchanged."""
    import torch
    shape, bps = (5, 6, 3, 1024, 8), 4
    F, S, R, C, cp = shape
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    X = to_dev(c["X"], dev)

    def chain(yh):
        ws = ofdm.workspace(F, S, R, C, dev)
        z = ofdm.frame_demod(to_dev(yh, dev), X, cp, ws=ws)
        nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, bps)
        return nv, ofdm.frame_soft_demap(z, ws, F, S, R, C, bps, nv)

    (nv0, l0), (nv1, l1) = chain(c["y"]), chain(fc.scaled(c["y"], k))
    assert all_finite(l1) and np.array_equal(bits(host(nv1)), bits(fc.scaled(host(nv0), 2 * k)))
    assert np.array_equal(bits(host(l1)), bits(host(l0)))


@pytest.mark.parametrize("k", [20, -20])  # the acquisition metric is a second power and its comparison a fourth
@pytest.mark.parametrize("C,cp", [(1024, 8), (600, 5)])
def test_cfo_estimators_are_scale_exact(ofdm, dev, C, cp, k):
    import torch
    F, S, R, D = 5, 4, 3, 3
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004, 0.1], seed=C)
    X, eps = to_dev(c["X"], dev), to_dev(c["eps"], dev)

    def run(yh):
        y = to_dev(yh, dev)
        g = nans((F,), dev)
        e = ofdm.frame_cfo_estimate(y, cp, gamma=g)
        sh = torch.full((F,), -99, dtype=torch.int32, device=dev)
        o = ofdm.frame_cfo_acquire(y, X, cp, D, eps=eps, shift=sh)
        return host(g), host(e), host(sh), host(o)

    (g0, e0, s0, o0), (g1, e1, s1, o1) = run(c["y"]), run(fc.scaled(c["y"], k))
    assert np.array_equal(bits(e0), bits(e1)) and np.array_equal(bits(g1), bits(fc.scaled(g0, 2 * k)))
    assert np.array_equal(s0, s1) and np.array_equal(bits(o0), bits(o1))


@pytest.mark.parametrize("k", [40, -40])  # ZF forms second powers of H (the Gram matrix) and first powers of Y
@pytest.mark.parametrize("U,R,K,n", [(4, 16, 1023, 9), (3, 5, 64, 9), (16, 64, 255, 9), (1, 1, 5, 1)])
def test_zf_is_scale_exact(ofdm, dev, U, R, K, n, k):
    """W(2^k H) = 2^-k W(H) exactly, and zf_detect(Wt(2^k H), 2^k Y) is bit-identical."""
    d = fc.zf_inputs(U, R, K, n)
    W0, Wt0 = ofdm.zf_precoder(to_dev(d["H"], dev))
    W1, Wt1 = ofdm.zf_precoder(to_dev(fc.scaled(d["H"], k), dev))
    assert all_finite(W1)
    assert np.array_equal(bits(host(W1)), bits(fc.scaled(host(W0), -k)))
    assert np.array_equal(bits(host(Wt1)), bits(fc.scaled(host(Wt0), -k)))
    x0 = ofdm.zf_detect(Wt0, to_dev(d["Y"], dev))
    x1 = ofdm.zf_detect(Wt1, to_dev(fc.scaled(d["Y"], k), dev))
    assert np.array_equal(bits(host(x1)), bits(host(x0)))
