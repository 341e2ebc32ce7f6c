"""The footprint table of footprint_cases.py pinned to the CPU references (no
GPU): on every spoiled input the reference's set of non-finite cells EQUALS the
geometric footprint and every other cell holds the clean output's bits; and the
references are exact under the power-of-two scalings the GPU file uses.

References: the oracle (oracle/) for the receivers and zero forcing, float64
numpy for the stage entries, the FFT, the modulator, the CFO entries and the
denoiser, as the other *_cases.py do."""
import numpy as np
import pytest

import acquire_cases as ac
import cfo_cases as cc
import footprint_cases as fc
import tx_cases
from footprint_cases import bits, nonfinite

# (F, S, R, C, prefix): the issue's shape; odd C (even K: shiftOneRow's three memmoves); C = 2
RX_SHAPES = [(4, 4, 3, 64, 5), (3, 3, 2, 7, 2), (3, 3, 2, 2, 1)]


def check(got, clean, mask, label, nonfinite_is_footprint=True):
    fc.assert_outside_identical(got, clean, mask, label)
    if nonfinite_is_footprint:
        bad = nonfinite(got) != mask
        assert not bad.any(), f"{label}: the reference's non-finite set differs from the footprint at " \
            f"{np.argwhere(bad)[:4].tolist()}"


def spoils_finite(sp):
    """Spoils whose footprint changes but need not turn non-finite: a silent
    frame's estimate is exactly 0 (its output 0 / 0 is not), another eps moves values."""
    return sp["kind"] in ("silent", "eps")


@pytest.mark.parametrize("F,S,R,C,cp", RX_SHAPES)
def test_time_domain_receiver(oracle, F, S, R, C, cp):
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    clean = oracle.frames_demod(c["y"], c["X"], cp)
    Hc, Pc = fc.oracle_estimates(oracle, c["y"], c["X"], cp)
    assert np.all(np.isfinite(clean)) and np.all(Pc > 0)
    for sp in fc.rx_placements(F, S, R, C, cp, fc.straddle_frame(F, S, 8)):
        y, X, _ = fc.spoil_rx(c["y"], c["X"], None, sp)
        fp = fc.rx_footprint(sp, F, S, R, C, cp)
        check(oracle.frames_demod(y, X, cp), clean, fp["out"], fc.label(sp))
        H, P = fc.oracle_estimates(oracle, y, X, cp)
        check(H, Hc, fp["H"], fc.label(sp) + " H", not spoils_finite(sp))
        check(P, Pc, fp["P"], fc.label(sp) + " P", not spoils_finite(sp))
        if sp["kind"] == "silent":
            assert not H[sp["f"]].any() and not P[sp["f"]].any()


def test_the_checks_notice_a_leak():
    """One changed bit, and one NaN, in a cell outside the mask fail (a); a finite cell where the reference is not fails (b)."""
    clean = np.arange(12, dtype=np.float32).reshape(3, 4).astype(np.complex64) + 1
    mask = np.zeros((3, 4), bool)
    mask[1] = True
    got = clean.copy()
    got[1] = fc.NAN
    fc.assert_outside_identical(got, clean, mask, "row 1")
    fc.assert_inside_nonfinite(got, got, mask, "row 1")
    for value in (np.nextafter(np.float32(1), np.float32(2)), np.float32("nan")):
        leak = got.copy()
        leak[2, 3] = value
        with pytest.raises(AssertionError, match="outside the footprint"):
            fc.assert_outside_identical(leak, clean, mask, "leak")
    zero, negzero = clean.copy(), clean.copy()
    zero[0, 0], negzero[0, 0] = 0.0, complex(-0.0, 0.0)
    assert np.array_equal(zero, negzero)
    with pytest.raises(AssertionError, match="outside the footprint"):  # -0 against +0: bits, not values
        fc.assert_outside_identical(negzero, zero, mask, "sign of zero")
    with pytest.raises(AssertionError, match="are finite"):
        fc.assert_inside_nonfinite(clean, got, mask, "dead bin reported finite")


def test_prefix_is_never_read(oracle):
    F, S, R, C, cp = RX_SHAPES[0]
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    y = np.array(c["y"])
    y[..., :cp] = np.nan
    assert np.array_equal(bits(oracle.frames_demod(y, c["X"], cp)), bits(oracle.frames_demod(c["y"], c["X"], cp)))
    assert not fc.rx_footprint(fc.sample(1, 2, 1, cp - 1), F, S, R, C, cp)["frame"].any()


def test_column_of_pilot_10(oracle):
    """The issue's own reading: pilot index 10 lands in output column 42 at K = 63."""
    assert fc.pos(10, 63) == 42
    fp = fc.rx_footprint(fc.zero_pilot(10), 4, 4, 3, 64, 5)
    assert fp["out"][:, :, 42].all() and fp["out"].sum() == 4 * 3


@pytest.mark.parametrize("F,S,R,C", [(4, 4, 3, 64), (3, 3, 16, 7)])
def test_frequency_domain_receiver(oracle, F, S, R, C):
    c = fc.rx_frames(F, S, R, C, 0, seed=C + 1)
    Y = np.fft.fft(c["y"].astype(np.complex128), axis=-1).astype(np.complex64)
    clean = oracle.frames_demod_freq(Y, c["X"])
    assert np.all(np.isfinite(clean))
    for sp in fc.freq_placements(F, S, R, C, 1):
        Ys, X = fc.spoil_freq(Y, c["X"], sp)
        fp = fc.rx_footprint(sp, F, S, R, C, freq=True)
        check(oracle.frames_demod_freq(Ys, X), clean, fp["out"], fc.label(sp))


def test_sc16_reference(oracle):
    """The sc16 entries are the fp32 ones on i16 * scale: zero_pilot and silent_frame, the spoils an int16 can carry."""
    F, S, R, C, cp = RX_SHAPES[0]
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    q = fc.to_sc16(c["y"])
    clean = oracle.frames_demod(fc.from_sc16(q, 2.0 ** -15), c["X"], cp)
    assert np.all(np.isfinite(clean))
    for sp in (fc.zero_pilot(0), fc.zero_pilot(C - 2), fc.silent_frame(0), fc.silent_frame(F - 1), fc.silent_frame(1)):
        qs, X, _ = fc.spoil_rx(q, c["X"], None, sp)
        check(oracle.frames_demod(fc.from_sc16(qs, 2.0 ** -15), X, cp), clean, fc.rx_footprint(sp, F, S, R, C, cp)["out"],
              fc.label(sp))


def test_cfo_reference(oracle):
    """The *_cfo entries are the fp32 ones on the derotated frames: the sample
    spoils as for the plain receiver, and another eps[f] moves frame f alone."""
    F, S, R, C, cp = RX_SHAPES[0]
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004], seed=C)
    run = lambda y, X, eps: oracle.frames_demod(cc.derotate_ref(y, eps, cp), X, cp)
    clean = run(c["y"], c["X"], c["eps"])
    sps = fc.rx_placements(F, S, R, C, cp, 0) + [fc.eps_change(f, 0.11) for f in (0, 1, F - 1)]
    for sp in sps:
        y, X, eps = fc.spoil_rx(c["y"], c["X"], c["eps"], sp)
        got = run(y, X, eps)
        check(got, clean, fc.rx_footprint(sp, F, S, R, C, cp)["out"], fc.label(sp), sp["kind"] != "eps")
        if sp["kind"] == "eps":
            assert np.all(np.isfinite(got)) and not np.array_equal(got[sp["f"]], clean[sp["f"]])
    # frame_cfo_derotate itself: frame f alone
    d0 = cc.derotate_ref(c["y"], c["eps"], cp)
    e = np.array(c["eps"])
    e[2] = 0.11
    d1 = cc.derotate_ref(c["y"], e, cp)
    assert np.array_equal(bits(d0[[0, 1, 3]]), bits(d1[[0, 1, 3]])) and not np.array_equal(d0[2], d1[2])


def test_cfo_estimators_reference():
    """A sample of frame f reaches the per-frame outputs of f alone; the prefix
    estimator reads the first and last cp samples of a row only."""
    F, S, R, C, cp = 4, 4, 3, 64, 5
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004], seed=C)
    g0, e0 = cc.gamma_ref(c["y"], cp)
    s0, o0, M0, _ = ac.acquire(c["y"], c["X"], cp, 3, c["eps"])
    for f, s, r, i, read_by_cp, read_by_acq in ((0, 0, 0, 0, True, False), (F - 1, S - 1, R - 1, C + cp - 1, True, False),
                                                (1, 0, 1, cp + C // 2, False, True), (2, 1, 1, cp + 3, False, False)):
        y, _, _ = fc.spoil_rx(c["y"], c["X"], None, fc.sample(f, s, r, i))
        with np.errstate(all="ignore"):
            g, e = cc.gamma_ref(y, cp)
            sh, o, M, _ = ac.acquire(y, c["X"], cp, 3, c["eps"])
        other = np.arange(F) != f
        assert np.array_equal(g[other], g0[other]) and np.array_equal(e[other], e0[other])
        assert np.isnan(e[f]) == read_by_cp and (read_by_cp or e[f] == e0[f])
        assert np.array_equal(M[other], M0[other]) and np.array_equal(sh[other], s0[other])
        assert np.array_equal(bits(o[other]), bits(o0[other]))
        if read_by_acq:  # the model: no finite metric, shift 0, eps passed through
            assert nonfinite(M[f]).all() and sh[f] == 0 and o[f] == c["eps"][f]
        else:
            assert np.array_equal(M[f], M0[f]) and sh[f] == s0[f]


@pytest.mark.parametrize("n,R,C", [(5, 3, 64), (3, 16, 7)])
def test_stage_references(n, R, C):
    d = fc.stage_inputs(n, R, C, seed=C)
    d = dict(d, prod=fc.ref_conj_product(d["Yd"], d["H"]))
    clean = {e: fc.stage_reference(e, d) for e in ("ls", "mrc", "numerator", "conj_product", "combine", "dist")}
    for e in clean:
        assert all(np.all(np.isfinite(v)) for v in clean[e].values())
    for entry, name, idx, masks in fc.stage_cases(n, R, C):
        for value in (fc.NAN,) if name in ("X", "P") else (fc.NAN, fc.INF):  # dividing by Inf gives a finite 0
            x = np.array(d[name])
            x[idx] = value if np.iscomplexobj(x) else value.real
            got = fc.stage_reference(entry, dict(d, **{name: x}))
            for out, mask in masks.items():
                check(got[out], clean[entry][out], mask, f"{entry} {name}{idx} {out}")


@pytest.mark.parametrize("C", [1024, 600, 5000, 6])
def test_fft_and_modulator_rows(C):
    nrows = 9
    x = fc.rows_input(nrows, C)
    X = fc.rows_input(nrows, C - 1, seed=1)
    f0, i0 = fc.ref_fft_rows(x), fc.ref_fft_rows(x, inverse=True)
    cp, modes = 5 if C > 6 else 2, (("rx", "scale"), ("reference", "peak"))
    tx0 = {m: tx_cases.tx_numpy(X, C, cp, m[0], m[1], 0.25) for m in modes}
    for row, col, value in fc.row_placements(nrows, C - 1):
        xs, Xs = x.copy(), X.copy()
        xs[row, col] = value
        Xs[row, col] = value
        check(fc.ref_fft_rows(xs), f0, fc.row_footprint(nrows, C, row), f"fft {row},{col}")
        check(fc.ref_fft_rows(xs, True), i0, fc.row_footprint(nrows, C, row), f"ifft {row},{col}")
        for m in modes:
            with np.errstate(all="ignore"):
                t, p = tx_cases.tx_numpy(Xs, C, cp, m[0], m[1], 0.25)
            check(fc.c64(t), fc.c64(tx0[m][0]), fc.row_footprint(nrows, C + cp, row), f"tx {m} {row},{col}")
            check(p.astype(np.float32), tx0[m][1].astype(np.float32), fc.row_footprint(nrows, 1, row)[:, 0],
                  f"peak {m} {row},{col}")


@pytest.mark.parametrize("U,R,K,n", [(3, 5, 64, 9), (2, 4, 33, 7), (1, 1, 5, 1)])
def test_zero_forcing(oracle, U, R, K, n):
    d = fc.zf_inputs(U, R, K, n)
    clean = dict(detect=oracle.zf_detect(d["W"], d["Y"]), apply=oracle.zf_apply(d["W"], d["X"]))
    assert all(np.all(np.isfinite(v)) for v in clean.values())
    for entry, name, idx, mask in fc.zf_cases_of(U, R, K, n):
        for value in (fc.NAN, fc.INF):
            W, X, Y = d["W"].copy(), d["X"].copy(), d["Y"].copy()
            if name == "Wt":
                u, r, k = idx
                W[k, u, r] = value
            else:
                (Y if name == "Y" else X)[idx] = value
            got = oracle.zf_detect(W, Y) if entry == "detect" else oracle.zf_apply(W, X)
            check(got, clean[entry], mask, f"zf_{entry} {name}{idx}")
    W0 = oracle.zf_precoder(d["H"])
    for u, r, k in ((0, 0, 0), (U - 1, R - 1, K - 1), (U // 2, R // 2, K // 2)):
        H = d["H"].copy()
        H[u, r, k] = fc.NAN
        check(oracle.zf_precoder(H), W0, fc.zf_precoder_footprint(U, R, K, k)["W"], f"zf_precoder H{u, r, k}")


def test_denoise_reference(oracle):
    """The float64 statement of frame_estimate_denoise works row by row: a NaN
    pilot sample of (f, 0, r) reaches the estimate rows of (f, r) and P[f]."""
    from denoise_cases import ref_denoise
    F, S, R, C, cp = RX_SHAPES[0]
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    H0, _ = fc.oracle_estimates(oracle, c["y"], c["X"], cp)
    Hd0, Pd0 = ref_denoise(H0, C, 8, 2)
    for f, r, i in ((0, 0, cp), (F - 1, R - 1, C + cp - 1), (1, 1, cp + C // 2)):
        y, X, _ = fc.spoil_rx(c["y"], c["X"], None, fc.sample(f, 0, r, i))
        H, _ = fc.oracle_estimates(oracle, y, X, cp)
        with np.errstate(all="ignore"):
            Hd, Pd = ref_denoise(H, C, 8, 2)
        fp = fc.rx_footprint(fc.sample(f, 0, r, i), F, S, R, C, cp)
        check(fc.c64(Hd), fc.c64(Hd0), fp["H"], f"denoise H {f, r, i}")
        check(Pd.astype(np.float32), Pd0.astype(np.float32), fp["P"], f"denoise P {f, r, i}")


def test_soft_chain_references():
    """The float64 statements of the noise estimate and the demapper (test_soft_demap_gpu) and the tracker's model
    (phase_cases) on one NaN in z[f, s, k]: frame f's noise_var, that element's LLRs, that element of the tracked
    output (and the later rows of frame f at most); every other frame unchanged."""
    import phase_cases as pc
    from soft_cases import ref_llr, ref_noise_var
    F, N, K, bps = 4, 5, 63, 4
    z = np.array(pc.case(F, N, K, bps, 0.03, 0.005, 25)["z"])
    P = np.random.default_rng(5).uniform(0.5, 2.0, (F, K))
    nv0, l0 = ref_noise_var(z, P[:, None, :], bps), ref_llr(z, 1.0, bps)
    o0, t0, _ = pc.track(z, P, bps)
    for f, s, k in ((0, 0, 0), (F - 1, N - 1, K - 1), (1, N - 1, K // 2)):
        zs = z.copy()
        zs[f, s, k] = fc.NAN
        other = np.arange(F) != f
        with np.errstate(all="ignore"):
            nv, l = ref_noise_var(zs, P[:, None, :], bps), ref_llr(zs, 1.0, bps)
            o, t, _ = pc.track(zs, P, bps)
        assert np.isnan(nv[f]) and np.array_equal(nv[other], nv0[other])
        m = np.zeros(l0.shape, bool)
        m[f, s, k] = True
        assert np.array_equal(nonfinite(l), m) and np.array_equal(l[~m], l0[~m])
        bad = nonfinite(o)
        assert bad[f, s, k] and bad.sum() == 1 and np.all(np.isfinite(t))
        assert np.array_equal(o[other], o0[other]) and np.array_equal(t[other], t0[other])
        assert np.array_equal(o[f, :s], o0[f, :s]) and np.array_equal(t[f, :s], t0[f, :s])


# ------------------------------------------------------ the scale property

# entries that form at most second powers of the input: 2^+-40; fourth powers: 2^+-20
@pytest.mark.parametrize("k", [40, -40, 20, -20])
def test_receiver_reference_is_scale_exact(oracle, k):
    F, S, R, C, cp = RX_SHAPES[0]
    c = fc.rx_frames(F, S, R, C, cp, seed=C)
    ys = fc.scaled(c["y"], k)
    assert np.array_equal(bits(oracle.frames_demod(ys, c["X"], cp)), bits(oracle.frames_demod(c["y"], c["X"], cp)))
    H0, P0 = fc.oracle_estimates(oracle, c["y"], c["X"], cp)
    H1, P1 = fc.oracle_estimates(oracle, ys, c["X"], cp)
    assert np.all(np.isfinite(P1)) and np.all(P1 > 0)
    assert np.array_equal(bits(H1), bits(fc.scaled(H0, k))) and np.array_equal(bits(P1), bits(fc.scaled(P0, 2 * k)))
    Y = np.fft.fft(c["y"][..., cp:].astype(np.complex128), axis=-1).astype(np.complex64)
    assert np.array_equal(bits(oracle.frames_demod_freq(fc.scaled(Y, k), c["X"])),
                          bits(oracle.frames_demod_freq(Y, c["X"])))
    q = fc.to_sc16(c["y"])
    assert np.array_equal(bits(oracle.frames_demod(fc.from_sc16(q, 2.0 ** (k - 15)), c["X"], cp)),
                          bits(oracle.frames_demod(fc.from_sc16(q, 2.0 ** -15), c["X"], cp)))


@pytest.mark.parametrize("k", [40, -40])
def test_soft_chain_references_are_scale_exact(k):
    """IQ x 2^k leaves z alone and scales P by 2^2k: the float64 noise estimate scales with it, rounded to f32
    exactly, and P / noise_var, so every LLR, is unchanged."""
    import phase_cases as pc
    from soft_cases import ref_llr, ref_noise_var
    F, N, K, bps = 4, 5, 63, 4
    z = pc.case(F, N, K, bps, 0.03, 0.005, 25)["z"]
    P = np.random.default_rng(5).uniform(0.5, 2.0, (F, 1, K)).astype(np.float32)
    Ps = fc.scaled(P, 2 * k)
    nv0, nv1 = ref_noise_var(z, P.astype(np.float64), bps), ref_noise_var(z, Ps.astype(np.float64), bps)
    assert np.array_equal(nv1, nv0 * 4.0 ** k)
    assert np.array_equal(bits(nv1.astype(np.float32)), bits(fc.scaled(nv0.astype(np.float32), 2 * k)))
    l0 = ref_llr(z, P / nv0[:, None, None], bps)
    l1 = ref_llr(z, Ps.astype(np.float64) / nv1[:, None, None], bps)
    assert np.all(np.isfinite(l1)) and np.array_equal(l0, l1)


def test_zf_shapes_reach_every_kernel():
    """zf.hip's dispatch restated in footprint_cases: the GPU file's shapes select every detect and apply kernel."""
    shapes = fc.ZF_SHAPES + fc.ZF_DEGENERATE
    assert {fc.zf_detect_kernel(U, R, K) for U, R, K, _ in shapes} == fc.ZF_DETECT_KERNELS
    assert {fc.zf_apply_kernel(U, R, K) for U, R, K, _ in shapes} == fc.ZF_APPLY_KERNELS


@pytest.mark.parametrize("k", [40, -40])
def test_zero_forcing_reference_is_scale_exact(oracle, k):
    U, R, K, n = 3, 5, 64, 9
    d = fc.zf_inputs(U, R, K, n)
    W0, W1 = oracle.zf_precoder(d["H"]), oracle.zf_precoder(fc.scaled(d["H"], k))
    assert np.all(np.isfinite(W1)) and np.array_equal(bits(W1), bits(fc.scaled(W0, -k)))
    assert np.array_equal(bits(oracle.zf_detect(W1, fc.scaled(d["Y"], k))), bits(oracle.zf_detect(W0, d["Y"])))


@pytest.mark.parametrize("k", [20, -20])
def test_cfo_references_are_scale_exact(k):
    F, S, R, C, cp = 4, 4, 3, 64, 5
    c = fc.rx_frames(F, S, R, C, cp, eps=[0.03, -0.2, 0.45, -0.004], seed=C)
    ys = fc.scaled(c["y"], k)
    g0, e0 = cc.gamma_ref(c["y"], cp)
    g1, e1 = cc.gamma_ref(ys, cp)
    assert np.array_equal(e0, e1) and np.array_equal(g1, g0 * 4.0 ** k)
    assert np.all(np.isfinite(g1.astype(np.complex64))) and np.all(np.abs(g1) > 2.0 ** -126)
    s0, _, M0, _ = ac.acquire(c["y"], c["X"], cp, 3, c["eps"])
    s1, _, M1, _ = ac.acquire(ys, c["X"], cp, 3, c["eps"])
    assert np.array_equal(s0, s1)
    # the metric is a second power and its square a fourth: inside f32 at 2^+-20
    assert np.all(np.isfinite((M1 ** 2).astype(np.float32))) and np.all((M1 ** 2).astype(np.float32) > 2.0 ** -126)
