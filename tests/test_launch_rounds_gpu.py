"""Every launcher past its first chunk and its first round of resident
workgroups: the loops that run only once a call outgrows one launch (65 535
grid rows, the 256 MiB staging buffer, 2^32 threads) or one round of a
persistent grid, and the state they carry from one iteration to the next (a
prefetched row, an (f, s) counter pair advanced by gridDim, a (q, j) pair
advanced by the stride, a base pointer advanced per chunk).  The other GPU
tests of these kernels all finish inside the first iteration.

Rules of this module:
  * every output buffer is NaN-filled before the call and all finite after
    it: an element the loop never reached fails the test, not a norm;
  * shapes are derived from the device's CU count with the launchers' own
    factors, and the first line of each test asserts that the shape is past
    its boundary (more than 2x: the third iteration, with a remainder);
  * receivers are checked (A) against the float64 oracle at helpers.RTOL, on
    all frames where that costs under about 2 s on 8 threads, else on twelve
    frames (the first two, the last two, eight evenly spaced), and (B) bit for
    bit against the same entry point called on consecutive sub-batches that
    each stay inside half a round: frames are independent and a symbol's
    arithmetic does not depend on the round it is computed in;
  * no new tolerance: helpers.RTOL for the receivers, the modulator tests' own
    bound (RTOL, peaks within 1e-5), test_fft_rows_any_c_vs_numpy's bound.
"""
import time

import numpy as np
import pytest

import tx_cases
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

NAN = float("nan")
GRID_ROWS = 65535              # grid rows per launch (stages.hip, launch_ls_freq, launch_ls_lane512)
FINALIZE_STRIDE = 8192 * 256   # k_mrc_finalize: at most 8192 workgroups of 256 lanes
SC16_STRIDE = 8192 * 256 * 4   # k_iq_sc16_to_cf32: the same grid, four samples per lane
STAGING_BYTES = 256 << 20      # include/ofdm_lsmrc.h: a staging buffer of at most 256 MiB
SYNTH_ROWS = 0xffffffff // 64  # synth_t at C = 4: rows (workgroups of 64 threads) per launch, < 2^32 threads


# ------------------------------------------------------------------ helpers

def cus(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def any_cap(C):
    return 2048 if C <= 2048 else 4096 if C <= 4096 else 8192


def fft_any_resident(C, dev):
    """Row groups of one round of k_fft_any / rows of k_tx_any (4 / 2 / 1 workgroups per CU)."""
    return {2048: 4, 4096: 2, 8192: 1}[any_cap(C)] * cus(dev)


def mrc_resident(C, dev):
    """Data symbols of one round of the fused MRC that ofdm_frame_demod runs at
    this C: k_mrc_td* (workgroups per CU x symbols per workgroup) or k_mrc_any
    (3 / 2 / 1 workgroups per CU)."""
    lane = {128: 16, 256: 16, 512: 16, 1536: 8, 3072: 4, 6144: 2}
    if C in lane:
        return lane[C] * cus(dev)
    return {2048: 3, 4096: 2, 8192: 1}[any_cap(C)] * cus(dev)


def qpsk(K, seed=7):
    rng = np.random.default_rng(seed)
    a = np.float32(0.70710678)
    return (rng.choice([-a, a], K) + 1j * rng.choice([-a, a], K)).astype(np.complex64)


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nans(shape, dev, dtype=None):
    import torch
    return torch.full(shape, NAN, dtype=dtype or torch.complex64, device=dev)


def finite(t):
    import torch
    return bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all().item())


def same_bits(a, b):
    import torch
    bits = lambda t: (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def subset(F, *also):
    """The first two frames, the last two, eight evenly spaced, and `also`."""
    sel = {0, 1, F - 2, F - 1, *also} | {int(f) for f in np.linspace(0, F - 1, 10)[1:-1]}
    return sorted(f for f in sel if 0 <= f < F)


def check_oracle(oracle, iq, X, prefix, out, sel=None, freq=False):
    """(A): the float64 oracle on frames `sel` (None: all) at helpers.RTOL."""
    import torch
    if sel is not None:
        idx = torch.tensor(sel, device=iq.device)
        iq, out = iq[idx], out[idx]
    iqh, Xh = host(iq), host(X)
    t0 = time.perf_counter()
    ref = oracle.frames_demod_freq(iqh, Xh, nthreads=8) if freq else oracle.frames_demod(iqh, Xh, prefix, nthreads=8)
    print(f"oracle: {iqh.shape[0]} frames of {tuple(iqh.shape[1:])} in {time.perf_counter() - t0:.2f} s")
    return parity(host(out), ref, RTOL)


def check_sub_batches(call, iq, out, f_sub):
    """(B): `call(frames, out)` on consecutive sub-batches of f_sub frames gives
    the bytes of the big call's slice, every element."""
    F = iq.shape[0]
    for f0 in range(0, F, f_sub):
        n = min(f_sub, F - f0)
        part = nans((n,) + tuple(out.shape[1:]), iq.device)
        call(iq[f0:f0 + n].clone(), part)  # a copy: its own 256-B aligned allocation
        assert finite(part), f0
        assert same_bits(part, out[f0:f0 + n]), f"frames {f0}..{f0 + n - 1} differ from the one call"


def check_estimate_combine(ofdm, iq, X, prefix, out):
    """The staged two-call flow on the same data: the one call's bytes."""
    F, S, R, Cp = iq.shape
    ws = ofdm.workspace(F, S, R, Cp - prefix, iq.device)
    ofdm.frame_estimate(iq, X, prefix, ws)
    out2 = nans(tuple(out.shape), iq.device)
    ofdm.frame_combine(iq, prefix, ws, out2)
    assert finite(out2) and same_bits(out2, out)


def check_partials(ofdm, iq, X, prefix, out, shards):
    """Mode 1 of the MRC loop: numerators and |H|^2 of antenna shards, summed
    and finalised, against the full result (as test_antenna_split_matches_full)."""
    import torch
    F, S, R, Cp = iq.shape
    K = Cp - prefix - 1
    num = torch.zeros((F, S - 1, K), dtype=torch.complex64, device=iq.device)
    P = torch.zeros((F, K), dtype=torch.float32, device=iq.device)
    for r0, r1 in shards:
        part = iq[:, :, r0:r1].contiguous()
        Pp, ws = ofdm.frame_ls_partial(part, X, prefix, P=nans((F, K), iq.device, torch.float32))
        n = ofdm.frame_mrc_partial(part, ws, prefix, num=nans((F, S - 1, K), iq.device))
        assert finite(Pp) and finite(n)
        P += Pp
        num += n
    fin = nans((F, S - 1, K), iq.device)
    ofdm.mrc_finalize(num.view(-1), 0, S - 1, K, P, fin)
    assert finite(fin)
    parity(host(fin), host(out), RTOL)


def demod_rounds(ofdm, oracle, dev, F, S, R, C, prefix, all_frames, shards):
    """frame_demod of one big batch, NaN-filled output, then (A), (B), the
    estimate + combine pair and the antenna partials."""
    units = mrc_resident(C, dev)
    X = to_dev(qpsk(C - 1, seed=C), dev)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=prefix, seed=C + F)
    out = ofdm.frame_demod(iq, X, prefix, out=nans((F, S - 1, C - 1), dev))
    assert finite(out)
    sel = None if all_frames else subset(F)
    assert all_frames or (F - 1) * (S - 1) >= 2 * units  # the subset holds a symbol of the third round
    nrel, erel = check_oracle(oracle, iq, X, prefix, out, sel)
    print(f"C={C} F={F} S={S}: nq={F * (S - 1)} units={units} norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    f_sub = (units // 2) // (S - 1)
    assert f_sub >= 1 and f_sub * (S - 1) <= units // 2
    check_sub_batches(lambda frames, o: ofdm.frame_demod(frames, X, prefix, out=o), iq, out, f_sub)
    check_estimate_combine(ofdm, iq, X, prefix, out)
    check_partials(ofdm, iq, X, prefix, out, shards)


# ------------------------------------------------ 1. the any-C receiver

# (S, R, C, prefix, frames per 256 CUs, oracle on all frames): S - 1 = 5 / 7 does
# not divide the grid (768 / 512 / 256 workgroups at 256 CUs), so k_mrc_any's
# carry t / nsd, t % nsd takes a quotient >= 1 and a non-zero remainder.
# C = 600 (G = 3 rows per group): F > 2 * 1024 pilot row groups as well, the
# rounds of k_fft_any with td_staged's pilot-row batch stride.
ANY_C = [(6, 3, 600, 5, 2100, False), (8, 3, 3000, 7, 150, True), (8, 3, 5000, 3, 75, True)]


@pytest.mark.parametrize("S,R,C,prefix,F256,all_frames", ANY_C)
def test_any_c_receiver_rounds(ofdm, oracle, dev, S, R, C, prefix, F256, all_frames):
    """k_mrc_any (modes 0 and 1) and, at C = 600, k_fft_any over the pilot rows,
    past two rounds.  Oracle on an 8-core host, 8 threads: C = 600 all 2100 frames
    2.5 s (so: the twelve-frame subset, 0.01 s); C = 3000 1.0 s; C = 5000 0.9 s."""
    F = -(-F256 * cus(dev) // 256)
    assert F * (S - 1) > 2 * mrc_resident(C, dev) and mrc_resident(C, dev) % (S - 1) != 0
    if C == 600:
        assert F * R // (2048 // C) > 2 * fft_any_resident(C, dev)
    demod_rounds(ofdm, oracle, dev, F, S, R, C, prefix, all_frames, ((0, 1), (1, 3)))


# ----------------------------------------------------- 2. fft_rows rounds

@pytest.mark.parametrize("C,groups256,extra", [(3000, 1029, 0), (5000, 517, 0), (600, 2 * 1024, 2)])
def test_fft_rows_rounds(ofdm, dev, C, groups256, extra):
    """k_fft_any past two rounds at CAP 4096 and 8192 (one row per group) and
    at CAP 2048 with a partial last group (C = 600: three rows per group, two
    in the last); forward, inverse and in place against numpy's float64 FFT,
    test_fft_rows_any_c_vs_numpy's bound."""
    import torch
    G = any_cap(C) // C
    nrows = -(-groups256 * cus(dev) // 256) * G + extra
    assert -(-nrows // G) > 2 * fft_any_resident(C, dev) and nrows % G == extra
    rng = np.random.default_rng(C)
    x = rng.standard_normal((nrows, C, 2)).astype(np.float32).view(np.complex64)[..., 0]
    d = to_dev(x, dev)
    tol = 2e-6 * max(np.log2(C), 1.0)
    x64 = x.astype(np.complex128)
    out = ofdm.fft_rows(d, nans((nrows, C), dev))
    assert finite(out)
    got = host(out)
    ref = np.fft.fft(x64, axis=-1)
    assert np.abs(got - ref).max() <= tol * np.abs(ref).max()
    inv = ofdm.fft_rows(d, nans((nrows, C), dev), inverse=True)
    assert finite(inv)
    refi = np.fft.ifft(x64, axis=-1) * C
    assert np.abs(host(inv) - refi).max() <= tol * np.abs(refi).max()
    assert torch.equal(d, to_dev(x, dev))  # out of place left the input alone
    assert same_bits(ofdm.fft_rows(d), out)  # in place


# ------------------------------------------------- 3. the fused LTE sizes

# (C, frames per 256 CUs, prefix, oracle on all frames); S = 8, R = 3
LTE = [(128, 1300, 5, True), (256, 1300, 9, True), (512, 1300, 3, True), (1536, 650, 7, True),
       (3072, 330, 5, True), (6144, 172, 3, False)]


@pytest.mark.parametrize("C,F256,prefix,all_frames", LTE)
def test_lane_order_receiver_rounds(ofdm, oracle, dev, C, F256, prefix, all_frames):
    """k_mrc_td128 ... k_mrc_td6144 (q += nw, the nxt prefetch) past two rounds,
    modes 0 and 1.  Oracle on an 8-core host, 8 threads, all frames: C = 128 0.01 s,
    256 0.03 s, 512 0.05 s, 1536 1.8 s, 3072 2.0 s, 6144 2.3 s (so: the subset,
    0.2 s)."""
    S, R = 8, 3
    F = -(-F256 * cus(dev) // 256)
    assert F * (S - 1) > 2 * mrc_resident(C, dev)
    demod_rounds(ofdm, oracle, dev, F, S, R, C, prefix, all_frames, ((0, R),))


# -------------------------------------------- 4. the 65 535-row launches

def _raw(ofdm, name, *args):
    """A C ABI entry with the caller's own (NaN-filled) output buffers."""
    import torch
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(ofdm.lib(), name)(*conv, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, ofdm.lib().ofdm_last_error()


@pytest.mark.parametrize("R,nsyms,factor", [(4, 16384 + 3, 1), (4, 2 * 16383 + 3, 2), (3, 2 * 21845 + 3, 2)])
def test_conj_product_launches(ofdm, dev, R, nsyms, factor):
    """launch_conj_product: chunks of (65535 / R) * R rows, so that r = row % R
    holds per chunk (R = 4: 65 532 rows; R = 3: exactly 65 535)."""
    assert nsyms * R > factor * (GRID_ROWS // R) * R and (nsyms * R) % ((GRID_ROWS // R) * R) != 0
    C = 4
    rng = np.random.default_rng(R)
    Y = rng.standard_normal((nsyms, R, C, 2)).astype(np.float32).view(np.complex64)[..., 0]
    H = rng.standard_normal((R, C - 1, 2)).astype(np.float32).view(np.complex64)[..., 0]
    prod = nans((nsyms, R, C - 1), dev)
    _raw(ofdm, "ofdm_channel_conj_product", to_dev(Y, dev), nsyms, to_dev(H, dev), R, C, prod)
    assert finite(prod)
    parity(host(prod), Y.astype(np.complex128)[:, :, 1:] * H.astype(np.complex128)[None], RTOL)


@pytest.mark.parametrize("K", [3, 6])  # 6: even K, shiftOneRow's three-memmove rotation
def test_combine_and_shift_launches(ofdm, dev, K):
    """launch_combine (rotate on and off) and launch_shift_rows: 65 535 rows per launch."""
    nrows, R = 2 * GRID_ROWS + 7, 2
    assert nrows > 2 * GRID_ROWS and nrows % GRID_ROWS != 0
    rng = np.random.default_rng(K)
    prod = rng.standard_normal((nrows, R, K, 2)).astype(np.float32).view(np.complex64)[..., 0]
    P = rng.uniform(0.5, 2.0, K).astype(np.float32)
    pos = [tx_cases.out_pos_any(j, K) for j in range(K)]
    want = prod.astype(np.complex128).sum(axis=1) / P.astype(np.float64)
    d_prod, d_P = to_dev(prod, dev), to_dev(P, dev)
    for rotate in (1, 0):
        out = nans((nrows, K), dev)
        _raw(ofdm, "ofdm_combine_products", d_prod, nrows, d_P, R, K, rotate, out)
        assert finite(out)
        ref = np.empty_like(want)
        ref[:, pos if rotate else list(range(K))] = want
        parity(host(out), ref, RTOL)
    rows = np.ascontiguousarray(prod[:, 0])
    out = nans((nrows, K), dev)
    _raw(ofdm, "ofdm_shift_rows", to_dev(rows, dev), nrows, K, out)
    ref = np.empty_like(rows)
    ref[:, pos] = rows
    assert np.array_equal(host(out).view(np.uint64), ref.view(np.uint64))


# frames 65 534 ... 65 536 straddle the first launch's end, 131 069 ... 131 071 the second's
@pytest.mark.parametrize("route", ["freq", "td"])
def test_ls_freq_launches(ofdm, oracle, dev, route):
    """launch_ls_freq, 65 535 frames per launch, from ofdm_frame_demod_freq and
    from td_staged (C = 6: no fused receiver); in the time-domain route also 171
    rounds of k_mrc_any.  Oracle on the subset: 0.01 s."""
    F, S, R, C = 2 * GRID_ROWS + 3, 2, 2, 6
    assert F > 2 * GRID_ROWS and F % GRID_ROWS != 0 and F * (S - 1) > 2 * mrc_resident(C, dev)
    X = to_dev(qpsk(C - 1), dev)
    sel = subset(F, GRID_ROWS - 1, GRID_ROWS, GRID_ROWS + 1, 2 * GRID_ROWS - 1, 2 * GRID_ROWS, 2 * GRID_ROWS + 1)
    f_sub = (mrc_resident(C, dev) // 2) // (S - 1)
    if route == "freq":
        Y = ofdm.synth_frames(F, S, R, C, X, seed=11, freq_domain=True)
        out = ofdm.frame_demod_freq(Y, X, out=nans((F, S - 1, C - 1), dev))
        assert finite(out)
        check_oracle(oracle, Y, X, 0, out, sel, freq=True)
        check_sub_batches(lambda frames, o: ofdm.frame_demod_freq(frames, X, out=o), Y, out, f_sub)
    else:
        iq = ofdm.synth_frames(F, S, R, C, X, seed=11)
        out = ofdm.frame_demod(iq, X, 0, out=nans((F, S - 1, C - 1), dev))
        assert finite(out)
        check_oracle(oracle, iq, X, 0, out, sel)
        check_sub_batches(lambda frames, o: ofdm.frame_demod(frames, X, 0, out=o), iq, out, f_sub)


def test_ls_lane512_launches(ofdm, oracle, dev):
    """launch_ls_lane512, 65 535 frames per launch: C = 128, 268 MB of IQ.
    Oracle on the subset: 0.01 s."""
    F, S, R, C = GRID_ROWS + 4, 2, 2, 128
    assert F > GRID_ROWS and F * (S - 1) > 2 * mrc_resident(C, dev)
    X = to_dev(qpsk(C - 1), dev)
    iq = ofdm.synth_frames(F, S, R, C, X, seed=12)
    out = ofdm.frame_demod(iq, X, 0, out=nans((F, S - 1, C - 1), dev))
    assert finite(out)
    check_oracle(oracle, iq, X, 0, out, subset(F, GRID_ROWS - 1, GRID_ROWS, GRID_ROWS + 1))
    f_sub = (mrc_resident(C, dev) // 2) // (S - 1)
    check_sub_batches(lambda frames, o: ofdm.frame_demod(frames, X, 0, out=o), iq, out, f_sub)


# ------------------------------------------------- 5. mrc_finalize's carry

@pytest.mark.parametrize("nsym,K", [(900, 1023), (1500, 600)])  # 600: even K; nsym for count > 2 strides there too
def test_mrc_finalize_carry(ofdm, dev, nsym, K):
    """k_mrc_finalize's carried (q, j) with dq, dj and the wrap, about 2.2
    strides of the grid; in one call and in three chunks whose e0 are no
    multiples of K (the first below one stride, the second above).  Reference:
    float64 numpy, out[q, out_pos_any(j, K)] = num / P[f, j]."""
    import torch
    nframes = 5
    count = nframes * nsym * K
    assert count > 2 * FINALIZE_STRIDE and count % FINALIZE_STRIDE != 0
    g = torch.Generator(device=dev).manual_seed(K)
    num = torch.view_as_complex(torch.randn((count, 2), generator=g, device=dev))
    P = torch.rand((nframes, K), generator=g, device=dev) * 1.5 + 0.5
    out = nans((nframes * nsym, K), dev)
    ofdm.mrc_finalize(num, 0, nsym, K, P, out)
    assert finite(out)
    pos = [tx_cases.out_pos_any(j, K) for j in range(K)]
    ref = np.empty((nframes, nsym, K), np.complex128)
    ref[:, :, pos] = host(num).astype(np.complex128).reshape(nframes, nsym, K) / host(P).astype(np.float64)[:, None, :]
    parity(host(out), ref, RTOL)
    cuts = [0, 1_000_003, 1_000_003 + FINALIZE_STRIDE + 400_001, count]
    assert all(c % K for c in cuts[1:3]) and cuts[1] < FINALIZE_STRIDE < cuts[2] - cuts[1] and cuts[2] < count
    out2 = nans((nframes * nsym, K), dev)
    for a, b in zip(cuts[:-1], cuts[1:]):
        ofdm.mrc_finalize(num[a:b].clone(), a, nsym, K, P, out2)
    assert finite(out2) and same_bits(out2, out)


# ------------------------------------------------------ 6. sc16 converter

_sc16 = {}


@pytest.mark.parametrize("scale", [np.float32(2.0 ** -15), np.float32(1.0) / np.float32(32767)])
def test_sc16_converter_rounds(ofdm, dev, scale):
    """k_iq_sc16_to_cf32's grid-stride loop, two strides and a remainder with
    an n % 4 tail; bit-exact against i16.astype(float32) * float32(scale)."""
    n = 2 * SC16_STRIDE + 4099
    assert n > 2 * SC16_STRIDE and n % 4 == 3
    if "q" not in _sc16:
        _sc16["q"] = np.random.default_rng(16).integers(-32768, 32768, (n, 2), dtype=np.int16)
    q = _sc16["q"]
    out = nans((n,), dev)
    ofdm.iq_convert_sc16(to_dev(q, dev), float(scale), out=out)
    want = np.ascontiguousarray(q.astype(np.float32) * np.float32(scale)).view(np.complex64)[..., 0]
    assert np.array_equal(host(out).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------- 7. the modulator

def tx_guarded(ofdm, dev, X, C, cp, map):
    """ofdm_tx_modulate, norm "peak", into NaN buffers with a guard row before
    and after d_iq and d_peak (as test_structure_is_exact) -> (iq, peak)."""
    import torch
    nrows, K = X.shape
    buf = nans((nrows + 2, C + cp), dev)
    peaks = nans((nrows + 2,), dev, torch.float32)
    _raw(ofdm, "ofdm_tx_modulate", X, K, nrows, C, cp, ofdm.TX_MAPS[map], ofdm.TX_NORMS["peak"], 1.0, buf[1:],
         peaks[1:])
    got, pk = host(buf), host(peaks)
    assert np.isnan(got[0]).all() and np.isnan(got[nrows + 1]).all() and np.isfinite(got[1:nrows + 1]).all()
    assert np.isnan(pk[0]) and np.isnan(pk[nrows + 1]) and np.isfinite(pk[1:nrows + 1]).all()
    return got[1:nrows + 1], pk[1:nrows + 1]


def check_tx(ofdm, dev, C, cp, nrows):
    Xh = tx_cases.rows_of(C + cp, nrows, C - 1)
    X = to_dev(Xh, dev)
    for map in ("reference", "rx"):
        got, pk = tx_guarded(ofdm, dev, X, C, cp, map)
        want, wpeak = tx_cases.tx_numpy(Xh, C, cp, map, "peak")
        parity(got, want, RTOL)
        assert np.allclose(pk, wpeak, rtol=1e-5, atol=0)


@pytest.mark.parametrize("cp", [16, 7])  # 16-B and 8-B stores
def test_tx_c1024_rounds(ofdm, dev, cp):
    """k_tx_mod1024 (two workgroups per CU, eight rows each) past two rounds."""
    nrows = 2 * (2 * cus(dev) * 8) + 5
    assert nrows > 2 * (2 * cus(dev) * 8)
    check_tx(ofdm, dev, 1024, cp, nrows)


@pytest.mark.parametrize("C", [600, 3000, 5000])
def test_tx_any_c_rounds(ofdm, dev, C):
    """k_tx_any's load_row(row + gridDim.x) past two rounds, the three CAPs."""
    nrows = 2 * fft_any_resident(C, dev) + 1
    assert nrows > 2 * fft_any_resident(C, dev)
    check_tx(ofdm, dev, C, 5, nrows)


# ------------------------------------------------ 8. the staging chunks

# C = 6144: the lane-order route (launch_ls_lane512); C = 5000: the bin layout
@pytest.mark.parametrize("F,S,R,C", [(173, 2, 32, 6144), (211, 2, 32, 5000)])
def test_staging_chunks(ofdm, oracle, dev, F, S, R, C):
    """td_staged's pilot FFT + LS per staging chunk: two chunks, 0.55 GB of IQ
    made on the device.  Oracle (0.3 s on an 8-core host, 8 threads) on the first
    frame, the last of the first chunk, the first of the second and the last."""
    per = (STAGING_BYTES // (S * R * C * 8)) * S  # frames whose pilot rows one staging buffer holds
    assert per < F < 2 * per
    X = to_dev(qpsk(C - 1, seed=C), dev)
    iq = ofdm.synth_frames(F, S, R, C, X, seed=C)
    out = ofdm.frame_demod(iq, X, 0, out=nans((F, S - 1, C - 1), dev))
    assert finite(out)
    check_oracle(oracle, iq, X, 0, out, [0, per - 1, per, F - 1])
    f_sub = min(per // 2, (mrc_resident(C, dev) // 2) // (S - 1))
    check_sub_batches(lambda frames, o: ofdm.frame_demod(frames, X, 0, out=o), iq, out, f_sub)


def test_synth_frames_past_one_launch(ofdm, dev):
    """synth_t launches whole frames, fewer than 2^32 threads at a time (C = 4:
    64 threads per row, 67 108 863 rows).  With S * R = 15 rows per frame a
    launch ends 3 rows short of that, and the next one must start where it
    ended: it started a full launch further, mid-frame and with the wrong frame
    number, and left the rows between unwritten (and, with 2^30 rows to a
    launch, HIP refused the launch and the next one hid the error).  34 GB, 17
    launches: the 12 frames around the end of the first launch, around row
    2^30 and at the end equal a small call's with the same frame numbers."""
    import torch
    S, R, C, n = 3, 5, 4, 12
    F = -(-(1 << 30) // (S * R)) + 10
    assert F * S * R > 2 * SYNTH_ROWS and SYNTH_ROWS % (S * R) != 0
    if torch.cuda.mem_get_info(dev)[0] < 48 << 30:
        pytest.skip("needs 48 GiB of free device memory")
    X = to_dev(qpsk(C - 1), dev)
    big = nans((F, S, R, C), dev)
    try:
        ofdm.synth_frames(F, S, R, C, X, seed=5, out=big)
        # the frame after the first launch's last, the frame that holds row 2^30, the end
        for f0 in (SYNTH_ROWS // (S * R) - n // 2, (1 << 30) // (S * R) - n // 2, F - n):
            small = ofdm.synth_frames(n, S, R, C, X, seed=5, frame0=f0)
            assert finite(big[f0:f0 + n]), f0
            assert torch.equal(big[f0:f0 + n], small), f0
    finally:
        del big
        torch.cuda.empty_cache()  # 34 GB back to the device, not kept in this process's cache
