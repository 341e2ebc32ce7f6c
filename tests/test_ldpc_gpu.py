"""The QC-LDPC decoder on the GPU (include/ofdm_lsmrc_ldpc.h): ofdm_ldpc_decode
against the integer model (ldpc_cases.decode, the definition).  Bits and
d_iters are compared for EQUALITY, never with a tolerance: integer arithmetic
makes the result unique.

Every run goes through `run`, which places the LLRs at an element offset and
stride of the test's choosing inside a buffer whose other elements hold +-127
(int8) or NaN (f32), the bits between 0xA5 guard bytes, d_iters between
sentinels and the scratch buffer, at its exact size, between guard bands; it
checks that nothing but the stated bytes changed.  The noisy cases are
ldpc_cases.NOISY's, whose noise levels tests/test_ldpc_cpu.py vouches for."""
import os
import re

import numpy as np
import pytest

import ldpc_cases as lc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 0xA5, -0x5A5A5A5B
LAUNCH_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-accel-ofdm-ls-mrc_amd", "csrc",
                          "launch.hpp")
_HANDLES = {}


def launch_constant(name):
    return int(re.search(rf"constexpr int {name} = (\d+);", open(LAUNCH_HPP).read()).group(1))


def handle(ofdm, c):
    """One QcLdpc per code for the whole module: the base table goes to the device once."""
    if c not in _HANDLES:
        _HANDLES[c] = ofdm.QcLdpc(c.mb, c.nb, c.Z, c.rows)
    return _HANDLES[c]


def per_workgroup(c):
    """Codewords a workgroup holds (launch.hpp, ldpc_plan): G * Z <= 64 and G * (2 N + nnz Z) within the LDS budget."""
    lds, per = launch_constant("LDPC_LDS_BYTES"), 2 * lc.N(c) + lc.nnz(c) * c.Z
    return max(1, min(64 // c.Z, lds // per)) if c.Z <= 32 and per <= lds else 1


def run(ofdm, dev, c, vals, pos0=0, n_bits=None, scale=1.0, offset=0, extra_stride=0, out_pad=0, with_iters=True,
        scratch_short=0, max_iter=lc.MAX_ITER, norm16=12, off=0, early_stop=True):
    """vals [ncw, n_rx] int8 or float32, the window at pos0 -> (packed bits [ncw, ceil(n_bits/8)], iters [ncw] or
    None) from the GPU."""
    import torch
    vals = np.ascontiguousarray(vals)
    ncw, n_rx = vals.shape
    code = handle(ofdm, c)
    n_bits = lc.N(c) if n_bits is None else n_bits
    stride, nbytes = n_rx + extra_stride, (n_bits + 7) // 8
    out_stride = nbytes + out_pad
    if vals.dtype == np.int8:
        host = np.where(np.arange(offset + ncw * stride + 7) % 2, 127, -127).astype(np.int8)
    else:
        host = np.full(offset + ncw * stride + 7, np.nan, np.float32)
    host[offset:offset + ncw * stride].reshape(ncw, stride)[:, :n_rx] = vals
    buf = torch.from_numpy(host).to(dev)
    out = torch.full((64 + ncw * out_stride + 64,), GUARD, dtype=torch.uint8, device=dev)
    iters = torch.full((ncw + 2,), SENTINEL, dtype=torch.int32, device=dev)
    need = ofdm.ldpc_workspace_bytes(code, ncw)
    ws = torch.full((64 + need + 64,), GUARD, dtype=torch.uint8, device=dev)
    rc = ofdm.lib().ofdm_ldpc_decode(
        ofdm._P(buf.data_ptr() + offset * buf.element_size()), 1 if vals.dtype == np.int8 else 0, scale, stride, ncw,
        code.handle, pos0, n_rx, max_iter, norm16, off, int(early_stop), n_bits, ofdm._P(out.data_ptr() + 64), out_stride,
        ofdm._P(iters.data_ptr() + 4) if with_iters else None, ofdm._P(ws.data_ptr() + 64) if need else None,
        need - scratch_short, ofdm._stream(None))
    if scratch_short:
        return rc
    ofdm._check(rc, "ofdm_ldpc_decode")
    torch.cuda.synchronize()
    out, iters, ws = out.cpu().numpy(), iters.cpu().numpy(), ws.cpu().numpy()
    assert np.array_equal(buf.cpu().numpy().view(np.uint8), host.view(np.uint8)), "the LLRs were written"
    assert np.all(out[:64] == GUARD) and np.all(out[-64:] == GUARD), "bytes around d_bits were written"
    rows = out[64:-64].reshape(ncw, out_stride)
    assert np.all(rows[:, nbytes:] == GUARD), "bytes of the stride beyond ceil(n_bits/8) were written"
    assert np.all(ws[:64] == GUARD) and np.all(ws[-64:] == GUARD), "bytes around d_scratch were written"
    assert iters[0] == SENTINEL and iters[-1] == SENTINEL
    if not with_iters:
        assert np.all(iters == SENTINEL)
    if n_bits % 8:
        assert not np.any(rows[:, nbytes - 1] >> (n_bits % 8)), "pad bits are not zero"
    return rows[:, :nbytes].copy(), (iters[1:-1].astype(np.int64) if with_iters else None)


def check(ofdm, dev, c, q, pos0=0, n_bits=None, **kw):
    """int8 q [ncw, n_rx] on the GPU equals the model; returns the model's (x, iters)."""
    ctl = {k: kw[k] for k in ("max_iter", "norm16", "early_stop") if k in kw}
    x, it = lc.decode(c, lc.full_q(c, lc.quant_i8(q), pos0), offset=kw.get("off", 0), **{"max_iter": lc.MAX_ITER, **ctl})
    bits, iters = run(ofdm, dev, c, q, pos0=pos0, n_bits=n_bits, **kw)
    ref = lc.packed(x, lc.N(c) if n_bits is None else n_bits)
    assert np.array_equal(bits, ref), f"{int(np.unpackbits(bits ^ ref).sum())} bits differ; iters {iters} model {it}"
    if iters is not None:
        assert np.array_equal(iters, it), (iters, it)
    return x, it


def random_q(c, ncw, seed, lo=-127, hi=127):
    return np.random.default_rng([seed, c.Z, c.nb]).integers(lo, hi + 1, (ncw, lc.N(c))).astype(np.int8)


# ---- 1. lifting sizes: below, at and above each wave multiple, an odd composite, a prime, the maximum

@pytest.mark.parametrize("Z", lc.ZS)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lifting_sizes(ofdm, dev, shape, Z):
    k, (x, it) = lc.case(f"grid-{shape[0]}x{shape[1]}-Z{Z}")
    c = k["code"]
    bits, iters = run(ofdm, dev, c, k["q"])
    assert np.array_equal(bits, lc.packed(x, lc.N(c))) and np.array_equal(iters, it)
    assert np.array_equal(bits, lc.packed(k["x"], lc.N(c)))  # the transmitted words
    # random LLRs: no convergence, so every iteration and both stopping rules are compared; small values
    # make equal minima (the first-minimum rule)
    check(ofdm, dev, c, random_q(c, 3, 1), max_iter=4)
    check(ofdm, dev, c, random_q(c, 3, 2, -2, 2), max_iter=3, early_stop=False, norm16=16)


# ---- 2. row degrees and the layer order

@pytest.mark.parametrize("name", ("deg2_and_32", "deg19", "shift_ends"))
def test_row_degrees_and_shifts(ofdm, dev, name):
    k, (x, it) = lc.case(name)
    c = k["code"]
    bits, iters = run(ofdm, dev, c, k["q"])
    assert np.array_equal(bits, lc.packed(x, lc.N(c))) and np.array_equal(iters, it)
    check(ofdm, dev, c, random_q(c, 3, 3), max_iter=5)
    check(ofdm, dev, c, random_q(c, 3, 4, -3, 3), max_iter=3, norm16=16, off=1)


def test_layer_order(ofdm, dev):
    """The last layer shares every column with the first: another order of the layers gives other bits
    (test_ldpc_cpu.py shows that of the model)."""
    c = lc.layer_order_code()
    rng = np.random.default_rng(8)
    noisy_zero = lc.quant_f32(lc.bpsk_llr(np.zeros((4, lc.N(c)), np.uint8), 0.8, rng), 8.0)
    x, it = check(ofdm, dev, c, noisy_zero)
    check(ofdm, dev, c, random_q(c, 4, 5, -20, 20), max_iter=1, early_stop=False)
    check(ofdm, dev, c, random_q(c, 4, 6), max_iter=6)


# ---- 3. storage: messages in LDS and in scratch, both sides of the threshold

@pytest.mark.parametrize("name", ("lds_last", "scratch_first", "nr_sized", "max_n"))
def test_message_storage(ofdm, dev, name):
    k, (x, it) = lc.case(name)
    c = k["code"]
    fits = 2 * lc.N(c) + lc.nnz(c) * c.Z <= launch_constant("LDPC_LDS_BYTES")
    assert fits == (name == "lds_last")
    need = ofdm.ldpc_workspace_bytes(handle(ofdm, c), k["q"].shape[0])
    assert need == (0 if fits else lc.nnz(c) * c.Z * k["q"].shape[0])
    bits, iters = run(ofdm, dev, c, k["q"])  # the exact size between 0xA5 guards
    assert np.array_equal(bits, lc.packed(x, lc.N(c))) and np.array_equal(iters, it)
    check(ofdm, dev, c, random_q(c, 2, 7), max_iter=3)
    if not fits:
        assert run(ofdm, dev, c, k["q"], scratch_short=1) == -1
        assert b"scratch_bytes" in ofdm.lib().ofdm_last_error()


# ---- 4. controls

def test_max_iter_and_early_stop(ofdm, dev):
    k, (x, it) = lc.case("n1944")
    c = k["code"]
    assert len(set(it.tolist())) > 1, "the codewords of one launch stop at different iterations"
    bits, iters = run(ofdm, dev, c, k["q"])
    assert np.array_equal(bits, lc.packed(x, lc.N(c))) and np.array_equal(iters, it)
    assert len(set(iters.tolist())) > 1
    for max_iter in (1, 2, 20):
        for early_stop in (False, True):
            xm, im = check(ofdm, dev, c, k["q"], max_iter=max_iter, early_stop=early_stop)
            if not early_stop:
                assert np.all(np.abs(im) == max_iter)
    assert np.all(im == it)


def test_never_converging_codeword(ofdm, dev):
    c = lc.code_1944()
    x, it = check(ofdm, dev, c, random_q(c, 3, 9), max_iter=7)
    assert np.all(it == -7)
    x, it = check(ofdm, dev, c, random_q(c, 3, 9), max_iter=7, early_stop=False)
    assert np.all(it == -7)


@pytest.mark.parametrize("ctl", lc.CONTROLS, ids=lambda v: f"{v[0]}-{v[1]}")
def test_normalisation_and_offset(ofdm, dev, ctl):
    k, _ = lc.case("n1944")
    check(ofdm, dev, k["code"], k["q"][:4], norm16=ctl[0], off=ctl[1])
    c = lc.gen_code(4, 8, 27)
    check(ofdm, dev, c, random_q(c, 5, 10, -40, 40), max_iter=4, norm16=ctl[0], off=ctl[1])


# ---- 5. input

SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan, 3e38, -3e38, 0.0625, -0.0625, 0.1875, 0.3125,
                    -0.1875, 15.8125, 15.9375, -15.9375, 100.0], np.float32)  # k + 1/2 after * 8: ties to even


def test_f32_equals_the_quantised_bytes(ofdm, dev):
    k, _ = lc.case("n1944")
    c = k["code"]
    rng = np.random.default_rng(11)
    llr = k["llr"][:4].copy()
    where = rng.random(llr.shape) < 0.1
    llr[where] = rng.choice(SPECIAL, int(where.sum()))
    q = lc.quant_f32(llr, 8.0)
    assert {-127, 127, 0, 2, -2, 126} <= set(q[where].tolist())
    x, it = lc.decode(c, lc.full_q(c, q), lc.MAX_ITER)
    for off in (0, 1):
        bits, iters = run(ofdm, dev, c, llr, scale=8.0, offset=off)
        assert np.array_equal(bits, lc.packed(x, lc.N(c))) and np.array_equal(iters, it)
    bits8, iters8 = run(ofdm, dev, c, q)
    assert np.array_equal(bits8, bits) and np.array_equal(iters8, iters)
    q3 = lc.quant_f32(llr, 3.0)  # another scale is another quantisation
    x3, it3 = lc.decode(c, lc.full_q(c, q3), lc.MAX_ITER)
    bits, iters = run(ofdm, dev, c, llr, scale=3.0)
    assert np.array_equal(bits, lc.packed(x3, lc.N(c))) and np.array_equal(iters, it3)


def test_int8_minus_128_is_minus_127(ofdm, dev):
    k, _ = lc.case("grid-4x8-Z65")
    c = k["code"]
    q = k["q"].copy()
    q[np.random.default_rng(2).random(q.shape) < 0.2] = -128
    check(ofdm, dev, c, q)  # check() decodes max(q, -127) in the model
    a, b = run(ofdm, dev, c, q), run(ofdm, dev, c, np.maximum(q, -127))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("fmt", ("i8", "f32"))
def test_addressing(ofdm, dev, fmt):
    k, (x, it) = lc.case("grid-4x8-Z27")
    c = k["code"]
    vals, scale = (k["q"], 1.0) if fmt == "i8" else (k["llr"], 8.0)
    n = 0
    for offset in (1, 2, 3):
        for extra in (0, 1, 13):
            n += 1
            bits, iters = run(ofdm, dev, c, vals, scale=scale, offset=offset, extra_stride=extra, out_pad=3 * (n % 2),
                              with_iters=n % 3 != 0)
            assert np.array_equal(bits, lc.packed(x, lc.N(c))), (offset, extra)
            assert iters is None or np.array_equal(iters, it)


@pytest.mark.parametrize("name", ("grid-12x24-Z27", "grid-4x8-Z3", "grid-4x8-Z129"))
def test_windows(ofdm, dev, name):
    """Positions outside (pos0, n_rx) are erasures: NR's punctured first 2 Z columns, a punctured tail, both,
    and a single LLR."""
    k, _ = lc.case(name)
    c = k["code"]
    Nc, Z = lc.N(c), c.Z
    for pos0, n_rx in ((0, Nc), (2 * Z, Nc - 2 * Z), (Z + 1, Nc - 2 * Z - 3), (0, 1)):
        for extra in (0, 5):
            check(ofdm, dev, c, k["q"][:, pos0:pos0 + n_rx], pos0=pos0, extra_stride=extra, offset=extra % 4)
    check(ofdm, dev, c, np.full((2, 1), -128, np.int8), pos0=Nc - 1, max_iter=3)


@pytest.mark.parametrize("name", ("grid-12x24-Z27", "grid-2x4-Z3"))
def test_n_bits(ofdm, dev, name):
    k, (x, it) = lc.case(name)
    c = k["code"]
    q = k["q"].copy()
    q[0] = random_q(c, 1, 12)[0]  # and a word with ones all over
    for n_bits in (1, 7, 8, 9, lc.K(c), lc.N(c)):
        for with_iters in (True, False):
            check(ofdm, dev, c, q, n_bits=n_bits, out_pad=n_bits % 3, with_iters=with_iters)


# ---- 6. the grid of workgroups

def test_one_codeword(ofdm, dev):
    for name in ("grid-2x4-Z2", "grid-12x24-Z81", "nr_sized"):
        k, (x, it) = lc.case(name)
        bits, iters = run(ofdm, dev, k["code"], k["q"][:1])
        assert np.array_equal(bits, lc.packed(x[:1], lc.N(k["code"]))) and np.array_equal(iters, it[:1])


def test_one_more_codeword_than_a_workgroup_holds(ofdm, dev):
    """Packed codewords (G * Z <= 64): the last workgroup holds one codeword and idle lanes; codewords of one
    wave stop at different iterations."""
    mixed = 0
    for Z in (2, 3, 5, 21, 32):
        c = lc.gen_code(2, 4, Z)
        G = per_workgroup(c)
        assert G == 64 // Z
        for ncw in (G + 1, 2 * G - 1, G):
            rng = np.random.default_rng([Z, ncw])
            q = lc.quant_f32(lc.bpsk_llr(lc.encode(c, rng.integers(0, 2, (ncw, lc.K(c)))), 0.7, rng), 8.0)
            x, it = check(ofdm, dev, c, q, max_iter=6)
            mixed += G > 1 and any(len(set(it[g:g + G].tolist())) > 1 for g in range(0, ncw, G))
    assert mixed, "codewords of one wave stop at different iterations"
    assert per_workgroup(lc.gen_code(2, 4, 33)) == 1


def test_more_codewords_than_a_round_lds(ofdm, dev):
    """Seven distinct codewords in turn (the model decodes each once): workgroup 0 takes a second group,
    another one than its first."""
    k, (x, it) = lc.case("packed")
    c = k["code"]
    ncw = launch_constant("LDPC_ROUND_LDS") * per_workgroup(c) + 1
    i = np.arange(ncw) % 7
    bits, iters = run(ofdm, dev, c, k["q"][i], extra_stride=1)
    assert np.array_equal(bits, lc.packed(x, lc.N(c))[i]) and np.array_equal(iters, it[i])


def test_more_codewords_than_a_round_scratch(ofdm, dev):
    """The scratch slots are reused by the codewords past the first round; the smallest code whose messages
    do not fit in LDS.  Two distinct codewords in turn at an odd round + 1: a slot's second user differs."""
    k, (x, it) = lc.case("scratch_first")
    c = k["code"]
    ncw = launch_constant("LDPC_ROUND_SCRATCH") + 1
    assert ofdm.ldpc_workspace_bytes(handle(ofdm, c), ncw) == lc.nnz(c) * c.Z * (ncw - 1)
    i = np.arange(ncw) % 2
    bits, iters = run(ofdm, dev, c, k["q"][i])
    assert np.array_equal(bits, lc.packed(x, lc.N(c))[i]) and np.array_equal(iters, it[i])


# ---- 7. isolation and determinism

@pytest.mark.parametrize("fmt", ("i8", "f32"))
@pytest.mark.parametrize("name", ("grid-2x4-Z3", "n1944"))
def test_a_bad_codeword_spoils_only_itself(ofdm, dev, fmt, name):
    k, (x, it) = lc.case(name)
    c = k["code"]
    vals, scale = (k["q"][:5].copy(), 1.0) if fmt == "i8" else (k["llr"][:5].copy(), 8.0)
    clean = run(ofdm, dev, c, vals, scale=scale, extra_stride=5)
    again = run(ofdm, dev, c, vals, scale=scale, extra_stride=5)
    assert np.array_equal(clean[0], again[0]) and np.array_equal(clean[1], again[1])  # byte-identical
    assert np.array_equal(clean[0], lc.packed(x[:5], lc.N(c))) and np.array_equal(clean[1], it[:5])
    rng = np.random.default_rng(13)
    vals[1] = rng.choice([-127, 127], vals.shape[1])
    if fmt == "f32":
        vals[1, ::3] = np.nan
    bad = run(ofdm, dev, c, vals, scale=scale, extra_stride=5)
    for i in (0, 2, 3, 4):
        assert np.array_equal(bad[0][i], clean[0][i]) and bad[1][i] == clean[1][i]
    vals[1] = np.nan if fmt == "f32" else 0  # erased altogether: the all-zero word after one iteration
    bad = run(ofdm, dev, c, vals, scale=scale, extra_stride=5)
    assert not bad[0][1].any() and bad[1][1] == 1
    assert np.array_equal(np.delete(bad[0], 1, 0), np.delete(clean[0], 1, 0))


# ---- 8. saturation

def test_saturation(ofdm, dev):
    """The clamp-hitting input of test_ldpc_cpu.py (it asserts there that the clamp is met)."""
    c, q, ctl = lc.saturation_case()
    check(ofdm, dev, c, q, max_iter=ctl["max_iter"], norm16=ctl["norm16"], off=ctl["offset"], early_stop=ctl["early_stop"])
    check(ofdm, dev, c, q, max_iter=12, norm16=16)


# ---- the binding

def test_binding_shapes(ofdm, dev):
    import torch
    k, (x, it) = lc.case("grid-12x24-Z27")
    c = k["code"]
    code, Nc, Kc = handle(ofdm, c), lc.N(c), lc.K(c)
    q = torch.from_numpy(k["q"].copy()).to(dev)
    bits, iters = ofdm.ldpc_decode(q, code)  # 2-D: ncw and stride from the shape; the defaults are lc.decode's
    assert bits.shape == (3, (Nc + 7) // 8) and bits.dtype == torch.uint8 and iters.shape == (3,) and iters.dtype == torch.int32
    assert np.array_equal(bits.cpu().numpy(), lc.packed(x, Nc)) and np.array_equal(iters.cpu().numpy(), it)
    llr = torch.from_numpy(k["llr"].copy()).to(dev)
    nb = (Kc + 7) // 8
    out = torch.full((3, nb + 4), GUARD, dtype=torch.uint8, device=dev)
    b2, i2 = ofdm.ldpc_decode(llr.reshape(-1), code, ncw=3, scale=8.0, n_bits=Kc, out=out, iters=iters)
    assert b2 is out and i2 is iters
    assert np.array_equal(out.cpu().numpy()[:, :nb], lc.packed(x, Kc)) and np.all(out.cpu().numpy()[:, nb:] == GUARD)
    assert ofdm.ldpc_decode(q[:0].reshape(-1), code, ncw=0)[0].shape == (0, (Nc + 7) // 8)
    with pytest.raises(ofdm.OfdmError):
        ofdm.ldpc_decode(q.reshape(-1), code, ncw=4)
    with pytest.raises(ofdm.OfdmError):
        ofdm.ldpc_decode(q.to(torch.int32), code)


# ---- 9. the chain: receiver -> noise estimate -> demapper -> decoder, on the code of N = 1944

S, R, C = 9, 4, 64
CHAIN_NOISE = {2: 0.55, 6: 0.15}
CHAIN_FRAMES = {2: 27, 6: 9}  # a frame carries 8 * 63 * bps bits: 27216 bits are 27 / 9 frames and 14 codewords


def coded_frames(bps, seed=0):
    """Frequency-domain frames as test_viterbi_gpu.coded_frames builds them; the data bits of all frames, in
    output order, are 14 codewords of N = 1944, which cross the frame boundaries."""
    from soft_cases import out_src
    from test_soft_demap_gpu import map_38211
    rng = np.random.default_rng([seed, S, R, C, bps, 9])
    c, Kc = lc.code_1944(), C - 1
    per_frame = (S - 1) * Kc * bps
    nframes = CHAIN_FRAMES[bps]
    ncw = nframes * per_frame // 1944
    assert ncw * 1944 == nframes * per_frame
    X = map_38211(rng.integers(0, 2, (Kc, 2)))
    H = (rng.standard_normal((nframes, 1, R, Kc)) + 1j * rng.standard_normal((nframes, 1, R, Kc))) / np.sqrt(2)
    info = rng.integers(0, 2, (ncw, lc.K(c))).astype(np.uint8)
    coded = lc.encode(c, info)
    bits = np.empty((nframes, S - 1, Kc, bps), np.uint8)
    bits[:, :, out_src(Kc), :] = coded.reshape(nframes, S - 1, Kc, bps)  # by subcarrier; output order is the codewords'
    sym = np.concatenate([np.broadcast_to(X, (nframes, 1, Kc)), map_38211(bits)], axis=1)
    Y = np.zeros((nframes, S, R, C), np.complex128)
    Y[..., 1:] = H * sym[:, :, None, :]
    Y += CHAIN_NOISE[bps] / np.sqrt(2) * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape))
    return Y.astype(np.complex64), X.astype(np.complex64), coded, nframes


@pytest.mark.parametrize("bps", (2, 6))
def test_chain(ofdm, dev, bps):
    import torch
    Yh, Xh, coded, nf = coded_frames(bps)
    c = lc.code_1944()
    code, ncw = handle(ofdm, c), coded.shape[0]
    Y, X = torch.from_numpy(Yh).to(dev), torch.from_numpy(Xh).to(dev)
    ws = ofdm.workspace(nf, S, R, C, dev)
    z = ofdm.frame_demod_freq(Y, X, ws=ws)
    nv = ofdm.frame_noise_estimate(z, ws, nf, S, R, C, bps)
    llr8 = ofdm.frame_soft_demap(z, ws, nf, S, R, C, bps, nv, fmt="i8", scale=2.0)
    llrf = ofdm.frame_soft_demap(z, ws, nf, S, R, C, bps, nv, fmt="f32")
    bits8, it8 = ofdm.ldpc_decode(llr8.reshape(ncw, -1), code)
    bitsf, itf = ofdm.ldpc_decode(llrf.reshape(ncw, -1), code, scale=2.0)
    torch.cuda.synchronize()
    q8, qf = llr8.cpu().numpy().reshape(ncw, -1), lc.quant_f32(llrf.cpu().numpy().reshape(ncw, -1), 2.0)
    bits8, bitsf, it8, itf = bits8.cpu().numpy(), bitsf.cpu().numpy(), it8.cpu().numpy(), itf.cpu().numpy()
    raw_wrong = int(((q8 < 0) != coded.astype(bool)).sum())
    print(f"bps {bps}: {raw_wrong} of {coded.size} hard decisions wrong before decoding, "
          f"{int(np.unpackbits(bits8 ^ lc.packed(coded, 1944)).sum())} decoded bits wrong, iterations {it8.tolist()}, "
          f"{int((q8 != qf).sum())} bytes differ between the demapper's formats")
    x8, i8 = lc.decode(c, lc.full_q(c, q8), lc.MAX_ITER)
    assert np.array_equal(bits8, lc.packed(x8, 1944)) and np.array_equal(it8, i8)  # the model
    assert np.array_equal(bits8, lc.packed(coded, 1944)) and np.all(it8 > 0)  # the transmitted bits
    assert raw_wrong >= 20
    xf, jf = lc.decode(c, lc.full_q(c, qf), lc.MAX_ITER)
    assert np.array_equal(bitsf, lc.packed(xf, 1944)) and np.array_equal(itf, jf)
    # the int8 and f32 routes, byte for byte: the f32 LLRs against their own quantised bytes, and against the
    # demapper's bytes wherever those are the same numbers
    bitsq, itq = ofdm.ldpc_decode(torch.from_numpy(qf.copy()).to(dev), code)
    assert np.array_equal(bitsq.cpu().numpy(), bitsf) and np.array_equal(itq.cpu().numpy(), itf)
    same = np.all(q8 == qf, axis=1)
    assert np.array_equal(bitsf[same], bits8[same]) and np.array_equal(itf[same], it8[same])
    assert np.array_equal(bitsf, lc.packed(coded, 1944))
