"""sc16 IQ on the GPU (include/ofdm_lsmrc.h, "sc16 IQ"): the converter bit for
bit, the sc16 instantiations of the two-launch C = 1024 receiver against the
CPU oracle on the dequantised input i16.astype(float32) * float32(scale), the
scale in the estimate, one workspace serving both formats, and the sc16
pipeline (C = 1024 fused, other C through the converter).

Test data: frames quantised on the host to a peak of about 16000, then ten
samples spread over the batch overwritten with -32768, 32767, -1, 0, 1 in re
and in im independently, so that a missing sign extension of either half, or
re and im swapped, shows."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, RTOL, parity
from test_pipeline_gpu import _copy_to_ptr

pytestmark = pytest.mark.gpu

S15 = np.float32(2.0 ** -15)
UHD = np.float32(1.0) / np.float32(32767)


def quantise(iq):
    """complex64 (..., Cp) -> int16 (..., Cp, 2), peak about 16000 + the extremes."""
    v = np.stack([iq.real, iq.imag], -1).astype(np.float64)
    q = np.rint(v * (16000.0 / np.abs(v).max())).astype(np.int16)
    flat = q.reshape(-1, 2)
    idx = np.linspace(0, flat.shape[0] - 1, 10).astype(np.int64)
    flat[idx[:5], 0] = [-32768, 32767, -1, 0, 1]
    flat[idx[5:], 1] = [-32768, 32767, -1, 0, 1]
    return np.ascontiguousarray(q)


def dequantise(q, scale):
    d = q.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(d).view(np.complex64)[..., 0]


def _pilots(C, seed):
    rng = np.random.default_rng(seed)
    a = np.float32(0.70710678)
    return (rng.choice([-a, a], C - 1) + 1j * rng.choice([-a, a], C - 1)).astype(np.complex64)


_cases = {}


def case(ofdm, dev, oracle, key):
    """(q int16 host, X host, prefix, {scale: oracle output}) of a synthetic
    (F, S, R, prefix) shape or a golden's name; built once, then read only."""
    import torch
    if key not in _cases:
        if isinstance(key, str):
            z = np.load(os.path.join(GOLDEN, key + ".npz"), allow_pickle=False)
            iq, Xh, prefix = np.ascontiguousarray(z["iq"], np.complex64), np.asarray(z["X"], np.complex64), int(z["prefix"])
        else:
            F, S, R, prefix = key
            Xh = _pilots(1024, F * 1000 + R)
            iq = ofdm.synth_frames(F, S, R, 1024, torch.from_numpy(Xh).to(dev), prefix=prefix, seed=F + R,
                                   noise_std=0.02).cpu().numpy()
        _cases[key] = (quantise(iq), Xh, prefix, {})
    q, Xh, prefix, refs = _cases[key]
    return q, Xh, prefix, refs


def reference(oracle, c, scale):
    q, Xh, prefix, refs = c
    k = float(scale)
    if k not in refs:
        refs[k] = oracle.frames_demod(dequantise(q, scale), Xh, prefix)
    return refs[k]


# ------------------------------------------------------------- 1. converter

@pytest.mark.parametrize("scale", [S15, UHD])
def test_converter_exhaustive_bit_exact(ofdm, dev, scale):
    import torch
    re = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    q = np.stack([re, re[::-1]], -1)
    for n in (65536, 1, 3, 5, 4099):
        qn = np.ascontiguousarray(q[:n])
        out = torch.full((n,), float("nan"), dtype=torch.complex64, device=dev)
        ofdm.iq_convert_sc16(torch.from_numpy(qn).to(dev), float(scale), out=out)
        got = out.cpu().numpy()
        want = dequantise(qn, scale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n


# -------------------------------------------------------- 2. receiver parity

PARITY = [(2, 9, 16, 0),    # every workgroup inside one frame: the shared-Hc loop
          (3, 4, 5, 7),     # workgroups straddle frames, tail waves; row pitch 1031: rows only 4-byte aligned
          (1, 2, 1, 0),     # R = 1
          (2, 3, 17, 16),   # the 16-wave LS takes a second pass
          (512, 2, 5, 0),   # the 4-wave LS, 21 MB
          "r16_c1024_s4_2frames", "r64_c1024_s2"]


@pytest.mark.parametrize("key,scale", [(k, S15) for k in PARITY] + [((3, 4, 5, 7), UHD), ((2, 9, 16, 0), UHD)])
def test_receiver_parity(ofdm, dev, oracle, key, scale):
    import torch
    c = case(ofdm, dev, oracle, key)
    q, Xh, prefix, _ = c
    ref = reference(oracle, c, scale)
    qd, X = torch.from_numpy(q).to(dev), torch.from_numpy(Xh).to(dev)
    outs = []
    for _ in range(2):
        out = torch.full(ref.shape, float("nan"), dtype=torch.complex64, device=dev)
        ofdm.frame_demod_sc16(qd, X, prefix, float(scale), out=out)
        outs.append(out.cpu().numpy())
    assert np.all(np.isfinite(outs[0])), "an output element was not written"
    nrel, erel = parity(outs[0], ref)
    print(f"{key} scale {float(scale):.6e}: norm-rel {nrel:.2e} elem-rel {erel:.2e}")
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ------------------------------------------------- 3. the scale in the estimate

@pytest.mark.parametrize("key", [(3, 4, 5, 7), (2, 3, 17, 16), (512, 2, 5, 0)])
def test_scale_reaches_the_estimate(ofdm, dev, oracle, key):
    import torch
    q, Xh, prefix, _ = case(ofdm, dev, oracle, key)
    F, S, R, Cp, _ = q.shape
    C = Cp - prefix
    qd, X = torch.from_numpy(q).to(dev), torch.from_numpy(Xh).to(dev)
    got = {}
    for scale in (S15, np.float32(1.7) * S15):
        ws = ofdm.workspace(F, S, R, C, dev)
        ofdm.frame_estimate_sc16(qd, X, prefix, ws, float(scale))
        wf = ofdm.workspace(F, S, R, C, dev)
        ofdm.frame_estimate(torch.from_numpy(dequantise(q, scale)).to(dev), X, prefix, wf)
        for frame in (0, F - 1):
            H, P = ofdm.frame_export_estimate(ws, F, S, R, C, frame)
            Hf, Pf = ofdm.frame_export_estimate(wf, F, S, R, C, frame)
            parity(H.cpu().numpy(), Hf.cpu().numpy())
            parity(P.cpu().numpy(), Pf.cpu().numpy())
            got[(float(scale), frame)] = H.cpu().numpy()
    for frame in (0, F - 1):
        a, b = got[(float(S15), frame)], got[(float(np.float32(1.7) * S15), frame)]
        assert np.abs(a).max() > 0
        parity(b, a.astype(np.complex128) * float(np.float32(1.7)))


# ------------------------------------------- 4. one workspace, both formats

def test_one_workspace_both_formats(ofdm, dev, oracle):
    import torch
    c = case(ofdm, dev, oracle, (3, 4, 5, 7))
    q, Xh, prefix, _ = c
    ref = reference(oracle, c, S15)
    F, S, R, Cp, _ = q.shape
    C = Cp - prefix
    qd, X = torch.from_numpy(q).to(dev), torch.from_numpy(Xh).to(dev)
    fd = torch.from_numpy(dequantise(q, S15)).to(dev)
    nan = lambda: torch.full(ref.shape, float("nan"), dtype=torch.complex64, device=dev)

    whole = ofdm.frame_demod_sc16(qd, X, prefix, float(S15), out=nan()).cpu().numpy()
    ws = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate_sc16(qd, X, prefix, ws, float(S15))
    two = ofdm.frame_combine_sc16(qd, prefix, ws, nan(), float(S15)).cpu().numpy()
    assert np.array_equal(two.view(np.uint32), whole.view(np.uint32))
    # the sc16 estimate under the fp32 combine
    parity(ofdm.frame_combine(fd, prefix, ws, nan()).cpu().numpy(), ref)
    # the fp32 estimate under the sc16 combine
    wf = ofdm.workspace(F, S, R, C, dev)
    ofdm.frame_estimate(fd, X, prefix, wf)
    parity(ofdm.frame_combine_sc16(qd, prefix, wf, nan(), float(S15)).cpu().numpy(), ref)
    # a released workspace holds no estimate
    ofdm.workspace_release(ws)
    with pytest.raises(ofdm.OfdmError, match="holds no estimate"):
        ofdm.frame_combine_sc16(qd, prefix, ws, nan(), float(S15))
    # no sc16 receiver at C = 2048: the converter is named
    q2 = torch.zeros((1, 2, 1, 2048, 2), dtype=torch.int16, device=dev)
    with pytest.raises(ofdm.OfdmError, match="ofdm_iq_convert_sc16"):
        ofdm.frame_demod_sc16(q2, torch.zeros(2047, dtype=torch.complex64, device=dev))


# ------------------------------------------------------------- 5. pipeline

@pytest.mark.parametrize("pinned", [True, False])
def test_pipeline_c1024(ofdm, dev, oracle, pinned):
    c = case(ofdm, dev, oracle, (13, 4, 8, 7))
    q, Xh, prefix, _ = c
    ref = reference(oracle, c, S15)
    F, S, R, Cp, _ = q.shape
    q = q.copy()
    out, out2 = np.full(ref.shape, np.nan, np.complex64), np.full(ref.shape, np.nan, np.complex64)
    bufs = (q, out, out2) if pinned else ()
    for b in bufs:
        ofdm.host_register(b)
    try:
        with ofdm.Pipeline(S, R, Cp - prefix, Xh, prefix, chunk_frames=4, depth=3, sample_format="sc16",
                           scale=float(S15)) as p:
            p.demod(q, out)
            p.sync()
            p.demod(q, out2)  # slots reused, events already recorded
            p.sync()
    finally:
        for b in bufs:
            ofdm.host_unregister(b)
    parity(out, ref)
    assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))


@pytest.mark.parametrize("name", ["r4_c256_s5_cp32", "r8_c2048_s3_cp16"])
def test_pipeline_convert_route(ofdm, dev, oracle, name):
    c = case(ofdm, dev, oracle, name)
    q, Xh, prefix, _ = c
    ref = reference(oracle, c, UHD)
    F, S, R, Cp, _ = q.shape
    out = np.full(ref.shape, np.nan, np.complex64)
    with ofdm.Pipeline(S, R, Cp - prefix, Xh, prefix, chunk_frames=1, depth=2, sample_format="sc16",
                       scale=float(UHD)) as p:
        p.demod(q, out)
        p.sync()
    parity(out, ref)


def test_pipeline_manual_slots_and_format_mismatch(ofdm, dev, oracle):
    """acquire_sc16 / copy / submit as the ring reader does it, with
    submit(n < chunk) and submit(0); each format's calls on the other's pipeline."""
    import torch
    c = case(ofdm, dev, oracle, (13, 4, 8, 7))
    q, Xh, prefix, _ = c
    ref = reference(oracle, c, S15)[:6]
    F, S, R, Cp, _ = q.shape
    C = Cp - prefix
    qd = torch.from_numpy(q[:6]).to(dev)
    out = torch.full(ref.shape, float("nan"), dtype=torch.complex64, device=dev)
    frame_bytes = qd[0].numel() * 2
    with ofdm.Pipeline(S, R, C, Xh, prefix, chunk_frames=4, depth=2, sample_format="sc16", scale=float(S15)) as p:
        for lo, hi in ((0, 3), (3, 3), (3, 6)):
            d, s = p.acquire_sc16()
            n = hi - lo
            if n:
                _copy_to_ptr(d, qd[lo:hi], frame_bytes * n, s)
            p.submit(n, out[lo:hi] if n else None)
        p.sync()
        torch.cuda.synchronize()
        parity(out.cpu().numpy(), ref)
        with pytest.raises(ofdm.OfdmError, match="holds sc16"):
            p.acquire()
        with pytest.raises(ofdm.OfdmError, match="holds sc16"):
            ofdm._check(ofdm.lib().ofdm_pipeline_demod(p._h, ofdm._dptr(qd), 1, ofdm._dptr(out)), "ofdm_pipeline_demod")
    with ofdm.Pipeline(S, R, C, Xh, prefix, chunk_frames=4, depth=2) as p:
        with pytest.raises(ofdm.OfdmError, match="holds fp32"):
            p.acquire_sc16()
        with pytest.raises(ofdm.OfdmError, match="holds fp32"):
            ofdm._check(ofdm.lib().ofdm_pipeline_demod_sc16(p._h, ofdm._dptr(qd), 1, ofdm._dptr(out)),
                        "ofdm_pipeline_demod_sc16")
