"""Cost of ofdm_frame_estimate_denoise on a device-resident estimate, in one
process, against yardsticks that are not the code under test.

  python scripts/denoise_bench.py [--json OUT] [--quick]

Shapes (S = 101): the headline F = 1250, R = 64, C = 1024; configs[1]
F = 100, R = 16, C = 1024; C = 2048 / 4096 / 1536 at R = 64 with as many
frames as the headline's IQ bytes hold (625 / 312 / 833).  Per shape, variants
alternated launch by launch after warm-up, HIP-event times, median with
p10-p90:

  denoise        the entry on the workspace ofdm_frame_estimate filled (at
                 C = 1024 the wave kernel, elsewhere the stage kernel)
  denoise_any    C = 1024 only: the stage kernel, reached through a bin-layout
                 workspace (ofdm_frame_estimate_freq, S = 2) of the same F, R
                 -- the same rows and transforms, position = bin
  (a) hbm_copy   ofdm_hbm_probe mode 0 over F R C 8 + F C 2 bytes, so that
                 read + write move the denoiser's 2 F R C 8 + F C 4
  (b) estimate   ofdm_frame_estimate on the same batch
  (c) step       ofdm_frame_estimate + ofdm_frame_combine, the receiver's step;
                 share = denoise / step

The window (taps_post, taps_pre) = (C / 16, 8): the time does not depend on
it (the mask is a select).  Denoising is in place and repeated on its own
output, which costs the same.  No threshold: the figures go to DESIGN.md."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))

S = 101
SHAPES = [(1250, 64, 1024, 20), (100, 16, 1024, 200), (625, 64, 2048, 12), (312, 64, 4096, 12), (833, 64, 1536, 12)]
QUICK = [(40, 64, 1024, 20), (20, 16, 1024, 50), (20, 64, 2048, 10), (10, 64, 4096, 10), (24, 64, 1536, 10)]


def pilots(C, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    a = np.float32(0.70710678)
    Xh = (rng.choice([-a, a], C - 1) + 1j * rng.choice([-a, a], C - 1)).astype(np.complex64)
    return torch.from_numpy(Xh).to(dev)


def stats(ts):
    t = sorted(ts)
    return {"median_s": statistics.median(t), "p10_s": t[len(t) // 10], "p90_s": t[(9 * len(t)) // 10], "n": len(t)}


def one_shape(ofdm, dev, F, R, C, steps, warmup):
    import torch
    X = pilots(C, dev)
    iq = ofdm.c64((F, S, R, C), dev)
    step = max(1, (1 << 30) // (S * R * C * 8))
    for f0 in range(0, F, step):
        n = min(step, F - f0)
        ofdm.synth_frames(n, S, R, C, X, seed=7, frame0=f0, noise_std=0.02, out=iq[f0:f0 + n])
    ws = ofdm.workspace(F, S, R, C, dev)
    out = ofdm.c64((F, S - 1, C - 1), dev)
    tp, tq = C // 16, 8
    nbytes = 2 * F * R * C * 8 + F * C * 4
    half = (nbytes // 2 + 15) & ~15
    src = torch.empty(half, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    ofdm.frame_estimate(iq, X, 0, ws)

    def step_fn():
        ofdm.frame_estimate(iq, X, 0, ws)
        ofdm.frame_combine(iq, 0, ws, out)

    run = {
        "denoise": lambda: ofdm.frame_estimate_denoise(ws, F, S, R, C, tp, tq),
        "hbm_copy": lambda: ofdm.hbm_probe(0, src, dst),
        "estimate": lambda: ofdm.frame_estimate(iq, X, 0, ws),
        "step": step_fn,
    }
    if C == 1024:  # the stage kernel at the same F, R through a bin-layout workspace
        Y = torch.fft.fft(iq[:, :2], dim=-1).contiguous()
        wsb = ofdm.workspace(F, 2, R, C, dev)
        ofdm.frame_estimate_freq(Y, X, wsb)
        run["denoise_any"] = lambda: ofdm.frame_estimate_denoise(wsb, F, 2, R, C, tp, tq)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        for k in run:
            run[k]()
    torch.cuda.synchronize()
    ts = {k: [] for k in run}
    for _ in range(steps):
        for k in run:  # alternated: every variant sees the same drift of clocks and neighbours
            e0, e1 = ev(), ev()
            e0.record()
            run[k]()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
    ofdm.device_status()
    res = {"F": F, "S": S, "R": R, "C": C, "taps": [tp, tq], "steps": steps, "denoise_bytes": nbytes,
           "iq_bytes": iq.numel() * 8}
    for k in run:
        res[k] = stats(ts[k])
    d = res["denoise"]["median_s"]
    res["denoise_GBps"] = nbytes / d / 1e9
    res["denoise_over_hbm_copy"] = d / res["hbm_copy"]["median_s"]
    res["denoise_over_estimate"] = d / res["estimate"]["median_s"]
    res["denoise_share_of_step"] = d / res["step"]["median_s"]
    line = (f"F={F} R={R} C={C}: denoise {d * 1e3:.3f} ms ({res['denoise_GBps']:.0f} GB/s; p10 "
            f"{res['denoise']['p10_s'] * 1e3:.3f} p90 {res['denoise']['p90_s'] * 1e3:.3f}) = "
            f"{res['denoise_over_hbm_copy']:.2f} x copy of its bytes ({res['hbm_copy']['median_s'] * 1e3:.3f} ms), "
            f"{res['denoise_over_estimate']:.2f} x estimate ({res['estimate']['median_s'] * 1e3:.3f} ms), "
            f"{100 * res['denoise_share_of_step']:.2f} % of a step ({res['step']['median_s'] * 1e3:.3f} ms)")
    if "denoise_any" in res:
        res["fused_over_any"] = d / res["denoise_any"]["median_s"]
        line += f"; stage kernel {res['denoise_any']['median_s'] * 1e3:.3f} ms, wave / stage = {res['fused_over_any']:.3f}"
    print(line, flush=True)
    del iq, ws, out, src, dst, run
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "denoise", "denoise_bench.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="small batches: a rehearsal, not a measurement")
    a = ap.parse_args()
    import torch
    import ofdm_lsmrc as ofdm
    if not torch.cuda.is_available():
        sys.exit("denoise_bench: no GPU")
    dev = torch.device("cuda:0")
    rows = []
    for F, R, C, steps in (QUICK if a.quick else SHAPES):
        rows.append(one_shape(ofdm, dev, F, R, C, steps, a.warmup))
        rows[-1]["quick"] = bool(a.quick)
        rows[-1]["build_id"] = ofdm.build_id()
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            for r in rows:
                fp.write(json.dumps(r) + "\n")
    print(json.dumps({"denoise_bench": "ok", "share_of_step": {f"F{r['F']}_R{r['R']}_C{r['C']}": r["denoise_share_of_step"]
                                                               for r in rows}}))


if __name__ == "__main__":
    main()
