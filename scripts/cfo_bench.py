"""Carrier frequency offset: what the derotating C = 1024 receiver costs, in
one process on one device-resident batch.

  python scripts/cfo_bench.py [--json OUT]

Shapes: C = 1024, S = 101, cp = 72 at R = 64 x 400 frames and at R = 16 x 100
frames.  Variants, alternated launch by launch on the same frames, HIP-event
times, medians with p10-p90 after warm-up:
  a  the fp32 two-launch receiver        frame_demod(flow=FLOW_TWO_LAUNCH)
  b  the derotating receiver             frame_demod_cfo
  c  frame_cfo_derotate in place, then a (a read and a write of the whole IQ
     in front of the receiver: three times b's bytes)
  d  frame_cfo_estimate alone, against a streaming read (hbm_probe mode 1) of
     as many bytes as it touches (the first and last cp samples of each row)
Accepted when b is faster than c with p10-p90 ranges that do not overlap, at
both shapes (asserted); b / a and d's fraction are recorded as they are."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))

C, S, CP = 1024, 101, 72


def pilots(dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    a = np.float32(0.70710678)
    Xh = (rng.choice([-a, a], C - 1) + 1j * rng.choice([-a, a], C - 1)).astype(np.complex64)
    return torch.from_numpy(Xh).to(dev)


def shape(a, ofdm, dev, X, F, R, steps):
    import torch
    iq = torch.empty((F, S, R, C + CP), dtype=torch.complex64, device=dev)
    for f0 in range(0, F, 8):
        n = min(8, F - f0)
        ofdm.synth_frames(n, S, R, C, X, prefix=CP, seed=7, frame0=f0, noise_std=0.02, out=iq[f0:f0 + n])
    g = torch.Generator(device="cpu").manual_seed(1)
    eps = ((torch.rand(F, generator=g) - 0.5) * 0.9).to(torch.float32).to(dev)  # |eps| < 0.45, a frame each
    eps_out = torch.empty(F, dtype=torch.float32, device=dev)
    ws = {k: ofdm.workspace(F, S, R, C, dev) for k in "abc"}
    out = {k: ofdm.c64((F, S - 1, C - 1), dev) for k in "abc"}
    touched = F * S * R * 2 * CP * 8  # the estimator's bytes
    probe_src = torch.empty(touched // 16 * 16, dtype=torch.uint8, device=dev)
    probe_dst = torch.empty(1 << 20, dtype=torch.uint8, device=dev)

    def run_c():
        ofdm.frame_cfo_derotate(iq, CP, eps, out=iq)
        ofdm.frame_demod(iq, X, CP, ws["c"], out["c"], flow=ofdm.FLOW_TWO_LAUNCH)

    run = {"a": lambda: ofdm.frame_demod(iq, X, CP, ws["a"], out["a"], flow=ofdm.FLOW_TWO_LAUNCH),
           "b": lambda: ofdm.frame_demod_cfo(iq, X, CP, eps, ws["b"], out["b"]),
           "c": run_c,
           "d": lambda: ofdm.frame_cfo_estimate(iq, CP, 0, eps=eps_out),
           "read": lambda: ofdm.hbm_probe(1, probe_src, probe_dst)}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(a.warmup):
        for k in run:
            run[k]()
    ts = {k: [] for k in run}
    for _ in range(steps):
        for k in run:
            e0, e1 = ev(), ev()
            e0.record()
            run[k]()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
    Q = F * (S - 1)
    res = {"mode": "cfo_hbm_resident", "frames": F, "R": R, "C": C, "S": S, "cp": CP, "steps": steps,
           "iq_bytes": iq.numel() * 8, "estimator_bytes": touched}
    for k in run:
        t = sorted(ts[k])
        med = statistics.median(t)
        res[k] = {"median_s": med, "p10_s": t[len(t) // 10], "p90_s": t[(9 * len(t)) // 10]}
        extra = f"{Q / med / 1e6:7.3f} M data symbols/s" if k in "abc" else f"{touched / med / 1e12:5.2f} TB/s of {touched / 1e6:.1f} MB"
        print(f"R={R} x {F} frames {k:>4}: {med * 1e3:8.4f} ms (p10 {res[k]['p10_s'] * 1e3:.4f}, p90 "
              f"{res[k]['p90_s'] * 1e3:.4f})  {extra}")
    res["b_over_a"] = res["b"]["median_s"] / res["a"]["median_s"]
    res["c_over_b"] = res["c"]["median_s"] / res["b"]["median_s"]
    res["d_fraction_of_streaming_read"] = res["read"]["median_s"] / res["d"]["median_s"]
    res["accepted"] = res["b"]["p90_s"] < res["c"]["p10_s"]
    print(f"R={R} x {F}: b / a = {res['b_over_a']:.3f}, c / b = {res['c_over_b']:.3f}, the estimator at "
          f"{100 * res['d_fraction_of_streaming_read']:.1f} % of a streaming read of its bytes; "
          f"b faster than c, ranges apart: {res['accepted']}")
    del iq, ws, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="JSON lines, one per shape")
    a = ap.parse_args()

    import torch
    import ofdm_lsmrc as ofdm
    if not torch.cuda.is_available():
        sys.exit("cfo_bench: no GPU")
    dev = torch.device("cuda:0")
    X = pilots(dev)
    rows = [shape(a, ofdm, dev, X, 400, 64, 30), shape(a, ofdm, dev, X, 100, 16, 300)]
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            for r in rows:
                fp.write(json.dumps(r) + "\n")
    print(json.dumps({"cfo_bench": "ok", "b_over_a": {f"R{r['R']}x{r['frames']}": r["b_over_a"] for r in rows},
                      "c_over_b": {f"R{r['R']}x{r['frames']}": r["c_over_b"] for r in rows}}))
    for r in rows:
        assert r["accepted"], f"R={r['R']} x {r['frames']}: the derotating receiver is not clear of derotate + receiver"


if __name__ == "__main__":
    main()
