"""Soft-output kernels at the headline geometry, timed with HIP events beside
the box's copy probe in the same process.

  python scripts/soft_demap_bench.py [--frames 1250 --S 101 --R 64 --C 1024] [--reps 20] [--json OUT]

One real frame_demod fills z and the workspace.  Then, for every modulation:
ofdm_frame_noise_estimate, and ofdm_frame_soft_demap in both formats.  Each
variant's algorithmic traffic (z read + P read once + output written) is set
against ofdm_hbm_probe mode 0 moving the SAME byte count (half read, half
written), alternated with it, and against the receiver's step time.
Times are medians of --reps event-timed launches after warm-up."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--S", type=int, default=101)
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import ofdm_lsmrc as ofdm

    if not torch.cuda.is_available():
        sys.exit("soft_demap_bench: no GPU")
    dev = torch.device("cuda:0")
    F, S, R, C = a.frames, a.S, a.R, a.C
    K = C - 1
    rng = np.random.default_rng(0)
    amp = np.float32(0.70710678)
    X = torch.from_numpy((rng.choice([-amp, amp], K) + 1j * rng.choice([-amp, amp], K)).astype(np.complex64)).to(dev)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=0, seed=1234, noise_std=a.noise)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.c64((F, S - 1, K), dev)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return statistics.median(ts), min(ts), max(ts)

    step, step_lo, step_hi = timed(lambda: ofdm.frame_demod(iq, X, 0, ws=ws, out=z))
    errs = int(ofdm.count_symbol_errors(z, S, seed=1234).item())
    nelem = F * (S - 1) * K
    zbytes, pbytes = nelem * 8, F * C * 4
    res = {"geometry": {"F": F, "S": S, "R": R, "C": C}, "reps": a.reps, "step_s": step,
           "step_min_max_s": [step_lo, step_hi], "qpsk_symbol_errors": errs, "variants": []}
    print(f"frame_demod F={F} S={S} R={R} C={C}: step {step * 1e3:.3f} ms "
          f"({iq.numel() * 8 / step / 1e12:.2f} TB/s of IQ), {errs} QPSK symbol errors")

    # one pair of probe buffers, large enough for the widest variant
    cap = ((zbytes + pbytes + F * 4 + nelem * 8 * 4) // 32 + 1) * 16
    src = torch.zeros(cap, dtype=torch.uint8, device=dev)
    dst = torch.empty(cap, dtype=torch.uint8, device=dev)

    def copy_rate(traffic):
        half = traffic // 32 * 16  # the probe reads `half` and writes `half`
        t, _, _ = timed(lambda: ofdm.hbm_probe(0, src[:half], dst[:half]))
        return 2 * half / t, t

    def record(name, bps, traffic, t, lo, hi):
        cr, ct = copy_rate(traffic)
        row = {"kernel": name, "bps": bps, "traffic_bytes": traffic, "time_s": t, "time_min_max_s": [lo, hi],
               "bytes_per_s": traffic / t, "copy_probe_bytes_per_s": cr, "copy_probe_time_s": ct,
               "fraction_of_copy": traffic / t / cr, "fraction_of_step": t / step}
        res["variants"].append(row)
        print(f"{name:<22} bps {bps}: {t * 1e6:8.1f} us  {traffic / 1e9:6.3f} GB  {traffic / t / 1e12:5.2f} TB/s  "
              f"copy probe {cr / 1e12:5.2f} TB/s  -> {row['fraction_of_copy']:.3f} of copy, "
              f"{row['fraction_of_step']:.4f} of the step")

    for bps in (2, 4, 6, 8):
        nv = torch.empty(F, dtype=torch.float32, device=dev)
        t, lo, hi = timed(lambda: ofdm.frame_noise_estimate(z, ws, F, S, R, C, bps, out=nv))
        record("noise_estimate", bps, zbytes + pbytes + F * 4, t, lo, hi)
        for fmt, esz in (("f32", 4), ("i8", 1)):
            out = torch.empty((F, S - 1, K, bps), dtype=torch.float32 if fmt == "f32" else torch.int8, device=dev)
            t, lo, hi = timed(lambda: ofdm.frame_soft_demap(z, ws, F, S, R, C, bps, nv, fmt=fmt, scale=4.0, out=out))
            record(f"soft_demap {fmt}", bps, zbytes + pbytes + F * 4 + nelem * bps * esz, t, lo, hi)
            del out
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            json.dump(res, fp, indent=1)
    print(json.dumps({"soft_demap_bench": "ok", "step_ms": step * 1e3,
                      "worst_fraction_of_copy": min(v["fraction_of_copy"] for v in res["variants"])}))


if __name__ == "__main__":
    main()
