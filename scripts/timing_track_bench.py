"""Phase and timing tracking (ofdm_frame_timing_track) timed with HIP events
beside the phase tracker and the box's copy probe in the same process
(DESIGN.md section 7o).

  python scripts/timing_track_bench.py [--S 101 --C 1024] [--json OUT]

Shapes: C = 1024, S = 101 at R = 64 x 1250 frames (the headline batch), at
R = 16 x 100 frames, and one frame alone (R = 16): one workgroup, so its time
over S - 1 is the serial chain per row.  At each shape one real frame_demod
fills z and the workspace; then, for every modulation, three launches are
alternated one by one: this tracker (out of place, phases and timing
written), ofdm_frame_phase_track (out of place, phases written) and
ofdm_hbm_probe mode 0 moving the SAME byte count (z read + out written: half
read, half written).  HIP-event times, medians with p10-p90 after warm-up."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))


def shape(a, ofdm, dev, X, F, R, reps):
    import torch
    S, C = a.S, a.C
    K = C - 1
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=0, seed=1234, noise_std=a.noise)
    ws = ofdm.workspace(F, S, R, C, dev)
    z = ofdm.c64((F, S - 1, K), dev)
    out = ofdm.c64((F, S - 1, K), dev)
    phase = torch.empty((F, S - 1), dtype=torch.float32, device=dev)
    timing = torch.empty((F, S - 1), dtype=torch.float32, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    ofdm.frame_demod(iq, X, 0, ws=ws, out=z)
    errs = int(ofdm.count_symbol_errors(z, S, seed=1234).item())
    del iq
    torch.cuda.empty_cache()
    nelem = F * (S - 1) * K
    traffic = 2 * nelem * 8  # z read + out written (P, the phases and the timing: under 0.1 %)
    half = traffic // 32 * 16
    src = torch.zeros(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    probe = lambda: ofdm.hbm_probe(0, src, dst)
    rows = []
    for bps in (2, 4, 6, 8):
        track = lambda: ofdm.frame_timing_track(z, ws, F, S, R, C, bps, out=out, phase=phase, timing=timing)
        ptrack = lambda: ofdm.frame_phase_track(z, ws, F, S, R, C, bps, out=out, phase=phase)
        for _ in range(a.warmup):
            track()
            ptrack()
            probe()
        tt, tq, tp = [], [], []
        for _ in range(reps):
            tt.append(timed(track))
            tq.append(timed(ptrack))
            tp.append(timed(probe))
        for v in (tt, tq, tp):
            v.sort()
        t, q, c = statistics.median(tt), statistics.median(tq), statistics.median(tp)
        p10, p90 = lambda v: v[len(v) // 10], lambda v: v[(9 * len(v)) // 10]
        row = {"mode": "timing_track", "frames": F, "R": R, "C": C, "S": S, "bps": bps, "reps": reps,
               "traffic_bytes": traffic, "time_s": t, "p10_s": p10(tt), "p90_s": p90(tt),
               "phase_track_time_s": q, "phase_track_p10_s": p10(tq), "phase_track_p90_s": p90(tq),
               "copy_probe_time_s": c, "copy_probe_p10_s": p10(tp), "copy_probe_p90_s": p90(tp),
               "copy_probe_bytes_per_s": 2 * half / c, "fraction_of_copy_rate": (traffic / t) / (2 * half / c),
               "phase_track_fraction_of_copy_rate": (traffic / q) / (2 * half / c), "ratio_to_phase_track": t / q,
               "per_row_s": t / (S - 1), "phase_track_per_row_s": q / (S - 1), "qpsk_symbol_errors_of_input": errs}
        rows.append(row)
        print(f"R={R} x {F} frames bps {bps}: {t * 1e6:9.1f} us (p10 {row['p10_s'] * 1e6:.1f}, p90 {row['p90_s'] * 1e6:.1f})  "
              f"{traffic / t / 1e12:5.2f} TB/s of {traffic / 1e9:.3f} GB; phase tracker {q * 1e6:.1f} us "
              f"(p10 {p10(tq) * 1e6:.1f}, p90 {p90(tq) * 1e6:.1f}) -> x{t / q:.3f}; copy probe {c * 1e6:.1f} us -> "
              f"{row['fraction_of_copy_rate']:.3f} of the copy rate (phase tracker "
              f"{row['phase_track_fraction_of_copy_rate']:.3f}); {t / (S - 1) * 1e6:.3f} us per row "
              f"(phase tracker {q / (S - 1) * 1e6:.3f})")
    del ws, z, out, src, dst
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=101)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--json", default=None, help="JSON lines, one per shape and modulation")
    a = ap.parse_args()

    import numpy as np
    import torch
    import ofdm_lsmrc as ofdm

    if not torch.cuda.is_available():
        sys.exit("timing_track_bench: no GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    amp = np.float32(0.70710678)
    K = a.C - 1
    X = torch.from_numpy((rng.choice([-amp, amp], K) + 1j * rng.choice([-amp, amp], K)).astype(np.complex64)).to(dev)
    rows = shape(a, ofdm, dev, X, 1250, 64, 30) + shape(a, ofdm, dev, X, 100, 16, 100) + shape(a, ofdm, dev, X, 1, 16, 100)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            for r in rows:
                fp.write(json.dumps(r) + "\n")
    key = lambda r: f"R{r['R']}x{r['frames']}bps{r['bps']}"
    print(json.dumps({"timing_track_bench": "ok",
                      "fraction_of_copy_rate": {key(r): round(r["fraction_of_copy_rate"], 4) for r in rows},
                      "ratio_to_phase_track": {key(r): round(r["ratio_to_phase_track"], 4) for r in rows},
                      "chain_us_per_row": {f"bps{r['bps']}": round(r["per_row_s"] * 1e6, 3)
                                           for r in rows if r["frames"] == 1}}))


if __name__ == "__main__":
    main()
