"""Integer carrier offset: what the pilot-symbol search costs and how far its
best shift stands above the runner-up, in one process.

  python scripts/acquire_bench.py [--frames 1250] [--steps 20] [--json OUT]

Timing, at the headline geometry (C = 1024, S = 101, R = 64, cp = 72, D = 16)
on one device-resident batch, variants alternated launch by launch, HIP-event
times, medians with p10-p90 after warm-up:
  p  frame_cfo_estimate -> frame_demod_cfo            (the chain without the search)
  q  frame_cfo_estimate -> frame_cfo_acquire -> frame_demod_cfo
  s  frame_cfo_acquire alone
  copy  a device copy (hbm_probe mode 0) of as many bytes as the search reads,
        the pilot symbol's: frames x R x (C + cp) x 8
Margins: the ratio of the largest to the second largest stored metric over
frames of tests/acquire_cases.py (4-tap channel, random QPSK pilots, sigma =
0.02) at offsets up to +-D, on noise-only frames and on the reference's
constant fallback pilots."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

C, S, R, CP, D = 1024, 101, 64, 72, 16


def timing(a, ofdm, dev):
    import numpy as np
    import torch
    F = a.frames
    rng = np.random.default_rng(0)
    h = np.float32(0.70710678)
    X = torch.from_numpy((rng.choice([-h, h], C - 1) + 1j * rng.choice([-h, h], C - 1)).astype(np.complex64)).to(dev)
    iq = torch.empty((F, S, R, C + CP), dtype=torch.complex64, device=dev)
    for f0 in range(0, F, 8):
        n = min(8, F - f0)
        ofdm.synth_frames(n, S, R, C, X, prefix=CP, seed=7, frame0=f0, noise_std=0.02, out=iq[f0:f0 + n])
    eps = {k: torch.empty(F, dtype=torch.float32, device=dev) for k in "pqs"}
    ws = {k: ofdm.workspace(F, S, R, C, dev) for k in "pq"}
    out = {k: ofdm.c64((F, S - 1, C - 1), dev) for k in "pq"}
    pilot_bytes = F * R * (C + CP) * 8
    src = torch.empty(pilot_bytes // 16 * 16, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ofdm.frame_cfo_estimate(iq, CP, 0, eps=eps["s"])

    def run_p():
        ofdm.frame_cfo_estimate(iq, CP, 0, eps=eps["p"])
        ofdm.frame_demod_cfo(iq, X, CP, eps["p"], ws["p"], out["p"])

    def run_q():
        ofdm.frame_cfo_estimate(iq, CP, 0, eps=eps["q"])
        ofdm.frame_cfo_acquire(iq, X, CP, D, eps=eps["q"], out=eps["q"])
        ofdm.frame_demod_cfo(iq, X, CP, eps["q"], ws["q"], out["q"])

    run = {"p": run_p, "q": run_q, "s": lambda: ofdm.frame_cfo_acquire(iq, X, CP, D, eps=eps["s"], out=eps["q"]),
           "copy": lambda: ofdm.hbm_probe(0, src, dst)}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(a.warmup):
        for k in run:
            run[k]()
    ts = {k: [] for k in run}
    for _ in range(a.steps):
        for k in run:
            e0, e1 = ev(), ev()
            e0.record()
            run[k]()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e-3)
    assert torch.equal(out["p"], out["q"]), "the synthetic frames carry no offset: the search must change nothing"
    res = {"mode": "acquire_hbm_resident", "frames": F, "R": R, "C": C, "S": S, "cp": CP, "max_shift": D,
           "steps": a.steps, "iq_bytes": iq.numel() * 8, "pilot_bytes": pilot_bytes}
    for k in run:
        t = sorted(ts[k])
        med = statistics.median(t)
        res[k] = {"median_s": med, "p10_s": t[len(t) // 10], "p90_s": t[(9 * len(t)) // 10]}
        print(f"R={R} x {F} frames {k:>4}: {med * 1e3:8.4f} ms (p10 {res[k]['p10_s'] * 1e3:.4f}, p90 "
              f"{res[k]['p90_s'] * 1e3:.4f})")
    res["q_over_p"] = res["q"]["median_s"] / res["p"]["median_s"]
    res["search_share_of_p"] = res["s"]["median_s"] / res["p"]["median_s"]
    res["search_read_TBps"] = pilot_bytes / res["s"]["median_s"] / 1e12
    res["copy_TBps_each_way"] = pilot_bytes / res["copy"]["median_s"] / 1e12
    res["copy_over_search"] = res["copy"]["median_s"] / res["s"]["median_s"]
    print(f"q / p = {res['q_over_p']:.4f}; the search alone is {100 * res['search_share_of_p']:.2f} % of p, reads its "
          f"{pilot_bytes / 1e6:.0f} MB at {res['search_read_TBps']:.2f} TB/s; a copy of those bytes takes "
          f"{100 * res['copy_over_search']:.1f} % of its time ({res['copy_TBps_each_way']:.2f} TB/s each way)")
    del iq, ws, out
    torch.cuda.empty_cache()
    return res


def margins(ofdm, dev):
    import numpy as np
    import torch
    import acquire_cases as ac
    import cfo_cases as cc
    rows = []

    def ratios(c, cp, Dm):
        y, X = torch.from_numpy(np.array(c["y"])).to(dev), torch.from_numpy(np.array(c["X"])).to(dev)
        F = y.shape[0]
        eps = ofdm.frame_cfo_estimate(y, cp)
        shift = torch.empty(F, dtype=torch.int32, device=dev)
        metric = torch.empty((F, 2 * Dm + 1), dtype=torch.float32, device=dev)
        ofdm.frame_cfo_acquire(y, X, cp, Dm, eps=eps, min_ratio=1.0, shift=shift, metric=metric)
        torch.cuda.synchronize()
        m = np.sort(metric.cpu().numpy().astype(np.float64), axis=1)
        want = np.rint(np.asarray(c["eps"], np.float64) - eps.cpu().numpy())
        return m[:, -1] / m[:, -2], shift.cpu().numpy(), want

    for Cm, Rm, cp, Dm in ((1024, 4, 16, 32), (600, 3, 9, 32), (256, 2, 16, 32), (64, 1, 8, 16)):
        eps = np.array([2.03, -3.2, 0.45, 7.0, -0.496, Dm - 0.45, -Dm + 0.3, 11.5 if Dm > 16 else 5.5], np.float32)
        lo, hi, ok = np.inf, 0.0, True
        for seed in range(4):
            c = ac.frames(len(eps), 2, Rm, Cm, cp, eps, ac.random_pilots(Cm - 1, seed=seed), seed=seed)
            r, sh, want = ratios(c, cp, Dm)
            lo, hi, ok = min(lo, r.min()), max(hi, r.max()), ok and np.array_equal(sh, want.astype(np.int32))
        rows.append({"case": f"C = {Cm}, R = {Rm}", "max_shift": Dm, "min": lo, "max": hi, "all_recovered": bool(ok)})
    z = np.zeros(8, np.float32)
    lo, hi = np.inf, 0.0
    for Cm, Rm, cp in ((1024, 4, 16), (256, 2, 16)):
        c = ac.frames(8, 2, Rm, Cm, cp, z, ac.random_pilots(Cm - 1, seed=1), seed=1, noise_only=True)
        r = ratios(c, cp, 16)[0]
        lo, hi = min(lo, r.min()), max(hi, r.max())
    rows.append({"case": "noise-only frames", "max_shift": 16, "min": lo, "max": hi})
    lo, hi = np.inf, 0.0
    for Cm, Rm, cp in ((1024, 4, 16), (256, 2, 16)):
        c = ac.frames(8, 2, Rm, Cm, cp, z + 2, ac.constant_pilots(Cm - 1), seed=2)
        r = ratios(c, cp, 16)[0]
        lo, hi = min(lo, r.min()), max(hi, r.max())
    rows.append({"case": "constant fallback pilots", "max_shift": 16, "min": lo, "max": hi})
    for r in rows:
        print(f"{r['case']:>28}: best / runner-up {r['min']:.2f} - {r['max']:.2f}"
              + ("" if "all_recovered" not in r else f", every offset recovered: {r['all_recovered']}"))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1250)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import ofdm_lsmrc as ofdm
    if not torch.cuda.is_available():
        sys.exit("acquire_bench: no GPU")
    dev = torch.device("cuda:0")
    res = {"margins": margins(ofdm, dev), "timing": timing(a, ofdm, dev)}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            fp.write(json.dumps(res) + "\n")
    print(json.dumps({"acquire_bench": "ok", "q_over_p": res["timing"]["q_over_p"],
                      "search_share_of_p": res["timing"]["search_share_of_p"]}))


if __name__ == "__main__":
    main()
