"""The OFDM modulator (ofdm_tx_modulate) timed with HIP events beside the box's
copy probe and beside the unfused route, in the same process (DESIGN.md
section 7e).

  python scripts/tx_bench.py [--rows 128000] [--reps 20] [--json OUT]

Shapes: C = 1024 with cp = 0 and cp = 72 (one wave per row), C = 1536, 2048
and 4096 (one workgroup per row), cp = 72.  For each:
  * the fused kernel (MAP_REFERENCE, NORM_PEAK, peaks stored): time and the
    rate on its algorithmic traffic, K * 8 B read + (C + cp) * 8 B written
    per row;
  * ofdm_hbm_probe mode 0 moving the SAME byte count (half read, half
    written), alternated with the kernel launch by launch;
  * the unfused chain the library allowed before: torch scatter of the K
    values into C bins, ofdm_fft_rows(inverse), torch abs / amax, scale and
    the concatenation behind the prefix, on the same input.
Times are medians of --reps event-timed runs after warm-up."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1024, 0), (1024, 72), (1536, 72), (2048, 72), (4096, 72)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64 * 2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import ofdm_lsmrc as ofdm
    from tx_cases import bin_of

    if not torch.cuda.is_available():
        sys.exit("tx_bench: no GPU")
    dev = torch.device("cuda:0")
    n = a.rows

    def event_timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def timed(*fns):
        """medians of the functions' times, run alternately"""
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        ts = [[] for _ in fns]
        for _ in range(a.reps):
            for i, fn in enumerate(fns):
                ts[i].append(event_timed(fn))
        return [statistics.median(t) for t in ts]

    res = {"rows": n, "reps": a.reps, "shapes": []}
    for C, cp in SHAPES:
        K = C - 1
        g = torch.Generator(device=dev)
        g.manual_seed(C + cp)
        X = torch.view_as_complex(torch.randn((n, K, 2), device=dev, generator=g))
        out = ofdm.c64((n, C + cp), dev)
        traffic = n * (K + C + cp) * 8
        half = traffic // 32 * 16  # the probe reads `half` and writes `half`
        src = torch.zeros(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        peak = torch.empty(n, dtype=torch.float32, device=dev)
        L = ofdm.lib()
        s = torch.cuda.current_stream().cuda_stream

        def fused():
            rc = L.ofdm_tx_modulate(X.data_ptr(), K, n, C, cp, 0, 0, 1.0, out.data_ptr(), peak.data_ptr(), s)
            assert rc == 0, L.ofdm_last_error()

        t_k, t_p = timed(fused, lambda: ofdm.hbm_probe(0, src, dst))
        del src, dst

        idx = torch.tensor([bin_of(k, C, "reference") for k in range(K)], device=dev)
        bins = torch.zeros((n, C), dtype=torch.complex64, device=dev)
        tmp = ofdm.c64((n, C), dev)

        def chain():
            bins[:, idx] = X
            ofdm.fft_rows(bins, out=tmp, inverse=True)
            pk = tmp.abs().amax(dim=1, keepdim=True)
            y = tmp * (1.0 / pk)
            return torch.cat([y[:, C - cp:], y], dim=1)

        want = chain()
        fused()
        err = (torch.linalg.vector_norm(out - want) / torch.linalg.vector_norm(want)).item()
        del want
        (t_c,) = timed(chain)
        del bins, tmp, X, out
        torch.cuda.empty_cache()
        row = {"C": C, "cp": cp, "traffic_bytes": traffic, "time_s": t_k, "bytes_per_s": traffic / t_k,
               "copy_probe_time_s": t_p, "copy_probe_bytes_per_s": 2 * half / t_p,
               "fraction_of_copy": (traffic / t_k) / (2 * half / t_p), "unfused_chain_time_s": t_c,
               "chain_over_fused": t_c / t_k, "fused_vs_chain_norm_rel": err}
        res["shapes"].append(row)
        print(f"C={C:<5} cp={cp:<3}: {t_k * 1e6:9.1f} us  {traffic / 1e9:6.3f} GB  {traffic / t_k / 1e12:5.2f} TB/s  "
              f"copy probe {2 * half / t_p / 1e12:5.2f} TB/s -> {row['fraction_of_copy']:.3f} of copy;  "
              f"unfused chain {t_c * 1e6:9.1f} us = {t_c / t_k:5.2f} x the fused kernel  (agree to {err:.1e})")
        assert err < 1e-5, "the fused kernel and the unfused chain disagree"
        if C == 1024:
            assert t_k < t_c, "the fused C = 1024 kernel must beat the chain that moves three times its bytes"
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            json.dump(res, fp, indent=1)
    print(json.dumps({"tx_bench": "ok", "c1024_chain_over_fused": [r["chain_over_fused"] for r in res["shapes"][:2]]}))


if __name__ == "__main__":
    main()
