"""The QC-LDPC decoder (ofdm_ldpc_decode) timed with HIP events beside the
receiver, the demapper and the Viterbi decoder, in the same process
(DESIGN.md section 7r).

  python scripts/ldpc_bench.py [--json OUT] [--isa-only]

The code is the tests' rate-1/2 code of N = 1944 (Z = 81, nb = 24, mb = 12, row
degrees 7 and 8: tests/ldpc_cases.code_1944).  Shapes, int8 LLRs: 125 000
codewords (one per QPSK symbol of the headline step, F = 1250, S = 101,
C = 1024), 10 000, and one codeword alone; each at early_stop = 0 with 1 and
with 10 iterations, whose difference over 9 is the time of one iteration
without the load, the syndrome and the output.  The LLRs are the all-zero
codeword as BPSK +1 plus Gaussian noise of std 0.7, LLR = 2 x / sigma^2, int8
at scale 8.  Then one run with early_stop = 1 and max_iter = 20 on the same
LLRs (the iterations it took and the words it recovered are printed), and
frame_demod, frame_soft_demap (int8) and viterbi_decode at their headline
shapes.  HIP-event times, medians of 20 with p10-p90 after warm-up.

Beside the times: the instructions of k_ldpc<true>'s three edge loops (pass 1,
pass 2, syndrome), counted per edge from the disassembly of the code object
inside the library (llvm-objdump), and the time they imply for an iteration at
one vector instruction per 4 cycles per wave and at most one per 2 cycles per
SIMD (MI355X: 1024 SIMDs), as scripts/viterbi_bench.py counts, at the clock
given by --ghz; and the LDS bound at one wave access per clock per CU."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "k_ldpcILb1E"


def disassembly(lib, kernel):
    """[(label or None, mnemonic or None, branch target or None)] of `kernel` in the gfx950 code object inside lib."""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib], check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)] + [len(data)]
        for i in range(len(starts) - 1):
            b, o = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"b{i}.o")
            with open(b, "wb") as fp:
                fp.write(data[starts[i]:starts[i + 1]])
            r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={b}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={o}"], capture_output=True)
            if r.returncode or not os.path.exists(o) or os.path.getsize(o) == 0:
                continue
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--symbolize-operands", "--no-show-raw-insn", o],
                                 capture_output=True, text=True, check=True).stdout
            if kernel in dis:
                break
        else:
            raise RuntimeError(f"{kernel} not found in {lib}")
    body = dis.split(kernel, 1)[1]
    body = re.split(r"\n[0-9a-f]+ <_Z", body, 1)[0]  # up to the next function
    lines = []
    for ln in body.splitlines():
        ln = ln.split("//")[0]
        m = re.match(r"\s*[0-9a-f]* ?<(L\d+)>:", ln)
        if m:
            lines.append((m.group(1), None, None))
            continue
        m = re.match(r"\s*([a-z_0-9]+)\b(.*)", ln)
        if m and re.match(r"^(v_|s_|ds_|global_|buffer_|flat_)", m.group(1)):
            t = re.search(r"\b(L\d+)\b", m.group(2)) if m.group(1).startswith(("s_branch", "s_cbranch")) else None
            lines.append((None, m.group(1), t.group(1) if t else None))
    return lines


def edge_loops(lib):
    """{pass1, pass2, syndrome: (vector, LDS, scalar instructions per edge, edges per trip)} of KERNEL's innermost
    loops: pass 2 is the one that writes message bytes, pass 1 the other one that reads them, the syndrome loop
    the one of the others with the most 16-bit LDS reads (the unrolled body, not its remainder)."""
    lines = disassembly(lib, KERNEL)
    labels = {lab: i for i, (lab, _, _) in enumerate(lines) if lab}
    back = [(labels[t], i) for i, (_, op, t) in enumerate(lines)
            if op and op.startswith(("s_branch", "s_cbranch")) and t in labels and labels[t] <= i]
    inner = [(h, e) for h, e in back if not any((h2, e2) != (h, e) and h <= h2 and e2 <= e for h2, e2 in back)]
    out = {}
    for h, e in inner:
        ops = [op for _, op, _ in lines[h:e + 1] if op]
        n = lambda name: sum(op == name for op in ops)
        vec = sum(op.startswith(("v_", "ds_", "global_", "buffer_", "flat_")) for op in ops)
        lds = sum(op.startswith("ds_") for op in ops)
        if n("ds_write_b8"):
            kind, edges = "pass2", n("ds_write_b8")
        elif n("ds_read_i8"):
            kind, edges = "pass1", n("ds_read_i8")
        elif n("ds_read_i16") and n("ds_read_i16") > out.get("syndrome", (0, 0, 0, 0))[3]:
            kind, edges = "syndrome", n("ds_read_i16")
        else:
            continue
        out[kind] = (vec / edges, lds / edges, (len(ops) - vec) / edges, edges)
    if set(out) != {"pass1", "pass2", "syndrome"}:
        raise RuntimeError(f"edge loops not recognised: {sorted(out)}")
    return out


def timed_median(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ghz", type=float, default=2.4, help="clock for the issue-bound estimate")
    ap.add_argument("--no-receiver", action="store_true", help="skip frame_demod / frame_soft_demap / viterbi_decode")
    ap.add_argument("--isa-only", action="store_true", help="only count the edge loops' instructions (no GPU needed)")
    ap.add_argument("--json", default=None, help="JSON lines, one per measurement")
    a = ap.parse_args()

    import ofdm_lsmrc as ofdm
    import ldpc_cases as lc
    loops = edge_loops(ofdm.LIB_PATH)
    for k, (vec, lds, sc, edges) in sorted(loops.items()):
        print(f"{KERNEL} {k}: {vec:.2f} vector instructions per edge, {lds:.2f} of them LDS accesses, {sc:.2f} scalar "
              f"({edges} edges per trip)")
    vec_iter = loops["pass1"][0] + loops["pass2"][0]  # per edge of an iteration without the syndrome
    lds_iter = loops["pass1"][1] + loops["pass2"][1]
    rows = [{"mode": "isa", "kernel": KERNEL, **{k: dict(zip(("vector_per_edge", "lds_per_edge", "scalar_per_edge",
                                                              "edges_per_trip"), v)) for k, v in loops.items()}}]
    if a.isa_only:
        print(json.dumps({"ldpc_bench": "isa", "vector_per_edge_iteration": round(vec_iter, 2),
                          "lds_per_edge_iteration": round(lds_iter, 2), "vector_per_edge_syndrome": round(loops["syndrome"][0], 2)}))
        return

    import torch
    if not torch.cuda.is_available():
        sys.exit("ldpc_bench: no GPU")
    dev = torch.device("cuda:0")
    c = lc.code_1944()
    code = ofdm.QcLdpc(c.mb, c.nb, c.Z, c.rows)
    Nc, nnz, waves = lc.N(c), lc.nnz(c), (c.Z + 63) // 64
    sigma, scale = 0.7, 8.0
    summary = {}
    for ncw, reps in ((125000, a.reps), (10000, a.reps), (1, 5 * a.reps)):
        g = torch.Generator(device=dev)
        g.manual_seed(ncw)
        llr = (2.0 / sigma ** 2) * (1.0 + sigma * torch.randn((ncw, Nc), generator=g, device=dev, dtype=torch.float32))
        q = torch.clamp(torch.round(llr * scale), -127, 127).to(torch.int8)
        raw_wrong = int((q < 0).sum().item())
        del llr
        bits = torch.empty((ncw, (Nc + 7) // 8), dtype=torch.uint8, device=dev)
        iters = torch.empty(ncw, dtype=torch.int32, device=dev)
        t = {}
        for mi in (1, 10):
            fn = lambda: ofdm.ldpc_decode(q, code, max_iter=mi, early_stop=False, out=bits, iters=iters)
            t[mi] = timed_median(torch, fn, a.warmup, reps)
        per_iter = (t[10][0] - t[1][0]) / 9
        # an iteration's wave instructions: every wave of a codeword runs every edge's; one wave issues a vector
        # instruction per 4 cycles, a SIMD (1024 of them) at most one per 2; an LDS access per clock per CU (256)
        issue = nnz * vec_iter * max(4.0, 2.0 * ncw * waves / 1024.0) / (a.ghz * 1e9)
        lds = nnz * lds_iter * max(1.0, ncw * waves / 256.0) / (a.ghz * 1e9)
        bound = max(issue, lds)
        fn = lambda: ofdm.ldpc_decode(q, code, max_iter=20, early_stop=True, out=bits, iters=iters)
        t_es = timed_median(torch, fn, a.warmup, reps)
        it = iters.cpu().numpy()
        wrong_words = int((torch.count_nonzero(bits, dim=1) > 0).sum().item())
        row = {"mode": "ldpc", "ncw": ncw, "N": Nc, "Z": c.Z, "nnz": nnz, "reps": reps, "time_1_iter_s": t[1][0],
               "p10_1_s": t[1][1], "p90_1_s": t[1][2], "time_10_iter_s": t[10][0], "p10_10_s": t[10][1], "p90_10_s": t[10][2],
               "per_iteration_s": per_iter, "issue_bound_s": issue, "lds_bound_s": lds, "per_iteration_over_bound": per_iter / bound,
               "early_stop_s": t_es[0], "early_stop_p10_s": t_es[1], "early_stop_p90_s": t_es[2],
               "early_stop_mean_iterations": float(abs(it).mean()), "early_stop_max_iterations": int(abs(it).max()),
               "early_stop_failed": int((it < 0).sum()), "early_stop_wrong_words": wrong_words, "raw_wrong_signs": raw_wrong,
               "coded_bits_per_s_early_stop": ncw * Nc / t_es[0]}
        rows.append(row)
        summary[str(ncw)] = row
        print(f"{ncw:6d} codewords: 1 iteration {t[1][0] * 1e6:9.1f} us (p10 {t[1][1] * 1e6:.1f}, p90 {t[1][2] * 1e6:.1f}), "
              f"10 iterations {t[10][0] * 1e6:9.1f} us (p10 {t[10][1] * 1e6:.1f}, p90 {t[10][2] * 1e6:.1f}) -> "
              f"{per_iter * 1e6:.2f} us per iteration; issue bound {issue * 1e6:.2f} us, LDS bound {lds * 1e6:.2f} us -> "
              f"x{per_iter / bound:.2f}")
        print(f"       early stop, max 20: {t_es[0] * 1e6:9.1f} us (p10 {t_es[1] * 1e6:.1f}, p90 {t_es[2] * 1e6:.1f}), "
              f"{abs(it).mean():.2f} iterations on average, {abs(it).max()} at most, {int((it < 0).sum())} not converged, "
              f"{wrong_words} words wrong; {raw_wrong} of {ncw * Nc} raw signs wrong; "
              f"{ncw * Nc / t_es[0] / 1e9:.2f} Gbit/s of coded bits")
        del q, bits, iters
        torch.cuda.empty_cache()

    rx = {}
    if not a.no_receiver:
        import numpy as np
        F, S, R, C = 1250, 101, 64, 1024
        rng = np.random.default_rng(0)
        amp = np.float32(0.70710678)
        X = torch.from_numpy((rng.choice([-amp, amp], C - 1) + 1j * rng.choice([-amp, amp], C - 1)).astype(np.complex64)).to(dev)
        iq = ofdm.synth_frames(F, S, R, C, X, prefix=0, seed=1234, noise_std=0.05)
        ws = ofdm.workspace(F, S, R, C, dev)
        z = ofdm.c64((F, S - 1, C - 1), dev)
        t_demod = timed_median(torch, lambda: ofdm.frame_demod(iq, X, 0, ws=ws, out=z), 2, 7)
        del iq
        torch.cuda.empty_cache()
        nv = ofdm.frame_noise_estimate(z, ws, F, S, R, C, 2)
        llr8 = torch.empty((F, S - 1, C - 1, 2), dtype=torch.int8, device=dev)
        t_demap = timed_median(torch, lambda: ofdm.frame_soft_demap(z, ws, F, S, R, C, 2, nv, fmt="i8", scale=2.0, out=llr8),
                               a.warmup, a.reps)
        vcode = ofdm.ConvCode.k7_rate_half()
        vbits = torch.empty((125000, 128), dtype=torch.uint8, device=dev)
        metric = torch.empty(125000, dtype=torch.int32, device=dev)
        t_vit = timed_median(torch, lambda: ofdm.viterbi_decode(llr8.reshape(125000, 2046), vcode, 1017, out=vbits,
                                                                metric=metric), a.warmup, a.reps)
        # the demapper's own bytes through the LDPC decoder, 1944 of each symbol's 2046 (random QPSK data, not
        # codewords: nothing converges, so this is the time of 10 full iterations with the syndrome after each)
        bits = torch.empty((125000, 243), dtype=torch.uint8, device=dev)
        iters = torch.empty(125000, dtype=torch.int32, device=dev)
        t_chain = timed_median(torch, lambda: ofdm.ldpc_decode(llr8.reshape(-1), code, ncw=125000, stride=2046, n_rx=1944,
                                                               max_iter=10, out=bits, iters=iters), a.warmup, a.reps)
        head = summary["125000"]
        rx = {"mode": "receiver", "frames": F, "S": S, "R": R, "C": C, "frame_demod_s": t_demod[0],
              "frame_soft_demap_i8_s": t_demap[0], "viterbi_decode_s": t_vit[0], "ldpc_10_iter_on_demapper_bytes_s": t_chain[0],
              "ldpc_early_stop_over_frame_demod": head["early_stop_s"] / t_demod[0],
              "ldpc_10_iter_over_frame_demod": head["time_10_iter_s"] / t_demod[0],
              "ldpc_early_stop_over_viterbi": head["early_stop_s"] / t_vit[0]}
        rows.append(rx)
        print(f"headline shape R={R} x {F} frames: frame_demod {t_demod[0] * 1e6:.1f} us, frame_soft_demap (i8) "
              f"{t_demap[0] * 1e6:.1f} us, viterbi_decode {t_vit[0] * 1e6:.1f} us, ldpc_decode on the demapper's bytes "
              f"(10 iterations, none converges) {t_chain[0] * 1e6:.1f} us; ldpc early stop / frame_demod "
              f"x{rx['ldpc_early_stop_over_frame_demod']:.3f}, 10 iterations / frame_demod x{rx['ldpc_10_iter_over_frame_demod']:.3f}, "
              f"early stop / viterbi x{rx['ldpc_early_stop_over_viterbi']:.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            for r in rows:
                fp.write(json.dumps(r) + "\n")
    print(json.dumps({"ldpc_bench": "ok", "vector_per_edge_iteration": round(vec_iter, 2),
                      "per_iteration_us": {k: round(r["per_iteration_s"] * 1e6, 2) for k, r in summary.items()},
                      "per_iteration_over_bound": {k: round(r["per_iteration_over_bound"], 2) for k, r in summary.items()},
                      "early_stop_us": {k: round(r["early_stop_s"] * 1e6, 1) for k, r in summary.items()},
                      "ldpc_early_stop_over_frame_demod": round(rx.get("ldpc_early_stop_over_frame_demod", float("nan")), 3)}))
    code.close()


if __name__ == "__main__":
    main()
