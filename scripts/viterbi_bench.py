"""The Viterbi decoder (ofdm_viterbi_decode) timed with HIP events beside the
receiver and the demapper whose LLRs it consumes, in the same process
(DESIGN.md section 7q).

  python scripts/viterbi_bench.py [--json OUT] [--isa-only]

Decoder shapes, for int8 and for f32 LLRs: 125 000 codewords of L = 1017 at
rate 1/2, terminated (2046 LLRs each: one headline step's QPSK LLRs, F = 1250,
S = 101, C = 1024), 10 000 such codewords, one codeword alone at L = 1017 and
one at L = 65 530 (one wave: its time over the steps is the serial time per
trellis step).  The LLRs are the all-zero codeword as BPSK +1 plus Gaussian
noise of std 0.7, LLR = 2 x / sigma^2, int8 at scale 8 (the decoder has no
data-dependent branch; the decoded bits are checked to be zero).  Then
frame_demod and frame_soft_demap (int8) at the headline shape, R = 64.
HIP-event times, medians with p10-p90 after warm-up.

Beside the times: the vector instructions (VALU and LDS / memory) of the
unpunctured rate-1/2 kernel's step loop, counted from the disassembly of the
code object inside the library (llvm-objdump), split into those every step
executes and those under a forward branch inside the loop (the store of 64
decision words, once per 64 steps), and the time the per-step count implies at
one wave-instruction per 4 cycles per wave and at most one per 2 cycles per SIMD
(MI355X: 1024 SIMDs), at the clock given by --ghz."""
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
LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "k_viterbiILi2ELb0E"


def step_loop_instructions(lib):
    """(vector instructions every step executes, those under a forward branch, scalar ones, all per step,
    and the steps the loop body holds) of KERNEL's step loop: the innermost loop around its first
    ds_bpermute_b32, two of which make a step."""
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
            if KERNEL in dis:
                break
        else:
            raise RuntimeError(f"{KERNEL} not found in {lib}")
    body = dis.split(KERNEL, 1)[1]
    body = re.split(r"\n[0-9a-f]+ <_Z", body, 1)[0]  # up to the next function
    lines = []  # (label or None, mnemonic or None, branch target or None)
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
    first = next(i for i, (_, op, _) in enumerate(lines) if op == "ds_bpermute_b32")
    labels = {lab: i for i, (lab, _, _) in enumerate(lines) if lab}
    # the innermost loop: the nearest back edge after `first` whose target lies at or before it
    end = next(i for i in range(first, len(lines))
               if lines[i][1] and lines[i][1].startswith(("s_branch", "s_cbranch")) and lines[i][2] in labels
               and labels[lines[i][2]] <= first)
    head = labels[lines[end][2]]
    vec = lambda op: op.startswith(("v_", "ds_", "global_", "buffer_", "flat_"))
    always = cond = scalar = 0
    steps = sum(op == "ds_bpermute_b32" for _, op, _ in lines[head:end + 1]) // 2  # the loop may hold 64 unrolled steps
    skip_to = -1
    for i in range(head, end + 1):
        lab, op, tgt = lines[i]
        if op is None:
            continue
        if i < skip_to:
            cond += vec(op)
            continue
        always += vec(op)
        scalar += not vec(op)
        if op.startswith("s_cbranch") and tgt in labels and i < labels[tgt] <= end:
            skip_to = labels[tgt]  # a forward branch inside the loop: what it jumps over is not every step's
    return always / steps, cond / steps, scalar / steps, steps


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
    ap.add_argument("--no-receiver", action="store_true", help="skip frame_demod / frame_soft_demap at the headline shape")
    ap.add_argument("--isa-only", action="store_true", help="only count the step loop's instructions (no GPU needed)")
    ap.add_argument("--json", default=None, help="JSON lines, one per measurement")
    a = ap.parse_args()

    import ofdm_lsmrc as ofdm
    always, cond, scalar, steps = step_loop_instructions(ofdm.LIB_PATH)
    print(f"{KERNEL} step loop ({steps} steps per iteration): {always:.2f} vector instructions per step, {cond:.2f} more "
          f"under a branch, {scalar:.2f} scalar instructions per step")
    rows = [{"mode": "isa", "kernel": KERNEL, "steps_per_iteration": steps, "vector_per_step": always,
             "vector_per_step_conditional": cond, "scalar_per_step": scalar}]
    if a.isa_only:
        print(json.dumps({"viterbi_bench": "isa", "steps_per_iteration": steps, "vector_per_step": round(always, 2),
                          "vector_per_step_conditional": round(cond, 2), "scalar_per_step": round(scalar, 2)}))
        return

    import torch
    if not torch.cuda.is_available():
        sys.exit("viterbi_bench: no GPU")
    dev = torch.device("cuda:0")
    code = ofdm.ConvCode.k7_rate_half()
    sigma, scale = 0.7, 8.0
    per_step = always + cond
    summary = {}
    for ncw, L, reps in ((125000, 1017, a.reps), (10000, 1017, a.reps), (1, 1017, 5 * a.reps), (1, 65530, a.reps)):
        n_rx, T = ofdm.conv_coded_len(code, L), L + 6
        g = torch.Generator(device=dev)
        g.manual_seed(ncw + L)
        llr = (2.0 / sigma ** 2) * (1.0 + sigma * torch.randn((ncw, n_rx), generator=g, device=dev, dtype=torch.float32))
        q = torch.clamp(torch.round(llr * scale), -127, 127).to(torch.int8)
        raw_wrong = int((q < 0).sum().item())
        ws_bytes = ofdm.viterbi_workspace_bytes(code, L, ncw)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        bits = torch.empty((ncw, (L + 7) // 8), dtype=torch.uint8, device=dev)
        metric = torch.empty(ncw, dtype=torch.int32, device=dev)
        for name, src in (("i8", q), ("f32", llr)):
            fn = lambda: ofdm.viterbi_decode(src, code, L, scale=scale, out=bits, metric=metric, ws=ws)
            t, p10, p90 = timed_median(torch, fn, a.warmup, reps)
            wrong = int(torch.count_nonzero(bits).item())
            # one wave issues a vector instruction per 4 cycles; a SIMD (1024 of them) at most one per 2
            bound = T * per_step * max(4.0, 2.0 * ncw / 1024.0) / (a.ghz * 1e9)
            row = {"mode": "viterbi", "format": name, "ncw": ncw, "L": L, "T": T, "n_rx": n_rx, "reps": reps, "time_s": t,
                   "p10_s": p10, "p90_s": p90, "info_bits_per_s": ncw * L / t, "us_per_step": t / T * 1e6,
                   "issue_bound_s": bound, "time_over_issue_bound": t / bound, "workspace_bytes": ws_bytes,
                   "raw_wrong_signs": raw_wrong, "decoded_nonzero_bytes": wrong}
            rows.append(row)
            summary[f"{name}_{ncw}x{L}"] = row
            print(f"{name:>3} {ncw:6d} x L={L:5d}: {t * 1e6:10.1f} us (p10 {p10 * 1e6:.1f}, p90 {p90 * 1e6:.1f})  "
                  f"{ncw * L / t / 1e9:7.3f} Gbit/s of information, {t / T * 1e6:.4f} us per step; issue bound "
                  f"{bound * 1e6:.1f} us -> x{t / bound:.2f}; {raw_wrong} raw signs wrong, {wrong} decoded bytes non-zero")
        del llr, q, ws, bits, metric
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
        # the demapper's own bytes through the decoder (random QPSK data, not codewords: the time is what counts)
        bits = torch.empty((125000, 128), dtype=torch.uint8, device=dev)
        metric = torch.empty(125000, dtype=torch.int32, device=dev)
        t_chain = timed_median(torch, lambda: ofdm.viterbi_decode(llr8.reshape(125000, 2046), code, 1017, out=bits,
                                                                  metric=metric), a.warmup, a.reps)
        head = summary["i8_125000x1017"]["time_s"]
        rx = {"mode": "receiver", "frames": F, "S": S, "R": R, "C": C, "frame_demod_s": t_demod[0],
              "frame_soft_demap_i8_s": t_demap[0], "viterbi_on_demapper_bytes_s": t_chain[0],
              "viterbi_over_frame_demod": head / t_demod[0], "viterbi_over_soft_demap": head / t_demap[0]}
        rows.append(rx)
        print(f"headline shape R={R} x {F} frames: frame_demod {t_demod[0] * 1e6:.1f} us, frame_soft_demap (i8) "
              f"{t_demap[0] * 1e6:.1f} us, the decoder on the demapper's bytes {t_chain[0] * 1e6:.1f} us; decoder / frame_demod "
              f"x{head / t_demod[0]:.3f}, decoder / soft_demap x{head / t_demap[0]:.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            for r in rows:
                fp.write(json.dumps(r) + "\n")
    print(json.dumps({"viterbi_bench": "ok", "vector_per_step": round(per_step, 2),
                      "time_us": {k: round(r["time_s"] * 1e6, 1) for k, r in summary.items()},
                      "info_gbit_per_s": {k: round(r["info_bits_per_s"] / 1e9, 3) for k, r in summary.items()},
                      "us_per_step_alone": {k: round(r["us_per_step"], 4) for k, r in summary.items() if r["ncw"] == 1},
                      "time_over_issue_bound": {k: round(r["time_over_issue_bound"], 2) for k, r in summary.items()},
                      "viterbi_over_frame_demod": round(rx.get("viterbi_over_frame_demod", float("nan")), 3),
                      "viterbi_over_soft_demap": round(rx.get("viterbi_over_soft_demap", float("nan")), 2)}))


if __name__ == "__main__":
    main()
