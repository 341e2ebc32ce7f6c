"""Per-kernel resource usage of a HIP source: python scripts/kres.py csrc/frame_td.hip [filter] [--loops]
(compiles for gfx950 with the package flags and prints VGPRs / scratch / occupancy / LDS).
--loops: also the instruction mix of every loop (label .. backward branch) with at least 100 VALU
instructions (the row loops) of the kernels shown."""
import os
import re
import subprocess
import sys
import tempfile

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-accel-ofdm-ls-mrc_amd")
src = sys.argv[1] if os.path.isabs(sys.argv[1]) else os.path.join(PKG, sys.argv[1])
loops = "--loops" in sys.argv
args = [a for a in sys.argv[2:] if a != "--loops"]
flt = args[0] if args else ""
asm = ""
with tempfile.TemporaryDirectory() as d:
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-fno-slp-vectorize", f"-I{PKG}/build/gen", f"-I{PKG}/csrc", f"-I{PKG}/../include",
                        "-c", src, "-o", os.path.join(d, "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    if loops:
        a = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17",
                            "-fPIC", "-fno-slp-vectorize", f"-I{PKG}/build/gen", f"-I{PKG}/csrc",
                            f"-I{PKG}/../include", "-S", src, "-o", os.path.join(d, "k.s")],
                           capture_output=True, text=True)
        asm = open(os.path.join(d, "k.s")).read() if a.returncode == 0 else ""


def loop_mix(name):
    """(first line, instructions, mix) of every label .. backward-branch region of kernel `name`"""
    m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    if not m:
        return
    lines = [ln.strip() for ln in m.group(1).splitlines()]
    at = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"\.LBB\w+:", ln)}
    last = -1  # end of the last region shown: a region that contains it is an outer loop
    for i, ln in enumerate(lines):
        b = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ln)
        if not b or at.get(b.group(1), i) >= i or at[b.group(1)] <= last:
            continue
        ins = [x.split()[0] for x in lines[at[b.group(1)]:i + 1] if re.match(r"[a-z]", x)]
        grp = {}
        for x in ins:
            k = ("v_fmac_dpp" if "dpp" in x else "v_fma*" if re.match(r"v_fma", x) else
                 re.sub(r"_(f32|b32|e32|e64|u32|i32)", "", x) if x.startswith("v_") else x.split("_")[0] + "_*")
            grp[k] = grp.get(k, 0) + 1
        valu = sum(1 for x in ins if x.startswith("v_"))
        if valu < 100:  # ticket / flag / fill loops
            continue
        last = i
        top = " ".join(f"{k} {v}" for k, v in sorted(grp.items(), key=lambda kv: -kv[1])[:10])
        print(f"    loop {b.group(1)}: {len(ins)} instructions, {valu} VALU | {top}")


cur = None
rows = {}
for ln in r.stderr.splitlines():
    m = re.search(r"remark: (.*?)\s*\[-Rpass", ln)
    if not m:
        continue
    t = m.group(1)
    if t.startswith("Function Name:"):
        cur = t.split(":", 1)[1].strip()
        rows[cur] = {}
    elif cur and ":" in t:
        k, v = t.split(":", 1)
        rows[cur][k.strip()] = v.strip()
for name, d in rows.items():
    dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    short = re.sub(r"\(.*", "", dm).replace("ofdm::", "")
    if flt in short:
        print(f"{short:60s} vgpr {d.get('VGPRs', '?'):>4} scratch {d.get('ScratchSize [bytes/lane]', '?'):>4} "
              f"occ {d.get('Occupancy [waves/SIMD]', '?')} lds {d.get('LDS Size [bytes/block]', '?')}")
        if loops:
            loop_mix(name)
if r.returncode:
    print(r.stderr[-2000:])
