"""Compare the gfx950 instruction streams of two builds of one HIP source, kernel by kernel:
    hipcc <the package's HIPFLAGS> --cuda-device-only -S csrc/frame_td.hip -o old.s     (at the old commit)
    hipcc ...                                                            -o new.s     (at the new one)
    python scripts/isa_diff.py old.s new.s [OLD=NEW ...]
Kernels are paired by demangled name without arguments and namespaces; an old k<a, b> also pairs with
the one new k<a, b, ...> still unpaired (a trailing template parameter added); OLD=NEW pairs two names
given in full.  Labels (.LBB<n>_) and symbol names are normalised, directives and comments dropped.  Per pair: the resource figures of both sides, whether the mnemonic sequences are equal,
and every line whose operands differ -- marked `swap` where only the sources of a commutative VALU
instruction changed places.  Nothing but normalise and diff: nothing is compiled or run."""
import re
import subprocess
import sys

COMM = re.compile(r"v_(pk_)?(add|mul|and|or|xor|max|min)_")   # all sources commute
FMA = re.compile(r"v_(pk_)?(fma|fmac)_")                      # the two factors commute
RES = ("TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy")


def kernels(path):
    """{short demangled name: (instructions, resources)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)^; COMPUTE_PGM_RSRC2", text, re.S | re.M):
        sym, body, tail = m.groups()
        if ".amdhsa_kernel " + sym not in text:
            continue
        dm = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void ", "", re.sub(r"\(.*", "", dm)).replace("HIP_vector_type<float, 2u>", "float2")
        name = re.sub(r"\w+::", "", name).replace(" >", ">")
        ins = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") and not ln.startswith(".LBB") or ln.endswith(":"):
                continue
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
            ln = re.sub(r"_Z\w+", "SYM", ln)
            ins.append(ln)
        res = {k: re.search(r";\s*" + k + r":\s*(\d+)", tail) for k in RES}
        out[name] = (ins, {k: v.group(1) if v else "?" for k, v in res.items()})
    return out


def ops(ln):
    p = ln.split(None, 1)
    return p[0], [x.strip() for x in p[1].split(",")] if len(p) > 1 else []


def same_but_swapped(a, b):
    (ma, oa), (mb, ob) = ops(a), ops(b)
    if ma != mb or len(oa) != len(ob) or not oa or oa[0] != ob[0]:
        return False
    if COMM.match(ma):
        return sorted(oa[1:]) == sorted(ob[1:])
    if FMA.match(ma) and len(oa) >= 3:
        return sorted(oa[1:3]) == sorted(ob[1:3]) and oa[3:] == ob[3:]
    return False


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
pairs = [(k, k) for k in old if k in new]
for arg in sys.argv[3:]:
    o, n = arg.split("=")
    pairs.append((o, n))
for a in old:
    ext = [b for b in new if a.endswith(">") and b.startswith(a[:-1] + ", ") and b not in [p[1] for p in pairs]]
    if a not in [p[0] for p in pairs] and len(ext) == 1:
        pairs.append((a, ext[0]))
for k in old:
    if k not in [p[0] for p in pairs]:
        print(f"only in {sys.argv[1]}: {k}")
for k in new:
    if k not in [p[1] for p in pairs]:
        print(f"only in {sys.argv[2]}: {k}")
for a, b in pairs:
    (ia, ra), (ib, rb) = old[a], new[b]
    print(f"{a}" + (f"  ->  {b}" if a != b else ""))
    print("    " + "  ".join(f"{k} {ra[k]}" + ("" if ra[k] == rb[k] else f" -> {rb[k]}") for k in RES))
    ma, mb = [x.split()[0] for x in ia], [x.split()[0] for x in ib]
    print(f"    instructions {len(ia)}" + ("" if len(ia) == len(ib) else f" -> {len(ib)}") +
          ("; mnemonic sequence identical" if ma == mb else "; mnemonic sequences DIFFER"))
    if ma != mb:
        continue
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(ia, ib)) if x != y]
    swaps = [d for d in diff if same_but_swapped(d[1], d[2])]
    print(f"    operands: {len(diff)} lines differ, {len(swaps)} of them commutative swaps")
    for i, x, y in diff:
        print(f"      {i:6d} {'swap ' if (i, x, y) in swaps else 'OTHER'} {x}   |   {y}")
