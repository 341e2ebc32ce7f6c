"""The refusals of the frame family of the C ABI, as a table of calls on fake
pointers (test_capi_refusals_cpu.py; the answers are recorded in
golden/capi_refusals.json).

Per entry: its parameters in order, and its checks in the order the entry makes
them, each as one fault -- a name and the arguments that trip it, over the
defaults below, which are a valid call.  CASES is derived from that: every fault
alone, and every two neighbours of the list together (the earlier one must
answer: that pins the order), where the two do not set one argument to two
values; and the empty batch with every pointer null, alone and with each
fault the entry checks before it.  A fault with no arguments is the valid
call itself, which a consumer of a workspace refuses because nothing ever
filled the fake one.

No case may get as far as a HIP call: the fake pointers are never valid device
memory, and the test also runs where a GPU is present.  So a list ends where
the next step would launch: a producer's at the workspace size and alignment,
a consumer's at the empty registry, and the entries without a workspace have
no valid call in the table at all.  `python tests/capi_refusal_cases.py LIB
OUT.json` records the answers of a build; it refuses to write a table in which
a case reached the runtime."""
import ctypes
import json
import sys

ARG, HIP, UNSUPPORTED, DEVICE = -1, -2, -3, -5
Z, X, WS, OUT = 4096, 8192, 1 << 20, 1 << 24

DEFAULTS = dict(
    iq=Z, Y=Z, z=Z, sym=Z, src=Z, F=2, S=5, R=8, C=1024, prefix=0, X=X, ws=WS, ws_bytes="need", out=OUT, stream=0,
    flow=0, spin=-1, scale=1.0, eps=1 << 26, P=OUT, num=OUT, f0=0, count=2, nsym=3, frame=0, Hconj=OUT, Hsqrd=1 << 25,
    taps_post=8, taps_pre=0, mod=2, nv=1 << 27, fmt=0, llr=OUT, phase=1 << 28, timing=1 << 29, cp_len=16, cp_skip=0,
    gamma=1 << 25, max_shift=4, min_ratio=2.0, eps_in=0, eps_out=1 << 26, shift=1 << 27, metric=1 << 28, n=1024)

POINTERS = set("iq Y z sym src X ws out eps P num Hconj Hsqrd nv llr phase timing gamma eps_in eps_out shift "
               "metric".split())
NAN, INF = float("nan"), float("inf")
STATUS = ("status raised", dict(inject=1))
EMPTY = ("empty batch", dict(F=0))
NO_ESTIMATE = ("no estimate", dict())


def frame_args(src, out, prefix="prefix"):
    """check_frame_args: the sample source, the geometry, the prefix (None: the entry has none)."""
    pre = [("prefix<0", {prefix: -1}), ("prefix>C", {prefix: 1025})] if prefix else []
    return [("nframes<0", dict(F=-1)), ("null source", {src: 0}), ("null " + out, {out: 0}), ("S<2", dict(S=1)),
            ("R<1", dict(R=0)), ("C<2", dict(C=1)), ("C>8192", dict(C=8193))] + pre + \
           [("misaligned source", {src: Z + 8})]


GEOMETRY = [("nframes<0", dict(F=-1)), ("S<2", dict(S=1)), ("R<1", dict(R=0)), ("C<2", dict(C=1)),
            ("C>8192", dict(C=8193))]
PILOTS = [("null pilots", dict(X=0))]
CARVE = [("null ws", dict(ws=0)), ("ws too small", dict(ws_bytes="need-1")), ("ws misaligned", dict(ws=WS + 128))]
SCALE = [("scale 0", dict(scale=0.0)), ("scale<0", dict(scale=-1.0)), ("scale nan", dict(scale=NAN)),
         ("scale inf", dict(scale=INF))]
NOT_1024 = [("C not 1024", dict(C=2048))]
NULL_EPS = [("null eps", dict(eps=0))]
MODULATION = [("modulation 3", dict(mod=3)), ("modulation 0", dict(mod=0)), ("modulation 10", dict(mod=10))]
SOFT = MODULATION + GEOMETRY + [
    EMPTY, ("null z", dict(z=0)), ("null nv", dict(nv=0)), ("null ws", dict(ws=0)), ("misaligned z", dict(z=Z + 8)),
    ("misaligned nv", dict(nv=(1 << 27) + 2)), ("frame too long", dict(S=300000, C=8192)),
    ("too many frames", dict(F=1 << 31)), NO_ESTIMATE]
ZB, PB = 2 * 4 * 1023 * 8, 2 * 4 * 4  # the default z / out and phase / timing arrays, in bytes
TRACK = MODULATION + GEOMETRY + [
    EMPTY, ("null z", dict(z=0)), ("null out", dict(out=0)), ("null ws", dict(ws=0)), ("misaligned z", dict(z=Z + 4)),
    ("misaligned out", dict(out=OUT + 4)), ("misaligned phase", dict(phase=(1 << 28) + 2))]
TRACK_OVERLAP = [("out overlaps z", dict(out=Z + 8)), ("out overlaps z's end", dict(out=Z + ZB - 8)),
                 ("phase overlaps z", dict(phase=Z)), ("phase overlaps out", dict(phase=OUT + 8))]
TRACK_END = [NO_ESTIMATE, ("in place", dict(out=Z)), ("out after z", dict(out=Z + ZB)), ("no phase", dict(phase=0))]

# entry -> (parameters in order, faults in the entry's order)
ENTRIES = {
    "ofdm_frame_estimate": ("iq F S R C prefix X ws ws_bytes stream",
                            frame_args("iq", "ws") + PILOTS + [EMPTY] + CARVE[1:]),
    "ofdm_frame_combine": ("iq F S R C prefix ws ws_bytes out stream",
                           [STATUS] + frame_args("iq", "out") + [EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_demod": ("iq F S R C prefix X ws ws_bytes out stream",
                         [STATUS] + frame_args("iq", "out") + PILOTS + [EMPTY] + CARVE),
    "ofdm_frame_demod_ex": ("iq F S R C prefix X ws ws_bytes out flow spin stream",
                            [STATUS] + frame_args("iq", "out") + PILOTS + [("flow 7", dict(flow=7)), EMPTY] + CARVE),
    "ofdm_frame_estimate_sc16": ("iq F S R C prefix scale X ws ws_bytes stream",
                                 frame_args("iq", "ws") + SCALE + NOT_1024 + PILOTS + [EMPTY] + CARVE[1:]),
    "ofdm_frame_combine_sc16": ("iq F S R C prefix scale ws ws_bytes out stream",
                                [STATUS] + frame_args("iq", "out") + SCALE + NOT_1024 + [EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_demod_sc16": ("iq F S R C prefix scale X ws ws_bytes out stream",
                              [STATUS] + frame_args("iq", "out") + SCALE + NOT_1024 + PILOTS + [EMPTY] + CARVE),
    "ofdm_frame_estimate_cfo": ("iq F S R C prefix X ws ws_bytes eps stream",
                                frame_args("iq", "ws") + NULL_EPS + NOT_1024 + PILOTS + [EMPTY] + CARVE[1:]),
    "ofdm_frame_combine_cfo": ("iq F S R C prefix ws ws_bytes out eps stream",
                               [STATUS] + frame_args("iq", "out") + NULL_EPS + NOT_1024 + [EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_demod_cfo": ("iq F S R C prefix X ws ws_bytes out eps stream",
                             [STATUS] + frame_args("iq", "out") + NULL_EPS + NOT_1024 + PILOTS + [EMPTY] + CARVE),
    "ofdm_frame_estimate_freq": ("Y F S R C X ws ws_bytes stream",
                                 frame_args("Y", "ws", None) + PILOTS + [EMPTY] + CARVE[1:]),
    "ofdm_frame_combine_freq": ("Y F S R C ws ws_bytes out stream",
                                frame_args("Y", "out", None) + [EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_demod_freq": ("Y F S R C X ws ws_bytes out stream",
                              frame_args("Y", "out", None) + PILOTS + [EMPTY] + CARVE),
    "ofdm_frame_demod_freq_mfma": ("Y F S R C X ws ws_bytes out stream",
                                   frame_args("Y", "out", None) + [("C not a multiple of 64", dict(C=1000))] + PILOTS +
                                   [EMPTY] + CARVE),
    "ofdm_frame_ls_partial": ("iq F S R C prefix X ws ws_bytes P stream",
                              frame_args("iq", "P") + PILOTS + [EMPTY] + CARVE),
    "ofdm_frame_mrc_partial": ("iq F S R C prefix ws ws_bytes num stream",
                               [STATUS] + frame_args("iq", "num") + [EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_mrc_partial_range": (
        "iq F f0 count S R C prefix ws ws_bytes num stream",
        [STATUS, ("nframes<0", dict(F=-1)), ("f0<0", dict(f0=-1)), ("count<0", dict(count=-1)),
         ("f0 past the end", dict(f0=3, count=0)), ("range past the end", dict(f0=1)), ("empty range", dict(count=0))] +
        frame_args("iq", "num")[1:] + [CARVE[0], NO_ESTIMATE]),
    "ofdm_symbols_demod": (
        "sym nsym R C prefix ws ws_bytes frame out stream",
        [STATUS, ("nsym<0", dict(nsym=-1)), ("nsym too large", dict(nsym=0x7fffffff)), ("null sym", dict(sym=0)),
         ("null out", dict(out=0)), ("R<1", dict(R=0)), ("C not fused", dict(C=1536)), ("C>8192", dict(C=8193)),
         ("prefix<0", dict(prefix=-1)), ("prefix>C", dict(prefix=1025)), ("misaligned source", dict(sym=Z + 8)),
         CARVE[0], NO_ESTIMATE, ("no symbols", dict(nsym=0)), ("frame<0", dict(frame=-1))]),
    "ofdm_frame_export_estimate": (
        "ws ws_bytes F S R C frame Hconj Hsqrd stream",
        [("null Hconj", dict(Hconj=0)), ("no frames", dict(F=0)), ("frame<0", dict(frame=-1)),
         ("frame past the end", dict(frame=2))] + GEOMETRY[1:] + [CARVE[0], NO_ESTIMATE, ("no Hsqrd", dict(Hsqrd=0))]),
    "ofdm_frame_estimate_denoise": (
        "ws ws_bytes F S R C taps_post taps_pre stream",
        GEOMETRY + [("taps_post<1", dict(taps_post=0)), ("taps_pre<0", dict(taps_pre=-1)),
                    ("taps past C", dict(taps_post=1000, taps_pre=100)), EMPTY, CARVE[0], NO_ESTIMATE]),
    "ofdm_frame_noise_estimate": ("z F S R C ws ws_bytes mod nv stream", SOFT),
    "ofdm_frame_soft_demap": (
        "z F S R C ws ws_bytes mod nv fmt scale llr stream",
        [("llr_format 2", dict(fmt=2)), ("i8 scale 0", dict(fmt=1, scale=0.0)), ("i8 scale nan", dict(fmt=1, scale=NAN)),
         ("i8 scale inf", dict(fmt=1, scale=INF))] + SOFT + [("i8", dict(fmt=1)), ("f32 scale 0", dict(scale=0.0)),
                                                            ("null llr", dict(llr=0))]),
    "ofdm_frame_phase_track": ("z F S R C ws ws_bytes mod out phase stream", TRACK + TRACK_OVERLAP + TRACK_END),
    "ofdm_frame_timing_track": (
        "z F S R C ws ws_bytes mod out phase timing stream",
        TRACK + [("misaligned timing", dict(timing=(1 << 29) + 2))] + TRACK_OVERLAP +
        [("timing overlaps z", dict(timing=Z + ZB - 4)), ("timing overlaps out", dict(timing=OUT - 4)),
         ("timing overlaps phase", dict(timing=(1 << 28) + PB - 4))] + TRACK_END +
        [("no timing", dict(timing=0)), ("timing after phase", dict(timing=(1 << 28) + PB))]),
    "ofdm_frame_cfo_estimate": (
        "iq F S R C cp_len cp_skip gamma eps stream",
        frame_args("iq", "eps", "cp_len") + [("cp_len<1", dict(cp_len=0)), ("cp_skip<0", dict(cp_skip=-1)),
                                             ("cp_skip past cp_len", dict(cp_skip=16)), EMPTY]),
    "ofdm_frame_cfo_derotate": (
        "src out F S R C cp_len eps stream",
        frame_args("src", "out", "cp_len") + NULL_EPS + [("misaligned out", dict(out=OUT + 8)), EMPTY,
                                                         ("out overlaps in", dict(out=Z + 16)),
                                                         ("out overlaps in from below", dict(src=OUT, out=OUT - 16))]),
    "ofdm_frame_cfo_acquire": (
        "iq F S R C cp_len X max_shift min_ratio eps_in eps_out shift metric stream",
        GEOMETRY[:3] + [("cp_len<0", dict(cp_len=-1)), ("cp_len>C", dict(cp_len=1025)), ("null source", dict(iq=0)),
                        ("null pilots", dict(X=0)), ("null eps_out", dict(eps_out=0)),
                        ("misaligned source", dict(iq=Z + 8)), ("max_shift 0", dict(max_shift=0)),
                        ("max_shift 65", dict(max_shift=65)), ("min_ratio<1", dict(min_ratio=0.5)),
                        ("min_ratio nan", dict(min_ratio=NAN)), ("min_ratio inf", dict(min_ratio=INF)),
                        ("eps_out overlaps metric", dict(metric=(1 << 26) + 4)),
                        ("eps_out overlaps shift", dict(shift=(1 << 26) - 4)), ("C<8", dict(C=6, cp_len=0)),
                        ("C>8192", dict(C=8193)), ("search wider than C", dict(C=8, cp_len=0)), EMPTY]),
    "ofdm_iq_convert_sc16": (
        "src n scale out stream",
        [("n<0", dict(n=-1))] + SCALE + [("empty batch", dict(n=0)), ("null source", dict(src=0)),
                                         ("null out", dict(out=0)), ("misaligned source", dict(src=Z + 8)),
                                         ("misaligned out", dict(out=OUT + 8))]),
}


def _cases():
    out = {}
    for entry, (_, faults) in ENTRIES.items():
        for i, (name, kw) in enumerate(faults):
            out[f"{entry}: {name}"] = (entry, kw)
            if i + 1 < len(faults):
                nname, nkw = faults[i + 1]
                if kw and nkw and kw != nkw and all(kw[k] == nkw[k] for k in kw.keys() & nkw.keys()):
                    out[f"{entry}: {name} + {nname}"] = (entry, {**kw, **nkw})
        # an empty batch may come with every pointer null (an empty tensor's address is 0): the no-op itself, and
        # every check the entry makes before it, on null pointers
        empty = [i for i, (name, _) in enumerate(faults) if name in ("empty batch", "empty range")]
        if empty:
            nulls = {p: 0 for p in ENTRIES[entry][0].split() if p in POINTERS}
            base = {**nulls, **faults[empty[0]][1]}
            out[f"{entry}: empty batch, every pointer null"] = (entry, base)
            for name, kw in faults[:empty[0]]:
                if name != "status raised":
                    out[f"{entry}: empty batch, every pointer null + {name}"] = (entry, {**base, **kw})
        if faults[0] is not STATUS:  # no work tickets: a raised status is left for the entries that have them
            out[f"{entry}: status raised + {faults[0][0]}"] = (entry, dict(inject=1, **faults[0][1]))
    return out


CASES = _cases()  # id -> (entry, arguments over DEFAULTS; `inject`: device status bits raised before the call)


def is_empty(case_id):
    """The case asks for no work: the only kind that may answer OFDM_OK."""
    kw = CASES[case_id][1]
    return any(kw.get(k) == 0 for k in ("F", "count", "n"))


def run(L, case_id):
    """One call: {"rc", "error" (None after OFDM_OK), and for a case that raises the status first,
    "status_after": what ofdm_device_status() answers then (0: the call consumed it)}."""
    entry, kw = CASES[case_id]
    a = {**DEFAULTS, **kw}
    need = L.ofdm_frame_workspace_bytes(a["F"], a["S"], a["R"], a["C"])
    a["ws_bytes"] = {"need": need, "need-1": max(need - 1, 0)}.get(a["ws_bytes"], a["ws_bytes"])
    fn = getattr(L, entry)
    args = [(a[p] or None) if t is ctypes.c_void_p else a[p] for p, t in zip(ENTRIES[entry][0].split(), fn.argtypes)]
    assert len(args) == len(fn.argtypes), entry
    L.ofdm_workspace_release(ctypes.c_void_p(WS))
    if "inject" in kw:
        L.ofdm_device_status_inject(kw["inject"])
    rc = fn(*args)
    got = {"rc": rc, "error": L.ofdm_last_error().decode() if rc else None}
    if "inject" in kw:
        got["status_after"] = L.ofdm_device_status()
    return got


def check_recordable(case_id, got):
    """The table's hard rule: a refusal, or OFDM_OK for a case that asks for no work."""
    assert got["rc"] in (ARG, UNSUPPORTED, DEVICE) or (got["rc"] == 0 and is_empty(case_id)), \
        f"{case_id}: rc {got['rc']} ({got['error']}): the case reached the runtime, take it out of the table"


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "gpu-accel-ofdm-ls-mrc_amd"))
    import ofdm_lsmrc
    lib = ofdm_lsmrc.load_library(sys.argv[1])
    lib.ofdm_device_status()
    table = {}
    for cid in CASES:
        table[cid] = run(lib, cid)
        check_recordable(cid, table[cid])
    with open(sys.argv[2], "w") as fp:
        json.dump(table, fp, indent=0, sort_keys=True)
        fp.write("\n")
    print(f"{len(table)} cases recorded from {sys.argv[1]}")
