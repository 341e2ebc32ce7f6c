"""Where the kernels write and what they read: every device entry of
include/ofdm_lsmrc.h with every caller-supplied device buffer between guard
bands (guard_cases.py), the workspace at exactly ofdm_frame_workspace_bytes.

One table row per (entry or chain of entries, shape).  A row runs its chain
on the same host inputs
  plain     as the suite calls the entries today (fresh tensors);
  guarded   every input, output and workspace in an arena of its own;
  poisoned  (time-domain rows) guarded, the cyclic prefix of every IQ row
            overwritten with NaN (sc16: +-32767);
  aligned   (rows with a stated alignment) guarded, each such buffer at exactly
            that alignment: address mod 2*align == align;
and asserts
  (a) the bands around every buffer are intact, outputs and workspaces first;
  (b) every output word was written, but for the positions the header
      documents as never written, which still hold the prefill;
  (c) every input is unmodified bit for bit, outputs that a later entry of the
      chain only reads and `const` workspaces included (the 4 KiB work-ticket
      area aside where a ticketed entry ran: the header says they write it);
  (d) guarded outputs == plain outputs, bit for bit;
  (e) poisoned outputs == guarded outputs, and finite;
  (f) the plain outputs against the reference the suite has for the entry, at
      the bound it has there (helpers.parity at RTOL unless said otherwise);
  aligned: (a), (b), (f) -- not (d): a kernel choice may depend on alignment.
Every call runs once; nothing is retried.  Shapes: the smallest that reach
each kernel and its tail path."""
import numpy as np
import pytest

import guard_cases as gc
from helpers import RTOL, parity

pytestmark = pytest.mark.gpu

C64, F32, I8, I64 = "complex64", "float32", "int8", "int64"
FUSED = (1024, 2048, 4096)

# Entries that touch no caller-supplied device memory: name (a trailing * is a
# prefix) -> why.  test_guard_cpu.py holds the set this dict may contain.
EXCLUDED = {
    "ofdm_version": "returns a constant",
    "ofdm_last_error": "returns the calling thread's host string",
    "ofdm_pilot_rotate": "host arrays only",
    "ofdm_read_pilots": "host file to host array",
    "ofdm_frame_workspace_bytes": "arithmetic on the host",
    "ofdm_device_status*": "reads or sets the library's own status word",
    "ofdm_workspace_release": "host-side registry only",
    "ofdm_host_register": "page-locks a host range, no device access",
    "ofdm_host_unregister": "releases a host range, no device access",
    "ofdm_pipeline_create*": "allocates the pipeline's own device memory",
    "ofdm_pipeline_destroy": "frees the pipeline's own device memory",
    "ofdm_pipeline_sync": "waits on the pipeline's own streams",
    "ofdm_pipeline_set_*": "sets host-side state of the pipeline",
}

TABLE = []


class Row:
    def __init__(self, id, entries, setup, run, check, prefix=False, aligned=True):
        self.id, self.entries, self.setup, self.run, self.check = id, tuple(entries), setup, run, check
        self.prefix, self.aligned = prefix, aligned
        TABLE.append(self)


# --------------------------------------------------------------- the context

class Env:
    def __init__(self, ofdm, dev, oracle):
        self.ofdm, self.dev, self.oracle = ofdm, dev, oracle


class Ctx:
    """What a row's chain allocates through: plain tensors or guarded arenas."""

    def __init__(self, env, mode):
        self.env, self.ofdm, self.dev, self.mode = env, env.ofdm, env.dev, mode
        self.guarded = mode != "plain"
        self.bufs, self.tensors, self.outs, self.never, self.frozen, self.geom = {}, {}, [], {}, {}, {}
        self.bin0 = None

    NATURAL = {"complex64": 8, "float32": 4, "int32": 4, "int64": 8}

    def _offset(self, align, dtype):
        """aligned mode: the stated alignment (align=), else the element's natural one, and no more"""
        if self.mode != "aligned":
            return 0
        return align if align is not None else self.NATURAL[np.dtype(dtype).name]

    def inp(self, name, a, prefix=None, align=None):
        import torch
        a = np.ascontiguousarray(a)
        if self.mode == "poisoned" and prefix:
            a = gc.poison_prefix(a, prefix)
        if self.guarded:
            g = self.bufs[name] = gc.guarded(a.shape, a.dtype, self.dev, offset=self._offset(align, a.dtype), fill=a)
            t = g.view
        else:
            t = torch.from_numpy(a.copy()).to(self.dev)
        self.tensors[name] = t
        return t

    def out(self, name, shape, dtype, never=None, align=None, fill=None):
        """An output; never: bool mask of the elements the header documents as
        never written; fill: initial contents of a buffer the entry updates."""
        import torch
        shape = tuple(int(s) for s in shape)
        if self.guarded:
            g = self.bufs[name] = gc.guarded(shape, dtype, self.dev, offset=self._offset(align, dtype))
            t = g.view
        else:
            t = torch.empty(shape, dtype=gc.torch_dtype(dtype), device=self.dev)
        if fill is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(fill, np.dtype(dtype))).to(self.dev))
        self.tensors[name] = t
        self.outs.append(name)
        if never is not None:
            self.never[name] = np.asarray(never, bool)
        return t

    def ws(self, name, F, S, R, C):
        self.geom[name] = (F, S, R, C)
        if self.guarded:
            g = self.bufs[name] = gc.guarded_workspace(F, S, R, C, self.dev, offset=256 if self.mode == "aligned" else 0)
            t = g.view
        else:
            t = self.ofdm.workspace(F, S, R, C, self.dev)
        self.tensors[name] = t
        return t

    def freeze(self, name, tickets=False):
        """The buffer is only read from here on (tickets: but for the workspace's work-ticket area)."""
        import torch
        if self.guarded:
            torch.cuda.synchronize()
            g = self.bufs[name].freeze()
            self.frozen[name] = g.ticket_mask() if tickets else None
        return self.tensors[name]

    def poke_bin0(self, name):
        """Put the prefill into bin 0 of every Hc row and P[f][0] of a workspace
        holding an estimate: ofdm_frame_estimate_denoise neither reads nor
        writes them (position 0 in every layout)."""
        import torch
        t = self.tensors[name]
        F, S, R, C = self.geom[name]
        nh = (F * R * C * 8 + 255) // 256 * 256
        t[:F * R * C * 8].view(torch.int32).view(F * R, C, 2)[:, 0, :] = gc.FILL_WORD
        t[nh:nh + F * C * 4].view(torch.int32).view(F, C)[:, 0] = gc.FILL_WORD
        self.bin0 = name

    def host(self, name):
        import torch
        torch.cuda.synchronize()
        return self.tensors[name].detach().cpu().numpy()

    def results(self):
        return {n: self.host(n) for n in self.outs}

    def close(self):
        for g in self.bufs.values():
            if isinstance(g, gc.GuardedWorkspace):
                g.release()


def P(t):
    import ofdm_lsmrc as ofdm
    return None if t is None else ofdm._dptr(t)


def call(fn, *args):
    """ofdm.lib().<fn>(*args, stream) with the binding's error check."""
    import ofdm_lsmrc as ofdm
    ofdm._check(getattr(ofdm.lib(), fn)(*args, ofdm._stream(None)), fn)


# ------------------------------------------------------------------ helpers

def qpsk(K, seed=7):
    rng = np.random.default_rng(seed)
    a = np.float32(0.70710678)
    return (rng.choice([-a, a], K) + 1j * rng.choice([-a, a], K)).astype(np.complex64)


def crandn(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def out_src(K):
    k = np.arange(K)
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return np.where(k < n2, k + h, np.where(k < n2 + h, k - n2, k))


def words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def synth(env, F, S, R, C, X, prefix, seed, freq=False):
    import torch
    iq = env.ofdm.synth_frames(F, S, R, C, torch.from_numpy(X).to(env.dev), prefix=prefix, seed=seed, noise_std=0.05,
                               freq_domain=freq)
    torch.cuda.synchronize()
    return iq.cpu().numpy()


# ------------------------------------------------- time-domain frame chains

def td_row(F, S, R, C, p, kind="fp32", flow=None, tag=""):
    K = C - 1
    tp, tq = max(1, min(12, C // 4)), min(4, C // 8)
    entries = {"fp32": ["ofdm_frame_demod" if flow is None else "ofdm_frame_demod_ex", "ofdm_frame_estimate",
                        "ofdm_frame_combine", "ofdm_frame_ls_partial", "ofdm_frame_mrc_partial",
                        "ofdm_frame_mrc_partial_range", "ofdm_mrc_finalize", "ofdm_frame_export_estimate",
                        "ofdm_frame_estimate_denoise"] + (["ofdm_symbols_demod"] if C in FUSED else []),
               "sc16": ["ofdm_frame_demod_sc16", "ofdm_frame_estimate_sc16", "ofdm_frame_combine_sc16",
                        "ofdm_frame_export_estimate", "ofdm_frame_estimate_denoise"],
               "cfo": ["ofdm_frame_demod_cfo", "ofdm_frame_estimate_cfo", "ofdm_frame_combine_cfo",
                       "ofdm_frame_export_estimate", "ofdm_frame_estimate_denoise"]}[kind]

    def setup(env):
        if kind == "cfo":
            import cfo_cases as cc
            c = cc.frames(F, S, R, C, p, None, seed=F + R)
            iq, X, eps = np.array(c["y"]), np.array(c["X"]), np.array(c["eps"], np.float32)
            eff = cc.derotate_ref(iq, eps, p)
            return dict(iq=iq, X=X, eps=eps, eff=eff)
        X = qpsk(K, seed=C + R)
        iq = synth(env, F, S, R, C, X, p, seed=99 + C)
        if kind == "sc16":
            from test_sc16_gpu import dequantise, quantise
            q = quantise(iq)
            return dict(iq=q, X=X, eff=dequantise(q, env.ofdm.SC16_SCALE))
        return dict(iq=iq, X=X, eff=iq)

    def run(cx, d):
        o = cx.ofdm
        iq, X = cx.inp("iq", d["iq"], prefix=p, align=16), cx.inp("X", d["X"])
        eps = cx.inp("eps", d["eps"]) if kind == "cfo" else None
        shape = (F, S - 1, K)
        ws0, out = cx.ws("ws0", F, S, R, C), cx.out("demod", shape, C64)
        ws1, comb = cx.ws("ws1", F, S, R, C), cx.out("combine", shape, C64)
        if kind == "fp32":
            o.frame_demod(iq, X, p, ws=ws0, out=out, flow=flow)
            o.frame_estimate(iq, X, p, ws1)
            o.frame_combine(iq, p, ws1, comb)
        elif kind == "sc16":
            o.frame_demod_sc16(iq, X, p, ws=ws0, out=out)
            o.frame_estimate_sc16(iq, X, p, ws1)
            o.frame_combine_sc16(iq, p, ws1, comb)
        else:
            o.frame_demod_cfo(iq, X, p, eps, ws=ws0, out=out)
            o.frame_estimate_cfo(iq, X, p, ws1, eps)
            o.frame_combine_cfo(iq, p, ws1, comb, eps)
        cx.freeze("ws1", tickets=True)  # from here on ws1 is a const argument
        if kind == "fp32" and C in FUSED:
            sym = cx.inp("sym", d["iq"][F - 1, 1:], prefix=p, align=16)
            o.symbols_demod(sym, ws1, p, frame=F - 1, out=cx.out("symdemod", (S - 1, K), C64))
        H, Pq = cx.out("Hconj", (R, K), C64), cx.out("Hsqrd", (K,), F32)
        call("ofdm_frame_export_estimate", P(ws1), ws1.numel(), F, S, R, C, F - 1, P(H), P(Pq))
        if kind == "fp32":
            ws2 = cx.ws("ws2", F, S, R, C)
            Pp, num = cx.out("Ppart", (F, K), F32), cx.out("num", shape, C64)
            o.frame_ls_partial(iq, X, p, ws=ws2, P=Pp)
            o.frame_mrc_partial(iq, ws2, p, num=num)
            o.frame_mrc_partial_range(iq, ws2, p, F - 1, 1, num=cx.out("num_range", (1, S - 1, K), C64))
            cx.freeze("Ppart"), cx.freeze("num")
            o.mrc_finalize(num.view(-1), 0, S - 1, K, Pp, cx.out("final", shape, C64))
        # the denoiser, on a workspace of its own: bin 0 of every row is neither read nor written
        ws3 = cx.ws("ws3", F, S, R, C)
        if kind == "fp32":
            o.frame_estimate(iq, X, p, ws3)
        elif kind == "sc16":
            o.frame_estimate_sc16(iq, X, p, ws3)
        else:
            o.frame_estimate_cfo(iq, X, p, ws3, eps)
        H0, P0 = cx.out("Hconj_raw", (R, K), C64), cx.out("Hsqrd_raw", (K,), F32)
        call("ofdm_frame_export_estimate", P(ws3), ws3.numel(), F, S, R, C, 0, P(H0), P(P0))
        cx.poke_bin0("ws3")
        o.frame_estimate_denoise(ws3, F, S, R, C, tp, tq)
        H1, P1 = cx.out("Hconj_dn", (R, K), C64), cx.out("Hsqrd_dn", (K,), F32)
        call("ofdm_frame_export_estimate", P(ws3), ws3.numel(), F, S, R, C, 0, P(H1), P(P1))

    def check(env, d, o):
        from test_denoise_gpu import ref_denoise
        ref = env.oracle.frames_demod(d["eff"], d["X"], p)
        parity(o["demod"], ref)
        parity(o["combine"], ref)
        if "symdemod" in o:
            parity(o["symdemod"], o["combine"][F - 1], rtol=1e-6)  # test_symbols_demod_matches_frame_combine's bound
        Href, Pref = env.oracle.ls(env.oracle.fft_rows(d["eff"][F - 1, 0, :, p:]), d["X"])
        parity(o["Hconj"], Href)
        parity(o["Hsqrd"], Pref)
        if kind == "fp32":
            parity(o["final"], ref)
            parity(o["num_range"], o["num"][F - 1:], rtol=1e-6)
            for f in (0, F - 1):
                parity(o["Ppart"][f], env.oracle.ls(env.oracle.fft_rows(d["eff"][f, 0, :, p:]), d["X"])[1])
        if tp + tq == C:
            Hd, Pd = o["Hconj_raw"], o["Hsqrd_raw"]
        else:
            Hd, Pd = ref_denoise(o["Hconj_raw"], C, tp, tq)
        parity(o["Hconj_dn"], Hd)
        parity(o["Hsqrd_dn"], Pd)

    Row(f"td_{kind}_{F}x{S}x{R}x{C}p{p}{tag}", entries, setup, run, check, prefix=True)


td_row(2, 4, 3, 1024, 7, tag="_auto")
td_row(2, 4, 3, 1024, 7, flow=1, tag="_two_launch")
td_row(1, 10, 2, 1024, 0)                    # 9 data symbols: a workgroup of 8 and one of 1
td_row(2, 4, 3, 1024, 7, kind="sc16")        # rows of 1031 samples: 4-byte aligned
td_row(2, 4, 3, 1024, 7, kind="cfo")
td_row(2, 3, 3, 2048, 9)
td_row(1, 10, 3, 4096, 1)
td_row(2, 7, 2, 4096, 0)
for _C in (128, 256, 512, 1536, 3072, 6144):  # the FFT512 family
    td_row(2, 3, 2, _C, 7)
for _C in (6, 12, 600, 1021, 3000, 5000, 8192):  # the generic path: rows per LDS group, prime, each capacity
    td_row(2, 3, 2, _C, 3)


# ------------------------------------------- frequency-domain frame chains

def fd_row(F, S, R, C, mfma=False, plain=True):
    K = C - 1
    entries = (["ofdm_frame_demod_freq", "ofdm_frame_estimate_freq", "ofdm_frame_combine_freq"] if plain else []) + (
        ["ofdm_frame_demod_freq_mfma"] if mfma else [])

    def setup(env):
        X = qpsk(K, seed=C)
        return dict(Y=synth(env, F, S, R, C, X, 0, seed=5 + C, freq=True), X=X)

    def run(cx, d):
        o = cx.ofdm
        Y, X = cx.inp("Y", d["Y"], align=16), cx.inp("X", d["X"])
        shape = (F, S - 1, K)
        if plain:
            o.frame_demod_freq(Y, X, ws=cx.ws("ws0", F, S, R, C), out=cx.out("demod", shape, C64))
            ws1 = cx.ws("ws1", F, S, R, C)
            o.frame_estimate_freq(Y, X, ws1)
            o.frame_combine_freq(Y, ws1, cx.out("combine", shape, C64))
        if mfma:
            o.frame_demod_freq_mfma(Y, X, ws=cx.ws("ws2", F, S, R, C), out=cx.out("mfma", shape, C64))

    def check(env, d, o):
        ref = env.oracle.frames_demod_freq(d["Y"], d["X"])
        for n in o:
            parity(o[n], ref)

    Row(f"fd_{F}x{S}x{R}x{C}" + ("_mfma" if mfma else ""), entries, setup, run, check)


fd_row(2, 10, 5, 64, mfma=True)   # k_mrc_freq
fd_row(2, 10, 5, 601)             # k_mrc_freq1
fd_row(2, 10, 5, 512)             # k_mrc_freq_frames
fd_row(2, 10, 5, 1200)            # ... partial last chunk
fd_row(2, 10, 5, 4096)            # 4 symbols per lane
fd_row(2, 10, 5, 1024, mfma=True, plain=False)


# ------------------------------------------------------------ stage entries

def stage_row(R, C):
    K, n = C - 1, 5
    e0, count = K + 3, 2 * K - 5  # starts and ends inside a row

    def setup(env):
        rng = np.random.default_rng(R * 7 + C)
        X = qpsk(K)
        H = (crandn(rng, (R, K)) / np.sqrt(2)).astype(np.complex64)
        Yp = np.zeros((R, C), np.complex64)
        Yp[:, 1:] = H * X
        Yp += 0.01 * crandn(rng, (R, C))
        Yd = crandn(rng, (n, R, C))
        Hin, Pin = env.oracle.ls(Yp, X)
        numflat = np.stack([env.oracle.mrc_numerator(Yd[s], Hin) for s in range(n)]).reshape(-1)
        pos = (np.arange(n)[:, None] * K + out_src(K)[None, :])  # flat numerator element behind each output position
        return dict(X=X, Yp=Yp, Yd=Yd, Hin=Hin, Pin=Pin, chunk=numflat[e0:e0 + count].copy(), numflat=numflat,
                    never=~((pos >= e0) & (pos < e0 + count))[None], rows=crandn(rng, (3, K)))

    def run(cx, d):
        Yp, X, Yd = cx.inp("Yp", d["Yp"]), cx.inp("X", d["X"]), cx.inp("Yd", d["Yd"], align=16)
        Hin, Pin = cx.inp("Hin", d["Hin"]), cx.inp("Pin", d["Pin"])
        Hc, Pq = cx.out("Hc", (R, K), C64), cx.out("P", (K,), F32)
        call("ofdm_ls_estimate", P(Yp), P(X), R, C, P(Hc), P(Pq))
        call("ofdm_mrc_demod", P(Yd), n, P(Hin), P(Pin), R, C, P(cx.out("mrc", (n, K), C64)))
        call("ofdm_mrc_numerator", P(Yd), n, P(Hin), R, C, P(cx.out("num", (n, K), C64)))
        chunk = cx.inp("chunk", d["chunk"])
        fin = cx.out("fin", (1, n, K), C64, never=d["never"])
        call("ofdm_mrc_finalize", P(chunk), e0, count, n, K, P(Pin), P(fin))
        prod = cx.out("prod", (n, R, K), C64)
        call("ofdm_channel_conj_product", P(Yd), n, P(Hin), R, C, P(prod))
        cx.freeze("prod")
        call("ofdm_combine_products", P(prod), n, P(Pin), R, K, 1, P(cx.out("comb", (n, K), C64)))
        call("ofdm_combine_products", P(prod), n, P(Pin), R, K, 0, P(cx.out("comb0", (n, K), C64)))
        rows = cx.inp("rows", d["rows"])
        call("ofdm_shift_rows", P(rows), 3, K, P(cx.out("shift", (3, K), C64)))
        call("ofdm_dist_sqrd", P(Hin), R, K, P(cx.out("dist", (K,), F32)))

    def check(env, d, o):
        oc = env.oracle
        parity(o["Hc"], d["Hin"])
        parity(o["P"], d["Pin"])
        ref = np.stack([oc.mrc(d["Yd"][s], d["Hin"], d["Pin"]) for s in range(n)])
        parity(o["mrc"], ref)
        parity(o["num"], d["numflat"].reshape(n, K))
        w = ~d["never"]
        full = (d["numflat"].astype(np.complex128).reshape(n, K) / d["Pin"].astype(np.float64))[:, out_src(K)][None]
        parity(o["fin"][w], full[w])
        parity(o["prod"], d["Yd"][:, :, 1:] * d["Hin"][None])
        parity(o["comb"], ref)
        parity(np.stack([oc.shift_one_row(u) for u in o["comb0"]]), ref)
        assert np.array_equal(o["shift"], np.stack([oc.shift_one_row(r) for r in d["rows"]]))
        parity(o["dist"], (np.abs(d["Hin"].astype(np.complex128)) ** 2).sum(0))

    Row(f"stages_{R}x{C}", ["ofdm_ls_estimate", "ofdm_mrc_demod", "ofdm_mrc_numerator", "ofdm_mrc_finalize",
                            "ofdm_channel_conj_product", "ofdm_combine_products", "ofdm_shift_rows", "ofdm_dist_sqrd"],
        setup, run, check)


def fft_row(C, nrows=37):
    def setup(env):
        return dict(x=crandn(np.random.default_rng(C), (nrows, C)))

    def run(cx, d):
        x = cx.inp("x", d["x"])
        cx.ofdm.fft_rows(x, cx.out("fwd", (nrows, C), C64))
        cx.ofdm.fft_rows(x, cx.out("inv", (nrows, C), C64), inverse=True)

    def check(env, d, o):  # the bound of test_fft_rows_vs_numpy / test_fft_rows_any_c_vs_numpy
        tol = 2e-6 * max(np.log2(C), 1.0)
        x = d["x"].astype(np.complex128)
        for got, ref in ((o["fwd"], np.fft.fft(x, axis=-1)), (o["inv"], np.fft.ifft(x, axis=-1) * C)):
            assert np.isfinite(got).all() and np.abs(got - ref).max() <= tol * np.abs(ref).max()

    Row(f"fft_rows_{nrows}x{C}", ["ofdm_fft_rows"], setup, run, check)


for _R, _C in ((3, 7), (5, 64), (16, 1024)):
    stage_row(_R, _C)
for _C in (12, 1024, 1536, 2047, 8192):
    fft_row(_C)


# -------------------------------------------------------------- soft output

def soft_row(F, S, C, R=2):
    K = C - 1
    BPS = (2, 4, 6, 8)

    def setup(env):
        from test_soft_demap_gpu import make_frames
        Y, X, _ = make_frames(F, S, R, C, 4, seed=3)
        if C in FUSED:  # the lane-order workspace comes from the time-domain receiver only
            return dict(iq=np.fft.ifft(Y.astype(np.complex128), axis=-1).astype(np.complex64), X=X, qs={})
        return dict(Y=Y, X=X, qs={})

    def run(cx, d):
        o = cx.ofdm
        X, ws = cx.inp("X", d["X"]), cx.ws("ws", F, S, R, C)
        z = cx.out("z", (F, S - 1, K), C64, align=16)
        if C in FUSED:
            o.frame_demod(cx.inp("iq", d["iq"], align=16), X, 0, ws=ws, out=z)
        else:
            o.frame_demod_freq(cx.inp("Y", d["Y"], align=16), X, ws=ws, out=z)
        cx.freeze("z"), cx.freeze("ws")
        Pq = cx.out("Pexp", (F, K), F32)
        for f in range(F):
            call("ofdm_frame_export_estimate", P(ws), ws.numel(), F, S, R, C, f, P(cx.out(f"H{f}", (R, K), C64)), P(Pq[f]))
        for b in BPS:
            nv = o.frame_noise_estimate(z, ws, F, S, R, C, b, out=cx.out(f"nv{b}", (F,), F32))
            cx.freeze(f"nv{b}")
            llr = o.frame_soft_demap(z, ws, F, S, R, C, b, nv, out=cx.out(f"f32_{b}", (F, S - 1, K, b), F32, align=16))
            if b not in d["qs"]:  # the plain run picks the int8 scale once: ~5 % of the values saturate
                d["qs"][b] = float(np.float32(127.0 / np.quantile(np.abs(cx.host(f"f32_{b}")), 0.95)))
            o.frame_soft_demap(z, ws, F, S, R, C, b, nv, fmt="i8", scale=d["qs"][b],
                               out=cx.out(f"i8_{b}", (F, S - 1, K, b), I8, align=16))

    def check(env, d, o):
        from test_soft_demap_gpu import llr_bound, ref_llr, ref_noise_var
        Z = o["z"]
        Pk = o["Pexp"].astype(np.float64)[:, out_src(K)][:, None, :]
        for b in BPS:
            nv = o[f"nv{b}"]
            ref_nv = ref_noise_var(Z, Pk, b)
            assert np.all(np.abs(nv.astype(np.float64) - ref_nv) <= 1e-5 * ref_nv)
            scale = Pk / nv.astype(np.float64)[:, None, None]
            ref, bound = ref_llr(Z, scale, b), llr_bound(Z, scale)
            assert np.all(np.isfinite(o[f"f32_{b}"])) and np.all(np.abs(o[f"f32_{b}"] - ref) <= bound)
            q, qs = o[f"i8_{b}"].astype(np.int64), np.float64(np.float32(d["qs"][b]))
            v, band = ref * qs, bound * qs
            want = np.clip(np.rint(v), -127, 127)
            sure = np.clip(np.rint(v - band), -127, 127) == np.clip(np.rint(v + band), -127, 127)
            assert q.min() >= -127 and np.all(np.abs(q - want) <= 1) and np.array_equal(q[sure], want[sure])

    Row(f"soft_{F}x{S}x{C}", ["ofdm_frame_noise_estimate", "ofdm_frame_soft_demap"], setup, run, check)


soft_row(1, 2, 8)      # 7 elements: int8 at bps 2 is 14 bytes, the remainder path
soft_row(3, 4, 64)
soft_row(2, 3, 1024)   # three full tiles and a ragged one


# ----------------------------------------------------------- phase tracking

def phase_row(F, S, R, C, cp, bps, snr):
    K = C - 1

    def setup(env):
        import cfo_cases as cc
        import phase_cases as pc
        c = cc.frames(F, S, R, C, cp, [0.0] * F, seed=C)
        return dict(iq=np.array(c["y"]), X=np.array(c["X"]), z=np.array(pc.case(F, S - 1, K, bps, 0.03, 0.005, snr)["z"]))

    def run(cx, d):
        o = cx.ofdm
        ws = cx.ws("ws", F, S, R, C)
        o.frame_estimate(cx.inp("iq", d["iq"], align=16), cx.inp("X", d["X"]), cp, ws)
        cx.freeze("ws")
        Pq = cx.out("Pexp", (F, K), F32)
        for f in range(F):
            call("ofdm_frame_export_estimate", P(ws), ws.numel(), F, S, R, C, f, P(cx.out(f"H{f}", (R, K), C64)), P(Pq[f]))
        z = cx.inp("z", d["z"])
        o.frame_phase_track(z, ws, F, S, R, C, bps, out=cx.out("out", (F, S - 1, K), C64),
                            phase=cx.out("phase", (F, S - 1), F32))

    def check(env, d, o):
        import phase_cases as pc
        ref, theta, margin = pc.track(d["z"], pc.p_by_position(o["Pexp"]), bps)
        assert margin >= pc.MARGIN_MIN
        parity(o["out"], ref)
        assert np.all(np.abs(o["phase"].astype(np.float64) - theta) <= RTOL + np.spacing(np.abs(o["phase"])))

    Row(f"phase_{F}x{S}x{R}x{C}_bps{bps}", ["ofdm_frame_phase_track"], setup, run, check)


phase_row(2, 11, 2, 64, 4, 4, 25)      # K = 63, 10 rows: the row loop's three-row trips leave one
phase_row(3, 13, 4, 9, 2, 4, 25)       # K = 8: less than a wave, even K
phase_row(3, 13, 4, 1024, 16, 8, 38)   # the lane-order workspace, four elements per thread
phase_row(2, 3, 1, 2048, 16, 6, 30)    # the 1024-thread kernel


# ---------------------------------------------------------------------- CFO

def cfo_row(F, S, R, C, cp, skip):
    def setup(env):
        import cfo_cases as cc
        c = cc.frames(F, S, R, C, cp, None, seed=cp)
        return dict(y=np.array(c["y"]), eps=np.array(c["eps"], np.float32))

    def run(cx, d):
        y = cx.inp("y", d["y"], align=16)
        cx.ofdm.frame_cfo_estimate(y, cp, skip, eps=cx.out("eps", (F,), F32), gamma=cx.out("gamma", (F,), C64))
        cx.ofdm.frame_cfo_derotate(y, cp, cx.inp("eps_in", d["eps"]), out=cx.out("derot", d["y"].shape, C64, align=16))

    def check(env, d, o):
        import cfo_cases as cc
        g64, e64 = cc.gamma_ref(d["y"], cp, skip)  # test_estimator's bounds
        assert np.all(np.abs(o["gamma"] - g64) <= 1e-5 * np.abs(g64))
        assert np.all(np.abs(o["eps"].astype(np.float64) - e64) <= 1e-5 / (2 * np.pi))
        parity(o["derot"], cc.derotate_ref(d["y"], d["eps"], cp))

    Row(f"cfo_{F}x{S}x{R}x{C}cp{cp}skip{skip}", ["ofdm_frame_cfo_estimate", "ofdm_frame_cfo_derotate"], setup, run, check)


cfo_row(3, 4, 5, 1024, 7, 3)
cfo_row(3, 3, 3, 600, 9, 0)


# --------------------------------------------------------- sc16 conversion

def convert_row(n):
    def setup(env):
        rng = np.random.default_rng(n)
        q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        q[:2] = [[-32768, 32767], [-1, 1]]
        return dict(q=q)

    def run(cx, d):
        cx.ofdm.iq_convert_sc16(cx.inp("q", d["q"], align=16), out=cx.out("x", (n,), C64, align=16))

    def check(env, d, o):
        from test_sc16_gpu import dequantise
        assert np.array_equal(words(o["x"]), words(dequantise(d["q"], env.ofdm.SC16_SCALE)))

    Row(f"iq_convert_sc16_{n}", ["ofdm_iq_convert_sc16"], setup, run, check)


for _n in (4100, 4097, 4098, 4099):
    convert_row(_n)


# ------------------------------------------------------------------ PN sync

def pn_correlate_row(R, N, L):
    nl = N - L + 1

    def setup(env):
        from pn_cases import rx_buffer
        buf, pn = rx_buffer(R, N, L, {R - 1: ((N - L) // 2, 0.7 + 0.4j)}, seed=R * N + L)
        return dict(buf=buf, pn=pn)

    def run(cx, d):
        buf, pn = cx.inp("buf", d["buf"]), cx.inp("pn", d["pn"])
        call("ofdm_pn_correlate", P(buf), R, N, P(pn), L, 0.5, P(cx.out("pos", (1,), I64)),
             P(cx.out("mag", (R, nl), F32)))
        call("ofdm_pn_correlate", P(buf), R, N, P(pn), L, 0.5, P(cx.out("pos_early", (1,), I64)), None)

    def check(env, d, o):
        ref_pos, ref_mag = env.oracle.pn_correlate(d["buf"], d["pn"], 0.5, mag=True)
        assert np.array_equal(words(o["mag"]), words(ref_mag))
        assert int(o["pos"][0]) == ref_pos == int(o["pos_early"][0])

    Row(f"pn_correlate_{R}x{N}x{L}", ["ofdm_pn_correlate"], setup, run, check)


def pn_extract_row(lag, cp, hit=True):
    R, N, L, C = 3, 12000, 511, 1024
    nsym = (N - L) // (C + cp)

    def setup(env):
        rng = np.random.default_rng(lag + cp)
        return dict(b1=crandn(rng, (R, N)), b2=crandn(rng, (R, N)),
                    pos=np.array([2 * (N - L + 1) + lag if hit else -1], np.int64))

    def run(cx, d):
        cx.ofdm.pn_extract(cx.inp("b1", d["b1"]), cx.inp("b2", d["b2"]), L, cx.inp("pos", d["pos"]), C, cp,
                           nsym, out=cx.out("sym", (nsym, R, C), C64, never=None if hit else np.ones((nsym, R, C), bool)))

    def check(env, d, o):
        if hit:  # no hit: nothing is written (the header), which (b) has checked
            assert np.array_equal(words(o["sym"]), words(env.oracle.pn_extract(d["b1"], d["b2"], L, lag, C, cp, nsym)))

    Row(f"pn_extract_lag{lag}_cp{cp}" + ("" if hit else "_no_hit"), ["ofdm_pn_extract"], setup, run, check)


for _s in ((2, 5000, 127), (3, 3000, 1500), (1, 2100, 2047), (4, 1030, 1024), (2, 9000, 1023), (5, 1100, 1)):
    pn_correlate_row(*_s)
for _s in ((0, 0), (1, 16), (4000, 72)):
    pn_extract_row(*_s)
pn_extract_row(1, 16, hit=False)


# ---------------------------------------------------------------- modulator

def tx_row(nrows, C, cp):
    K = C - 1
    combos = [(m, n) for m in ("reference", "rx") for n in ("peak", "scale")]

    def setup(env):
        import tx_cases
        return dict(X=tx_cases.rows_of(100 * nrows + cp + C, nrows, K))

    def run(cx, d):
        X = cx.inp("X", d["X"])
        for m, n in combos:
            iq, peak = cx.out(f"iq_{m}_{n}", (nrows, C + cp), C64), cx.out(f"peak_{m}_{n}", (nrows,), F32)
            call("ofdm_tx_modulate", P(X), K, nrows, C, cp, cx.ofdm.TX_MAPS[m], cx.ofdm.TX_NORMS[n], 0.25, P(iq), P(peak))

    def check(env, d, o):
        import tx_cases
        for m, n in combos:  # test_tx_gpu.check
            want, wpeak = tx_cases.tx_numpy(d["X"], C, cp, m, n, 0.25)
            parity(o[f"iq_{m}_{n}"], want, RTOL)
            assert np.allclose(o[f"peak_{m}_{n}"], wpeak, rtol=1e-5, atol=0)

    Row(f"tx_modulate_{nrows}x{C}cp{cp}", ["ofdm_tx_modulate"], setup, run, check)


for _s in ((3, 1024, 7), (9, 1024, 16), (3, 600, 5), (2, 9, 9), (2, 8192, 0)):
    tx_row(*_s)


# ------------------------------------------------------------- zero forcing

def zf_precoder_row(U, R, K):
    def setup(env):
        from zf_cases import channel
        return dict(H=channel(U, R, K, seed=U * 7 + R + K))

    def run(cx, d):
        H = cx.inp("H", d["H"])
        W, Wt = cx.out("W", (K, U, R), C64), cx.out("Wt", (U, R, K), C64)
        call("ofdm_zf_precoder", P(H), U, R, K, P(W), P(Wt))
        cx.freeze("W")
        call("ofdm_zf_transpose", P(W), U, R, K, P(cx.out("Wt2", (U, R, K), C64)))

    def check(env, d, o):  # bit-identical to the oracle (test_zf_precoder_parity)
        ref = env.oracle.zf_precoder(d["H"])
        assert np.array_equal(o["W"], ref)
        assert np.array_equal(o["Wt"], ref.transpose(1, 2, 0)) and np.array_equal(o["Wt2"], o["Wt"])

    Row(f"zf_precoder_{U}x{R}x{K}", ["ofdm_zf_precoder", "ofdm_zf_transpose"], setup, run, check)


def zf_apply_detect_row(U, R, K, n, degenerate):
    def setup(env):
        from zf_cases import channel, qpsk as zq
        if degenerate:
            W = np.ascontiguousarray(channel(U, R, K, seed=n).transpose(2, 0, 1))
        else:
            W = env.oracle.zf_precoder(channel(U, R, K, seed=n))
        X = zq(n, U, K, seed=n + 1)
        Y = env.oracle.zf_apply(W, X)
        Yn = (Y + 0.05 * zq(n, R, K, seed=n + 2)).astype(np.complex64)
        return dict(W=W, Wt=np.ascontiguousarray(W.transpose(1, 2, 0)), X=X, Y=Y, Yn=Yn)

    def run(cx, d):
        Wt = cx.inp("Wt", d["Wt"])
        cx.ofdm.zf_apply(Wt, cx.inp("X", d["X"]), out=cx.out("Y", (n, R, K), C64))
        cx.ofdm.zf_detect(Wt, cx.inp("Yn", d["Yn"]), out=cx.out("Xh", (n, U, K), C64))

    def check(env, d, o):
        parity(o["Y"], d["Y"])
        parity(o["Xh"], env.oracle.zf_detect(d["W"], d["Yn"]))

    Row(f"zf_apply_detect_{U}x{R}x{K}x{n}", ["ofdm_zf_apply", "ofdm_zf_detect"], setup, run, check)


def zf_pitched_row(kind, U, R, K, n, ld_in, ld_out):
    """detect: Y (n, R, ld_in) -> X (n, U, ld_out); apply: X (n, U, ld_in) -> Y (n, R, ld_out).  The input pad
    holds the band word (a read of it reaches the output), the output pad is documented as never written."""
    rows_in, rows_out = (R, U) if kind == "detect" else (U, R)

    def setup(env):
        from zf_cases import channel, qpsk as zq
        W = env.oracle.zf_precoder(channel(U, R, K, seed=n + 5))
        X = zq(n, U, K, seed=n + 6)
        src = X if kind == "apply" else (env.oracle.zf_apply(W, X) + 0.05 * zq(n, R, K, seed=n + 7)).astype(np.complex64)
        padded = np.full((n, rows_in, ld_in), np.array([gc.BAND_WORD] * 2, np.uint32).view(np.complex64)[0], np.complex64)
        padded[:, :, :K] = src
        never = np.zeros((n, rows_out, ld_out), bool)
        never[:, :, K:] = True
        return dict(W=W, Wt=np.ascontiguousarray(W.transpose(1, 2, 0)), src=src, padded=padded, never=never)

    def run(cx, d):
        Wt, src = cx.inp("Wt", d["Wt"]), cx.inp("src", d["padded"])
        out = cx.out("out", (n, rows_out, ld_out), C64, never=d["never"])
        (cx.ofdm.zf_detect_pitched if kind == "detect" else cx.ofdm.zf_apply_pitched)(Wt, src, out=out)

    def check(env, d, o):
        ref = env.oracle.zf_detect(d["W"], d["src"]) if kind == "detect" else env.oracle.zf_apply(d["W"], d["src"])
        parity(o["out"][:, :, :K], ref)

    Row(f"zf_{kind}_pitched_{U}x{R}x{K}x{n}_{ld_in}_{ld_out}", [f"ofdm_zf_{kind}_ex"], setup, run, check)


for _s in ((1, 1, 5), (3, 7, 100), (16, 64, 65)):
    zf_precoder_row(*_s)


def _zf_lists():
    import test_zf_gpu as tz
    marks = {f.__name__: [m for m in f.pytestmark if m.name == "parametrize"][0].args[1]
             for f in (tz.test_zf_apply_detect_parity, tz.test_zf_apply_detect_degenerate_shapes,
                       tz.test_zf_detect_pitched, tz.test_zf_apply_pitched)}
    return marks


_Z = _zf_lists()
for _U, _R, _K, _n in _Z["test_zf_apply_detect_parity"]:
    zf_apply_detect_row(_U, _R, _K, min(_n, 9), False)
for _U, _R, _K, _n in _Z["test_zf_apply_detect_degenerate_shapes"]:
    zf_apply_detect_row(_U, _R, _K, min(_n, 9), True)
for _U, _R, _K, _n, _a, _b in _Z["test_zf_detect_pitched"]:
    zf_pitched_row("detect", _U, _R, _K, min(_n, 9), _a, _b)
for _U, _R, _K, _n, _a, _b in _Z["test_zf_apply_pitched"]:
    zf_pitched_row("apply", _U, _R, _K, min(_n, 9), _a, _b)


# ------------------------------------------------- hash, probe, synth, count

def hash_row(nwords):
    def setup(env):
        a = np.random.default_rng(nwords).integers(0, 2 ** 32, nwords, dtype=np.uint64).astype(np.uint32).view(np.int32)
        b = a.copy()
        b[[0, -1]] = b[[-1, 0]]  # the same words in another order
        return dict(a=a, b=b)

    def run(cx, d):
        for n in ("a", "b"):
            call("ofdm_buffer_hash", P(cx.inp(n, d[n])), 4 * nwords, P(cx.out(f"h{n}", (1,), I64)))

    def check(env, d, o):  # no numeric reference in the suite: the documented property, order sensitivity
        assert o["ha"][0] != o["hb"][0] or d["a"][0] == d["a"][-1]

    Row(f"buffer_hash_{nwords}", ["ofdm_buffer_hash"], setup, run, check)


hash_row(1000)
hash_row(65537)


def probe_row(nbytes):
    SINK = 1024 * 256 * 4

    def setup(env):
        return dict(src=np.random.default_rng(nbytes).standard_normal(nbytes // 4).astype(np.float32))

    def run(cx, d):
        src = cx.inp("src", d["src"], align=16)
        cx.ofdm.hbm_probe(0, src, cx.out("copy", (nbytes // 4,), F32, align=16))
        cx.ofdm.hbm_probe(1, src, cx.out("sink", (SINK // 4,), F32, align=16))

    def check(env, d, o):
        assert np.array_equal(words(o["copy"]), words(d["src"]))
        # every thread adds its few loads in f32: the partial sums add up to the buffer's sum
        s64 = d["src"].astype(np.float64)
        assert abs(o["sink"].astype(np.float64).sum() - s64.sum()) <= 1e-5 * np.abs(s64).sum()

    Row(f"hbm_probe_{nbytes}", ["ofdm_hbm_probe"], setup, run, check)


probe_row(3 * 16384 + 5 * 16)   # three 16-KiB chunks and a tail of five 16-byte loads
probe_row(48)


def synth_row(F, S, R, C, p):
    K = C - 1

    def setup(env):
        import torch
        Xh = qpsk(K, seed=C)
        X = torch.from_numpy(Xh).to(env.dev)
        z = env.ofdm.frame_demod(env.ofdm.synth_frames(F, S, R, C, X, prefix=p, seed=42, noise_std=0.02), X, p).cpu().numpy()
        idx = np.arange(0, z.size, 97)  # the real part of every 97th symbol flipped: that many decision errors
        z.reshape(-1)[idx] = -z.reshape(-1)[idx].real + 1j * z.reshape(-1)[idx].imag
        return dict(X=Xh, zbad=z, nbad=idx.size)

    def run(cx, d):
        X = cx.inp("X", d["X"])
        iq = cx.ofdm.synth_frames(F, S, R, C, X, prefix=p, seed=42, noise_std=0.02,
                                  out=cx.out("iq", (F, S, R, C + p), C64, align=16))
        cx.freeze("iq")
        z = cx.ofdm.frame_demod(iq, X, p, ws=cx.ws("ws", F, S, R, C), out=cx.out("z", (F, S - 1, K), C64))
        cx.freeze("z")
        err = cx.out("err", (1,), I64, fill=[5])  # the entry ADDS to the counter
        call("ofdm_count_symbol_errors", P(z), F, S, C, 42, 0, P(err))
        call("ofdm_count_symbol_errors", P(cx.inp("zbad", d["zbad"])), F, S, C, 42, 0,
             P(cx.out("err_bad", (1,), I64, fill=[0])))

    def check(env, d, o):
        # the synthetic frames are the reference's model: cyclic prefix exact, and they decode to their own symbols
        assert np.array_equal(words(o["iq"][..., :p]), words(o["iq"][..., C:]))
        parity(o["z"], env.oracle.frames_demod(o["iq"], d["X"], p))
        assert int(o["err"][0]) == 5
        assert int(o["err_bad"][0]) == d["nbad"]

    Row(f"synth_count_{F}x{S}x{R}x{C}p{p}", ["ofdm_synth_frames", "ofdm_count_symbol_errors"], setup, run, check)


synth_row(2, 3, 2, 1024, 7)
synth_row(2, 3, 2, 600, 5)


# ----------------------------------------------------------------- pipeline

def pipeline_row(C, sc16=False, manual=False):
    F, S, R, p, chunk = 5, 3, 2, 7, 2  # chunks of 2, 2 and a tail of one frame
    K = C - 1
    entries = (["ofdm_pipeline_acquire_sc16" if sc16 else "ofdm_pipeline_acquire", "ofdm_pipeline_submit"] if manual
               else ["ofdm_pipeline_demod_sc16" if sc16 else "ofdm_pipeline_demod"])

    def setup(env):
        X = qpsk(K, seed=C + 1)
        iq = synth(env, F, S, R, C, X, p, seed=C)
        if sc16:
            from test_sc16_gpu import dequantise, quantise
            q = quantise(iq)
            return dict(iq=q, X=X, eff=dequantise(q, env.ofdm.SC16_SCALE))
        return dict(iq=iq, X=X, eff=iq)

    def run(cx, d):
        import torch
        from test_pipeline_gpu import _copy_to_ptr
        if manual:  # the ring reader's form: device frames into the slot, outputs to a caller's device buffer
            out = cx.out("out", (F, S - 1, K), C64)
            src = cx.inp("iq", d["iq"])
        else:       # host frames, and a host output array with bands, carved from a larger array
            if cx.guarded:
                g = cx.bufs["out"] = gc.guarded((F, S - 1, K), C64, "cpu")
                out = g.view.numpy()
            else:
                out = np.empty((F, S - 1, K), np.complex64)
            cx.outs.append("out")
            cx.tensors["out"] = torch.from_numpy(out)
            src = d["iq"]
        with cx.ofdm.Pipeline(S, R, C, d["X"], p, chunk_frames=chunk, depth=2,
                              sample_format="sc16" if sc16 else "fc32") as pl:
            if manual:
                fb = src[0].numel() * src.element_size()
                for lo in range(0, F, chunk):
                    n = min(chunk, F - lo)
                    dptr, s = pl.acquire_sc16() if sc16 else pl.acquire()
                    _copy_to_ptr(dptr, src[lo:lo + n], fb * n, s)
                    pl.submit(n, out[lo:lo + n])
            else:
                pl.demod(src, out)
            pl.sync()
        torch.cuda.synchronize()

    def check(env, d, o):
        parity(o["out"], env.oracle.frames_demod(d["eff"], d["X"], p))

    # no aligned run: the pipeline copies into and out of the caller's buffers with hipMemcpyAsync, no kernel touches them
    Row(f"pipeline_{'manual' if manual else 'demod'}_{'sc16' if sc16 else 'fc32'}_C{C}", entries, setup, run, check,
        aligned=False)


pipeline_row(256)
pipeline_row(1024)
pipeline_row(1024, sc16=True)
pipeline_row(256, manual=True)
pipeline_row(1024, sc16=True, manual=True)


# ------------------------------------------------------------------ the test

_data = {}


def _run(env, row, mode):
    import torch
    if row.id not in _data:
        _data[row.id] = row.setup(env)
    cx = Ctx(env, mode)
    try:
        row.run(cx, _data[row.id])
        torch.cuda.synchronize()
        res = cx.results()
    finally:
        cx.close()
    return cx, res


def _contained(cx, row, mode):
    """(a), (b), (c) and the denoiser's never-written positions of one guarded run"""
    order = [n for n in cx.bufs if n in cx.outs or isinstance(cx.bufs[n], gc.GuardedWorkspace)]
    for n in order + [n for n in cx.bufs if n not in order]:
        cx.bufs[n].assert_bands(f"{row.id} [{mode}] {n}")
    for n in cx.outs:
        g = cx.bufs[n]
        left = g.unwritten()
        if n in cx.never:
            doc = g.element_words(cx.never[n])
            assert np.all(np.isin(doc, left)), f"{row.id} [{mode}] {n}: a documented never-written position was written"
            left = np.setdiff1d(left, doc)
        assert left.size == 0, f"{row.id} [{mode}] {n}: {left.size} word(s) never written, first {left[:8].tolist()}"
    for n, g in cx.bufs.items():
        if g.is_input:
            g.assert_unmodified(f"{row.id} [{mode}] {n}", mask=cx.frozen.get(n))
    if cx.bin0:
        g = cx.bufs[cx.bin0]
        F, S, R, C = g.geom
        b, pc = g.body_bytes(), g.pieces()
        hc = b[pc["Hc"][0]:pc["Hc"][1]].view(np.uint32).reshape(F * R, C, 2)
        pp = b[pc["P"][0]:pc["P"][1]].view(np.uint32).reshape(F, C)
        assert np.all(hc[:, 0, :] == gc.FILL_WORD) and np.all(pp[:, 0] == gc.FILL_WORD), \
            f"{row.id} [{mode}]: ofdm_frame_estimate_denoise wrote bin 0 of an Hc row or P[f][0]"


def _same(row, what, a, b, never):
    for n in a:
        x, y = words(a[n]), words(b[n])
        if n in never:
            keep = np.repeat(~never[n].reshape(-1), a[n].dtype.itemsize)
            x, y = x[keep], y[keep]
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, f"{row.id}: {n} differs between {what} in {bad.size} byte(s), first at {bad[:4].tolist()}"


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r.id)
def test_containment(ofdm, oracle, dev, row):
    env = Env(ofdm, dev, oracle)
    _, plain = _run(env, row, "plain")
    cx, guarded = _run(env, row, "guarded")
    _contained(cx, row, "guarded")                                   # (a) (b) (c)
    _same(row, "the plain and the guarded run", plain, guarded, cx.never)   # (d)
    if row.prefix:                                                   # (e)
        px, poisoned = _run(env, row, "poisoned")
        _contained(px, row, "poisoned")
        _same(row, "the guarded run and the run with a poisoned prefix", guarded, poisoned, px.never)
        for n, v in poisoned.items():
            assert np.isfinite(v).all(), f"{row.id}: {n} is not finite with a poisoned prefix"
    row.check(env, _data[row.id], plain)                             # (f)
    if row.aligned:                                                  # section 4: (a), (b), (f)
        ax, at = _run(env, row, "aligned")
        _contained(ax, row, "aligned")
        row.check(env, _data[row.id], at)
    ofdm.device_status()
    _data.pop(row.id, None)
