"""Shared by test_footprint_cpu and test_footprint_gpu: which outputs may
depend on one spoiled input (include/ofdm_lsmrc.h, "degenerate and non-finite
input"; DESIGN.md, "Footprints").

A case is an entry point, a shape, a spoil and a footprint.  A spoil is a dict
that says where one input is made degenerate; `spoil_*` returns the spoiled
copy of the clean input and `*_footprint` the boolean mask, over every output,
of the cells that may differ from the clean run.  THE MASKS ARE BUILT FROM THE
GEOMETRY AND THE DEPENDENCY RULES WRITTEN HERE, never from an output: no
function of this module that returns a mask takes an output as an argument.

Indices: f frame, s symbol (0 the pilot), r antenna, i time sample of a row
(prefix included), b FFT bin, k / j index into the rotated pilots X (subcarrier
j sits in bin j + 1), n symbol of a zero-forcing batch, u user.  Output columns
go through tx_cases.out_pos_any.

Inputs are numpy arrays or torch tensors: a spoil copies (`.copy()` /
`.clone()`) and assigns by index, which both understand."""
import numpy as np

import cfo_cases as cc
import tx_cases
import zf_cases

NAN = complex(float("nan"), float("nan"))  # both components: at bins 0 and C/2 an FFT's real output ignores Im
INF = complex(float("inf"), 0.0)


def pos(j, K):
    return tx_cases.out_pos_any(j, K)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


def nonfinite(a):
    return ~np.isfinite(a)


def _copy(a):
    return a.copy() if isinstance(a, np.ndarray) else a.clone()


def assert_outside_identical(got, clean, mask, label):
    """(a): outside the footprint every cell is finite and holds the clean run's bits."""
    assert got.shape == clean.shape == mask.shape, (label, got.shape, clean.shape, mask.shape)
    keep = ~mask
    assert np.all(np.isfinite(got[keep])), f"{label}: non-finite value outside the footprint at " \
        f"{np.argwhere(keep & nonfinite(got))[:4].tolist()}"
    gb, cb = bits(got), bits(clean)
    if gb.shape != got.shape:  # complex64 -> one uint64 per element
        gb, cb = gb.reshape(got.shape), cb.reshape(got.shape)
    diff = keep & (gb != cb)
    assert not diff.any(), f"{label}: {int(diff.sum())} cells outside the footprint changed, first at " \
        f"{np.argwhere(diff)[:4].tolist()}"


def assert_inside_nonfinite(got, ref, mask, label):
    """(b): every footprint cell the reference makes non-finite is non-finite (NaN against Inf is not compared)."""
    need = mask & nonfinite(ref)
    miss = need & np.isfinite(got)
    assert not miss.any(), f"{label}: {int(miss.sum())} of {int(need.sum())} cells the reference makes non-finite " \
        f"are finite, first at {np.argwhere(miss)[:4].tolist()}"


# ------------------------------------------------------------ the receivers

def rx_frames(F, S, R, C, cp, eps=None, seed=0):
    """cfo_cases.frames without rotation (eps None) or with the given offsets:
    dict(y (F, S, R, C + cp) complex64, X (K,), eps (F,) float32), read-only, cached."""
    return cc.frames(F, S, R, C, cp, [0.0] * F if eps is None else eps, seed=seed)


def to_sc16(y, amp=4096.0):
    """(F, S, R, Cp) complex64 -> (F, S, R, Cp, 2) int16, y * amp rounded and clipped."""
    q = np.clip(np.rint(np.stack([y.real, y.imag], axis=-1) * amp), -32767, 32767)
    return np.ascontiguousarray(q.astype(np.int16))


def from_sc16(q, scale):
    """What the sc16 entries are defined on: i16 * scale per component, one f32 rounding."""
    x = q.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(x).view(np.complex64)[..., 0]


def sample(f, s, r, i, value=NAN):
    return dict(kind="sample", f=f, s=s, r=r, i=i, value=value)


def zero_pilot(k):
    return dict(kind="zero_pilot", k=k)


def silent_frame(f):
    return dict(kind="silent", f=f)


def eps_change(f, value):
    return dict(kind="eps", f=f, value=value)


def label(sp):
    v = sp.get("value")
    tag = "" if v is None else ("nan" if v != v else "inf" if abs(v) == float("inf") else f"{v:g}")
    return sp["kind"] + tag + "@" + ",".join(f"{k}{sp[k]}" for k in ("f", "s", "r", "i", "b", "k", "n", "u") if k in sp)


def spoil_rx(y, X, eps, sp):
    """The spoiled copies (y, X, eps) of a receiver's inputs; y (F, S, R, Cp)
    complex, or (F, S, R, Cp, 2) int16 (zero_pilot and silent only: an int16
    cannot be non-finite).  The untouched ones are returned as they came."""
    kind = sp["kind"]
    if kind == "sample":
        y = _copy(y)
        y[sp["f"], sp["s"], sp["r"], sp["i"]] = sp["value"]
    elif kind == "zero_pilot":
        X = _copy(X)
        X[sp["k"]] = 0
    elif kind == "silent":
        y = _copy(y)
        y[sp["f"], 0] = 0
    elif kind == "eps":
        eps = _copy(eps)
        eps[sp["f"]] = sp["value"]
    else:
        raise ValueError(kind)
    return y, X, eps


def rx_footprint(sp, F, S, R, C, cp=0, freq=False):
    """Masks of a receiver's outputs: out (F, S-1, K), H (F, R, K) and P (F, K)
    (the exported estimate, by subcarrier), frame (F,).

    Rules.  The FFT of a row spreads a time sample over every bin, the prefix is
    never read, the estimate of frame f comes from its pilot symbol alone and
    serves every data symbol of f, antennas are summed per bin, and output
    column pos(j) holds subcarrier j.  Frequency-domain entries (freq=True,
    sp["b"] a bin): bin 0 is dropped, bin b is subcarrier b - 1."""
    K = C - 1
    out = np.zeros((F, S - 1, K), bool)
    H = np.zeros((F, R, K), bool)
    P = np.zeros((F, K), bool)
    kind = sp["kind"]
    if kind == "sample" and not freq:
        f, s, r, i = sp["f"], sp["s"], sp["r"], sp["i"]
        if i >= cp:                       # a prefix sample reaches nothing
            if s == 0:
                out[f], H[f, r], P[f] = True, True, True
            else:
                out[f, s - 1] = True
    elif kind == "sample":
        f, s, r, b = sp["f"], sp["s"], sp["r"], sp["b"]
        if b >= 1:                        # the DC bin reaches nothing
            if s == 0:
                out[f, :, pos(b - 1, K)], H[f, r, b - 1], P[f, b - 1] = True, True, True
            else:
                out[f, s - 1, pos(b - 1, K)] = True
    elif kind == "zero_pilot":
        k = sp["k"]
        out[:, :, pos(k, K)], H[:, :, k], P[:, k] = True, True, True
    elif kind in ("silent", "eps"):
        f = sp["f"]
        out[f], H[f], P[f] = True, True, True
    else:
        raise ValueError(kind)
    return dict(out=out, H=H, P=P, frame=out.any(axis=(1, 2)) | P.any(axis=1))


def spoil_freq(Y, X, sp):
    """As spoil_rx on frequency-domain frames Y (F, S, R, C): a sample spoil names a bin."""
    if sp["kind"] == "sample":
        Y = _copy(Y)
        Y[sp["f"], sp["s"], sp["r"], sp["b"]] = sp["value"]
        return Y, X
    Y, X, _ = spoil_rx(Y, X, None, sp)
    return Y, X


def bin_sample(f, s, r, b, value=NAN):
    return dict(kind="sample", f=f, s=s, r=r, b=b, value=value)


def straddle_frame(F, S, W):
    """The first frame fb whose last data symbol shares a workgroup of W
    consecutive data symbols with frame fb + 1's first, or None."""
    for fb in range(F - 1):
        if ((fb + 1) * (S - 1)) % W:
            return fb
    return None


def rx_placements(F, S, R, C, cp, fb, short=False):
    """The spoils of a time-domain receiver, each at the first element, the
    last element (clamped tail loads, ragged last groups) and the frame
    boundary fb | fb + 1 that a straddling workgroup spans (fb None: frame 0 | 1)."""
    Cp, K = C + cp, C - 1
    fb = 0 if fb is None else fb
    fn = min(fb + 1, F - 1)
    rm, im = R // 2, cp + min(C // 2 + 1, C - 1)
    sps = [sample(fb, S - 1, rm, im), sample(fn, 0, rm, im), sample(fn, 1, R - 1, Cp - 1, INF),
           sample(F - 1, S - 1, R - 1, Cp - 1), sample(F - 1, 0, R - 1, Cp - 1, INF),
           zero_pilot(K - 1), silent_frame(fn)]
    if cp:
        sps.append(sample(fb, S - 1, R - 1, cp - 1))
    if not short:
        sps += [sample(0, 1, 0, cp), sample(0, 0, 0, cp), sample(fn, 0, 0, cp, INF), sample(fb, S - 1, 0, Cp - 1, INF),
                zero_pilot(0), zero_pilot(min(10, K - 1)), silent_frame(0), silent_frame(F - 1)]
        if cp:
            sps.append(sample(0, 0, 0, 0))
    return sps


def freq_placements(F, S, R, C, fb=0):
    fn = min(fb + 1, F - 1)
    K = C - 1
    return [bin_sample(0, 1, 0, 0), bin_sample(0, 0, 0, 0),               # the DC bin: nothing
            bin_sample(0, 1, 0, 1), bin_sample(0, 0, 0, 1, INF),
            bin_sample(F - 1, S - 1, R - 1, C - 1), bin_sample(F - 1, 0, R - 1, C - 1),
            bin_sample(fb, S - 1, R // 2, C // 2, INF), bin_sample(fn, 0, R // 2, C // 2 + 1),
            zero_pilot(0), zero_pilot(K - 1), zero_pilot(min(10, K - 1)), silent_frame(0), silent_frame(F - 1),
            silent_frame(fn)]


def oracle_estimates(oracle, y, X, cp):
    """(H (F, R, K), P (F, K)) of the oracle's per-frame estimate."""
    HP = [oracle.frame_demod(y[f], X, cp)[1:] for f in range(y.shape[0])]
    return np.stack([h for h, _ in HP]), np.stack([p for _, p in HP])


# -------------------------------------------------- float64 stage references

def out_src_index(K):
    return np.array([tx_cases.out_src(k, K) for k in range(K)])


def rotate(Z):
    """(..., K) by subcarrier -> by output position."""
    return Z[..., out_src_index(Z.shape[-1])]


def c64(a):
    with np.errstate(all="ignore"):
        return np.asarray(a).astype(np.complex64)


def ref_ls(Y, X):
    """ofdm_ls_estimate: Y (R, C), X (K,) -> (Hconj (R, K) complex64, Hsqrd (K,) float32)."""
    with np.errstate(all="ignore"):
        H = np.conj(Y[:, 1:].astype(np.complex128) / X.astype(np.complex128))
        return c64(H), (np.abs(H) ** 2).sum(0).astype(np.float32)


def ref_numerator(Y, H):
    with np.errstate(all="ignore"):
        return c64((Y[:, :, 1:].astype(np.complex128) * H.astype(np.complex128)[None]).sum(1))


def ref_conj_product(Y, H):
    with np.errstate(all="ignore"):
        return c64(Y[:, :, 1:].astype(np.complex128) * H.astype(np.complex128)[None])


def ref_combine(prod, P):
    with np.errstate(all="ignore"):
        return c64(rotate(prod.astype(np.complex128).sum(1) / P.astype(np.float64)))


def ref_mrc(Y, H, P):
    with np.errstate(all="ignore"):
        return c64(rotate(ref_numerator(Y, H).astype(np.complex128) / P.astype(np.float64)))


def ref_dist(H):
    with np.errstate(all="ignore"):
        return (np.abs(H.astype(np.complex128)) ** 2).sum(0).astype(np.float32)


def stage_inputs(n, R, C, seed=0):
    """A frequency-domain pilot symbol, its estimate and n data symbols (float64 references)."""
    c = rx_frames(1, n + 1, R, C, 0, seed=seed)
    Y = np.fft.fft(c["y"][0].astype(np.complex128), axis=-1).astype(np.complex64)  # (n + 1, R, C)
    H, P = ref_ls(Y[0], c["X"])
    return dict(Yp=Y[0], Yd=np.ascontiguousarray(Y[1:]), X=c["X"], H=H, P=P)


def stage_cases(n, R, C):
    """(entry, input name, index, {output name: mask}) of the stage entries:
    first, last and a middle element of every input each reads.  Entries: ls
    (Yp, X -> H, P), mrc (Yd, H, P -> out), numerator (Yd, H -> num),
    conj_product (Yd, H -> prod), combine (prod, P -> out), dist (H -> P)."""
    K = C - 1

    def m(shape, idx):
        a = np.zeros(shape, bool)
        if idx is not None:
            a[idx] = True
        return a

    cases = []
    for r, b in ((0, 0), (0, 1), (R - 1, C - 1), (R // 2, C // 2)):
        j = b - 1
        cases.append(("ls", "Yp", (r, b), dict(H=m((R, K), (r, j) if b else None), P=m((K,), j if b else None))))
    for j in (0, K - 1):
        cases.append(("ls", "X", (j,), dict(H=m((R, K), (slice(None), j)), P=m((K,), j))))
    for q, r, b in ((0, 0, 0), (0, 0, 1), (n - 1, R - 1, C - 1), (n // 2, R // 2, C // 2)):
        j = b - 1
        cases.append(("mrc", "Yd", (q, r, b), dict(out=m((n, K), (q, pos(j, K)) if b else None))))
        cases.append(("numerator", "Yd", (q, r, b), dict(num=m((n, K), (q, j) if b else None))))
        cases.append(("conj_product", "Yd", (q, r, b), dict(prod=m((n, R, K), (q, r, j) if b else None))))
    for r, j in ((0, 0), (R - 1, K - 1), (R // 2, K // 2)):
        cases.append(("mrc", "H", (r, j), dict(out=m((n, K), (slice(None), pos(j, K))))))
        cases.append(("numerator", "H", (r, j), dict(num=m((n, K), (slice(None), j)))))
        cases.append(("conj_product", "H", (r, j), dict(prod=m((n, R, K), (slice(None), r, j)))))
        cases.append(("dist", "H", (r, j), dict(P=m((K,), j))))
        cases.append(("mrc", "P", (j,), dict(out=m((n, K), (slice(None), pos(j, K))))))
        cases.append(("combine", "P", (j,), dict(out=m((n, K), (slice(None), pos(j, K))))))
    for q, r, j in ((0, 0, 0), (n - 1, R - 1, K - 1), (n // 2, R // 2, K // 2)):
        cases.append(("combine", "prod", (q, r, j), dict(out=m((n, K), (q, pos(j, K))))))
    return cases


def stage_reference(entry, d):
    """The float64 reference of a stage entry on the inputs d (stage_inputs' names, plus prod)."""
    if entry == "ls":
        H, P = ref_ls(d["Yp"], d["X"])
        return dict(H=H, P=P)
    if entry == "mrc":
        return dict(out=ref_mrc(d["Yd"], d["H"], d["P"]))
    if entry == "numerator":
        return dict(num=ref_numerator(d["Yd"], d["H"]))
    if entry == "conj_product":
        return dict(prod=ref_conj_product(d["Yd"], d["H"]))
    if entry == "combine":
        return dict(out=ref_combine(d["prod"], d["P"]))
    if entry == "dist":
        return dict(P=ref_dist(d["H"]))
    raise ValueError(entry)


# ---------------------------------------------------------- rows: FFT, TX

def rows_input(nrows, n, seed=0):
    return tx_cases.rows_of(9000 + seed + n, nrows, n)


def row_placements(nrows, n):
    """(row, column, value): the middle row and the last, first and last element."""
    return [(nrows // 2, 0, NAN), (nrows // 2, n - 1, INF), (nrows - 1, n - 1, NAN), (nrows - 1, n // 2, INF),
            (0, 0, NAN)]


def row_footprint(nrows, ncols, row):
    a = np.zeros((nrows, ncols), bool)
    a[row] = True
    return a


def ref_fft_rows(x, inverse=False):
    with np.errstate(all="ignore"):
        x = x.astype(np.complex128)
        return c64(np.fft.ifft(x, axis=-1) * x.shape[-1] if inverse else np.fft.fft(x, axis=-1))


# ------------------------------------------------------------ zero forcing

# (U, R, K, n): test_zf_apply_detect_parity's and ..._degenerate_shapes' tuples (one per kernel of the dispatch
# table above launch_zf_apply), n cut to at most 9
ZF_SHAPES = [(1, 1, 5, 1), (2, 4, 1023, 7), (3, 5, 64, 9), (4, 16, 1023, 9), (5, 12, 130, 9), (8, 64, 1023, 9),
             (12, 40, 200, 9), (16, 64, 1023, 9), (17, 64, 65, 3), (32, 64, 255, 9), (16, 100, 1023, 8),
             (24, 100, 130, 9)]
ZF_DEGENERATE = [(8, 6, 65, 5), (16, 5, 130, 9), (32, 6, 40, 9), (8, 16, 1, 5), (12, 40, 1, 3), (32, 64, 1, 4)]


def _zf_gemm_tile(M):
    """zf.hip gemm_by_rows: (rows per wave tile, row groups per workgroup), the smallest that holds M rows."""
    return (2, 1) if M <= 2 else (4, 1) if M <= 4 else (8, 1) if M <= 8 else (8, 2) if M <= 16 else (8, 4)


def zf_detect_kernel(U, R, K):
    """The kernel launch_zf_detect runs, by shape alone (zf.hip, `detect`; M = U rows)."""
    if R < 8 or U <= 8:
        return ("k_zf_gemm",) + _zf_gemm_tile(U)
    if R <= 72:
        return ("k_zf_wstat",)
    return ("k_zf_mfma_lds8",) if U > 16 else ("k_zf_mfma_w128",)


def zf_apply_kernel(U, R, K):
    """The kernel launch_zf_apply runs, by shape alone (zf.hip, `launch_zf_apply` and `apply_ws16`; M = R rows)."""
    if K >= 2 and R >= 8:
        return ("k_zf_apply_ws16", 8 if U <= 20 else 4)  # rows per tile
    if 5 <= R < 8 and U >= 8:
        return ("k_zf_gemm_lds",)
    return ("k_zf_gemm",) + _zf_gemm_tile(R)


_GEMM_TILES = [(2, 1), (4, 1), (8, 1), (8, 2), (8, 4)]
ZF_DETECT_KERNELS = {("k_zf_gemm",) + t for t in _GEMM_TILES} | {("k_zf_wstat",), ("k_zf_mfma_lds8",), ("k_zf_mfma_w128",)}
ZF_APPLY_KERNELS = {("k_zf_gemm",) + t for t in _GEMM_TILES} | {("k_zf_gemm_lds",), ("k_zf_apply_ws16", 8),
                                                               ("k_zf_apply_ws16", 4)}


def zf_inputs(U, R, K, n, precoder=True):
    """dict(H (U, R, K), W (K, U, R): the float64 precoder (or, where R < U
    and none exists, a seeded array), X (n, U, K), Y (n, R, K) = W x + noise)."""
    H = zf_cases.channel(U, R, K, seed=n)
    W = c64(zf_cases.zf_numpy(H)) if precoder else np.ascontiguousarray(H.transpose(2, 0, 1))
    X = zf_cases.qpsk(n, U, K, seed=n + 1)
    Y = np.einsum("kur,nuk->nrk", W.astype(np.complex128), X.astype(np.complex128))
    Y = c64(Y + 0.05 * zf_cases.qpsk(n, R, K, seed=n + 2))
    return dict(H=H, W=np.ascontiguousarray(W), X=X, Y=Y)


def zf_cases_of(U, R, K, n):
    """(entry, input name, index, mask over the entry's output): the clamped
    lanes (k = K - 1, n - 1), k = 0, and a middle element.  detect: Y (n, R, K),
    Wt (U, R, K) -> (n, U, K); apply: X (n, U, K), Wt -> (n, R, K)."""
    def m(shape, idx):
        a = np.zeros(shape, bool)
        a[idx] = True
        return a

    A = slice(None)
    cases = []
    for q, k in ((n - 1, K - 1), (0, 0), (n // 2, K // 2)):
        cases.append(("detect", "Y", (q, R - 1 if k else 0, k), m((n, U, K), (q, A, k))))
        cases.append(("apply", "X", (q, U - 1 if k else 0, k), m((n, R, K), (q, A, k))))
    for u, r, k in ((U - 1, R - 1, K - 1), (0, 0, 0)):
        cases.append(("detect", "Wt", (u, r, k), m((n, U, K), (A, u, k))))
        cases.append(("apply", "Wt", (u, r, k), m((n, R, K), (A, r, k))))
    return cases


def zf_precoder_footprint(U, R, K, k):
    """H[u, r, k] reaches subcarrier k's matrix alone: W (K, U, R), Wt (U, R, K)."""
    W = np.zeros((K, U, R), bool)
    W[k] = True
    return dict(W=W, Wt=np.ascontiguousarray(W.transpose(1, 2, 0)))


# ------------------------------------------------------- the scale property

def pow2(k):
    return np.float32(2.0) ** np.float32(k)


def scaled(a, k):
    """a * 2^k, exact while nothing overflows or goes subnormal (asserted)."""
    b = (a * pow2(k)).astype(a.dtype)
    back = (b * pow2(-k)).astype(a.dtype)
    assert np.array_equal(bits(back), bits(a)), f"2^{k} is not exact on this input"
    return b
