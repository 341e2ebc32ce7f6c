"""Guard bands and exact-size workspaces for the containment tests
(test_containment_gpu.py, self-tested on CPU tensors by test_guard_cpu.py).

Every guarded buffer is one allocation of its own, [band | body | band], a
torch.uint8 tensor on the target device ("cpu" works: the harness is tested
without a GPU).  The body starts at a 256-byte-aligned address plus `offset`,
so a kernel selection that looks at pointer alignment sees what a fresh
tensor shows it (offset 0) or exactly the alignment the header states
(offset = that alignment: address mod 2*align == align).  Each band is at
least 4 KiB and at least one row of the buffer's last dimension.

The whole arena is first filled with BAND_WORD, a quiet NaN with a payload:
anything that reads a band as float is poisoned, and the word is compared bit
for bit as a canary.  An output body is prefilled with FILL_WORD, a second
NaN payload; an input body holds the caller's bytes, of which a snapshot is
kept on the host.  Comparisons are on bytes and 32-bit words, never on
floats (NaN != NaN).

What this sees: any stray WRITE into a band, any body word left unwritten,
any change to an input.  A stray READ is seen only when the value read
reaches an output (as a NaN, or as a difference from the plain run); a
read-ahead whose value is discarded stays invisible.  A body word is four
bytes: of an int8 output, four neighbouring elements left unwritten show, a
single one between written neighbours does not."""
import numpy as np

BAND_WORD = 0x7FC0BEEF  # quiet NaN, payload 0x00BEEF
FILL_WORD = 0x7FC0F111  # quiet NaN, payload 0x00F111
BAND_MIN = 4096
ALIGN = 256

_TORCH = {"complex64": "complex64", "float32": "float32", "int8": "int8", "uint8": "uint8", "int16": "int16",
          "int32": "int32", "int64": "int64", "uint64": "int64"}


def torch_dtype(dtype):
    import torch
    return getattr(torch, _TORCH[np.dtype(dtype).name])


def _pattern(word, nbytes, phase=0):
    """nbytes bytes of the little-endian `word` repeated, starting at byte `phase` of the word."""
    w = np.frombuffer(np.uint32(word).tobytes(), np.uint8)
    return np.resize(np.roll(w, -phase), nbytes) if nbytes else np.empty(0, np.uint8)


def _up(n, a):
    return (n + a - 1) // a * a


class Guarded:
    """One guarded buffer (see the module docstring).  .view is the body as a
    contiguous tensor of `shape` and `dtype`; .arena the whole allocation."""

    def __init__(self, shape, dtype, dev, offset=0, fill=None, band=None):
        import torch
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in shape)
        self.shape, self.dtype, self.offset = shape, dtype, int(offset)
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        assert offset % 4 == 0 and 0 <= offset <= ALIGN and offset % min(dtype.itemsize, 16) == 0, offset
        grid = ALIGN if offset < ALIGN else 2 * ALIGN  # offset == ALIGN: 256-byte aligned and no more
        row = (shape[-1] if shape else 1) * dtype.itemsize
        self.band = _up(max(BAND_MIN, row, band or 0), ALIGN)
        total = self.band + grid + offset + _up(self.nbytes, 4) + self.band + ALIGN
        self.arena = torch.empty(total, dtype=torch.uint8, device=dev)
        base = self.arena.data_ptr()
        assert base % 16 == 0, "the allocator returned a pointer that is not 16-byte aligned"
        self.lo = _up(base + self.band, grid) - base + offset
        self.hi = self.lo + self.nbytes
        self.arena.view(torch.int32).fill_(BAND_WORD)
        body = self.arena[self.lo:self.hi]
        self.is_input = fill is not None
        if fill is None:
            image = _pattern(FILL_WORD, self.nbytes)
        else:
            a = fill.detach().cpu().numpy() if isinstance(fill, torch.Tensor) else np.asarray(fill)
            a = np.ascontiguousarray(a)
            assert a.dtype == dtype and a.shape == shape, (a.dtype, a.shape, dtype, shape)
            image = a.reshape(-1).view(np.uint8)
        self.snapshot = image.copy()
        if self.nbytes:
            body.copy_(torch.from_numpy(self.snapshot.copy()).to(dev))
        self.view = body.view(torch_dtype(dtype)).view(shape) if self.nbytes else torch.empty(
            shape, dtype=torch_dtype(dtype), device=dev)
        if self.nbytes:
            assert self.view.data_ptr() == base + self.lo and self.view.is_contiguous()

    # ---- what the arena holds now, on the host
    def _host(self):
        return self.arena.detach().cpu().numpy()

    def body_bytes(self):
        return self._host()[self.lo:self.hi].copy()

    def address(self):
        return self.arena.data_ptr() + self.lo

    # ---- the assertions
    def assert_bands(self, what="buffer"):
        a = self._host()
        for name, lo, hi in (("before", 0, self.lo), ("after", self.hi, a.size)):
            bad = np.flatnonzero(a[lo:hi] != _pattern(BAND_WORD, hi - lo, lo % 4))
            if bad.size:
                d = bad + lo - (self.lo if name == "before" else self.hi)
                raise AssertionError(f"{what}: {bad.size} band byte(s) {name} the body changed, at byte offsets "
                                     f"{d[:8].tolist()} from the body's {'start' if name == 'before' else 'end'}")

    def unwritten(self):
        """Indices of the body's 32-bit words (a ragged tail of fewer than four
        bytes counts as the last word) that still hold the prefill."""
        b = self.body_bytes()
        n4 = self.nbytes // 4
        idx = np.flatnonzero(b[:4 * n4].view(np.uint32) == np.uint32(FILL_WORD))
        tail = self.nbytes - 4 * n4
        if tail and np.array_equal(b[4 * n4:], _pattern(FILL_WORD, tail)):
            idx = np.append(idx, n4)
        return idx

    def assert_unmodified(self, what="input", mask=None):
        """The body against the snapshot taken at creation (or by freeze()),
        byte for byte; mask (bool per byte, True = compare) leaves bytes out."""
        b = self.body_bytes()
        diff = b != self.snapshot
        if mask is not None:
            diff &= mask
        bad = np.flatnonzero(diff)
        if bad.size:
            raise AssertionError(f"{what}: {bad.size} byte(s) modified, first at byte offsets {bad[:8].tolist()}")

    def freeze(self):
        """From now on the body is an input: snapshot what it holds."""
        self.snapshot = self.body_bytes()
        self.is_input = True
        return self

    def element_words(self, mask):
        """A bool mask over the elements of `shape` -> the indices of their body words."""
        assert self.dtype.itemsize % 4 == 0
        m = np.repeat(np.asarray(mask, bool).reshape(-1), self.dtype.itemsize // 4)
        return np.flatnonzero(m)


def guarded(shape, dtype, dev, offset=0, fill=None):
    """offset: 0, or the alignment the body is to have and no more (4, 8, 16, ... 256)."""
    return Guarded(shape, dtype, dev, offset=offset, fill=fill)


class GuardedWorkspace(Guarded):
    """A frame workspace of exactly ofdm_frame_workspace_bytes bytes, 256-byte
    aligned, between bands.  The library's registry is keyed by address:
    release() (also run by `with` and by the finaliser) drops the entry."""

    def __init__(self, F, S, R, C, dev, offset=0):
        import ofdm_lsmrc as ofdm
        import weakref
        n = ofdm.workspace_bytes(F, S, R, C)
        assert n > 0, (F, S, R, C)
        assert offset in (0, ALIGN), "a workspace is 256-byte aligned"
        super().__init__((n,), np.uint8, dev, offset=offset)
        self.geom = (F, S, R, C)
        self._fin = weakref.finalize(self, ofdm.workspace_release, self.address())

    def release(self):
        self._fin()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False

    # the pieces, in the order the header lists them (256-byte-aligned each)
    def pieces(self):
        F, S, R, C = self.geom
        hc, p, fl = _up(F * R * C * 8, 256), _up(F * C * 4, 256), _up(F * 8, 256)
        return {"Hc": (0, F * R * C * 8), "P": (hc, hc + F * C * 4), "flags": (hc + p, hc + p + F * 8),
                "tickets": (hc + p + fl, hc + p + fl + 4096)}

    def ticket_mask(self):
        """bool per body byte, False over the 4 KiB work-ticket area (which
        the ticketed entries write, ofdm_symbols_demod's const d_ws included)."""
        m = np.ones(self.nbytes, bool)
        lo, hi = self.pieces()["tickets"]
        m[lo:hi] = False
        return m


def guarded_workspace(F, S, R, C, dev, offset=0):
    return GuardedWorkspace(F, S, R, C, dev, offset=offset)


def poison_prefix(iq, prefix):
    """A copy of host frames whose first `prefix` samples of every row are
    poisoned: complex64 (..., C + prefix) gets BAND_WORD in both halves (a NaN
    that any use carries to an output); sc16, int16 (..., C + prefix, 2), cannot
    hold a NaN and gets +-32767, alternating."""
    a = np.array(iq, order="C")
    if prefix == 0:
        return a
    if a.dtype == np.complex64:
        a.view(np.uint32).reshape(a.shape + (2,))[..., :prefix, :] = BAND_WORD
    elif a.dtype == np.int16 and a.shape[-1] == 2:
        sign = np.where(np.arange(prefix) % 2 == 0, 32767, -32767).astype(np.int16)
        a[..., :prefix, 0] = sign
        a[..., :prefix, 1] = -sign
    else:
        raise TypeError(f"poison_prefix: {a.dtype} {a.shape}")
    return a
