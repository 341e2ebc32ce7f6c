"""Shared generators and the integer model of the Viterbi decoder's tests
(include/ofdm_lsmrc_decode.h).

The model IS the definition of ofdm_viterbi_decode, restated in numpy:
vectorised over codewords and the 64 states, a loop over the steps.  State s_t
holds u_(t-1) at bit 5 .. u_(t-6) at bit 0; register r = (u_t << 6) | s_t;
coded bit c_i = parity(r & g[i]); next state r >> 1.  Branch metric
sum_i (1 - 2 c_i) q(t, i), maximised; at step t state s' has the candidates
b = 0, 1 with r = (s' << 1) | b, predecessor r & 63; the larger survives, b = 0
on equality; only paths from state 0 exist (the others carry -2^40 in int64,
below every real metric by far and gone after six steps); end state 0 when
terminated, else the best state, lowest index on equality.  Decoder outputs are
compared with it for equality, never with a tolerance.

Also here: the encoder, the quantisers of both LLR formats, and cached cases.
"""
import functools
from collections import namedtuple

import numpy as np

Code = namedtuple("Code", "n_out g terminated p mask")

G2, G3 = (0o133, 0o171), (0o133, 0o171, 0o165)
KINDS = {"half": (2, G2, 0, 0), "third": (3, G3, 0, 0), "r23": (2, G2, 2, 0x7), "r34": (2, G2, 3, 0x27)}
# noise std at which the model decodes L ~ 1000 of BPSK +-1 without error (LLR = 2 x / sigma^2, scale 8)
SIGMA = {"half": 0.7, "third": 0.95, "r23": 0.55, "r34": 0.45}
NEG = -(1 << 40)


def code(kind, terminated=True):
    n, g, p, mask = KINDS[kind]
    return Code(n, g, int(bool(terminated)), p, mask)


def to_c(ofdm, c):
    return ofdm.ConvCode(c.n_out, c.g, c.terminated, c.p, c.mask)


def steps(c, L):
    return L + 6 if c.terminated else L


def sent_mask(c, T):
    """[T, n_out] bool: mother position (t, i) was sent."""
    if c.p == 0:
        return np.ones((T, c.n_out), bool)
    t = np.arange(T)[:, None] % c.p
    i = np.arange(c.n_out)[None, :]
    return ((c.mask >> (t * c.n_out + i)) & 1).astype(bool)


def coded_len(c, L):
    return int(sent_mask(c, steps(c, L)).sum())


def _parity(x):
    x = np.asarray(x)
    r = np.zeros_like(x)
    for k in range(7):
        r ^= (x >> k) & 1
    return r


def encode(c, bits, punctured=True):
    """bits [ncw, L] of 0 / 1 -> the coded bits, uint8: the n_rx sent ones in
    stream order [ncw, n_rx], or all of them [ncw, T, n_out]."""
    bits = np.atleast_2d(np.asarray(bits, np.int64))
    ncw, L = bits.shape
    T = steps(c, L)
    u = np.zeros((ncw, T + 6), np.int64)  # six zeros in front (start state 0), the zero tail behind
    u[:, 6:6 + L] = bits
    r = np.zeros((ncw, T), np.int64)
    for d in range(7):  # bit 6 - d of r_t is u_(t-d)
        r |= u[:, 6 - d:6 - d + T] << (6 - d)
    mother = np.stack([_parity(r & g) for g in c.g[:c.n_out]], axis=-1).astype(np.uint8)
    return mother[:, sent_mask(c, T)] if punctured else mother


def quant_f32(llr, scale):
    """OFDM_LLR_F32's q: clamp(rint(llr * scale), -127, 127) in float32, ties to even, NaN -> 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(llr, np.float32) * np.float32(scale)
    x = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(-127), np.float32(127)))
    return np.rint(x).astype(np.int8)


def quant_i8(v):
    """OFDM_LLR_I8's q: max(value, -127)."""
    return np.maximum(np.asarray(v, np.int8), np.int8(-127))


def full_q(c, q, L):
    """The stream q [ncw, n_rx] placed at its mother positions [ncw, T, n_out], unsent ones 0."""
    q = np.atleast_2d(np.asarray(q)).astype(np.int64)
    T = steps(c, L)
    sent = sent_mask(c, T)
    assert q.shape[1] == sent.sum(), (q.shape, sent.sum())
    full = np.zeros((q.shape[0], T, c.n_out), np.int64)
    full[:, sent] = q
    return full


def correlation(c, bits, q, L):
    """sum (1 - 2 c_j) q_j over the received positions, c the encoding of bits [ncw, L], tail included."""
    cb = encode(c, bits, punctured=False).astype(np.int64)
    return ((1 - 2 * cb) * full_q(c, q, L)).sum(axis=(1, 2))


def decode_bits(c, q, L):
    """The definition: q [ncw, n_rx] integers in [-127, 127] ->
    (u [ncw, L] of 0 / 1, metric [ncw] int64)."""
    full = full_q(c, q, L)
    ncw, T, _ = full.shape
    s = np.arange(64)
    sg = np.empty((2, c.n_out, 64), np.int64)  # branch signs of state s', candidate b
    for b in range(2):
        r = (s << 1) | b
        for i in range(c.n_out):
            sg[b, i] = 1 - 2 * _parity(r & c.g[i])
    pm = np.full((ncw, 64), NEG, np.int64)
    pm[:, 0] = 0
    words = np.empty((T, ncw), np.uint64)  # bit s' of words[t]: the surviving candidate of state s' at step t
    chunk = max(1, (1 << 22) // (ncw * 64))  # the branch metrics of `chunk` steps at a time
    for t0 in range(0, T, chunk):
        bm0, bm1 = full[:, t0:t0 + chunk, :] @ sg[0], full[:, t0:t0 + chunk, :] @ sg[1]  # [ncw, steps, 64]
        for k in range(bm0.shape[1]):
            # states s' and s' + 32 share the predecessors 2 s' & 63 (b = 0) and 2 s' + 1 & 63 (b = 1)
            even, odd = pm[:, 0::2], pm[:, 1::2]
            c0 = np.concatenate((even, even), axis=1) + bm0[:, k]
            c1 = np.concatenate((odd, odd), axis=1) + bm1[:, k]
            d = c1 > c0
            pm = np.where(d, c1, c0)
            words[t0 + k] = np.packbits(d, axis=1, bitorder="little").view("<u8")[:, 0]
    end = np.zeros(ncw, np.int64) if c.terminated else np.argmax(pm, axis=1)  # argmax: the first maximum
    metric = pm[np.arange(ncw), end]
    u = np.empty((ncw, T), np.uint8)
    st = end.astype(np.uint64)
    for t in range(T - 1, -1, -1):
        u[:, t] = st >> np.uint64(5)
        b = (words[t] >> st) & np.uint64(1)
        st = ((st << np.uint64(1)) | b) & np.uint64(63)
    assert np.all(metric > NEG // 2)
    return u[:, :L], metric


def pack(u):
    """Bit t of a row -> bit t & 7 of byte t >> 3."""
    return np.packbits(np.asarray(u, np.uint8), axis=1, bitorder="little")


def decode(c, q, L):
    """(packed bits [ncw, ceil(L/8)] uint8, metric [ncw] int64) of the definition."""
    u, metric = decode_bits(c, q, L)
    return pack(u), metric


def bpsk_llr(c, bits, sigma, rng):
    """BPSK +-1 (bit 0 -> +1) plus Gaussian noise of std sigma -> float32 LLRs 2 x / sigma^2 of the sent positions."""
    cb = encode(c, bits).astype(np.float64)
    x = 1.0 - 2.0 * cb + sigma * rng.standard_normal(cb.shape)
    return (2.0 * x / sigma ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def noisy_case(kind, terminated, L, ncw, sigma=None, seed=0, scale=8.0):
    """A cached case: dict of the code, the information bits [ncw, L], the
    float LLRs, their int8 quantisation at `scale`, and the model's decode of
    it (packed bits, metric).  Read only."""
    c = code(kind, terminated)
    rng = np.random.default_rng([seed, L, ncw, int(terminated), sorted(KINDS).index(kind)])
    bits = rng.integers(0, 2, (ncw, L)).astype(np.uint8)
    llr = bpsk_llr(c, bits, SIGMA[kind] if sigma is None else sigma, rng)
    q = quant_f32(llr, scale)
    packed, metric = decode(c, q, L)
    out = dict(code=c, bits=bits, llr=llr, q=q, packed=packed, metric=metric, scale=scale)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
