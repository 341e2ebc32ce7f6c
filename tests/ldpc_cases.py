"""Shared generators and the integer models of the QC-LDPC decoder's tests
(include/ofdm_lsmrc_ldpc.h).

The model IS the definition of ofdm_ldpc_decode, restated in numpy: layered
min-sum in integers, base rows in order, per check T_j = L[v_j] - R_j, first
minimum, second minimum, mu' = min(127, max(0, ((mu * norm16) >> 4) - offset)),
the sign rule, L clamped to +-16383, the syndrome after an iteration.  `decode`
is vectorised over the Z lanes of a layer and over codewords; `decode_naive`
is the same definition in plain loops, one check at a time, written apart from
it on purpose.  Decoder outputs are compared with the model for equality,
never with a tolerance.

Also here: a seeded generator of codes with base matrix [A | D] (A random with
given row degrees and shifts, D lower-bidiagonal identity circulants, so
encoding is back-substitution), the encoder, and cached noisy cases.  The
quantisers are viterbi_cases's.
"""
import functools
from collections import namedtuple

import numpy as np

from viterbi_cases import pack, quant_f32, quant_i8  # noqa: F401  (re-exported: one definition of each)

Code = namedtuple("Code", "mb nb Z rows")  # rows: per base row a tuple of (column, shift), columns increasing
LCLAMP = 16383
CONTROLS = ((16, 0), (12, 0), (16, 1), (13, 2))  # (norm16, offset) used by the tests


def N(c):
    return c.nb * c.Z


def K(c):
    return (c.nb - c.mb) * c.Z


def nnz(c):
    return sum(len(r) for r in c.rows)


def gen_code(mb, nb, Z, degrees=None, seed=0, shifts=None):
    """[A | D]: row r has degrees[r] entries in all (default: as many as fit up to 3 + 3 in A), of which
    D holds column kb + r and, for r > 0, kb + r - 1, both with shift 0; the others are random columns of A
    with random shifts (or `shifts`, cycled through, for A's entries)."""
    rng = np.random.default_rng([seed, mb, nb, Z])
    kb = nb - mb
    rows, pool = [], []
    for r in range(mb):
        nd = 1 if r == 0 else 2
        deg = degrees[r] if degrees is not None else nd + min(kb, 4)
        da = deg - nd
        assert 0 <= da <= kb and deg >= 2, (r, deg, kb)
        cols = []  # dealt from shuffled decks of A's columns, so that the rows cover them evenly
        while len(cols) < da:
            if not pool:
                pool = rng.permutation(kb).tolist()
            k = next((k for k, v in enumerate(pool) if v not in cols), None)
            if k is None:
                pool += rng.permutation(kb).tolist()
            else:
                cols.append(pool.pop(k))
        cols.sort()
        sh = rng.integers(0, Z, da).tolist() if shifts is None else [shifts[k % len(shifts)] % Z for k in range(da)]
        row = list(zip(cols, sh)) + ([(kb + r - 1, 0)] if r else []) + [(kb + r, 0)]
        rows.append(tuple((int(a), int(b)) for a, b in row))
    return Code(mb, nb, Z, tuple(rows))


def var_index(c, r):
    """[d, Z]: variable of edge j of check r Z + i."""
    i = np.arange(c.Z)
    return np.stack([col * c.Z + (i + sh) % c.Z for col, sh in c.rows[r]])


def encode(c, info):
    """info [ncw, K] of 0 / 1 -> codewords [ncw, N] uint8 of an [A | D] code: p_0 = A_0 s, p_r = A_r s + p_(r-1)."""
    info = np.atleast_2d(np.asarray(info, np.uint8))
    kb, Z = c.nb - c.mb, c.Z
    x = np.zeros((info.shape[0], N(c)), np.uint8)
    x[:, :K(c)] = info
    for r in range(c.mb):
        acc = np.zeros((info.shape[0], Z), np.uint8)
        for j, (col, sh) in enumerate(c.rows[r]):
            if col < kb + r:
                acc ^= x[:, var_index(c, r)[j]]
            else:
                assert col == kb + r and sh == 0, "not an [A | D] code"
        x[:, (kb + r) * Z:(kb + r + 1) * Z] = acc
    return x


def syndrome(c, x):
    """[ncw, M] of 0 / 1: H x."""
    x = np.atleast_2d(np.asarray(x, np.uint8))
    return np.concatenate([np.bitwise_xor.reduce(x[:, var_index(c, r)], axis=1) for r in range(c.mb)], axis=1)


def full_q(c, q, pos0=0):
    """The window q [ncw, n_rx] at positions pos0 .. of the codeword, every other position 0: [ncw, N] int64."""
    q = np.atleast_2d(np.asarray(q)).astype(np.int64)
    full = np.zeros((q.shape[0], N(c)), np.int64)
    assert 0 <= pos0 and pos0 + q.shape[1] <= N(c)
    full[:, pos0:pos0 + q.shape[1]] = q
    return full


def _scale(mu, norm16, offset):
    return np.minimum(127, np.maximum(0, ((mu * norm16) >> 4) - offset))


def decode(c, q, max_iter=20, norm16=12, offset=0, early_stop=True, stats=None):
    """The definition: q [ncw, N] integers in [-127, 127] -> (x [ncw, N] uint8, iters [ncw] int64, +k / -k).
    stats, a dict, receives clamp_hits: how many L updates met the +-16383 clamp."""
    q = np.atleast_2d(np.asarray(q)).astype(np.int64)
    ncw = q.shape[0]
    assert q.shape[1] == N(c) and np.all(np.abs(q) <= 127)
    idxs = [var_index(c, r) for r in range(c.mb)]
    L = q.copy()
    R = [np.zeros((ncw, len(c.rows[r]), c.Z), np.int64) for r in range(c.mb)]
    iters = np.zeros(ncw, np.int64)
    live = np.arange(ncw)  # codewords still iterating
    hits = 0
    for it in range(1, max_iter + 1):
        Lw = L[live]
        for r in range(c.mb):
            v = idxs[r]
            T = Lw[:, v] - R[r][live]  # [n, d, Z]
            a, s = np.abs(T), T < 0
            S = np.bitwise_xor.reduce(s, axis=1, keepdims=True)
            idx = np.argmin(a, axis=1)[:, None, :]  # the first minimum
            min1 = np.take_along_axis(a, idx, axis=1)
            is_idx = np.arange(a.shape[1])[None, :, None] == idx
            min2 = np.where(is_idx, np.int64(1 << 40), a).min(axis=1, keepdims=True)
            mag = _scale(np.where(is_idx, min2, min1), norm16, offset)
            Rn = np.where(S ^ s, -mag, mag)
            new = T + Rn
            hits += int((np.abs(new) > LCLAMP).sum())
            Lw[:, v] = np.clip(new, -LCLAMP, LCLAMP)
            R[r][live] = Rn
        L[live] = Lw
        iters[live] = it
        if early_stop:
            live = live[syndrome(c, Lw < 0).any(axis=1)]
            if live.size == 0:
                break
    x = (L < 0).astype(np.uint8)
    ok = ~syndrome(c, x).any(axis=1)
    if stats is not None:
        stats["clamp_hits"] = hits
    return x, np.where(ok, iters, -iters)


def decode_naive(c, q, max_iter=20, norm16=12, offset=0, early_stop=True):
    """The definition once more, in plain loops: one codeword, one check, one edge at a time."""
    q = np.atleast_2d(np.asarray(q))
    xs, its = [], []
    for w in range(q.shape[0]):
        L = [int(t) for t in q[w]]
        R = {}
        k, zero = 0, False
        while k < max_iter:
            k += 1
            for r in range(c.mb):
                for i in range(c.Z):
                    vs = [col * c.Z + (i + sh) % c.Z for col, sh in c.rows[r]]
                    T = [L[v] - R.get((r, i, j), 0) for j, v in enumerate(vs)]
                    a = [abs(t) for t in T]
                    S = 0
                    for t in T:
                        S ^= t < 0
                    idx = a.index(min(a))
                    min1 = a[idx]
                    min2 = min(a[j] for j in range(len(a)) if j != idx)
                    for j, v in enumerate(vs):
                        mu = min2 if j == idx else min1
                        mu = min(127, max(0, ((mu * norm16) >> 4) - offset))
                        rn = -mu if S ^ (T[j] < 0) else mu
                        L[v] = min(LCLAMP, max(-LCLAMP, T[j] + rn))
                        R[(r, i, j)] = rn
            if early_stop or k == max_iter:
                zero = True
                for r in range(c.mb):
                    for i in range(c.Z):
                        p = 0
                        for col, sh in c.rows[r]:
                            p ^= L[col * c.Z + (i + sh) % c.Z] < 0
                        zero = zero and not p
                if zero and early_stop:
                    break
        xs.append([int(t < 0) for t in L])
        its.append(k if zero else -k)
    return np.array(xs, np.uint8), np.array(its, np.int64)


def packed(x, n_bits):
    """The first n_bits of each row of x, packed as the decoder packs."""
    return pack(np.asarray(x, np.uint8)[:, :n_bits])


def bpsk_llr(x, sigma, rng):
    """BPSK +-1 (bit 0 -> +1) plus Gaussian noise of std sigma -> float32 LLRs 2 y / sigma^2."""
    y = 1.0 - 2.0 * np.asarray(x, np.float64) + sigma * rng.standard_normal(np.shape(x))
    return (2.0 * y / sigma ** 2).astype(np.float32)


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def noisy_case(code, ncw, sigma, seed=0, scale=8.0):
    """A cached case on an [A | D] code: dict of the information bits, the codewords, the float LLRs of all N
    positions and their int8 quantisation at `scale`.  Read only."""
    rng = np.random.default_rng([seed, ncw, code.mb, code.nb, code.Z, int(sigma * 1000)])
    info = rng.integers(0, 2, (ncw, K(code))).astype(np.uint8)
    x = encode(code, info)
    llr = bpsk_llr(x, sigma, rng)
    return _freeze(dict(code=code, info=info, x=x, llr=llr, q=quant_f32(llr, scale), scale=scale))


@functools.lru_cache(maxsize=None)
def reference(code, ncw, sigma, max_iter=20, norm16=12, offset=0, early_stop=True, pos0=0, n_rx=None, seed=0):
    """The model's decode of noisy_case(code, ncw, sigma, seed)'s window (pos0, n_rx): (x, iters).  Read only."""
    k = noisy_case(code, ncw, sigma, seed)
    n_rx = N(code) - pos0 if n_rx is None else n_rx
    x, iters = decode(code, full_q(code, k["q"][:, pos0:pos0 + n_rx], pos0), max_iter, norm16, offset, early_stop)
    x.setflags(write=False)
    iters.setflags(write=False)
    return x, iters


@functools.lru_cache(maxsize=None)
def saturation_case(Z=3):
    """(code, q [3, N] int8, controls).  L[v] = q_v + the sum of the messages into v while nothing is clamped,
    so |L| <= 127 (1 + column degree): the clamp needs a column in 129 rows or more.  160 rows of degree 32
    over 32 columns of A put each of those in about 150.  q is +-127 everywhere: a codeword's signs (every
    check agrees, every message is 127 towards the variable's own sign at plain min-sum, and A's posteriors
    pass 16383 inside the first iteration), with the signs of some positions flipped (conflicting checks:
    the syndrome is not zero at once, and the decoder runs on at the clamp)."""
    c = gen_code(160, 192, Z, degrees=(32,) * 160, seed=3)
    rng = np.random.default_rng(17)
    x = encode(c, rng.integers(0, 2, (3, K(c))))
    flip = rng.random(x.shape) < 0.04
    flip[0] = False  # one codeword with no conflict at all
    q = np.where(x ^ flip, -127, 127).astype(np.int8)
    q.setflags(write=False)
    return c, q, dict(max_iter=3, norm16=16, offset=0, early_stop=False)


# ---- the cases of the GPU tests.  tests/test_ldpc_cpu.py asserts of every NOISY entry that some hard decisions
# are wrong before decoding and that the model alone recovers every codeword in fewer than MAX_ITER iterations,
# so no GPU test's noise level rests on a guess.

SHAPES = ((2, 4), (4, 8), (12, 24))
ZS = (2, 3, 27, 63, 64, 65, 81, 127, 128, 129, 192, 255, 256, 257, 383, 384)
SIGMA = {(2, 4): 0.38, (4, 8): 0.45, (12, 24): 0.45}
MAX_ITER = 20


def grid_ncw(code):
    return max(3, min(64, 2048 // N(code)))


@functools.lru_cache(maxsize=None)
def code_1944():
    """Rate 1/2, N = 1944 (Z = 81, nb = 24), row degrees 7 and 8 as 802.11n's code of that size has."""
    return gen_code(12, 24, 81, degrees=(7,) + (8,) * 11, seed=1)


@functools.lru_cache(maxsize=None)
def special_codes():
    Z = 384
    return {
        "deg2_and_32": gen_code(3, 36, 29, degrees=(2, 32, 32), seed=5),       # row 0: one entry of A and one of D
        "deg19": gen_code(3, 24, 65, degrees=(19, 19, 19), seed=6),
        "shift_ends": gen_code(4, 8, 70, shifts=(0, -1), seed=7),              # shifts 0 and Z - 1 in every row
        "lds_last": gen_code(12, 24, Z, degrees=(10,) * 10 + (11, 11), seed=8),   # 2 N + nnz Z = 170 Z = 65280
        "scratch_first": gen_code(12, 24, Z, degrees=(10,) * 9 + (11,) * 3, seed=8),  # 171 Z = 65664 > 65536
        "nr_sized": gen_code(46, 68, Z, seed=9),                               # 46 x 68 at Z = 384: scratch
        "max_n": gen_code(32, 128, 256, degrees=(9,) + (10,) * 31, seed=10),   # N = 32768: L alone fills 64 KiB of LDS
    }


def _noisy():
    out = {f"grid-{mb}x{nb}-Z{Z}": (gen_code(mb, nb, Z), None, SIGMA[(mb, nb)]) for mb, nb in SHAPES for Z in ZS}
    sp = special_codes()
    out.update({"n1944": (code_1944(), 8, 0.7), "deg2_and_32": (sp["deg2_and_32"], 4, 0.3), "deg19": (sp["deg19"], 3, 0.35),
                "shift_ends": (sp["shift_ends"], 4, 0.38), "lds_last": (sp["lds_last"], 2, 0.6),
                "scratch_first": (sp["scratch_first"], 2, 0.6), "nr_sized": (sp["nr_sized"], 3, 0.45),
                "max_n": (sp["max_n"], 2, 0.38),
                "packed": (gen_code(2, 4, 3), 64, 0.38)})
    return {k: (c, grid_ncw(c) if n is None else n, s) for k, (c, n, s) in out.items()}


NOISY = _noisy()


def case(name):
    """(noisy_case dict, (x, iters) of the model at the default controls) of a NOISY entry."""
    c, ncw, sigma = NOISY[name]
    return noisy_case(c, ncw, sigma), reference(c, ncw, sigma, MAX_ITER)


@functools.lru_cache(maxsize=None)
def layer_order_code(Z=37):
    """The last layer shares every column with the first (and the middle one overlaps both): decoding the
    layers in any other order gives other messages.  Not an [A | D] code: the all-zero word is its codeword."""
    return Code(3, 6, Z, (((0, 3), (1, 0), (2, 11), (3, Z - 1)), ((2, 5), (3, 1), (4, 0), (5, 9)),
                          ((0, 8), (1, 20), (2, 0), (3, 2))))
