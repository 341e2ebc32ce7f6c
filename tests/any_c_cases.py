"""The any-length FFT's plans (csrc/fft_any_plan.hpp, fft_any.hip): a
restatement of the planner's ordering rule, the classes of work the five
kernels do for a length C, and the lengths the GPU tests run.

plan(C) is written from the comment above make_plan, not from its code.  The
class functions are functions of C alone (through plan(C) and the CAP / NT the
header gives the length).  The lists at the end are literals;
tests/test_any_c_plan_cpu.py proves over C = 2 ... 8192 that they reach every
class, so tests/test_any_c_plans_gpu.py needs no planner logic of its own.
CPU only: nothing here imports a GPU module."""

C_MIN, C_MAX = 2, 8192
PRIME = "prime"  # the radix kind of a prime above 8 (stage_any, last_mac_any)


def factors(C):
    """prime factors of C, ascending, with multiplicity"""
    out, p = [], 2
    while p * p <= C:
        while C % p == 0:
            out.append(p)
            C //= p
        p += 1
    if C > 1:
        out.append(C)
    return out


def plan(C):
    """Radices in stage order: primes above 8 first, ascending; then the 8s,
    the 7s and the 5s; a 4 when two factors of 2 are left over; the 3s; a 2
    when one factor of 2 is left over.  A pure power of 8 beside primes above
    8 only ends in 4 x 2 in place of its last 8."""
    f = factors(C)
    big = [p for p in f if p > 8]
    twos = f.count(2)
    eights, left = divmod(twos, 3)
    tail = [[], [2], [4]][left]
    if left == 0 and eights and not any(p in (3, 5, 7) for p in f):
        eights -= 1
        tail = [4, 2]
    four, two = [r for r in tail if r == 4], [r for r in tail if r == 2]
    return big + [8] * eights + [7] * f.count(7) + [5] * f.count(5) + four + [3] * f.count(3) + two


def make_fdiv(d):
    """(m, l) with n // d == (((n * m) >> 32) + n) >> l for n < 2^24: l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1"""
    l = (d - 1).bit_length()
    return ((1 << 32) * ((1 << l) - d)) // d + 1, l


def cap_of(C):
    """the LDS variant that takes C.  Restated, with nt_of, because the class
    functions and the GPU file (its rows per group, G = CAP // C) need them
    where the table program is not built; test_any_c_plan_cpu.py holds both to
    the program's CAP and NT for every length"""
    return 2048 if C <= 2048 else 4096 if C <= 4096 else 8192


def nt_of(cap):
    return 256 if cap <= 4096 else 512


def kind(p):
    return p if p <= 8 else PRIME


# lengths whose fft_rows does not come to k_fft_any (k_fft_rows takes 4 ... 4096)
FFT_ROWS_POW2 = frozenset(1 << k for k in range(2, 13))
# lengths whose frame_demod does not come to k_mrc_any: the fused receivers
# (1024, 2048, 4096) and the lane-order family of frame_td_fft512.hip
NOT_MRC_ANY = frozenset((128, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144))


def stage_classes(C):
    """{(CAP, radix kind, position)} over every stage of the plan; position is
    only / first / middle / last.  First: Lp = 1, no twiddles; last: natural
    order out, the stage k_mrc_any fuses with the combine."""
    p = plan(C)
    n = len(p)
    pos = lambda s: "only" if n == 1 else "first" if s == 0 else "last" if s == n - 1 else "middle"
    return {(cap_of(C), kind(r), pos(s)) for s, r in enumerate(p)}


def last_class(C):
    """(CAP, kind of the last radix, accumulator slots used) of k_mrc_any: a
    thread owns ceil(cp / NT) butterflies of P bins, cp = C / P (P <= 7), or
    ceil(C / NT) single bins behind a prime above 8.  None where frame_demod
    does not come to k_mrc_any."""
    if C in NOT_MRC_ANY:
        return None
    P = plan(C)[-1]
    cp = C // P if P <= 8 else C
    cap = cap_of(C)
    return cap, kind(P), -(-cp // nt_of(cap))


def group_class(C, R):
    """kind of the last radix where the R antenna rows of a symbol make
    several LDS groups of G = CAP // C >= 2 rows with a ragged last one"""
    if C in NOT_MRC_ANY:
        return None
    G = cap_of(C) // C
    return kind(plan(C)[-1]) if 2 <= G < R and R % G else None


def wanted_last_classes():
    """for every reachable (CAP, kind): its smallest and its largest slot count"""
    seen = {}
    for C in range(C_MIN, C_MAX + 1):
        c = last_class(C)
        if c:
            seen.setdefault(c[:2], set()).add(c[2])
    return {k + (s,) for k, v in seen.items() for s in (min(v), max(v))}


# ----------------------------------------------------------------- the lists
# Chosen by a greedy cover over C = 2 ... 8192 (the length that reaches the
# most classes not yet reached, the smallest such length first) and recorded
# here as literals; test_any_c_plan_cpu.py asserts what they reach.

# fft_rows (k_fft_any): every stage class a length outside FFT_ROWS_POW2
# reaches, 2187 / 2916 / 4374 the only lengths of theirs; 121 = 11 * 11 (a
# prime stage twice), 704 = 11 * 8 * 4 * 2 (a prime stage before the tail of a
# pure power of 8)
STAGE_LENGTHS = [2, 3, 5, 6, 7, 11, 12, 35, 49, 121, 484, 704, 896, 900, 2051, 2052, 2053, 2057, 2187, 2205, 2240, 2288,
                 2500, 2916, 4097, 4099, 4108, 4109, 4140, 4374, 4375, 4480, 4500]

# frame_demod (k_mrc_any): (CAP, last kind) at its fewest and its most slots.
# The fewest at the smallest length; the most at the largest length of the
# class (the top of the accumulator budget) whose oracle DFT, C * (the sum of
# C's prime factors) terms per row, stays at or under 4e6 (about a second for
# a 2 x 3 x 4 batch): 8189 = 19 * 431, 8183 = 7 * 7 * 167, 4088 = 73 * 8 * 7,
# 4085 = 43 * 19 * 5; 8165 = 71 * 23 * 5 stands for 8185 = 1637 * 5 (1.3e7),
# 8184 = 31 * 11 * 8 * 3 for 8187 = 2729 * 3, 4064 = 127 * 8 * 4 for
# 4084 = 1021 * 4: the same slot counts.
LAST_LENGTHS = [2, 3, 4, 5, 7, 11, 2023, 2043, 2044, 2045, 2046, 2047, 2049, 2050, 2051, 2053, 2060, 2065, 4064, 4085, 4087,
                4088, 4094, 4095, 4097, 4098, 4100, 4101, 4105, 4109, 8165, 8183, 8184, 8188, 8189, 8192]

# one prime length per variant: no stage before the fused one (4099 is the
# smallest there is for CAP 8192; its oracle is the slowest of the file)
ONLY_LENGTHS = [11, 2053, 4099]

# the tails of the pure powers of two, [4, 2] and [8, 4, 2] (a pure power of 8
# ends in 4 x 2 in place of its last 8): fft_rows gives these lengths to
# k_fft_rows, frame_demod brings them to k_fft_any (pilot rows) and k_mrc_any
POW2_TAIL_LENGTHS = [8, 64]

# (C, R): 2 <= G < R, R % G != 0, one per last-radix kind
GROUP_CASES = [(513, 4), (514, 4), (515, 4), (517, 4), (524, 4), (539, 4)]

# prefix = 0 once per variant (every other frame_demod case: prefix 3)
NO_PREFIX = [2046, 4094, 8188]

# the numerator store (mode 1): one length per last-radix kind
NUMERATOR_LENGTHS = [513, 514, 515, 517, 524, 539]

# k_tx_any, k_denoise_any, k_acquire_any: per variant a plan with a prime above
# 8, a 7 and a 5 (770 = 11 * 7 * 5 * 2, 2310 = 11 * 7 * 5 * 3 * 2,
# 8190 = 13 * 7 * 5 * 3 * 3 * 2), and 49 = 7 * 7
CALLER_LENGTHS = [49, 770, 2310, 8190]
