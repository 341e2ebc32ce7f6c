"""csrc/fft_any_plan.hpp against the rule it documents, for every length.

A small program (tests/cpp/fft_any_plan_table.cpp) built with the host
compiler prints make_plan's result for C = 2 ... 8192 and checks the device's
magic-number division in the host's arithmetic.  Here every line is held to
any_c_cases.plan (the ordering rule restated from the comment above
make_plan), the divisors to the stage sizes, and the claims fft_any.hip makes
in comments to the numbers: the accumulator slots of k_mrc_any, the twiddle
tables, the last radix.  CAP, NT and MAX_STAGES are read from the program's
output.  Then the classes of any_c_cases.py are enumerated over all 8191
lengths and the literal case lists of the GPU tests are shown to reach every
one of them.  CPU only."""
import os
import subprocess

import pytest

import any_c_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd", "csrc")
LENGTHS = range(ac.C_MIN, ac.C_MAX + 1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("fft_any_plan") / "fft_any_plan_table"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "cpp", "fft_any_plan_table.cpp"), "-o", str(path)], check=True)
    return str(path)


@pytest.fixture(scope="module")
def table(exe):
    """MAX_STAGES and {C: dict(cap, nt, G, ns, p, div = [(cp, Lp, L) as (m, l)] per stage, dC)}"""
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    head = lines[0].split()
    assert head[0] == "MAX_STAGES"
    rows = {}
    for ln in lines[1:]:
        assert "refused" not in ln, ln
        a, p, d, dc = (list(map(int, part.split())) for part in ln.split("|"))
        C, cap, nt, G, ns = a
        assert len(d) == 6 * len(p) and len(dc) == 2
        div = [tuple((d[6 * s + 2 * k], d[6 * s + 2 * k + 1]) for k in range(3)) for s in range(len(p))]
        rows[C] = dict(cap=cap, nt=nt, G=G, ns=ns, p=p, div=div, dC=tuple(dc))
    return int(head[1]), rows


def ceil_div(a, b):
    return -(-a // b)


def test_every_length_has_a_plan(table):
    assert sorted(table[1]) == list(LENGTHS)


def test_radices_follow_the_ordering_rule(table):
    max_stages, rows = table
    for C in LENGTHS:
        r = rows[C]
        want = ac.plan(C)
        assert r["p"] == want, (C, r["p"], want)
        prod = 1
        for p in r["p"]:
            prod *= p
        assert prod == C and r["ns"] == len(r["p"]) <= max_stages, C
        big = [p for p in r["p"] if p > 8]
        assert all(ac.factors(p) == [p] for p in big), (C, "a radix above 8 that is no prime")


def test_variant_and_rows_per_group(table):
    _, rows = table
    for C in LENGTHS:
        r = rows[C]
        assert r["cap"] in (2048, 4096, 8192) and r["cap"] >= C, C
        assert r["cap"] == 2048 or C > r["cap"] // 2, (C, "a smaller variant holds this length")
        assert r["G"] == r["cap"] // C >= 1, C
        # the restatement the class functions and the GPU file use is the program's, for every length
        assert (r["cap"], r["nt"]) == (ac.cap_of(C), ac.nt_of(ac.cap_of(C))), C


def test_divisors_are_the_stage_sizes(table):
    _, rows = table
    for C in LENGTHS:
        r = rows[C]
        assert r["dC"] == ac.make_fdiv(C), C
        Lp = 1
        for p, (dcp, dLp, dL) in zip(r["p"], r["div"]):
            assert dcp == ac.make_fdiv(C // p), (C, p, "C / p")
            assert dLp == ac.make_fdiv(Lp), (C, p, "the product of the earlier radices")
            assert dL == ac.make_fdiv(Lp * p), (C, p, "that product times p")
            Lp *= p


def test_last_radix_is_never_8(table):
    """last_mac<8> and store_acc<8> of k_mrc_any are unreachable"""
    _, rows = table
    assert not [C for C in LENGTHS if rows[C]["p"][-1] == 8]


def test_accumulator_slots_hold_every_last_stage(table):
    """k_mrc_any: NACC = CAP / NT + 8 slots, NACC / P butterflies of P bins per
    thread (last_mac), or NACC single bins behind a prime above 8 (last_mac_any)"""
    _, rows = table
    for C in LENGTHS:
        r = rows[C]
        nacc = r["cap"] // r["nt"] + 8
        P = r["p"][-1]
        if P <= 7:
            assert ceil_div(C // P, r["nt"]) <= nacc // P, (C, P)
        else:
            assert ceil_div(C, r["nt"]) <= nacc, (C, P)


def test_twiddle_indices_stay_inside_the_tables(table):
    """W_C^e = lo[e % 64] * hi[e // 64] with C / 64 (rounded up) <= 128 entries
    of hi: every index a stage forms is below C"""
    _, rows = table
    for C in LENGTHS:
        assert ceil_div(C, 64) <= 128, C
        Lp = 1
        for p in rows[C]["p"]:
            L = Lp * p
            if p <= 8:
                assert (p - 1) * (Lp - 1) * (C // L) < C, (C, p, "twiddle_powers: t * k1 * M")
                assert (p - 1) * (C // p) < C, (C, p, "the roots: j * C / p")
            else:
                assert (L - 1) * (C // L) < C, (C, p, "stage_any: e * M, e < L")
            Lp = L


def test_division_is_exact(exe):
    """every d in 1 ... 8192, every n < 16384 and the two largest n below 2^24 at a multiple of d"""
    out = subprocess.run([exe, "fdiv"], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["mismatches", "0"], out


# ------------------------------------------------------------ what the lists reach

def test_stage_lengths_reach_every_stage_class():
    reachable, by_fft_rows = set(), set()
    for C in LENGTHS:
        reachable |= ac.stage_classes(C)
        if C not in ac.FFT_ROWS_POW2:
            by_fft_rows |= ac.stage_classes(C)
    assert len(reachable) == 61 and len(by_fft_rows) == 60
    # a single radix-4 stage is C = 4 alone, which fft_rows gives to k_fft_rows:
    # frame_demod's pilot rows come to k_fft_any at every length
    assert reachable - by_fft_rows == {(2048, 4, "only")} and 4 in ac.LAST_LENGTHS
    assert not set(ac.STAGE_LENGTHS) & ac.FFT_ROWS_POW2
    got = set().union(*(ac.stage_classes(C) for C in ac.STAGE_LENGTHS))
    assert got == by_fft_rows, sorted(by_fft_rows - got, key=str)
    # the classes a single length reaches
    for cls, only in (((4096, 3, "first"), [2187]), ((4096, 4, "first"), [2916]), ((8192, 3, "first"), [4374, 6561])):
        assert [C for C in LENGTHS if cls in ac.stage_classes(C)] == only
    assert ac.plan(121) == [11, 11] and ac.plan(704) == [11, 8, 4, 2]
    assert {121, 704} <= set(ac.STAGE_LENGTHS)


def test_last_lengths_reach_every_last_stage_class():
    want = ac.wanted_last_classes()
    kinds = {c[:2] for c in want}
    assert kinds == {(cap, k) for cap in (2048, 4096, 8192) for k in (2, 3, 4, 5, 7, ac.PRIME)}
    assert len(want) == 36 and len(ac.LAST_LENGTHS) <= 36
    assert not set(ac.LAST_LENGTHS) & ac.NOT_MRC_ANY
    got = {ac.last_class(C) for C in ac.LAST_LENGTHS}
    assert want <= got, sorted(want - got, key=str)
    # every slot of the budget: 3 of 3 and 2 of 2 at radix 7, 4 of 4 at radix 5
    for cls in ((4096, 7, 3), (8192, 7, 3), (2048, 7, 2), (4096, 5, 4), (8192, 5, 4)):
        cap = cls[0]
        assert cls in got and cls[2] == (cap // ac.nt_of(cap) + 8) // cls[1]
    # no stage before the fused one, in each variant
    assert [(ac.cap_of(C), ac.plan(C)) for C in ac.ONLY_LENGTHS] == [(2048, [11]), (4096, [2053]), (8192, [4099])]
    assert sorted(ac.cap_of(C) for C in ac.NO_PREFIX) == [2048, 4096, 8192] and set(ac.NO_PREFIX) <= set(ac.LAST_LENGTHS)
    # the tails of the pure powers of two, which fft_rows never brings to k_fft_any
    assert ac.POW2_TAIL_LENGTHS == [8, 64] and ac.plan(8) == [4, 2] and ac.plan(64) == [8, 4, 2]
    assert set(ac.POW2_TAIL_LENGTHS) <= ac.FFT_ROWS_POW2 and not set(ac.POW2_TAIL_LENGTHS) & ac.NOT_MRC_ANY


def test_group_cases_reach_every_last_kind():
    got = {ac.group_class(C, R) for C, R in ac.GROUP_CASES}
    assert None not in got and got == {2, 3, 4, 5, 7, ac.PRIME}
    assert {ac.kind(ac.plan(C)[-1]) for C in ac.NUMERATOR_LENGTHS} == got
    assert not set(ac.NUMERATOR_LENGTHS) & ac.NOT_MRC_ANY


def test_caller_lengths_mix_a_prime_a_7_and_a_5():
    caps = set()
    for C in ac.CALLER_LENGTHS:
        p = ac.plan(C)
        if C == 49:
            assert p == [7, 7]
            continue
        assert p[0] > 8 and 7 in p and 5 in p, (C, p)
        caps.add(ac.cap_of(C))
    assert caps == {2048, 4096, 8192}
