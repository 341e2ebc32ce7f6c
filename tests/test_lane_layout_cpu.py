"""csrc/lane_layout.hpp against the documented ownership of every lane order.

The header gives the position of bin b inside one lane-ordered Hc row (the LS
kernels store through it, ofdm_frame_export_estimate reads through it).  A
small program (tests/cpp/lane_layout_table.cpp) built with the host compiler
prints that table for the nine sizes; here each table is rebuilt the other way
round, by walking every (wave, lane, slot) of the receiver and writing down
which bin it owns and where it is stored, with none of the header's inverse
formulas.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd", "csrc")
SIZES = (128, 256, 512, 1024, 1536, 2048, 3072, 4096, 6144)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lane_layout") / "lane_layout_table"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "cpp", "lane_layout_table.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = [np.array(ln.split(), dtype=np.int64) for ln in out.splitlines()]
    return {int(r[0]): r[1:] for r in rows}


def forward(C):
    """pos[b] = position of bin b, from the ownership each receiver documents."""
    pos = np.full(C, -1, dtype=np.int64)
    if C in (1536, 3072, 6144):
        # wave e, lane 8 s + c, slot 8 j + d holds bin 3 (W (s + 8 c + 64 d) + e) + j at e * 1536 + slot * 64 + lane
        W = C // 1536
        e, s, c, j, d = np.meshgrid(np.arange(W), np.arange(8), np.arange(8), np.arange(3), np.arange(8), indexing="ij")
        pos[3 * (W * (s + 8 * c + 64 * d) + e) + j] = e * 1536 + (8 * j + d) * 64 + 8 * s + c
    elif C in (128, 256, 512):
        # slot d of lane-mod-8P 8 s' + c holds bin s' + P c + 8 P d at d * 8 P + 8 s' + c
        P = C // 64
        s, c, d = np.meshgrid(np.arange(P), np.arange(8), np.arange(8), indexing="ij")
        pos[s + P * c + 8 * P * d] = d * 8 * P + 8 * s + c
    else:
        # lane t owns b' = b0(t) + 16 k, b0(t) = (t >> 2) + 256 c(t & 3), c(a) = (a >> 1) + 2 (a & 1)
        t, k = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
        a = t & 3
        bp = (t >> 2) + 256 * ((a >> 1) + 2 * (a & 1)) + 16 * k
        if C == 1024:  # float4 (k >> 1) * 64 + t holds bins (k & ~1, k | 1) of lane t
            pos[bp] = 2 * ((k >> 1) * 64 + t) + (k & 1)
        elif C == 2048:  # float4 k * 64 + t = (Hc[2 b'], Hc[2 b' + 1])
            for h in range(2):
                pos[2 * bp + h] = 2 * (k * 64 + t) + h
        else:  # float2 e * 2048 + h * 1024 + (k >> 1) * 128 + 2 t + (k & 1) = Hc[4 b' + 2 h + e]
            assert C == 4096
            for h in range(2):
                for e in range(2):
                    pos[4 * bp + 2 * h + e] = e * 2048 + h * 1024 + (k >> 1) * 128 + 2 * t + (k & 1)
    return pos


@pytest.mark.parametrize("C", SIZES)
def test_position_table_matches_forward_enumeration(tables, C):
    got, want = tables[C], forward(C)
    assert got.shape == (C,)
    assert np.array_equal(np.sort(want), np.arange(C)), "the enumeration itself covers every position once"
    assert np.array_equal(np.sort(got), np.arange(C)), "hc_pos is not a permutation of [0, C)"
    assert np.array_equal(got, want), f"first mismatch at bin {int(np.argmax(got != want))}"
