"""bench.py's plain run on the GPU: `--steps` timed steps, the headline
fields, nothing of the --full legs, and --dump-outputs holding what the timed
path computed (the same frames demodulated in this process, bit for bit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dump(ofdm, dev, tmp_path):
    import torch
    F, S, R, C, steps, seed = 6, 5, 64, 1024, 3, 1234
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "OFDM_BENCH_SHARE_GPU", "OFDM_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--frames", str(F), "--S", str(S), "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["unit"] == "symbols/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert abs(line["value"] - F * (S - 1) / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    # the --full legs did not run
    assert line["check"] is None and line["clock"] is None and line["cpu_baseline"] is None
    assert "mode_a" not in line and line["roofline"]["box_copy_GBps"] is None
    assert os.listdir(tmp_path / "d") == ["demod.npy"]
    got = np.load(tmp_path / "d" / "demod.npy")
    assert got.dtype == np.float32 and got.shape == (F, S - 1, C - 1, 2)

    # bench.py's inputs from its seed, demodulated here
    rng = np.random.default_rng(seed)
    a = np.float32(0.70710678)
    X = torch.from_numpy((rng.choice([-a, a], C - 1) + 1j * rng.choice([-a, a], C - 1)).astype(np.complex64)).to(dev)
    iq = ofdm.synth_frames(F, S, R, C, X, prefix=0, seed=seed, noise_std=0.01)
    out = ofdm.frame_demod(iq, X, 0)
    torch.cuda.synchronize()
    assert int(ofdm.count_symbol_errors(out, S, seed=seed).item()) == 0
    assert np.array_equal(got, torch.view_as_real(out).cpu().numpy())
