"""GPU: a plain bench.py run is the headline figure and nothing else, and --dump-outputs writes what its last timed step
returned (a small workload: 8 frames of 16 384 points)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DPM_") and k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "8",
           "--points", "16384", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["unit"] == "frames/s"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"].startswith("f32")
    assert abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) <= 1e-2 * line["value"]
    for key in ("roofline", "roofline_mfma", "parity_gate", "cpu_baseline", "sustained", "pcie_inclusive_fps", "latency_mode_ms_per_frame"):
        assert key not in line, key
    desc, edges = np.load(out_dir / "descriptors.npy"), np.load(out_dir / "edges.npy")
    assert desc.dtype == np.float32 and desc.shape == (8, 131, 256) and np.isfinite(desc).all()
    assert edges.dtype == np.float32 and edges.shape == (8, 56) and np.isfinite(edges).all()
