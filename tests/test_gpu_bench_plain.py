"""GPU: a plain `python bench.py --gpus 1 --steps K --warmup W` does what its headline figure needs and no more -- ONE JSON line
with the headline keys and the HIP-event kernel table of its K timed steps, none of the sub-records, checks and baselines that
`--full` adds, and with `--dump-outputs` the (overlap, yaw) of every candidate of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FULL_ONLY = ("warm_serial", "dense_walk", "trained_like", "fp32_mode", "cold", "fullstack", "corr_head", "infer_api", "latency",
             "cpu_baseline", "cpu_baseline_preprocess", "value_dense_walk", "value_trained_like", "overlap_maxerr_vs_oracle",
             "yaw_exact_rate", "accuracy_pairs")


def test_plain_run_is_the_headline_alone(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["metric"] == "scan-pairs/s (64x900 range images)" and r["unit"] == "pairs/s" and r["higher_is_better"] is True
    assert r["dtype"].startswith("f32") and r["steps"] == 3 and r["warmup"] == 1 and r["config"]["full"] is False
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] - 1024 * 1e3) < 1e-6 * 1024 * 1e3
    assert r["kernels"]["delta_c12"]["launches"] == 3                  # the timed steps' own launches, one 1024-pair sweep each
    assert [k for k in FULL_ONLY if k in r] == []
    assert r["roofline"]["traffic"] is None and r["roofline"]["k_walk_frac"] is None
    ov, yw = np.load(tmp_path / "overlap.npy"), np.load(tmp_path / "yaw.npy")
    assert ov.shape == (1024,) and ov.dtype == np.float32 and yw.shape == (1024,) and yw.dtype == np.float64
    assert np.all((ov >= 0) & (ov <= 1)) and np.all((yw > -180) & (yw <= 180))        # a sigmoid; yaw in degrees
