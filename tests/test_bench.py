"""bench.py's two kinds of run: a plain run measures the headline and nothing else, `--full` adds the checks and legs."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT


def test_full_is_off_by_default(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not bench.parse_args().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--no-single", "--no-config5", "--no-round5-legs"])
    a = bench.parse_args()
    assert a.full and a.no_cpu_baseline and a.no_single and a.no_config5 and a.no_round5_legs


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only(tmp_path):
    batch, iters, steps = 512, 200, 2
    env = dict(os.environ)
    env.pop("TINYMPC_LAYOUT", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch-per-gpu", str(batch), "--iters", str(iters), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)  # a child process: nothing is exec'ed over this one
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["value"] > 0 and out["unit"] == "ADMM iters/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] == pytest.approx(batch * iters * steps / (out["ms_per_step"] * 1e-3 * steps), rel=1e-9)
    assert out["summary"]["instances"] == batch and out["summary"]["total_iterations"] == batch * iters
    # nothing of --full: no reference comparison, no CPU baseline, no leg
    assert out["parity_check"] is None and out["process_group"] is None
    for key in ("cpu_baseline", "gpu_over_cpu", "config5_single_gpu", "converging_batch", "single_instance", "setup", "batched_tick"):
        assert key not in out, key
    assert list(out["legs"]) == ["value_as_asked"] and not [k for k in out["roofline"] if k.startswith("leg_")]
    # ... and what --dump-outputs writes
    d = out["dump_outputs"]
    assert d["instances"] == batch and not d["sampled"]
    states = np.load(tmp_path / "out" / "states.npy")
    assert states.shape == (12, 50, batch) and np.all(np.isfinite(states))
    assert np.array_equal(np.load(tmp_path / "out" / "iterations.npy"), np.full(batch, float(iters)))
