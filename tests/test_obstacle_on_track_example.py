"""examples/obstacle_on_track.py runs to completion on a GPU box (per-instance tracks with auto-advance and per-knot half-spaces of a
moving cylinder, re-sent every tick, on a handle that called prepare()): its own assertions hold -- no vehicle enters its cylinder, every
vehicle reaches the end of its track -- and the kernel line shows layout D's per-instance families on the track's rows."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_obstacle_on_track_example_runs():
    env = dict(os.environ)
    env.pop("TINYMPC_LAYOUT", None)  # (the example names the throughput layout itself)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "obstacle_on_track.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"), env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    kernel = [l for l in res.stdout.splitlines() if l.startswith("kernel:")]
    assert len(kernel) == 1 and kernel[0].startswith("kernel: D") and "refused" not in kernel[0], res.stdout[-2000:]
    for word in ("per-knot-linear", "per-instance-trajectories", "reference-track", "per-instance-refs"):
        assert word in kernel[0], kernel[0]
    assert "closest approach to the moving axis" in res.stdout and "0 of 64 vehicles inside their cylinder" in res.stdout, res.stdout[-2000:]
