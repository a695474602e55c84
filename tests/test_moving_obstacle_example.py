"""examples/moving_obstacle.py runs to completion on a GPU box (per-instance goals and per-knot half-spaces of a moving cylinder, re-sent
every tick): its own assertions hold -- no vehicle enters its cylinder, every vehicle reaches its goal -- and it prints the kernel line
and the closest approach."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_moving_obstacle_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "moving_obstacle.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    assert "kernel: A" in res.stdout and "per-knot-linear" in res.stdout and "per-instance-refs" in res.stdout, res.stdout[-2000:]
    assert "closest approach to the moving axis" in res.stdout and "one plane per horizon" in res.stdout, res.stdout[-2000:]
