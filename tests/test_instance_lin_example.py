"""examples/obstacle_avoidance.py runs to completion on a GPU box (per-instance goals and per-instance half-spaces, re-sent every tick)."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_obstacle_avoidance_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "obstacle_avoidance.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "per-instance-linear" in res.stdout and "per-instance-refs" in res.stdout and "closest approach" in res.stdout, res.stdout[-2000:]
