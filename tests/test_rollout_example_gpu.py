"""examples/closed_loop_rollout.py runs to completion on a GPU box (per-instance tracks with auto-advance and process noise, one rollout call)."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_closed_loop_rollout_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "closed_loop_rollout.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "reference-track" in res.stdout and "tracking error" in res.stdout and "us per tick" in res.stdout, res.stdout[-2000:]
