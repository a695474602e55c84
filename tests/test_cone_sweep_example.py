"""examples/cone_sweep.py runs to completion on a GPU box (one rocket landing under a batch of per-instance cone slopes, one launch)."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cone_sweep_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cone_sweep.py"), "--count", "16"], capture_output=True, text=True,
                         timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "per-instance-cones" in res.stdout and "touchdown error" in res.stdout and "one launch" in res.stdout, res.stdout[-2000:]
    assert res.stdout.count("glide slope") == 16, res.stdout[-2000:]
