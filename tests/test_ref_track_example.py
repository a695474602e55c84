"""examples/track_following.py runs to completion on a GPU box (reference tracks with auto-advance and a mid-run reset)."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_track_following_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "track_following.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "reference-track" in res.stdout and "position error" in res.stdout, res.stdout[-2000:]
