"""examples/converging_tracks.py runs to completion on a GPU box (a converging batch with a reference track per instance: layout D's
trajectory form with and without slot refill) and reports identical results."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_converging_tracks_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "converging_tracks.py")], capture_output=True, text=True,
                         timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "identical first controls and iteration counts: True" in res.stdout, res.stdout[-2000:]
    plain, refill = (next(l for l in res.stdout.splitlines() if l.startswith(w)) for w in ("plain trajectory form", "slot refill"))
    assert "per-instance-trajectories" in plain and "slot-refill" not in plain, plain
    assert "per-instance-trajectories" in refill and "slot-refill" in refill, refill
