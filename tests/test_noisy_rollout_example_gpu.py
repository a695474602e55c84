"""examples/noisy_rollout.py runs to completion on a GPU box at a small batch (a sweep of sensor-noise levels in one scored rollout with the
noise drawn on the device), its self-check passes, and the mean closed-loop cost it prints does not decrease from the lowest level to the
highest (the levels double, so the noise's share of the cost quadruples from one line to the next)."""
import os
import re
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_noisy_rollout_example_runs_and_the_cost_grows_with_the_level():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "noisy_rollout.py"), "--levels", "5", "--realisations", "32", "--ticks", "100"],
                         capture_output=True, text=True, timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "self-check passed" in res.stdout, res.stdout[-2000:]
    rows = re.findall(r"^level\s+([0-9.]+): cost\s+([0-9.eE+-]+)", res.stdout, re.M)
    levels, costs = [float(r[0]) for r in rows], [float(r[1]) for r in rows]
    print(res.stdout)
    assert len(rows) == 5 and levels[0] == 0.0 and levels == sorted(levels) and levels[-1] == 0.08
    assert all(b >= a for a, b in zip(costs, costs[1:])), costs
    assert costs[-1] > costs[0]
