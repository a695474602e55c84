"""examples/rollout_scores.py runs to completion on a GPU box at a small batch (a rho sweep scored by the rollout metrics, no logs), and its
self-check -- the best candidate's cost recomputed in numpy from a logged rerun -- passes."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_rollout_scores_example_runs_and_checks_itself():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rollout_scores.py"), "--count", "12", "--ticks", "20"],
                         capture_output=True, text=True, timeout=600, cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "best rho" in res.stdout and "closed-loop cost" in res.stdout and "self-check passed" in res.stdout, res.stdout[-2000:]
