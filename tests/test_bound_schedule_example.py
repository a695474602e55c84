"""examples/bound_schedule.py runs to completion on a GPU box (input limits that ramp up over the horizon, each instance at its own rate,
on a prepared handle): its own assertions hold -- every control inside its instance's schedule, the first knot's authority used, the
slower ramps binding for longer -- and it prints the kernel line: layout D's per-knot bounds form."""
import os
import subprocess
import sys

import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bound_schedule_example_runs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bound_schedule.py")], capture_output=True, text=True, timeout=600,
                         cwd=os.path.join(ROOT, "examples"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    assert "kernel: D" in res.stdout and " per-knot-bounds" in res.stdout and "per-instance-bounds" in res.stdout, res.stdout[-2000:]
    assert "refused" not in res.stdout and "(no plan)" not in res.stdout, res.stdout[-2000:]
    assert "controls at their scheduled limit" in res.stdout, res.stdout[-2000:]
