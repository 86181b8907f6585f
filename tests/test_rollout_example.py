"""examples/rollout_start_mpc.py runs as a user would run it (GPU box)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_rollout_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rollout_start_mpc.py"), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "solved from the rollout start: 4 of 4 (from the zero start: 0)" in r.stdout, r.stdout[-2000:]
    assert "zero start: first QP primal_infeasible" in r.stdout and "rollout start: first QP solved," in r.stdout
