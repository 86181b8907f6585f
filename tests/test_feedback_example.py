"""examples/feedback_gain_mpc.py runs as a user would run it (GPU box): a solve every fourth plant step, holds that track the plan in between."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_feedback_gain_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "feedback_gain_mpc.py"), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"mean deviation from the plan: (\S+) with the gains, (\S+) with open-loop holds", r.stdout)
    assert m and "mean closed-loop cost" in r.stdout, r.stdout[-2000:]
    assert float(m.group(1)) < float(m.group(2)), r.stdout[-2000:]      # the holds with the gains stay nearer the plan
