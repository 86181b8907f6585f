"""examples/direct_qp_mpc.py runs as a user would run it (GPU box): the first ticks saturate the input and are rejected, later ticks are accepted."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_direct_qp_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "direct_qp_mpc.py"), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"accepted share: first tick (\S+) %, last tick (\S+) %", r.stdout)
    assert m, r.stdout[-2000:]
    assert float(m.group(1)) == 0.0 and float(m.group(2)) == 100.0, r.stdout[-2000:]
    m = re.search(r"largest difference of an applied frame to the loop without the option: (\S+)", r.stdout)
    # both loops solve every QP to eps = 1e-3 or better; the applied frames differ by no more than a few of those tolerances
    assert m and float(m.group(1)) < 1e-2, r.stdout[-2000:]
