#!/usr/bin/env python3
"""Converged instances leave the QP launch: options["skip_converged_qps"] next to options["kkt_tol"].

kkt_tol freezes an instance that meets the NLP's first-order residuals: its x is not stepped any more.  Its QP was still set up and solved in
every later iteration.  With skip_converged_qps the verdicts of the check are the QP handle's skip array (mpcqp_set_skip): a frozen instance's
workgroup returns at once, and the point the loop returns is the same, bit for bit.  admm_iterations shows what was left out.
usage: python examples/skip_converged_sqp.py [batch]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
TOL = 2e-3
mdl = models.CartPole(20, 0.02)
frame0 = np.zeros((B, mdl.f))
frame0[:, 1] = np.geomspace(0.01, 0.7, B)                 # start angles: the small ones are all but linear, the large ones need more QPs
lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)

out = {}
for name, opt in (("kkt_tol", {}), ("kkt_tol + skip_converged_qps", {"skip_converged_qps": True})):
    sol = DeviceSQPOptimizationSolver(mdl, dict(opt, max_iter=12, alpha=1.0, kkt_tol=TOL), batch=B)
    res = sol.getOptimalSolution(arg)
    solved = [int((it > 0).sum()) for it in sol.admm_iterations]
    at = sol.converged_at.cpu().numpy()
    print("%s: %d iterations, converged_at min %d max %d; QPs solved per iteration %s (of %d)" % (name, sol.iterations_done, at[at >= 0].min(), at.max(), solved, B))
    out[name] = res["x"]
    sol.close()
same = np.array_equal(out["kkt_tol"].view(np.int64), out["kkt_tol + skip_converged_qps"].view(np.int64))
print("x is bit for bit the same: %s" % same)
