#!/usr/bin/env python3
"""A damped SQP loop that knows when it is done: options["kkt_tol"] next to options["sqp_tol"].

With the reference's own damping (alpha = 0.1) the applied step is a tenth of the Newton step: the step-size stop sqp_tol ends the loop at an
iterate whose stationarity residual is still well above the tolerance.  kkt_tol measures the NLP's first-order residuals per instance on the device
(mpcqp_stage_kkt) and runs on until every instance meets them; at a wide batch the instances converge at different iterations and are frozen one
by one.
usage: python examples/kkt_stop_sqp.py [batch]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
TOL = 1e-2
mdl = models.DoubleIntegrator(20, 0.05)
rng = np.random.default_rng(1)
frame0 = np.concatenate([rng.uniform([-3.0, -1.5], [3.0, 1.5], size=(B, 2)) * rng.uniform(0.02, 1.0, size=(B, 1)), np.zeros((B, 1))], axis=1)
lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)

for name, opt in (("sqp_tol", {"sqp_tol": TOL}), ("kkt_tol", {"kkt_tol": TOL})):
    sol = DeviceSQPOptimizationSolver(mdl, dict(opt, max_iter=150, alpha=0.1), batch=B)
    sol.getOptimalSolution(arg)
    now = sol.kkt(arg, TOL)
    res = now["res"].cpu().numpy()
    rel = res[:, 0] / np.maximum(1.0, res[:, 3])
    print("%s = %g: stopped after %d QPs; stat / max(1, scale) worst %.2e (tolerance %g), feas %.1e, compl %.1e; %d of %d instances at a first-order point"
          % (name, TOL, sol.iterations_done, rel.max(), TOL, res[:, 1].max(), res[:, 2].max(), int(now["converged"].sum()), B))
    if name == "kkt_tol":
        at = sol.converged_at.cpu().numpy()
        print("converged_at: min %d, median %d, max %d (%d distinct iterations)" % (at.min(), int(np.median(at)), at.max(), len(set(at.tolist()))))
    sol.close()
