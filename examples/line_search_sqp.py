#!/usr/bin/env python3
"""A step length per instance: 32 quadrotors started far from hover, four SQP iterations from x = 0 with the full step, once with the
reference's single alpha and once with options["line_search"] -- an l1-merit backtracking search that runs as one kernel in place of the step and
merit kernels (mpcqp_stage_linesearch).  Most instances take the full step either way; the few for which it is bad are damped."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import DeviceSQPOptimizationSolver, models

B, ITERS = 32, 4
quad = models.Quadrotor(20, 0.02)
rng = np.random.default_rng(5)
s0 = np.zeros((B, 12))
s0[:, 0:3] = rng.normal(0.0, 1.5, (B, 3)); s0[:, 3:6] = rng.normal(0.0, 0.6, (B, 3)); s0[:, 6:9] = rng.normal(0.0, 1.0, (B, 3))
frame0 = np.concatenate([s0, np.full((B, 4), quad.hover_thrust)], axis=1)
lbx, ubx, lbg, ubg = quad.stacked_bounds(frame0)
arg = dict(p=np.zeros((B, quad.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
for label, extra in (("alpha = 1 for everyone", {}), ("line search from alpha = 1", {"line_search": {"candidates": 4, "beta": 0.5}})):
    sol = DeviceSQPOptimizationSolver(quad, dict({"max_iter": 1, "alpha": 1.0}, **extra), batch=B)
    taken = []
    for _ in range(ITERS):
        sol.getOptimalSolution(arg, to_host=False)
        if sol.alpha_taken is not None:
            taken.append(float(sol.alpha_taken.mean()))
    g = sol.gmax.cpu().numpy()
    print("%-28s worst violation %.3g, median %.3g%s" % (label, g.max(), np.median(g), "" if not taken else ", mean alpha per iteration %s" % np.round(taken, 3)))
    sol.close()
