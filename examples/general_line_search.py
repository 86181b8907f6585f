#!/usr/bin/env python3
"""A step length per instance on the general (non-stage) path: a small convex problem whose Newton steps overshoot -- the cost terms are
sqrt(1 + e^2) -- from 32 starts drawn wide, ten SQP iterations on the device, once with the reference's single alpha = 1 and once with
options["line_search"]: the l1-merit backtracking search that runs as one kernel in place of the step and merit kernels
(mpcqp_nlp_linesearch).  With alpha = 1 most instances run away to the box at +-50; with the search every one arrives at the optimum x = p."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import DeviceSQPOptimizationSolver
from optimal_control_problem_amd.general_eval import GeneralEvaluator
from optimal_control_problem_amd.general_nlp import GeneralNLP

B, ITERS, P = 32, 10, 0.3


def cost(w):
    p, x = w[0], w[1:]
    return sum(np.sqrt(1.0 + (x[i] - p) ** 2) for i in range(6)) + 0.05 * sum((x[i + 1] - x[i]) ** 2 for i in range(5))


def constraints(w):
    x = w[1:]
    return [x[2] - x[0] - 0.1 * np.sin(x[1]), x[5] - x[3] + 0.1 * x[4] ** 2]


nlp = GeneralNLP(6, 1, cost, constraints)
arg = dict(p=np.full((B, 1), P), lbx=np.full((B, 6), -50.0), ubx=np.full((B, 6), 50.0), lbg=np.full((B, 2), -0.5), ubg=np.full((B, 2), 0.5))
x0 = np.random.default_rng(5).normal(0.0, 2.0, (B, 6))
for label, extra in (("alpha = 1 for everyone", {}), ("line search from alpha = 1", {"line_search": True})):
    sol = DeviceSQPOptimizationSolver(nlp, dict({"max_iter": ITERS, "alpha": 1.0}, **extra), batch=B, evaluator=GeneralEvaluator(nlp))
    sol.setInitialGuess(x0)
    r = sol.getOptimalSolution(arg)
    home = int((np.abs(r["x"] - P).max(axis=1) < 1e-2).sum())
    print("%-28s %2d of %d instances at the optimum, largest objective %.3f" % (label, home, B, r["f"].max()))
    sol.close()
