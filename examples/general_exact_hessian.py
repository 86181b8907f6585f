#!/usr/bin/env python3
"""The exact Hessian of the Lagrangian on the general (non-stage) path: a point on the unit sphere that also satisfies x0 x1 - 0.3 x2 = 0.2, closest
to (p, 1, -0.5).  Both constraints are curved, and the QP of the reference carries hessian(f, w) only: with full steps its loop keeps circling.
options["exact_hessian"] adds the curvature of the constraints under the current multipliers (mpcqp_nlp_lagrangian, two kernels between the
evaluation and the QP); "dominant" also adds the diagonal shift that keeps the QP convex when that curvature is indefinite, as it is on the way
for p = -2.  Twenty SQP iterations on the device from six starts."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import DeviceSQPOptimizationSolver
from optimal_control_problem_amd.general_eval import GeneralEvaluator
from optimal_control_problem_amd.general_nlp import GeneralNLP

B, ITERS = 6, 20


def cost(w):
    p, x = w[0], w[1:]
    return (x[0] - p) ** 2 + (x[1] - 1.0) ** 2 + (x[2] + 0.5) ** 2


def constraints(w):
    x = w[1:]
    return [x[0] * x[0] + x[1] * x[1] + x[2] * x[2] - 1.0, x[0] * x[1] - 0.3 * x[2] - 0.2]


nlp = GeneralNLP(3, 1, cost, constraints, exact_hessian=True)
arg = dict(p=np.array([[3.0]] * 3 + [[-2.0]] * 3), lbx=np.full((B, 3), -5.0), ubx=np.full((B, 3), 5.0), lbg=np.zeros((B, 2)), ubg=np.zeros((B, 2)))
x0 = np.array([0.8, 0.5, 0.1]) + 0.2 * np.random.default_rng(11).normal(size=(B, 3))
for label, extra in (("hessian(f, w) (the reference)", {}), ("exact_hessian = 'dominant'", {"exact_hessian": "dominant"})):
    sol = DeviceSQPOptimizationSolver(nlp, dict({"max_iter": ITERS, "alpha": 1.0, "skip_failed_steps": True}, **extra), batch=B, evaluator=GeneralEvaluator(nlp))
    sol.setInitialGuess(x0)
    r = sol.getOptimalSolution(arg)
    print("%-30s last step %.1e .. %.1e, worst violation %.1e" % (label, float(sol.step_max.min()), float(sol.step_max.max()), float(sol.gmax.max())))
    sol.close()
