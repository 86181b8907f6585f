#!/usr/bin/env python3
"""A least-squares cost over a nonlinear output on the fast path: a pendulum whose cost is the distance of its tip to the target's tip,
sum_k |rcost(s_k, u_k, r)|^2 (models.StageOCP.rcost, a Gauss-Newton frame cost).  Written as a scalar lcost the same cost has an indefinite exact
Hessian away from the target: the QP comes back NON_CVX (status 9) and the instance gets no step.  With rcost the QP takes 2 J'J -- positive
semidefinite by construction, formed by the generated library's evaluation kernel from one pass of the residual on dual numbers and one pass of its
transposed Jacobian -- and every start moves.  Both models run the device SQP loop here, side by side.

usage: gauss_newton_mpc.py [iterations]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import DeviceSQPOptimizationSolver, models


class TipPendulum(models.StageOCP):
    nx, nu, name = 2, 1, "tip_pendulum"

    def __init__(self, N=12):
        super().__init__(N, 0.05, [1.0, 1.0], [1.0])                # (the diagonal weights are not used: the model states its own cost)

    def F(self, s, u):                                             # discrete map, NumPy; traced once, emitted as device code
        th, om = s[..., 0], s[..., 1]
        return np.stack([th + 0.05 * om, om + 0.05 * (u[..., 0] - 9.81 * np.sin(th) - 0.1 * om)], axis=-1)

    def rcost(self, s, u, r):                                      # the residual; the user scales its rows (no 1/2, no weight vector)
        return [np.sin(s[..., 0]) - np.sin(r[..., 0]), np.cos(s[..., 0]) - np.cos(r[..., 0]), 0.3 * (s[..., 1] - r[..., 1]), 0.1 * u[..., 0]]

    def frame_bounds(self):
        return np.array([-np.inf, -8.0, -6.0]), np.array([np.inf, 8.0, 6.0])


class ScalarTwin(TipPendulum):
    """the same cost as one scalar: its QP takes the exact Hessian"""
    name = "tip_pendulum_scalar"; rcost = None

    def lcost(self, s, u, r):
        return sum(v * v for v in TipPendulum.rcost(self, s, u, r))


ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 12
theta0 = np.array([0.2, 0.9, 1.4, 1.9, 2.4, 2.8, 3.0, 3.1])
B = len(theta0)
print("start angles   ", " ".join("%5.1f" % v for v in theta0))
for m in (ScalarTwin(), TipPendulum()):
    frame0 = np.zeros((B, m.f)); frame0[:, 0] = theta0
    lbx, ubx, lbg, ubg = m.stacked_bounds(frame0)
    arg = dict(p=np.zeros((B, m.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    sol = DeviceSQPOptimizationSolver(m, {"max_iter": 1, "alpha": 0.7, "skip_failed_steps": True}, batch=B)
    sol.setInitialGuess(np.tile(frame0, (1, m.N)))                 # the first frame held over the horizon
    stuck = np.zeros(B, np.int64)
    for _ in range(ITERS):
        res = sol.getOptimalSolution(arg)
        st = sol.status.cpu().numpy()
        stuck += ~np.isin(st, (1, 2, 7))
    kind = "residual, 2 J'J" if sol.ev.gauss_newton else "scalar, exact H"
    print("status %-16s" % kind, " ".join("%5d" % v for v in st), " (last of %d iterations; nr = %d)" % (ITERS, sol.ev.nr))
    print("  iterations without a step", " ".join("%5d" % v for v in stuck))
    print("  objective              ", " ".join("%7.3f" % v for v in res["f"]))
    sol.close()
