#!/usr/bin/env python3
"""The Hessian of the Lagrangian in the QP: 16 pendulums swung from rest towards th = 2 (more than the torque limit holds) under the nonlinear path
constraint th^2 + 0.5 u^2 + 0.3 th w <= 2, twelve SQP iterations with the full step, once with the reference's QP (the Hessian of the cost alone) and
once with options["exact_hessian"] -- the curvature of the dynamics and of the path constraint under the loop's multiplier estimate, added to P by
one kernel after every evaluation (mpcqp_stage_lagrangian).  Printed: the largest step of the batch per iteration.  The QPs are solved to the
reference's 1e-3 in both runs, which bounds how small a step can become (DESIGN.md 6.18 has the counts with QPs solved tightly)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import DeviceSQPOptimizationSolver, models

B, N, ITERS, DT = 16, 10, 12, 0.2


class Pendulum(models.StageOCP):
    nx, nu, name = 2, 1, "swing_pendulum"
    nh = 1; h_lo = [-np.inf]; h_hi = [2.0]
    exact_hessian = True                                          # put the curvature's structure into the pattern, generate FG / HG, export the kernel

    def F(self, s, u):
        th, w = s[..., 0], s[..., 1]
        return np.stack([th + self.dt * w, w + self.dt * (-9.81 * np.sin(th) + 0.5 * u[..., 0] * np.cos(th) - 0.1 * w)], axis=-1)

    def hfun(self, s, u):
        th, w, v = s[..., 0], s[..., 1], u[..., 0]
        return np.stack([th * th + 0.5 * v * v + 0.3 * th * w], axis=-1)

    def lcost(self, s, u, r):
        e0, e1 = s[..., 0] - r[..., 0], s[..., 1] - r[..., 1]
        return 2.0 * e0 * e0 + 0.5 * e1 * e1 + 0.05 * u[..., 0] * u[..., 0]

    def frame_bounds(self):
        return np.array([-10.0, -20.0, -3.0]), np.array([10.0, 20.0, 3.0])


def main():
    mdl = Pendulum(N, DT, Q=[2.0, 0.5], R=[0.05])
    frame0 = np.zeros((B, mdl.f))
    frame0[:, 0] = np.linspace(-0.3, 0.2, B)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.tile([2.0, 0.0], (B, 1)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    x0 = np.tile(frame0[:, None, :], (1, N, 1)).reshape(B, -1)
    for label, extra in (("Hessian of the cost (the reference)", {}), ("Hessian of the Lagrangian", {"exact_hessian": True})):
        sol = DeviceSQPOptimizationSolver(mdl, dict({"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True}, **extra), batch=B)
        sol.setInitialGuess(x0)
        steps = []
        for _ in range(ITERS):
            sol.getOptimalSolution(arg, to_host=False)
            steps.append(float(sol.step_max.max()))
        print("%-38s max |dx| per iteration: %s" % (label, " ".join("%.1e" % s for s in steps)))
        print("%-38s objective %.6f, worst violation %.2e" % ("", float(sol.f.mean()), float(sol.gmax.max())))
        sol.close()


if __name__ == "__main__":
    main()
