"""Trajectory tracking through the reference-shaped host API: a quadrotor follows a figure-eight.  The reference vector stacks one state per
frame (setReference(horizon * 12)) and the cost of step k subtracts its own slice, reference.frame(k) -- in the reference project that is all
there is to it (setReference takes an SX of any size, computeOptimalTrajectory checks the size only).  genSolver() recognises the pattern, the
dynamics are traced and compiled for gfx950 (solver_settings.gen_code: true) and every MPC tick -- local system, QP with the pinned parameter
rows and first frame eliminated, step -- runs on the GPU.  Needs an MI355X.
usage: python examples/tracking_mpc.py [batch] [ticks]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import yaml  # noqa: E402

from optimal_control_problem_amd import models  # noqa: E402
from optimal_control_problem_amd.ocp import Dynamics, OptimalControlProblem  # noqa: E402

HORIZON, DT = 20, 0.02
plant = models.Quadrotor(HORIZON, DT)          # its discrete map F(s, u), weights and thrust limits; any NumPy callable works
CONFIG = """
optimal_control_problem:
  discretization_settings: {dt: %g, horizon: %d}
  solver_settings: {verbose: false, gen_code: true, load_lib: false, max_iter: 1000, warm_start: true, solve_method: CUDA_SQP,
                    SQP_settings: {alpha: 1.0, step_num: 2}}
  OCP_variables:
    - {name: state, size: 12, lower_bound: [%s], upper_bound: [%s]}
    - {name: input, size: 4, lower_bound: [0.0, 0.0, 0.0, 0.0], upper_bound: [%g, %g, %g, %g]}
""" % ((DT, HORIZON, ", ".join(["-.inf"] * 12), ", ".join([".inf"] * 12)) + (2.0 * plant.hover_thrust,) * 4)


class FigureEightOCP(OptimalControlProblem):
    def deployConstraintsAndAddCost(self):
        cfg = self.OCPConfigPtr_; N = cfg.getHorizon()
        ref = self.setReference(N * 12)
        for k in range(N):
            st, inp = cfg.getVariable(k, "state"), cfg.getVariable(k, "input")
            self.addVectorCost(plant.Q * (1.0 if k < N - 1 else 5.0), st - ref.frame(k))     # every step tracks its own reference state
            self.addVectorCost(plant.R, inp)
            if k < N - 1:
                self.addEquationConstraint("dynamics", cfg.getVariable(k + 1, "state"), Dynamics(plant.F, st, inp))


def figure_eight(t, phase):
    """reference states [..., 12] at times t: position on a lemniscate at height 1, its velocity, level attitude"""
    w, a = 1.5, 0.6
    th = w * t + phase
    r = np.zeros(np.shape(th) + (12,))
    r[..., 0] = a * np.sin(th); r[..., 1] = 0.5 * a * np.sin(2.0 * th); r[..., 2] = 1.0
    r[..., 6] = a * w * np.cos(th); r[..., 7] = a * w * np.cos(2.0 * th)
    return r


def main(batch=64, ticks=25, **kw):
    ocp = FigureEightOCP(yaml.safe_load(CONFIG)["optimal_control_problem"], batch=batch, **kw)
    ocp.deployConstraintsAndAddCost()
    ocp.genSolver()
    rng = np.random.default_rng(0)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(batch, 1))
    frame = np.concatenate([figure_eight(np.zeros((batch, 1)), phase)[:, 0], np.full((batch, 4), plant.hover_thrust)], axis=1)
    frame[:, 0:3] += rng.normal(0.0, 0.05, size=(batch, 3))                       # start beside the curve
    err = []
    for tick in range(ticks):
        t = (tick + np.arange(HORIZON)[None, :]) * DT
        traj = ocp.computeOptimalTrajectory(frame, figure_eight(t, phase).reshape(batch, -1)).reshape(batch, HORIZON, 16)
        s = plant.F(frame[:, :12], frame[:, 12:])                                  # the whole first frame is pinned: the plant moves on under its input ...
        u = np.clip(traj[:, 1, 12:], 0.0, 2.0 * plant.hover_thrust)
        frame = np.concatenate([s, u], axis=1)                                     # ... and the next tick pins the input planned for that step
        err.append(np.abs(s[:, 0:3] - figure_eight((tick + 1) * DT + np.zeros((batch, 1)), phase)[:, 0, 0:3]).max(axis=1))
    err = np.array(err)
    print("batch %d, %d ticks of horizon %d: tracking stage pattern %s, np = %d; position error max %.3f m at the start, %.3f m over the last five ticks"
          % (batch, ticks, HORIZON, not ocp.generalPath_, ocp.model_.np, err[0].max(), err[-5:].max()))
    return ocp, err


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64, int(sys.argv[2]) if len(sys.argv) > 2 else 25)
