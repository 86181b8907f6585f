#!/usr/bin/env python3
"""A non-uniform time grid on the device path: a cart-pole is held upright by two controllers with the same look-ahead, one on the grid
h_k = h_0 g^k -- fine steps near now, coarse steps far out -- and one on the uniform grid h_k = h_0, which needs several times the frames.  The
step length is stage data of the transition (models.StageOCP.transition_data): models.GridCartPole reads h_k as self.sdata[0] in its own RK4, in the
rate limit |u_{k+1} - u_k| / h_k <= rate (kfun) and in the move penalty (u_{k+1} - u_k)^2 / h_k (llink); the generated kernels take frame k's row
from a device array.  The rows belong to horizon positions, not to world time, so the closed loop keeps them where they are
(ClosedLoopMPC(..., shift_data=False)); the plant step between two ticks takes row 0, h_0 on both grids: the same plant.
Prints frames, QP size, accumulated stage cost and worst constraint violation of both."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import ClosedLoopMPC, models

B, TICKS = 4, 60
H0, GROWTH, N_GRID = 0.02, 1.3, 12


def run(name, model):
    import torch
    frame0 = np.zeros((B, model.f))
    frame0[:, 1] = 0.15 + 0.05 * np.arange(B)                       # the pole 0.15 .. 0.3 rad off upright, at rest
    mpc = ClosedLoopMPC(model, {"max_iter": 2, "alpha": 1.0}, batch=B, tail="rollout", shift_data=False)
    mpc.set_stage_data(model.grid_rows(B))
    mpc.reset(frame0, reference=np.zeros((B, model.nx)), x0=np.tile(frame0, (1, model.N)))
    cost = np.zeros(B)
    applied = []
    for _ in range(TICKS):
        out = mpc.tick()
        cost += out["stage_cost"].cpu().numpy()
        applied.append(out["applied"].cpu().numpy().copy())
    torch.cuda.synchronize()
    A = np.stack(applied, axis=1)                                    # [B, TICKS, f]: the frames that were applied
    lo, hi = model.frame_bounds()
    viol = max(np.max(lo - A), np.max(A - hi), np.max(np.abs(np.diff(A[:, :, model.nx], axis=1)) / H0 - model.rate), 0.0)
    final = mpc.x[:, :model.nx].cpu().numpy()
    print("%-11s %3d frames  look-ahead %.3f s  QP %d variables x %d rows  final cost %.4f  worst violation %.2e  final |theta| %.2e"
          % (name, model.N, model.steps[:-1].sum(), mpc.ev.n, mpc.ev.m, cost.sum(), viol, np.abs(final[:, 1]).max()))
    mpc.close()


def main():
    grid = models.GridCartPole(N_GRID, H0, GROWTH)
    look_ahead = grid.steps[:-1].sum()
    uniform = models.GridCartPole(int(round(look_ahead / H0)) + 1, H0, 1.0)
    print("%d cart-poles, %d ticks of %.2f s, grid h_k = %.2f * %.2f^k" % (B, TICKS, H0, H0, GROWTH))
    run("non-uniform", grid)
    run("uniform", uniform)


if __name__ == "__main__":
    main()
