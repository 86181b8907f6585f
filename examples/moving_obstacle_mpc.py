#!/usr/bin/env python3
"""Different worlds on one handle: a batch of point masses crosses the plane, every instance past its own disc, and every disc moves along a path
that is predicted over the horizon.  The disc's centre and radius are stage data -- the model's hfun reads them as self.sdata[i], the generated
kernels take frame k's row d[b, k] from a device array (ClosedLoopMPC.set_stage_data), and every tick the stored set moves up by one frame while the
newest prediction enters at the end of the horizon (tick(d_new=...)).  No number of the obstacle is a constant of the generated code, and none of them
is a QP variable.  Prints the minimum clearance per instance over the run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import ClosedLoopMPC, models


class PointMass(models.StageOCP):
    """s = [x, y, vx, vy], u = the acceleration; one path row keeps the mass outside a disc, d = [cx, cy, radius + margin] of the frame"""
    nx, nu, name = 4, 2, "point_mass_moving_obstacle"
    nh = 1; h_lo = [0.0]; h_hi = [np.inf]
    nsd = 3
    sdata = np.array([0.0, -10.0, 0.5])                             # the defaults: a disc far away

    def F(self, s, u):
        h = self.dt
        return np.stack([s[..., 0] + h * s[..., 2] + 0.5 * h * h * u[..., 0], s[..., 1] + h * s[..., 3] + 0.5 * h * h * u[..., 1],
                         s[..., 2] + h * u[..., 0], s[..., 3] + h * u[..., 1]], axis=-1)

    def hfun(self, s, u):
        ex, ey = s[..., 0] - self.sdata[0], s[..., 1] - self.sdata[1]
        return np.stack([ex * ex + ey * ey - self.sdata[2] * self.sdata[2]], axis=-1)

    def frame_bounds(self):
        return np.array([-np.inf, -np.inf, -3.0, -3.0, -4.0, -4.0]), np.array([np.inf, np.inf, 3.0, 3.0, 4.0, 4.0])


B, N, TICKS, MARGIN = 6, 12, 30, 0.15
model = PointMass(N, 0.2, Q=[1.0, 1.0, 0.1, 0.1], R=[0.05, 0.05])
radius = 0.35 + 0.05 * np.arange(B)


def discs(k):
    """[B, len(k), 3]: where every instance's disc is predicted to be at the absolute steps k -- it drifts upwards across the line y = 0.3"""
    k = np.asarray(k, float)
    d = np.zeros((B, len(k), 3))
    for b in range(B):
        d[b, :, 0] = 0.15 * b - 0.4
        d[b, :, 1] = -0.3 - 0.05 * b + 0.05 * (1.0 + 0.2 * b) * k
        d[b, :, 2] = radius[b] + MARGIN
    return d


def main():
    import torch
    frame0 = np.tile([-2.0, 0.3, 0.0, 0.0, 0.0, 0.0], (B, 1))
    goal = np.tile([2.0, 0.3, 0.0, 0.0], (B, 1))
    X0 = np.zeros((B, N, model.f))
    X0[:, :, 0] = -2.0; X0[:, :, 1] = 0.3                           # the start: at rest at the first state
    mpc = ClosedLoopMPC(model, {"max_iter": 2, "alpha": 1.0}, batch=B, tail="rollout")
    mpc.set_stage_data(discs(np.arange(N)))                         # frame k of the first tick sees the disc at step k
    mpc.reset(frame0, reference=goal, x0=X0.reshape(B, -1))
    clearance = np.full(B, np.inf)
    for t in range(TICKS):
        pos = mpc.x[:, :2].cpu().numpy()                            # where the mass is at step t
        c = discs([t])[:, 0]
        clearance = np.minimum(clearance, np.hypot(pos[:, 0] - c[:, 0], pos[:, 1] - c[:, 1]) - radius)
        out = mpc.tick(d_new=discs([t + N])[:, 0])                  # the prediction for the frame that enters the horizon
    torch.cuda.synchronize()
    final = mpc.x[:, :2].cpu().numpy()
    status = out["status"].cpu().numpy()
    print("%d point masses, %d ticks, horizon %d, every instance its own moving disc" % (B, TICKS, N))
    for b in range(B):
        print("  instance %d: radius %.2f  minimum clearance %.4f  final position (%+.3f, %+.3f)  last status %d"
              % (b, radius[b], clearance[b], final[b, 0], final[b, 1], status[b]))
    mpc.close()


if __name__ == "__main__":
    main()
