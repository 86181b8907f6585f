#!/usr/bin/env python3
"""A soft obstacle in the cost: a batch of cart-poles is asked to move the cart past a keep-out region that is not a constraint but a Gaussian bump
w exp(-(x - c)^2 / 2 sigma^2) on the cart position, its centre c stage data of the frame.  The bump is concave within sigma of its centre, so the
exact Hessian the device path carries into the QP is indefinite there and the QP comes back MPCQP_NON_CVX (status 9): with skip_failed_steps the
instance stands still forever.  options["convexify"] = "project" replaces the frame Hessians that have an eigenvalue below eps by their positive
definite projection before every QP (mpcqp_stage_convexify): the gradient stays exact, the loop moves again.  The run is done twice, with the
option off and on, and prints the QP statuses and the touched-frame counts.

The cost carries small absolute terms on s and r next to the tracking term: (s - r)^2 alone has a zero eigenvalue over [s; r], which would count
every frame as touched."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import ClosedLoopMPC, models


class SoftObstacleCartPole(models.StageOCP):
    nx, nu, name = 4, 1, "soft_obstacle_cartpole"
    convexify = True                                              # close the cost's pattern under the fill-in, export the kernel
    nsd = 2
    sdata = np.array([0.6, 8.0])                                  # d = [the bump's centre, its weight]
    SIGMA = 0.1                                                   # narrow and heavy: curvature -w / sigma^2 = -800 at the centre

    def cdyn(self, s, u):
        th, xd, thd = s[..., 1], s[..., 2], s[..., 3]
        sn, cs = np.sin(th), np.cos(th)
        tmp = (u[..., 0] + 0.05 * thd * thd * sn) / 1.1
        thdd = (9.81 * sn - cs * tmp) / (0.5 * (4.0 / 3.0 - 0.1 * cs * cs / 1.1))
        return np.stack([xd, thd, tmp - 0.05 * thdd * cs / 1.1, thdd], axis=-1)

    def lcost(self, s, u, r):
        v = 0.01 * u[..., 0] * u[..., 0]
        for i, q in enumerate((1.0, 10.0, 0.1, 0.1)):
            e = s[..., i] - r[..., i]
            v = v + q * e * e + 0.05 * s[..., i] * s[..., i] + 0.02 * r[..., i] * r[..., i]
        d0 = s[..., 0] - self.sdata[0]
        return v + self.sdata[1] * np.exp(-(d0 * d0) / (2.0 * self.SIGMA * self.SIGMA))

    def frame_bounds(self):
        return np.array([-2.4, -np.inf, -np.inf, -np.inf, -20.0]), np.array([2.4, np.inf, np.inf, np.inf, 20.0])


B, N, TICKS = 8, 12, 20
model = SoftObstacleCartPole(N, 0.02, Q=[1.0, 10.0, 0.1, 0.1], R=[0.01])


def bumps(k):
    """[B, len(k), 2]: every instance's bump at the absolute steps k: its own centre, drifting slowly, its own weight"""
    k = np.asarray(k, float)
    d = np.zeros((B, len(k), 2))
    d[..., 0] = 0.55 + 0.02 * np.arange(B)[:, None] + 0.002 * k[None, :]
    d[..., 1] = 8.0 + 0.25 * np.arange(B)[:, None]
    return d


def run(convexify):
    import torch
    frame0 = np.zeros((B, model.f))
    frame0[:, 0] = bumps([0])[:, 0, 0] + np.array([-0.5, -0.4, -0.3, -0.25, -0.2, -0.06, 0.0, 0.05])      # left of the bump; the last three on it
    goal = np.tile([1.2, 0.0, 0.0, 0.0], (B, 1))
    mpc = ClosedLoopMPC(model, {"max_iter": 1, "alpha": 0.7, "convexify": convexify}, batch=B, tail="rollout")
    mpc.set_stage_data(bumps(np.arange(N)))
    mpc.reset(frame0, reference=goal, x0=np.tile(frame0[:, None, :], (1, N, 1)).reshape(B, -1))
    failed = np.zeros(B, int)
    for t in range(TICKS):
        out = mpc.tick(d_new=bumps([t + N])[:, 0])
        failed += (out["status"].cpu().numpy() == 9)
    torch.cuda.synchronize()
    pos = mpc.x[:, 0].cpu().numpy()
    touched = None if convexify is None else torch.stack(mpc.sol.convexified).sum(dim=0).cpu().numpy()
    mpc.close()
    return failed, pos, touched, frame0[:, 0]


def main():
    print("%d cart-poles, %d ticks, horizon %d, every instance its own bump in the cost" % (B, TICKS, N))
    for label, option in (("off", None), ("project", "project")):
        failed, pos, touched, start = run(option)
        print("convexify %s" % label)
        for b in range(B):
            print("  instance %d: start %+.3f  final %+.3f  ticks with a NON_CVX QP %2d%s"
                  % (b, start[b], pos[b], failed[b], "" if touched is None else "  touched frames in all %d" % touched[b]))
        if option is not None and failed.any():
            raise SystemExit("a QP of the convexified loop came back NON_CVX")


if __name__ == "__main__":
    main()
