#!/usr/bin/env python3
"""A move penalty on the fast path: the README's pendulum with the cost term (u_{k+1} - u_k)' S (u_{k+1} - u_k) between consecutive frames
(models.StageOCP.llink, a link cost).  The term is traced, its gradient derived on the tape, and the generated library's kernels add its exact
Hessian to P -- frame k couples to frame k + 1, as the dynamics already couple them in A -- so the problem keeps the device SQP loop, the line
search and ClosedLoopMPC.  Open loop first (with and without the penalty), then the closed loop.

usage: smooth_input_mpc.py [batch] [ticks]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import ClosedLoopMPC, DeviceSQPOptimizationSolver, models


class MyPlant(models.StageOCP):
    nx, nu, name = 2, 1, "my_plant"

    def F(self, s, u):                                             # discrete map, NumPy; traced once, emitted as device code
        return np.stack([s[..., 0] + 0.05 * s[..., 1], s[..., 1] + 0.05 * (u[..., 0] - np.sin(s[..., 0]))], axis=-1)

    def frame_bounds(self):
        return np.array([-np.inf, -4.0, -2.0]), np.array([np.inf, 4.0, 2.0])


class SmoothPlant(MyPlant):
    name = "my_plant_smooth"

    def llink(self, s, u, sn, un):                                 # summed over the stages k = 0 .. N-2; no reference, no theta
        return 2.0 * (un[..., 0] - u[..., 0]) ** 2


def movement(x, m):
    X = np.asarray(x).reshape(-1, m.N, m.f)
    return (np.diff(X[:, :, m.nx:], axis=1) ** 2).sum(axis=(1, 2))


B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
frame0 = np.concatenate([np.random.default_rng(0).uniform(-1, 1, (B, 2)), np.zeros((B, 1))], axis=1)
plain, smooth = MyPlant(20, 0.05, Q=[10.0, 1.0], R=[0.1]), SmoothPlant(20, 0.05, Q=[10.0, 1.0], R=[0.1])

# open loop: six SQP iterations from x = 0
moved = {}
for m in (plain, smooth):
    lbx, ubx, lbg, ubg = m.stacked_bounds(frame0)
    sol = DeviceSQPOptimizationSolver(m, {"max_iter": 6, "alpha": 1.0, "line_search": True}, batch=B)
    if m is smooth:
        print("link cost on the stage path: %s (nnz(P) %d against %d)" % (sol.ev.link_cost, sol.ev.nnzP, len(plain.Pi)))
    res = sol.getOptimalSolution(dict(p=np.zeros((B, m.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg))
    moved[m.name] = movement(res["x"], m)
    print("open loop %-16s objective %.3f, sum (du)^2 %.3f, worst violation %.2e" % (m.name, res["f"].mean(), moved[m.name].mean(), float(sol.gmax.max())))
    sol.close()

# closed loop: one SQP iteration per tick, the hand-over between ticks on the device
for m in (plain, smooth):
    mpc = ClosedLoopMPC(m, {"warm_start_admm": True}, batch=B, tail="rollout")
    mpc.reset(frame0)
    applied = []
    held = torch.zeros(B, dtype=torch.int32, device="cuda")
    for _ in range(TICKS):
        out = mpc.tick()
        applied.append(out["applied"][:, m.nx:].clone())
        held += (out["status"] != 1).to(torch.int32)
    u = torch.stack(applied, dim=1).cpu().numpy()                  # [B, ticks, nu]: the inputs the plant saw
    state = mpc.x[:, :m.nx].cpu().numpy()
    print("closed loop %-16s %d ticks: mean |state| %.3f -> %.3f, applied sum (du)^2 %.3f, ticks that held the input: %d"
          % (m.name, TICKS, np.linalg.norm(frame0[:, :2], axis=1).mean(), np.linalg.norm(state, axis=1).mean(),
             (np.diff(u, axis=1) ** 2).sum(axis=(1, 2)).mean(), int(held.sum())))
    mpc.close()
