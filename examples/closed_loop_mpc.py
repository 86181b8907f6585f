#!/usr/bin/env python3
"""Closed-loop MPC of the README's pendulum with every tick on the GPU: ClosedLoopMPC solves at the pinned first frame, then one
mpcqp_stage_advance kernel applies the plant (the model's own traced map), shifts the trajectory and the ADMM start by one stage and pins the
new first frame.  Nothing is copied to the host inside the loop; the log is read back once at the end."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import ClosedLoopMPC, models


class MyPlant(models.StageOCP):
    nx, nu, name = 2, 1, "my_plant"

    def F(self, s, u):                                             # discrete map, NumPy; traced once, emitted as device code
        return np.stack([s[..., 0] + 0.05 * s[..., 1], s[..., 1] + 0.05 * (u[..., 0] - np.sin(s[..., 0]))], axis=-1)

    def frame_bounds(self):
        return np.array([-np.inf, -4.0, -2.0]), np.array([np.inf, 4.0, 2.0])


B, TICKS = 256, 30
plant = MyPlant(20, 0.05, Q=[10.0, 1.0], R=[0.1])
frame0 = np.concatenate([np.random.default_rng(0).uniform(-1, 1, (B, 2)), np.zeros((B, 1))], axis=1)
mpc = ClosedLoopMPC(plant, {"warm_start_admm": True}, batch=B, tail="rollout")
mpc.reset(frame0)                                                  # reference p = 0: drive the pendulum to the origin
cost = torch.zeros(B, dtype=torch.float64, device="cuda")
held = torch.zeros(B, dtype=torch.int32, device="cuda")
for _ in range(TICKS):
    out = mpc.tick()                                               # device tensors: applied, status, iters, stage_cost
    cost += out["stage_cost"]
    held += (out["status"] != 1).to(torch.int32)
state = mpc.x[:, :plant.nx].cpu().numpy()
print("%d pendulums, %d ticks: mean |state| %.3f -> %.3f, mean closed-loop cost %.3f, ticks that held the input: %d"
      % (B, TICKS, np.linalg.norm(frame0[:, :2], axis=1).mean(), np.linalg.norm(state, axis=1).mean(), float(cost.mean()), int(held.sum())))
mpc.close()
