#!/usr/bin/env python3
"""A fleet of cart-poles that are not the same cart-pole: one nominal controller (ClosedLoopMPC on the zoo model) and, per instance, a plant whose
pole mass and pole length are drawn around the nominal ones.  ClosedLoopMPC.set_instance_params(plant=...) hands every instance's row to the one
mpcqp_stage_advance kernel that plays the plant between two ticks, so the plant-model mismatch is studied without leaving the GPU.  Prints the
closed-loop cost per instance, next to the cost of the same start under the nominal plant."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import ClosedLoopMPC, models

B, TICKS = 8, 40
model = models.CartPole(20, 0.02)                                   # what the controller believes: mc 1.0, mp 0.1, length 0.5
rng = np.random.default_rng(0)
plant = np.tile(model.theta, (B, 1))                                # rows {mc, mp, length, grav}
plant[1:, 1] *= rng.uniform(0.5, 2.0, B - 1)                        # pole mass; instance 0 keeps the nominal plant
plant[1:, 2] *= rng.uniform(0.6, 1.6, B - 1)                        # pole length
frame0 = np.tile([0.0, 0.3, 0.0, 0.0, 0.0], (B, 1))                 # every pole starts 0.3 rad off upright
mpc = ClosedLoopMPC(model, {"warm_start_admm": True}, batch=B, tail="rollout")
mpc.set_instance_params(plant=plant)                                # the controller stays nominal
mpc.reset(frame0)
cost = torch.zeros(B, dtype=torch.float64, device="cuda")
for _ in range(TICKS):
    cost += mpc.tick()["stage_cost"]
state = mpc.x[:, :model.nx].cpu().numpy()
cost = cost.cpu().numpy()
print("%d cart-poles, %d ticks, nominal controller" % (B, TICKS))
for b in range(B):
    print("  plant %d: pole mass %.3f length %.3f  closed-loop cost %8.4f (nominal plant %8.4f)  final angle %+.4f"
          % (b, plant[b, 1], plant[b, 2], cost[b], cost[0], state[b, 1]))
mpc.close()
