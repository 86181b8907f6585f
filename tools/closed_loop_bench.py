#!/usr/bin/env python3
"""Closed-loop ticks per second and mean ADMM iterations per tick of mpc.ClosedLoopMPC -- the hand-over between two ticks in one kernel
(mpcqp_stage_advance) -- with the shifted start (shift=True), with the reference's unshifted one (shift=False), and of the loop composed from
torch launches the way tools/mpc_loop_bench.py composes it (slice assignments into lbx / ubx, torch.where on the status, the plant written out in
torch).  One QP per tick, full step, ADMM warm start, in every leg.  Double integrator N=20 at batch 1, 256 and 4096; quadrotor N=20 at batch
4096 without the composed leg (that loop has no quadrotor plant).  Every leg runs in this process after a warm-up loop.
usage: python tools/closed_loop_bench.py [ticks]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import models
from optimal_control_problem_amd.mpc import ClosedLoopMPC
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

T = int(sys.argv[1]) if len(sys.argv) > 1 else 60
WARMUP = 5
OPTS = {"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True, "warm_start_admm": True}


def _report(B, dt, its, failed):
    it = torch.stack(its).double()
    return {"s": dt, "ticks_per_s": B * T / dt, "mean_admm_iters": float(it.mean()), "infeasible_ticks": int(failed)}


def closed_loop(mdl, meta, B, shift):
    mpc = ClosedLoopMPC(mdl, OPTS, batch=B, tail="rollout", shift=shift)
    mpc.reset(meta["frame0"], meta["p"])
    for _ in range(WARMUP):
        mpc.tick()
    mpc.reset(meta["frame0"], meta["p"])
    failed = torch.zeros((), dtype=torch.int64, device="cuda")
    n0 = len(mpc.sol.admm_iterations)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(T):
        st = mpc.tick()["status"]
        failed += ((st != 1) & (st != 2) & (st != 7)).sum()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    out = _report(B, dt, mpc.sol.admm_iterations[n0:], failed)
    mpc.close()
    return out


def composed_loop(mdl, meta, B):
    """tools/mpc_loop_bench.py's loop (double integrator only: its plant is that model's formulas in torch)"""
    nx, nu, f, N, h = mdl.nx, mdl.nu, mdl.f, mdl.N, mdl.dt
    dev = DeviceSQPOptimizationSolver(mdl, OPTS, batch=B)
    out = None
    for timed in (False, True):
        arg = {k: torch.as_tensor(meta[k], dtype=torch.float64, device="cuda") for k in ("lbx", "ubx", "lbg", "ubg", "p")}
        state = torch.as_tensor(meta["frame0"][:, :nx], dtype=torch.float64, device="cuda").clone()
        u_now = torch.zeros((B, nu), dtype=torch.float64, device="cuda")
        dev.setInitialGuess(np.zeros(mdl.nvar))
        failed = torch.zeros((), dtype=torch.int64, device="cuda")
        n0 = len(dev.admm_iterations)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(T if timed else WARMUP):
            arg["lbx"][:, :nx] = state; arg["ubx"][:, :nx] = state
            arg["lbx"][:, nx:f] = u_now; arg["ubx"][:, nx:f] = u_now
            X = dev.getOptimalSolution(arg, to_host=False)["x"].view(B, N, f)
            pos = state[:, 0] + h * state[:, 1] + 0.5 * h * h * u_now[:, 0]
            vel = state[:, 1] + h * u_now[:, 0]
            state = torch.stack([pos, vel], dim=1)
            ok = (dev.status == 1).unsqueeze(1)
            u_now = torch.where(ok, X[:, 1, nx:], u_now)
            failed += (~ok).sum()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        out = _report(B, dt, dev.admm_iterations[n0:], failed)
    dev.close()
    return out


res = {"ticks": T, "options": OPTS}
legs = [("double_integrator", 20, b) for b in (1, 256, 4096)] + [("quadrotor", 20, 4096)]
closed_loop(*models.make_workload("double_integrator", 16)[::2], 16, True)      # the first loop in a process pays torch / HIP lazy initialisation
for name, N, B in legs:
    mdl, _, meta = models.make_workload(name, B, N=N)
    leg = {"shift": closed_loop(mdl, meta, B, True), "no_shift": closed_loop(mdl, meta, B, False)}
    if name == "double_integrator":
        leg["composed_torch"] = composed_loop(mdl, meta, B)
    res["%s N=%d batch=%d" % (name, N, B)] = leg
print(json.dumps(res))
