#!/usr/bin/env python3
"""What the dynamically feasible start (mpcqp_stage_rollout, options["initial_guess"]) costs and what it saves.

Kernel: time of one mpcqp_stage_rollout (in place, inputs held, with the box) from HIP events around REPS back-to-back launches, at quadrotor N=20 x 8192 and
cart-pole N=100 x 16384.
First QP: one mpcqp_solve (full set-up + iteration, cold start) on the first local system of the workload, linearised at x = 0 and at the rolled-out start: ms from
HIP events, the status histogram, mean and max ADMM iterations.
Loop: ticks per second of DeviceSQPOptimizationSolver (2 SQP iterations per tick, every tick from a fresh zero iterate) with and without the option.
usage: python tools/rollout_bench.py [reps] [ticks]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
CASES = (("quadrotor", 20, 8192), ("cartpole", 100, 16384))


def _timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _args(sol, mdl, meta):
    return {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}


def kernel_and_first_qp(name, N, B):
    mdl, _, meta = models.make_workload(name, B, N=N)
    res = {}
    for key, extra in (("zero_start", {}), ("rollout_start", {"initial_guess": "rollout"})):
        sol = DeviceSQPOptimizationSolver(mdl, dict({"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True}, **extra), batch=B)
        arg = _args(sol, mdl, meta)
        if extra:
            x = torch.zeros((B, mdl.nvar), dtype=torch.float64, device=sol.dev)
            res["rollout_kernel_ms"] = _timed(lambda: sol.ev.rollout(x, None, arg["lbx"], arg["ubx"], inputs="hold"))
            res["rollout_bytes_moved"] = 2 * 8 * mdl.nvar * B
        sol.getOptimalSolution(arg, to_host=False)                 # leaves the first local system on the device, borrowed by the handle
        if extra:
            res["rollout_diverged_instances"] = int((sol.rollout_diverged >= 0).sum())
            res["rollout_box_viol_max"] = float(sol.rollout_box_viol.max())
        ms = _timed(lambda: sol.qp.solve(None))
        st = sol.status.cpu().numpy(); it = sol.iters.cpu().numpy()
        res[key] = {"variant": sol.qp.plan_info()["variant"], "first_solve_ms": ms, "status_histogram": {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                    "admm_iterations_mean": float(it.mean()), "admm_iterations_max": int(it.max())}
        sol.close()
    return res


def loop_leg(name, N, B, option):
    mdl, _, meta = models.make_workload(name, B, N=N)
    opts = {"max_iter": 2, "alpha": 1.0, "skip_failed_steps": True}
    if option:
        opts["initial_guess"] = option
    sol = DeviceSQPOptimizationSolver(mdl, opts, batch=B)
    arg = _args(sol, mdl, meta)
    x0 = torch.zeros(mdl.nvar, dtype=torch.float64)
    for timed in (False, True):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.setInitialGuess(x0)
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    st = sol.status.cpu().numpy()
    res = {"ticks_per_s": TICKS / dt, "last_status_histogram": {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
           "admm_iterations_mean": [float(t.double().mean()) for t in sol.admm_iterations[-2:]]}
    sol.close()
    return res


if __name__ == "__main__":
    out = {"reps": REPS, "ticks": TICKS, "first_qp": {}, "loop": {}}
    for name, N, B in CASES:
        tag = "%s_N%d_B%d" % (name, N, B)
        out["first_qp"][tag] = kernel_and_first_qp(name, N, B)
        out["loop"][tag] = {"zero_start": loop_leg(name, N, B, None), "initial_guess_rollout": loop_leg(name, N, B, "rollout")}
    print(json.dumps(out))
