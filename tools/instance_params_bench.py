#!/usr/bin/env python3
"""Per-instance plant parameters (mpcqp_stage_set_instance_params) next to the shared ones.

Kernel: time of one mpcqp_stage_eval, one mpcqp_stage_merit and one mpcqp_stage_linesearch (K = 4) launch of the per-instance-parameter (PP)
instance against the shared instance of the same kernel, from HIP events around REPS back-to-back launches on the first local system of the
workload (quadrotor N=20 x 8192, cart-pole N=100 x 16384).  The rows are the shared values, scaled per instance by up to +-20 % on mass / pole length.
Loop: ticks per second of DeviceSQPOptimizationSolver, 2 SQP iterations per tick (alpha = 1, ADMM warm start), with and without the rows, three
runs each; the run without rows is the figure to hold against the parent commit.
usage: python tools/instance_params_bench.py [reps] [ticks]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from optimal_control_problem_amd import models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K = 4
WORKLOADS = (("quadrotor", 20, 8192, 0), ("cartpole", 100, 16384, 2))      # name, N, batch, the parameter scaled (mass; pole length)


def _timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _rows(mdl, B, col):
    th = np.tile(np.asarray(mdl.theta, float), (B, 1))
    th[:, col] *= np.random.default_rng(11).uniform(0.8, 1.2, B)
    return th


def kernel_leg(name, N, B, col):
    mdl, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "line_search": {"candidates": K}}, batch=B)
    has_entry = hasattr(sol, "setInstanceParams")                  # (the parent commit runs the shared legs of this script only)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False)                     # leaves q, dw, y, status of the first QP on the device
    ev = sol.ev
    x0 = torch.zeros_like(sol.x); x = x0.clone(); mu = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = dict(sol._ls_out)

    def search():
        x.copy_(x0)
        ev.line_search(arg["p"], x, arg["lbx"], arg["ubx"], sol.ls["q"], sol.dw, sol.y, status=sol.status, mu=mu, alpha0=1.0, candidates=K, out=out)

    legs = {"eval_ms": lambda: ev.eval(arg["p"], x0, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls), "merit_ms": lambda: ev.merit(arg["p"], x0),
            "linesearch_ms": search}
    res = {}
    for tag in ("shared", "pp") if has_entry else ("shared",):
        sol.setInstanceParams(_rows(mdl, B, col)) if tag == "pp" else None
        copy_ms = _timed(lambda: x.copy_(x0))
        res[tag] = {k: _timed(fn) - (copy_ms if k == "linesearch_ms" else 0.0) for k, fn in legs.items()}      # the search restores x first; that copy is not its own
    sol.close()
    return res


def loop_leg(name, N, B, col, rows):
    mdl, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 2, "alpha": 1.0, "warm_start_admm": True}, batch=B)
    if rows:
        sol.setInstanceParams(_rows(mdl, B, col))
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False); torch.cuda.synchronize()       # warm-up: the first tick pays the set-up
    runs = []
    for _ in range(3):
        sol.setInitialGuess(np.zeros(mdl.nvar))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        runs.append(TICKS / (time.perf_counter() - t0))
    sol.close()
    return runs


if __name__ == "__main__":
    res = {"reps": REPS, "ticks": TICKS, "sqp_iterations_per_tick": 2, "device": torch.cuda.get_device_name(0), "kernel_ms": {}, "loop_ticks_per_s": {}}
    for name, N, B, col in WORKLOADS:
        key = "%s_N%d_x%d" % (name, N, B)
        res["kernel_ms"][key] = kernel_leg(name, N, B, col)
        res["loop_ticks_per_s"][key] = {"shared": loop_leg(name, N, B, col, False)}
        if hasattr(DeviceSQPOptimizationSolver, "setInstanceParams"):
            res["loop_ticks_per_s"][key]["pp"] = loop_leg(name, N, B, col, True)
    print(json.dumps(res))
