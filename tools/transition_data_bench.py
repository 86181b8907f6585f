#!/usr/bin/env python3
"""Transition data on the stage path (models.StageOCP.transition_data): what reading the frame's row in F, kfun and llink costs.

Two generated libraries of one model, same build, same box: models.GridCartPole (the step length h_k is stage data of its own RK4, of the rate limit
and of the move penalty; a stored set [batch, N, 1] in force) against its twin with the same number written as a constant.
Kernel: time of one mpcqp_stage_eval, _merit, _linesearch (K = 4), _rollout and _advance launch of either library, from HIP events around REPS
back-to-back launches, median of RUNS such measurements after a warm-up launch.
Loop: ticks per second of DeviceSQPOptimizationSolver, 2 SQP iterations per tick (alpha = 1, ADMM warm start), median of RUNS runs of TICKS ticks.
usage: python tools/transition_data_bench.py [reps] [ticks] [runs]     prints one JSON line"""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import _lib, models

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
K = 4
WORKLOADS = ((100, 16384), (20, 8192))

BakedGridCartPole = type("BakedGridCartPole", (models.GridCartPole,), {"nsd": 0, "transition_data": False, "name": "grid_cartpole_baked"})


def _median_ms(fn):
    import torch
    fn(); torch.cuda.synchronize()                                 # warm-up
    runs = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record(); torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / REPS)
    return float(np.median(runs))


def _solver(cls, N, B, options):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl = cls(N, 0.02)
    _, _, meta = models.make_workload("cartpole", B, N=N)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(meta["frame0"])
    sol = DeviceSQPOptimizationSolver(mdl, options, batch=B, codegen=True)
    if mdl.nsd:
        sol.setStageData(mdl.grid_rows(B))
    arg = {k: sol._dev(v, w) for k, v, w in (("p", meta["p"], mdl.np), ("lbx", lbx, mdl.nvar), ("ubx", ubx, mdl.nvar), ("lbg", lbg, mdl.ng), ("ubg", ubg, mdl.ng))}
    return mdl, sol, arg, meta


def kernel_leg(cls, N, B):
    import torch
    mdl, sol, arg, meta = _solver(cls, N, B, {"max_iter": 1, "alpha": 1.0, "line_search": {"candidates": K}})
    sol.setInitialGuess(meta["x_iterate"])
    x0 = sol.x.clone()
    sol.getOptimalSolution(arg, to_host=False)                     # leaves q, dw, y, status of the first QP on the device
    ev = sol.ev
    assert ev.transition_data == bool(mdl.transition_data)
    x = x0.clone(); mu = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = dict(sol._ls_out)
    x2 = torch.empty_like(x0); lbx, ubx = arg["lbx"].clone(), arg["ubx"].clone()
    div = torch.zeros(B, dtype=torch.int32, device="cuda"); viol = torch.zeros(B, dtype=torch.float64, device="cuda")

    def search():
        x.copy_(x0)
        ev.line_search(arg["p"], x, arg["lbx"], arg["ubx"], sol.ls["q"], sol.dw, sol.y, status=sol.status, mu=mu, alpha0=1.0, candidates=K, out=out)

    copy_ms = _median_ms(lambda: x.copy_(x0))
    res = {"eval_ms": _median_ms(lambda: ev.eval(arg["p"], x0, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls)),
           "merit_ms": _median_ms(lambda: ev.merit(arg["p"], x0)),
           "linesearch_ms": _median_ms(search) - copy_ms,          # the search restores x first; that copy is not its own
           "rollout_ms": _median_ms(lambda: ev.rollout(x0, x2, arg["lbx"], arg["ubx"], diverged=div, box_viol=viol)),
           "advance_ms": _median_ms(lambda: ev.advance(x0, x2, lbx, ubx, status=sol.status, tail="rollout", p=arg["p"]))}
    sol.close()
    return res


def loop_leg(cls, N, B):
    import torch
    mdl, sol, arg, meta = _solver(cls, N, B, {"max_iter": 2, "alpha": 1.0, "warm_start_admm": True})
    sol.getOptimalSolution(arg, to_host=False); torch.cuda.synchronize()       # warm-up: the first tick pays the set-up
    runs = []
    for _ in range(RUNS):
        sol.setInitialGuess(np.zeros(mdl.nvar))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        runs.append(TICKS / (time.perf_counter() - t0))
    sol.close()
    return {"median": float(np.median(runs)), "runs": runs}


if __name__ == "__main__":
    import torch
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    res = {"reps": REPS, "ticks": TICKS, "runs": RUNS, "sqp_iterations_per_tick": 2, "device": torch.cuda.get_device_name(0), "lib_sha16": sha,
           "date": time.strftime("%Y-%m-%d"), "kernel_ms": {}, "loop_ticks_per_s": {}}
    for N, B in WORKLOADS:
        key = "grid_cartpole_N%d_x%d" % (N, B)
        res["kernel_ms"][key] = {"baked": kernel_leg(BakedGridCartPole, N, B), "data": kernel_leg(models.GridCartPole, N, B)}
        res["loop_ticks_per_s"][key] = {"baked": loop_leg(BakedGridCartPole, N, B), "data": loop_leg(models.GridCartPole, N, B)}
        print(key, json.dumps(res["kernel_ms"][key]), file=sys.stderr, flush=True)
    print(json.dumps(res))
