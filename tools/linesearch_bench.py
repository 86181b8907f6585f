#!/usr/bin/env python3
"""The per-instance merit line search (mpcqp_stage_linesearch) next to what it replaces.

Kernel: time of one mpcqp_stage_linesearch launch (K = 4 candidates) against one mpcqp_stage_step + one mpcqp_stage_merit launch, from HIP events
around REPS back-to-back launches, on the first local system of the workload (quadrotor N=20 x 8192, double integrator N=20 x 4096); the QP solve
of the same system is timed the same way for scale.
Loop: SQP iterations per second of DeviceSQPOptimizationSolver with and without options["line_search"] (alpha = 1, one QP per call, ADMM warm
start), the mean accepted alpha per iteration and the worst violation at the end.
usage: python tools/linesearch_bench.py [reps] [iterations]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from optimal_control_problem_amd import models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K = 4


def _timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_leg(name, N, B):
    mdl, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "line_search": {"candidates": K}}, batch=B)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False)                     # leaves q, dw, y, status of the first QP on the device
    ev = sol.ev
    x0 = torch.zeros_like(sol.x); x = x0.clone(); mu = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = dict(sol._ls_out)

    def search():
        x.copy_(x0)
        ev.line_search(arg["p"], x, arg["lbx"], arg["ubx"], sol.ls["q"], sol.dw, sol.y, status=sol.status, mu=mu, alpha0=1.0, candidates=K, out=out)

    def pair():
        x.copy_(x0)
        ev.step(1.0, sol.dw, x, status=sol.status)
        ev.merit(arg["p"], x)

    res = {"copy_ms": _timed(lambda: x.copy_(x0)), "linesearch_ms": _timed(search), "step_plus_merit_ms": _timed(pair), "qp_solve_ms": _timed(lambda: sol.qp.solve(None), 3)}
    for k in ("linesearch_ms", "step_plus_merit_ms"):
        res[k] -= res["copy_ms"]                                    # both legs restore x first; that copy is not theirs
    res["mean_alpha_first_iteration"] = float(sol.alpha_taken.mean())
    sol.close()
    return res


def loop_leg(name, N, B, search):
    mdl, _, meta = models.make_workload(name, B, N=N)
    opts = {"max_iter": 1, "alpha": 1.0, "warm_start_admm": True, "skip_failed_steps": True}
    if search:
        opts["line_search"] = {"candidates": K}
    sol = DeviceSQPOptimizationSolver(mdl, opts, batch=B)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    alphas = []
    for timed in (False, True):
        sol.setInitialGuess(torch.zeros(mdl.nvar, dtype=torch.float64))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(ITERS):
            sol.getOptimalSolution(arg, to_host=False)
            if search and timed:
                alphas.append(sol.alpha_taken.mean())
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    res = {"s": dt, "iterations_per_s": B * ITERS / dt, "worst_gmax": float(sol.gmax.max()), "median_gmax": float(sol.gmax.median()),
           "mean_admm_iters": float(torch.stack(sol.admm_iterations[-ITERS:]).double().mean())}
    if search:
        res["mean_alpha_per_iteration"] = [float(a) for a in alphas]
    sol.close()
    return res


res = {"reps": REPS, "iterations": ITERS, "candidates": K}
for name, N, B in (("quadrotor", 20, 8192), ("double_integrator", 20, 4096)):
    res["%s N=%d batch=%d" % (name, N, B)] = {"kernel": kernel_leg(name, N, B), "loop_fixed_alpha": loop_leg(name, N, B, False),
                                              "loop_line_search": loop_leg(name, N, B, True)}
print(json.dumps(res))
