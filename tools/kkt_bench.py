#!/usr/bin/env python3
"""The NLP optimality residuals on the device (mpcqp_stage_kkt) next to the launches around them.

Kernel: time of one mpcqp_stage_kkt launch against one mpcqp_stage_eval launch and one QP solve of the same build, from HIP events around REPS
back-to-back launches, on the first local system of the workload (quadrotor N=20 x 8192, cart-pole N=100 x 16384), and the bytes the kernel streams
per instance (q, A, l, u, y once) with the bandwidth that makes.
Loop: ticks per second of DeviceSQPOptimizationSolver (one tick = one getOptimalSolution of up to MAX_ITER iterations, all instances) with and
without options["kkt_tol"], on a quadrotor batch of which a known share starts at the reference -- those instances meet the tolerance at the first
check, the others later or never within MAX_ITER; the saving comes only when the whole batch is done, so both shares 100 % and 50 % are run.
usage: python tools/kkt_bench.py [reps] [ticks]"""
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
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
MAX_ITER, TOL = 6, 1e-2


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
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0}, batch=B)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False)                     # leaves the local system and y of the first QP on the device
    ev = sol.ev
    out = ev.kkt(sol.ls, sol.y, TOL)
    res = {"kkt_ms": _timed(lambda: ev.kkt(sol.ls, sol.y, TOL, out=out)),
           "eval_ms": _timed(lambda: ev.eval(arg["p"], sol.x, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls)),
           "qp_solve_ms": _timed(lambda: sol.qp.solve(None), 3)}
    per = 8 * (ev.n + ev.nnzA + 3 * ev.m)
    res["bytes_per_instance"] = per
    res["kkt_GBps"] = per * B / (res["kkt_ms"] * 1e-3) / 1e9
    sol.close()
    return res


def loop_leg(B, share, kkt):
    """quadrotor N = 20: `share` of the instances start at the hover reference (converged at the first check), the rest at the workload's states"""
    mdl, _, meta = models.make_workload("quadrotor", B, N=20)
    easy = int(round(share * B))
    lbx, ubx = meta["lbx"].copy(), meta["ubx"].copy()
    frame0 = np.concatenate([np.zeros(12), np.full(4, mdl.hover_thrust)])
    lbx[:easy, :mdl.f] = frame0; ubx[:easy, :mdl.f] = frame0
    opts = {"max_iter": MAX_ITER, "alpha": 1.0, "skip_failed_steps": True}
    if kkt:
        opts["kkt_tol"] = TOL
    sol = DeviceSQPOptimizationSolver(mdl, opts, batch=B)
    arg = {k: sol._dev(v, w) for k, v, w in (("p", meta["p"], mdl.np), ("lbx", lbx, mdl.nvar), ("ubx", ubx, mdl.nvar), ("lbg", meta["lbg"], mdl.ng),
                                             ("ubg", meta["ubg"], mdl.ng))}
    x0 = torch.zeros(mdl.nvar, dtype=torch.float64)
    done = []
    for timed in (False, True):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.setInitialGuess(x0)
            sol.getOptimalSolution(arg, to_host=False)
            done.append(sol.iterations_done)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    res = {"ticks_per_s": TICKS / dt, "qps_per_tick": done[-1]}
    if kkt:
        res["converged_share"] = float(sol.converged.double().mean())
        res["converged_at_histogram"] = np.bincount(sol.converged_at.cpu().numpy() + 1, minlength=MAX_ITER + 1).tolist()    # index 0: never
    sol.close()
    return res


if __name__ == "__main__":
    out = {"reps": REPS, "ticks": TICKS, "max_iter": MAX_ITER, "kkt_tol": TOL, "kernel": {}, "loop": {}}
    for name, N, B in (("quadrotor", 20, 8192), ("cartpole", 100, 16384)):
        out["kernel"]["%s_N%d_B%d" % (name, N, B)] = kernel_leg(name, N, B)
    for share in (1.0, 0.5):
        out["loop"]["quadrotor_N20_B2048_easy_%d" % round(100 * share)] = {"fixed": loop_leg(2048, share, False), "kkt_tol": loop_leg(2048, share, True)}
    print(json.dumps(out))
