#!/usr/bin/env python3
"""What leaving instances out of a QP launch (mpcqp_set_skip) saves, and what it costs a launch that skips nothing.

QP launch: time of one mpcqp_solve (full set-up + iteration, cold start; the compaction kernel, the validation and the dispatch-order kernel included) from HIP events
around REPS back-to-back solves, on the first local system of the workload -- quadrotor N=20 x 8192 (four-wave two-kernel on-chip form) and cart-pole N=100 x 16384
(the eight-wave ticket form) -- without a skip array, with an all-zero array (the price of the feature where it saves nothing: the compaction kernel and one
indirection), and with a seeded random 50 %, 90 %, 99 % and 100 % of the instances skipped (100 %: what a launch of empty workgroups costs).
Loop: ticks per second of DeviceSQPOptimizationSolver on the second case of tools/kkt_bench.py (quadrotor N=20 x 2048, max_iter 6, half of the instances starting at
the reference) with the fixed iteration count, with options["kkt_tol"], and with options["skip_converged_qps"] next to it.
usage: python tools/skip_bench.py [reps] [ticks]"""
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
MAX_ITER, TOL = 6, 1e-2
SHARES = (0.5, 0.9, 0.99, 1.0)


def _timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launch_leg(name, N, B):
    mdl, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0}, batch=B)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False)                     # leaves the first local system on the device, borrowed by the handle
    qp = sol.qp
    res = {"variant": qp.plan_info()["variant"], "no_skip_array_ms": _timed(lambda: qp.solve(None))}
    skip = torch.zeros(B, dtype=torch.int32, device=sol.dev)
    qp.set_skip(skip)
    res["all_zero_array_ms"] = _timed(lambda: qp.solve(None))
    rng = np.random.default_rng(7)
    for share in SHARES:
        mk = np.zeros(B, np.int32)
        mk[rng.permutation(B)[:int(round(share * B))]] = 1
        skip.copy_(torch.as_tensor(mk))                            # (in place: the array is borrowed)
        res["skipped_%g_percent_ms" % (100 * share)] = _timed(lambda: qp.solve(None))
    qp.set_skip(None)
    res["no_skip_array_again_ms"] = _timed(lambda: qp.solve(None))
    sol.close()
    return res


def loop_leg(B, share, kkt, skip):
    """quadrotor N = 20: `share` of the instances start at the hover reference (converged at the first check), the rest at the workload's states"""
    mdl, _, meta = models.make_workload("quadrotor", B, N=20)
    easy = int(round(share * B))
    lbx, ubx = meta["lbx"].copy(), meta["ubx"].copy()
    frame0 = np.concatenate([np.zeros(12), np.full(4, mdl.hover_thrust)])
    lbx[:easy, :mdl.f] = frame0; ubx[:easy, :mdl.f] = frame0
    opts = {"max_iter": MAX_ITER, "alpha": 1.0, "skip_failed_steps": True}
    if kkt:
        opts["kkt_tol"] = TOL
    if skip:
        opts["skip_converged_qps"] = True
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
        res["x_checksum"] = float(sol.x.double().nan_to_num().abs().sum())      # (equal with and without skip_converged_qps: the loop's x is bit for bit the same)
    sol.close()
    return res


if __name__ == "__main__":
    out = {"reps": REPS, "ticks": TICKS, "max_iter": MAX_ITER, "kkt_tol": TOL, "launch": {}, "loop": {}}
    for name, N, B in (("quadrotor", 20, 8192), ("cartpole", 100, 16384)):
        out["launch"]["%s_N%d_B%d" % (name, N, B)] = launch_leg(name, N, B)
    out["loop"]["quadrotor_N20_B2048_easy_50"] = {"fixed": loop_leg(2048, 0.5, False, False), "kkt_tol": loop_leg(2048, 0.5, True, False),
                                                  "kkt_tol+skip_converged_qps": loop_leg(2048, 0.5, True, True)}
    print(json.dumps(out))
