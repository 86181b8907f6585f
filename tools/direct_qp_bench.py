#!/usr/bin/env python3
"""What the direct solve of the stage QP (mpcqp_stage_riccati_solve, options["direct_qp"]) costs and buys.

Kernels: HIP-event times of the direct solve at quadrotor N=20 x 8192 and cart-pole N=100 x 16384, next to the gain sweep (mpcqp_stage_riccati without V)
and one mpcqp_solve (full set-up + iteration, cold start) of the same handle, and the share of the batch the kernel accepted on that system.
Loop: ClosedLoopMPC from a rolled-out start, one SQP iteration per tick: the accepted share per tick, and ticks per second with the option and on the same commit with the option off
(the two loops alternate, so that drift of the box hits both).  Break-even: the option pays when the accepted share exceeds kernel time / solve time.
JSON to profiles/direct_qp_bench.json.
usage: python tools/direct_qp_bench.py [reps] [ticks]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from optimal_control_problem_amd import ClosedLoopMPC, models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
CASES = (("quadrotor", 20, 8192), ("cartpole", 100, 16384))


def _timed(fn, reps=REPS):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(name, N, B):
    mdl, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True, "initial_guess": "rollout"}, batch=B)
    ev = sol.ev
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False)
    ev.eval(arg["p"], sol.x, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls)
    out = ev.riccati_solve(sol.ls)
    g = ev.riccati(sol.ls, V=False)
    f = ev.nx + ev.nu
    res = {"direct_ms": _timed(lambda: ev.riccati_solve(sol.ls, out=out)),
           "direct_without_z_ms": _timed(lambda: ev.riccati_solve(sol.ls, out=dict(out, z=None))),
           "riccati_without_V_ms": _timed(lambda: ev.riccati(sol.ls, K=g["K"], V=False, failed=g["failed"])),
           "solve_ms": _timed(lambda: sol.qp.solve(None)),
           "accepted_share_at_the_second_iterate": float((out["direct"] > 0).double().mean()),
           "verdicts": {str(v): int((out["direct"] == v).sum()) for v in (1, 0, -1, -2)},
           "workspace_bytes": 8 * B * N * (ev.nu * (ev.nx + 1) + f)}
    res["break_even_share"] = res["direct_without_z_ms"] / res["solve_ms"]
    sol.close()
    return res


def loops(name, N, B):
    """accepted share per tick, and ticks per second of both loops, alternating"""
    mdl, _, meta = models.make_workload(name, B, N=N)
    mpc = {True: ClosedLoopMPC(mdl, {"warm_start_admm": True, "direct_qp": True}, batch=B), False: ClosedLoopMPC(mdl, {"warm_start_admm": True}, batch=B)}
    rate = {True: [], False: []}
    shares = None
    for rep in range(3):                                # the first repetition warms both loops up and is not counted
        for on in (True, False):
            m = mpc[on]
            m.reset(meta["frame0"], x0="rollout")
            m.sol.direct_history = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(TICKS):
                m.tick()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep:
                rate[on].append(TICKS / dt)
            if on:
                shares = [float((d > 0).double().mean()) for d in m.sol.direct_history]
    for m in mpc.values():
        m.close()
    return {"accepted_share_per_tick": shares, "ticks_per_s_with": rate[True], "ticks_per_s_without": rate[False]}


def main():
    out = {"reps": REPS, "ticks": TICKS, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, N, B in CASES:
        key = "%s_N%d_x%d" % (name, N, B)
        out["cases"][key] = kernels(name, N, B)
        out["cases"][key]["closed_loop"] = loops(name, N, B)
        print(key, json.dumps(out["cases"][key]), flush=True)
    path = os.environ.get("DIRECT_QP_BENCH_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "direct_qp_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
