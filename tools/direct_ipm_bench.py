#!/usr/bin/env python3
"""What the interior-point iterations of the direct solve (mpcqp_stage_riccati_solve_ipm, options["direct_qp"]["interior_point"]) cost and buy.

Kernels: HIP-event times of the entry at quadrotor N=20 x 8192 and cart-pole N=100 x 16384, next to mpcqp_stage_riccati_solve, mpcqp_stage_riccati_solve_active
(rounds 4) and one mpcqp_solve (full set-up + iteration, cold start) of the same handle, with the verdicts and the mean and largest number of iterations on that system.
Loop: ClosedLoopMPC from a rolled-out start, one SQP iteration per tick: accepted share and mean iterations per tick, and ticks per second with
"interior_point", with direct_qp alone and with it off (the three loops alternate, so that drift of the box hits all).
JSON to profiles/direct_ipm_bench.json.
usage: python tools/direct_ipm_bench.py [reps] [ticks]"""
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
ITERS = (10, 30)


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
    plain = ev.riccati_solve(sol.ls)
    act = ev.riccati_solve_active(sol.ls, rounds=4)
    res = {"direct_ms": _timed(lambda: ev.riccati_solve(sol.ls, out=plain)), "active4_ms": _timed(lambda: ev.riccati_solve_active(sol.ls, rounds=4, out=act)),
           "solve_ms": _timed(lambda: sol.qp.solve(None)), "accepted_share_direct": float((plain["direct"] > 0).double().mean()),
           "accepted_share_active4": float((act["direct"] > 0).double().mean()), "iters": {}}
    for it in ITERS:
        out = ev.riccati_solve_ipm(sol.ls, iters=it)
        ms = _timed(lambda: ev.riccati_solve_ipm(sol.ls, iters=it, out=out))
        acc = out["direct"] > 0
        took = out["iters_used"][acc]
        res["iters"][str(it)] = {"ipm_ms": ms, "accepted_share": float(acc.double().mean()),
                                 "verdicts": {str(v): int((out["direct"] == v).sum()) for v in (1, 0, -1, -2)},
                                 "mean_iters_of_the_accepted": float(took.double().mean()) if took.numel() else None,
                                 "max_iters_of_the_accepted": int(took.max()) if took.numel() else None,
                                 "mean_iters_of_the_rejected": float(out["iters_used"][out["direct"] == 0].double().mean()) if bool((out["direct"] == 0).any()) else None,
                                 "worst_res_of_the_accepted": [float(v) for v in out["res"][acc].max(dim=0).values] if took.numel() else None}
    res["workspace_bytes"] = 8 * B * N * (ev.nu * (ev.nx + 1) + 7 * (ev.nx + ev.nu))
    sol.close()
    return res


def loops(name, N, B):
    """accepted share and mean iterations per tick, and ticks per second of the three loops, alternating"""
    mdl, _, meta = models.make_workload(name, B, N=N)
    opts = {"ipm": {"warm_start_admm": True, "direct_qp": {"interior_point": True}}, "direct": {"warm_start_admm": True, "direct_qp": True},
            "off": {"warm_start_admm": True}}
    mpc = {k: ClosedLoopMPC(mdl, o, batch=B) for k, o in opts.items()}
    rate = {k: [] for k in opts}
    out = {}
    for rep in range(3):                                # the first repetition warms the loops up and is not counted
        for k, m in mpc.items():
            m.reset(meta["frame0"], x0="rollout")
            m.sol.direct_history = []; m.sol.direct_iters_history = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(TICKS):
                m.tick()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep:
                rate[k].append(TICKS / dt)
            if k != "off":
                out["accepted_share_per_tick_" + k] = [float((d > 0).double().mean()) for d in m.sol.direct_history]
            if k == "ipm":
                out["mean_iters_per_tick"] = [float(r[d > 0].double().mean()) if bool((d > 0).any()) else None
                                              for d, r in zip(m.sol.direct_history, m.sol.direct_iters_history)]
                out["max_iters_per_tick"] = [int(r.max()) for r in m.sol.direct_iters_history]
    for m in mpc.values():
        m.close()
    out.update({"ticks_per_s_" + k: v for k, v in rate.items()})
    return out


def main():
    out = {"reps": REPS, "ticks": TICKS, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, N, B in CASES:
        key = "%s_N%d_x%d" % (name, N, B)
        out["cases"][key] = kernels(name, N, B)
        out["cases"][key]["closed_loop"] = loops(name, N, B)
        print(key, json.dumps(out["cases"][key]), flush=True)
    path = os.environ.get("DIRECT_IPM_BENCH_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "direct_ipm_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
