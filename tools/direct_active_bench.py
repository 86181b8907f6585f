#!/usr/bin/env python3
"""What the active-set rounds of the direct solve (mpcqp_stage_riccati_solve_active, options["direct_qp"]["active_set"]) cost and buy.

Kernels: HIP-event times of the entry per round count (1, 2, 4, 8) at quadrotor N=20 x 8192 and cart-pole N=100 x 16384, next to mpcqp_stage_riccati_solve
and one mpcqp_solve (full set-up + iteration, cold start) of the same handle, with the verdicts and the mean rounds used on that system.
Loop: ClosedLoopMPC from a rolled-out start, one SQP iteration per tick: accepted share and mean rounds per tick, and ticks per second with "active_set", with
direct_qp alone and with it off (the three loops alternate, so that drift of the box hits all).
JSON to profiles/direct_active_bench.json.
usage: python tools/direct_active_bench.py [reps] [ticks]"""
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
ROUNDS = (1, 2, 4, 8)


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
    res = {"direct_ms": _timed(lambda: ev.riccati_solve(sol.ls, out=plain)), "solve_ms": _timed(lambda: sol.qp.solve(None)),
           "accepted_share_direct": float((plain["direct"] > 0).double().mean()), "rounds": {}}
    for r in ROUNDS:
        out = ev.riccati_solve_active(sol.ls, rounds=r)
        ms = _timed(lambda: ev.riccati_solve_active(sol.ls, rounds=r, out=out))
        took = out["rounds_used"][out["direct"] > 0]
        res["rounds"][str(r)] = {"active_ms": ms, "accepted_share": float((out["direct"] > 0).double().mean()),
                                 "verdicts": {str(v): int((out["direct"] == v).sum()) for v in (1, 0, -1, -2)},
                                 "mean_rounds_of_the_accepted": float(took.double().mean()) if took.numel() else None,
                                 "rejected_in_round_0": int(((out["direct"] == 0) & (out["rounds_used"] == 0)).sum()),
                                 "held_inputs_per_instance": float((out["act"] != 0).double().sum(dim=(1, 2)).mean())}
    res["workspace_bytes"] = 8 * B * N * (ev.nu * (ev.nx + 1) + 2 * (ev.nx + ev.nu) + 1)
    sol.close()
    return res


def loops(name, N, B):
    """accepted share and mean rounds per tick, and ticks per second of the three loops, alternating"""
    mdl, _, meta = models.make_workload(name, B, N=N)
    opts = {"active": {"warm_start_admm": True, "direct_qp": {"active_set": True}}, "direct": {"warm_start_admm": True, "direct_qp": True},
            "off": {"warm_start_admm": True}}
    mpc = {k: ClosedLoopMPC(mdl, o, batch=B) for k, o in opts.items()}
    rate = {k: [] for k in opts}
    out = {}
    for rep in range(3):                                # the first repetition warms the loops up and is not counted
        for k, m in mpc.items():
            m.reset(meta["frame0"], x0="rollout")
            m.sol.direct_history = []; m.sol.direct_rounds_history = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(TICKS):
                m.tick()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep:
                rate[k].append(TICKS / dt)
            if k != "off":
                out["accepted_share_per_tick_" + k] = [float((d > 0).double().mean()) for d in m.sol.direct_history]
            if k == "active":
                out["mean_rounds_per_tick"] = [float(r[d > 0].double().mean()) if bool((d > 0).any()) else None
                                               for d, r in zip(m.sol.direct_history, m.sol.direct_rounds_history)]
                out["rejected_in_round_0_per_tick"] = [int(((d == 0) & (r == 0)).sum()) for d, r in zip(m.sol.direct_history, m.sol.direct_rounds_history)]
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
    path = os.environ.get("DIRECT_ACTIVE_BENCH_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "direct_active_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
