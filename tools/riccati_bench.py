#!/usr/bin/env python3
"""What the feedback gains (mpcqp_stage_riccati, mpcqp_stage_feedback) cost.

Kernels: HIP-event times of the Riccati sweep (with the clamp) and of the feedback launch at quadrotor N=20 x 8192 and cart-pole N=100 x 16384, next to the eval
kernel and one mpcqp_solve (full set-up + iteration, cold start) of the same batch, and the sweep as a share of both.
Loop: plant steps per second of ClosedLoopMPC(feedback=True) with a solve every 1, 2 and 4 plant steps (the others are holds), and of the loop without the option.
JSON to profiles/riccati_bench.json.
usage: python tools/riccati_bench.py [reps] [steps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from optimal_control_problem_amd import ClosedLoopMPC, models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
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
    nx, f = ev.nx, ev.nx + ev.nu
    g = ev.riccati(sol.ls, x=sol.x, lbx=arg["lbx"], ubx=arg["ubx"])
    x2 = sol.x.clone()
    res = {"riccati_ms": _timed(lambda: ev.riccati(sol.ls, x=sol.x, lbx=arg["lbx"], ubx=arg["ubx"], K=g["K"], V=g["V"], failed=g["failed"])),
           "riccati_without_V_ms": _timed(lambda: ev.riccati(sol.ls, x=sol.x, lbx=arg["lbx"], ubx=arg["ubx"], K=g["K"], V=False, failed=g["failed"])),
           "feedback_ms": _timed(lambda: ev.feedback(g["K"], 1, x2[:, :nx], sol.x[:, f:f + nx], sol.x[:, f + nx:2 * f], x2)),
           "eval_ms": _timed(lambda: ev.eval(arg["p"], sol.x, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls)),
           "solve_ms": _timed(lambda: sol.qp.solve(None)),
           "sweeps_failed": int((g["failed"] >= 0).sum()),
           "riccati_bytes_read": 8 * B * (N * f * f + (N - 1) * nx * f), "riccati_bytes_written": 8 * B * N * (ev.nu * nx + nx * nx)}
    res["riccati_share_of_eval"] = res["riccati_ms"] / res["eval_ms"]
    res["riccati_share_of_solve"] = res["riccati_ms"] / res["solve_ms"]
    sol.close()
    return res


def loop(name, N, B, every):
    """plant steps per second; every = 0: the loop without the option, a solve every step"""
    mdl, _, meta = models.make_workload(name, B, N=N)
    mpc = ClosedLoopMPC(mdl, {"warm_start_admm": True}, batch=B, feedback=True if every else None)
    for timed in (False, True):
        mpc.reset(meta["frame0"], x0="rollout")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(STEPS):
            if not every or i % every == 0:
                mpc.tick()
            else:
                mpc.hold()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    mpc.close()
    return STEPS / dt


def main():
    out = {"reps": REPS, "steps": STEPS, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, N, B in CASES:
        key = "%s_N%d_x%d" % (name, N, B)
        out["cases"][key] = kernels(name, N, B)
        out["cases"][key]["plant_steps_per_s"] = {"without_feedback": loop(name, N, B, 0), "solve_every_1": loop(name, N, B, 1),
                                                  "solve_every_2": loop(name, N, B, 2), "solve_every_4": loop(name, N, B, 4)}
        print(key, json.dumps(out["cases"][key]), flush=True)
    path = os.environ.get("RICCATI_BENCH_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "riccati_bench.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
