#!/usr/bin/env python3
"""The exact Lagrangian Hessian on the device (mpcqp_stage_lagrangian): what it costs next to the evaluation, and what it buys the loop.

Kernel: the cart-pole (N = 100, batch 16384) and the quadrotor (N = 20, batch 8192) written as generated models with a quadratic lcost, exact_hessian and
convexify, one library each: the time of one mpcqp_stage_eval launch, of eval + lagrangian with mode 0 (the add kernel) and of eval + lagrangian with
mode project (add, convexify H_k + C_k, sum) under random multipliers: HIP events around REPS back-to-back launches, median of RUNS such measurements
after a warm-up launch.  The comparison is against the eval kernel of the same library in the same run.
Loop: DeviceSQPOptimizationSolver on the pendulum swing of examples/exact_hessian_sqp.py (th = 2 beyond the torque limit, dt = 0.2, N = 10, batch 4096, alpha = 1,
skip_failed_steps, stop when every instance moved by less than 1e-3 or after 30 iterations), option off and on: SQP iterations to the stop and solves
per second, median of RUNS runs.
usage: python tools/exact_hessian_bench.py [reps] [runs]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import models

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LOOP_BATCH, LOOP_N, LOOP_DT, LOOP_MAX, LOOP_TOL = 4096, 10, 0.2, 30, 1e-3


def _tracking(s, u, r, wq, wr):
    v = 0.0
    for i, q in enumerate(wq):
        e = s[..., i] - r[..., i]
        v = v + q * e * e + 0.05 * s[..., i] * s[..., i] + 0.02 * r[..., i] * r[..., i]
    for i, q in enumerate(wr):
        v = v + q * u[..., i] * u[..., i]
    return v


class CartPoleExact(models.CartPole):
    name = "cartpole_exact_bench"
    exact_hessian = True
    convexify = True

    def lcost(self, s, u, r):
        return _tracking(s, u, r, (1.0, 10.0, 0.1, 0.1), (0.01,))


class QuadrotorExact(models.Quadrotor):
    name = "quadrotor_exact_bench"
    exact_hessian = True
    convexify = True

    def lcost(self, s, u, r):
        return _tracking(s, u, r, [10.0] * 3 + [1.0] * 6 + [0.1] * 3, [0.1] * 4)


class PendulumSwing(models.StageOCP):
    nx, nu, name = 2, 1, "pendulum_swing_bench"
    nh = 1; h_lo = [-np.inf]; h_hi = [2.0]
    exact_hessian = True

    def F(self, s, u):
        th, w = s[..., 0], s[..., 1]
        return np.stack([th + self.dt * w, w + self.dt * (-9.81 * np.sin(th) + 0.5 * u[..., 0] * np.cos(th) - 0.1 * w)], axis=-1)

    def hfun(self, s, u):
        th, w, v = s[..., 0], s[..., 1], u[..., 0]
        return np.stack([th * th + 0.5 * v * v + 0.3 * th * w], axis=-1)

    def lcost(self, s, u, r):
        e0, e1 = s[..., 0] - r[..., 0], s[..., 1] - r[..., 1]
        return 2.0 * e0 * e0 + 0.5 * e1 * e1 + 0.05 * u[..., 0] * u[..., 0]

    def frame_bounds(self):
        return np.array([-10.0, -20.0, -3.0]), np.array([10.0, 20.0, 3.0])


def _swing():
    return PendulumSwing(LOOP_N, LOOP_DT, Q=[2.0, 0.5], R=[0.05])


def models_to_build():
    """the models whose libraries this tool generates (for building them ahead of a run)"""
    return [CartPoleExact(100, 0.02), QuadrotorExact(20, 0.02), _swing()]


def _median_ms(fn, torch):
    fn(); torch.cuda.synchronize()                                 # warm-up
    t = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / REPS)
    return float(np.median(t)), [float(v) for v in t]


def kernel_times(mdl, B, torch):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    ev = StageEvaluator(mdl)
    rng = np.random.default_rng(3)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    X = rng.normal(0.0, 0.3, size=(B, mdl.N, mdl.f))
    if mdl.nu == 4:
        X[:, :, 12:] += mdl.hover_thrust
    lbx, ubx, lbg, ubg = [dev(v) for v in mdl.stacked_bounds(X[:, 0, :])]
    x, p, y = dev(X.reshape(B, -1)), dev(rng.normal(0.0, 0.1, size=(B, mdl.np))), dev(rng.normal(0.0, 3.0, size=(B, mdl.m)))
    out = ev.alloc(B)
    touched = torch.zeros(B, dtype=torch.int32, device="cuda")
    res = {"model": mdl.name, "N": mdl.N, "batch": B, "f": mdl.f, "nnzP": ev.nnzP}
    res["eval_ms"], res["eval_runs_ms"] = _median_ms(lambda: ev.eval(p, x, lbx, ubx, lbg, ubg, out=out), torch)
    for label, mode in (("add", None), ("project", "project")):
        both = lambda: (ev.eval(p, x, lbx, ubx, lbg, ubg, out=out), ev.lagrangian(p, x, y, out["P"], mode=mode, touched=touched))
        res["eval_lagrangian_%s_ms" % label], res["eval_lagrangian_%s_runs_ms" % label] = _median_ms(both, torch)
        res["lagrangian_%s_over_eval" % label] = (res["eval_lagrangian_%s_ms" % label] - res["eval_ms"]) / res["eval_ms"]
    res["touched_frames_fraction"] = float(touched.double().mean()) / mdl.N
    ev.close()
    return res


def loop(option, torch):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B, N = LOOP_BATCH, LOOP_N
    mdl = _swing()
    rng = np.random.default_rng(11)
    frame0 = np.zeros((B, mdl.f))
    frame0[:, 0] = rng.uniform(-0.3, 0.2, size=B)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.tile([2.0, 0.0], (B, 1)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    x0 = np.tile(frame0[:, None, :], (1, N, 1)).reshape(B, -1)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": LOOP_MAX, "alpha": 1.0, "skip_failed_steps": True, "sqp_tol": LOOP_TOL,
                                            "exact_hessian": option}, batch=B)
    rates, iters = [], []
    for run in range(RUNS + 1):                                    # (the first run is the warm-up: it pays the set-up)
        sol.setInitialGuess(x0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        if run:
            rates.append(1.0 / (time.perf_counter() - t0)); iters.append(int(sol.iterations_done))
    failed = int((~((sol.status == 1) | (sol.status == 2) | (sol.status == 7))).sum())
    res = {"solves_per_s": float(np.median(rates)), "runs": [float(v) for v in rates], "sqp_iterations": iters, "instances_without_a_point_last_qp": failed,
           "objective_mean": float(sol.f.mean()), "violation_max": float(sol.gmax.max())}
    sol.close()
    return res


def main():
    import torch
    res = {"reps": REPS, "runs": RUNS,
           "kernel": [kernel_times(CartPoleExact(100, 0.02), 16384, torch), kernel_times(QuadrotorExact(20, 0.02), 8192, torch)],
           "loop": {"batch": LOOP_BATCH, "N": LOOP_N, "max_iterations": LOOP_MAX, "step_tolerance": LOOP_TOL, "off": loop(False, torch), "on": loop(True, torch)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
