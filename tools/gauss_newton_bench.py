#!/usr/bin/env python3
"""Gauss-Newton frame costs on the device (models.StageOCP.rcost): what the evaluation kernel costs next to the exact Hessian of the
same cost written as a scalar, and next to that Hessian convexified.

Kernel: two workloads -- the quadrotor with a tilt term and the position error (nr = 15, nl = 28; N = 20, batch 8192) and the cart-pole with six rows,
two of them mixing all four states (N = 100, batch 16384) -- each in three variants: the residual model (2 J'J), its scalar twin lcost = sum rcost^2
(exact Hessian), and the twin with convexify = True followed by mpcqp_stage_convexify ("project").  One mpcqp_stage_eval launch (plus the
convexify launch in the third variant): HIP events around REPS back-to-back launches, median of RUNS such measurements after a warm-up launch.  The
comparison is with the twin of the same build in the same run.
Loop: DeviceSQPOptimizationSolver on the tip-pendulum recipe (N = 12, alpha = 0.7, skip_failed_steps, LOOP_ITERS iterations a tick) at batch 4096,
starts drawn uniformly in theta0 in [0, 3.1]: the share of instances with a NON_CVX (status 9) iteration and ticks per second -- median of RUNS runs
of TICKS ticks -- for the twin, the twin + project, and the residual model.
usage: python tools/gauss_newton_bench.py [reps] [ticks] [runs]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import models

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
LOOP_BATCH, LOOP_N, LOOP_ITERS, LOOP_ALPHA = 4096, 12, 12, 0.7


def _twin(cls, convexify=False):
    """the scalar twin of a residual model class: lcost = sum rcost^2"""
    class Twin(cls):
        name = cls.name + ("_twin_cvx" if convexify else "_twin")
        rcost = None

        def lcost(self, s, u, r):
            return sum(v * v for v in cls.rcost(self, s, u, r))
    Twin.convexify = convexify
    return Twin


class QuadTilt(models.Quadrotor):
    name = "quad_tilt_bench"

    def rcost(self, s, u, r):
        e = s - r
        hov = 9.81 / 4.0
        return ([3.0 * e[..., i] for i in range(3)] + [2.0 * (1.0 - np.cos(s[..., 3]) * np.cos(s[..., 4])), e[..., 5]]
                + [e[..., i] for i in range(6, 9)] + [0.3 * e[..., i] for i in range(9, 12)] + [0.3 * (u[..., i] - hov) for i in range(4)])


class CartWide(models.CartPole):
    name = "cart_wide_bench"

    def rcost(self, s, u, r):
        e = s - r
        return [e[..., 0] + 0.5 * np.sin(s[..., 1]) + 0.1 * e[..., 2] * e[..., 3],
                np.cos(s[..., 1]) - np.cos(r[..., 1]) + 0.2 * e[..., 0] * e[..., 2] + 0.1 * e[..., 3],
                0.3 * e[..., 2], 0.3 * e[..., 3], 0.1 * u[..., 0], 0.05 * u[..., 0] * s[..., 2]]


class Tip(models.StageOCP):
    nx = 2; nu = 1; name = "tip_bench"

    def __init__(self, N=LOOP_N):
        super().__init__(N, 0.05, [1.0, 1.0], [1.0])

    def F(self, s, u):
        th, om = s[..., 0], s[..., 1]
        return np.stack([th + 0.05 * om, om + 0.05 * (u[..., 0] - 9.81 * np.sin(th) - 0.1 * om)], axis=-1)

    def rcost(self, s, u, r):
        return [np.sin(s[..., 0]) - np.sin(r[..., 0]), np.cos(s[..., 0]) - np.cos(r[..., 0]), 0.3 * (s[..., 1] - r[..., 1]), 0.1 * u[..., 0]]

    def frame_bounds(self):
        return np.array([-np.inf, -8.0, -6.0]), np.array([np.inf, 8.0, 6.0])


WORKLOADS = ((QuadTilt, (20, 0.02), 8192), (CartWide, (100, 0.02), 16384))
VARIANTS = (("residual", lambda c: c), ("twin", lambda c: _twin(c)), ("twin_project", lambda c: _twin(c, True)))


def models_to_build():
    """the models whose libraries this tool generates (for building them ahead of a run)"""
    return [mk(cls)(*args) for cls, args, _ in WORKLOADS for _, mk in VARIANTS] + [mk(Tip)() for _, mk in VARIANTS]


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


def kernel_times(cls, args, B, torch):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    res = {"model": cls.name, "N": args[0], "batch": B}
    rng = np.random.default_rng(3)
    X = p = None
    for label, mk in VARIANTS:
        mdl = mk(cls)(*args)
        if X is None:                                              # one point for the three variants: a tilted, displaced iterate
            X = rng.normal(0.0, 0.4, size=(B, mdl.N, mdl.f))
            if mdl.nu == 4:
                X[:, :, :12] *= 0.5; X[:, :, 12:] += mdl.hover_thrust
            p = rng.normal(0.0, 0.3, size=(B, mdl.np))
            res["nl"], res["nr"] = 2 * mdl.nx + mdl.nu, mdl.nr
        ev = StageEvaluator(mdl)
        lbx, ubx, lbg, ubg = [dev(v) for v in mdl.stacked_bounds(X[:, 0, :])]
        x, pd = dev(X.reshape(B, -1)), dev(p)
        out = ev.alloc(B)
        if label == "twin_project":
            touched = torch.zeros(B, dtype=torch.int32, device="cuda")
            fn = lambda: (ev.eval(pd, x, lbx, ubx, lbg, ubg, out=out), ev.convexify(pd, x, out["P"], "project", 1e-6, touched=touched))
            fn(); torch.cuda.synchronize()
            res["touched_frames_share"] = float(touched.double().mean()) / mdl.N
        else:
            fn = lambda: ev.eval(pd, x, lbx, ubx, lbg, ubg, out=out)
        res[label + "_ms"], res[label + "_runs_ms"] = _median_ms(fn, torch)
        res[label + "_nnzP"] = ev.nnzP
        ev.close()
    res["residual_over_twin"] = res["residual_ms"] / res["twin_ms"]
    res["twin_project_over_twin"] = res["twin_project_ms"] / res["twin_ms"]
    return res


def loop(label, mk, torch):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B = LOOP_BATCH
    mdl = mk(Tip)()
    frame0 = np.zeros((B, mdl.f)); frame0[:, 0] = np.random.default_rng(5).uniform(0.0, 3.1, B)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    x0 = np.tile(frame0, (1, mdl.N))
    opts = {"alpha": LOOP_ALPHA, "skip_failed_steps": True}
    if label == "twin_project":
        opts["convexify"] = "project"
    # the statuses, one iteration per call (not timed)
    sol = DeviceSQPOptimizationSolver(mdl, dict(opts, max_iter=1), batch=B)
    sol.setInitialGuess(x0)
    bad = torch.zeros(B, dtype=torch.bool, device="cuda")
    for _ in range(LOOP_ITERS):
        sol.getOptimalSolution(arg, to_host=False)
        bad |= sol.status == 9
    share = float(bad.double().mean())
    sol.close()
    sol = DeviceSQPOptimizationSolver(mdl, dict(opts, max_iter=LOOP_ITERS), batch=B)
    rates = []
    for run in range(RUNS + 1):                                    # (the first run is the warm-up: it pays the set-up)
        sol.setInitialGuess(x0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        if run:
            rates.append(TICKS / (time.perf_counter() - t0))
    sol.close()
    return {"non_cvx_share": share, "ticks_per_s": float(np.median(rates)), "runs": [float(v) for v in rates]}


def main():
    import torch
    res = {"reps": REPS, "ticks": TICKS, "runs": RUNS, "kernel": [kernel_times(cls, args, B, torch) for cls, args, B in WORKLOADS],
           "loop": dict({"batch": LOOP_BATCH, "N": LOOP_N, "iterations_per_tick": LOOP_ITERS}, **{label: loop(label, mk, torch) for label, mk in VARIANTS})}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
