#!/usr/bin/env python3
"""Convexification of indefinite frame Hessians on the device (mpcqp_stage_convexify): what it costs next to the evaluation.

Kernel: for the cart-pole with a Gaussian bump cost (N = 100, batch 16384) and the quadrotor with a dense tracking matrix and a spherical bump (N = 20,
batch 8192), one generated library each, the time of one mpcqp_stage_eval launch, of eval + convexify at a point where no frame is touched (every
instance far from its bump) and of eval + convexify where every frame is touched (every instance on it): HIP events around REPS back-to-back launches,
median of RUNS such measurements after a warm-up launch.  The comparison is against the eval kernel of the same library in the same run.
Loop: ticks per second of DeviceSQPOptimizationSolver on the recipe of tests/support/convexify_cases.py's shape (cart-pole, bump centre and weight from
stage data, N = 12, 6 iterations a tick, alpha = 0.7, skip_failed_steps) at batch 4096, option off and on, median of RUNS runs of TICKS ticks.
usage: python tools/convexify_bench.py [reps] [ticks] [runs]     prints one JSON line"""
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
LOOP_BATCH, LOOP_N, LOOP_ITERS, LOOP_ALPHA = 4096, 12, 6, 0.7


class BumpCartPole(models.CartPole):
    """quadratic tracking, small absolute terms on s and r (so that a frame away from the bump is positive definite), a bump on the cart position"""
    name = "cartpole_bump_bench"
    convexify = True
    CENTRE, WEIGHT, SIGMA = 0.6, 8.0, 0.1

    def _quad(self, s, u, r):
        v = 0.01 * u[..., 0] * u[..., 0]
        for i, q in enumerate((1.0, 10.0, 0.1, 0.1)):
            e = s[..., i] - r[..., i]
            v = v + q * e * e + 0.05 * s[..., i] * s[..., i] + 0.02 * r[..., i] * r[..., i]
        return v

    def lcost(self, s, u, r):
        d0 = s[..., 0] - self.CENTRE
        return self._quad(s, u, r) + self.WEIGHT * np.exp(-(d0 * d0) / (2.0 * self.SIGMA * self.SIGMA))


class BumpCartPoleData(BumpCartPole):
    name = "cartpole_bump_data_bench"
    nsd = 2
    sdata = np.array([0.6, 8.0])

    def lcost(self, s, u, r):
        d0 = s[..., 0] - self.sdata[0]
        return self._quad(s, u, r) + self.sdata[1] * np.exp(-(d0 * d0) / (2.0 * self.SIGMA * self.SIGMA))


class QuadDense(models.Quadrotor):
    name = "quadrotor_dense_bump_bench"
    convexify = True
    CENTRE = (0.3, -0.2, 0.5)

    def lcost(self, s, u, r):
        rng = np.random.default_rng(41)
        G = rng.normal(0.0, 0.3, size=(12, 12))
        W = G @ G.T + np.diag([10.0] * 3 + [1.0] * 6 + [0.1] * 3)
        e = [s[..., i] - r[..., i] for i in range(12)]
        v = 0.0
        for i in range(12):
            v = v + W[i, i] * e[i] * e[i] + 0.05 * s[..., i] * s[..., i] + 0.02 * r[..., i] * r[..., i]
            for j in range(i + 1, 12):
                v = v + (2.0 * W[i, j]) * e[i] * e[j]
        for i in range(4):
            v = v + 0.1 * u[..., i] * u[..., i]
        d2 = 0.0
        for i, c in enumerate(self.CENTRE):
            d2 = d2 + (s[..., i] - c) * (s[..., i] - c)
        return v + 30.0 * np.exp(-d2 / (2.0 * 0.4 * 0.4))


def models_to_build():
    """the models whose libraries this tool generates (for building them ahead of a run)"""
    return [BumpCartPole(100, 0.02), QuadDense(20, 0.02), BumpCartPoleData(LOOP_N, 0.02)]


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


def kernel_times(mdl, B, centre, torch):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    ev = StageEvaluator(mdl)
    rng = np.random.default_rng(3)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    res = {"model": mdl.name, "N": mdl.N, "batch": B, "nl": 2 * mdl.nx + mdl.nu}
    nc = len(centre)
    for label, shift in (("none_touched", 3.0), ("all_touched", 0.0)):
        X = rng.normal(0.0, 0.05, size=(B, mdl.N, mdl.f))
        if mdl.nu == 4:
            X[:, :, 12:] += mdl.hover_thrust
        X[:, :, :nc] = np.asarray(centre) + shift + rng.uniform(-0.03, 0.03, size=(B, mdl.N, nc))      # (bounded: every frame on the bump, or none)
        lbx, ubx, lbg, ubg = [dev(v) for v in mdl.stacked_bounds(X[:, 0, :])]
        x, p = dev(X.reshape(B, -1)), dev(rng.normal(0.0, 0.1, size=(B, mdl.np)))
        out = ev.alloc(B)
        touched = torch.zeros(B, dtype=torch.int32, device="cuda")
        both = lambda: (ev.eval(p, x, lbx, ubx, lbg, ubg, out=out), ev.convexify(p, x, out["P"], "project", 1e-6, touched=touched))
        both(); torch.cuda.synchronize()
        frac = float(touched.double().mean()) / mdl.N
        assert frac == (0.0 if label == "none_touched" else 1.0), (label, frac)
        if label == "none_touched":
            res["eval_ms"], res["eval_runs_ms"] = _median_ms(lambda: ev.eval(p, x, lbx, ubx, lbg, ubg, out=out), torch)
        res["eval_convexify_%s_ms" % label], res["eval_convexify_%s_runs_ms" % label] = _median_ms(both, torch)
        res["convexify_%s_over_eval" % label] = (res["eval_convexify_%s_ms" % label] - res["eval_ms"]) / res["eval_ms"]
    ev.close()
    return res


def loop_ticks(option, torch):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B, N = LOOP_BATCH, LOOP_N
    mdl = BumpCartPoleData(N, 0.02)
    off = np.array([-0.5, -0.4, -0.3, -0.25, -0.2, -0.06, 0.0, 0.05])
    centre = 0.55 + 0.02 * (np.arange(B) % 8)
    frame0 = np.zeros((B, mdl.f))
    frame0[:, 0] = centre + off[np.arange(B) % 8]
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    d = np.zeros((B, N, 2)); d[..., 0] = centre[:, None] + 0.002 * np.arange(N)[None, :]; d[..., 1] = 8.0 + 0.25 * (np.arange(B) % 8)[:, None]
    arg = dict(p=np.tile([1.2, 0.0, 0.0, 0.0], (B, 1)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    x0 = np.tile(frame0[:, None, :], (1, N, 1)).reshape(B, -1)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": LOOP_ITERS, "alpha": LOOP_ALPHA, "skip_failed_steps": True, "convexify": option}, batch=B)
    sol.setStageData(d)
    rates = []
    for run in range(RUNS + 1):                                    # (the first run is the warm-up: it pays the set-up)
        sol.setInitialGuess(x0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        if run:
            rates.append(TICKS / (time.perf_counter() - t0))
    non_cvx = int((sol.status == 9).sum())
    sol.close()
    return {"ticks_per_s": float(np.median(rates)), "runs": [float(v) for v in rates], "non_cvx_instances_last_qp": non_cvx}


def main():
    import torch
    res = {"reps": REPS, "ticks": TICKS, "runs": RUNS,
           "kernel": [kernel_times(BumpCartPole(100, 0.02), 16384, (BumpCartPole.CENTRE,), torch), kernel_times(QuadDense(20, 0.02), 8192, QuadDense.CENTRE, torch)],
           "loop": {"batch": LOOP_BATCH, "N": LOOP_N, "iterations_per_tick": LOOP_ITERS, "off": loop_ticks(None, torch), "project": loop_ticks("project", torch)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
