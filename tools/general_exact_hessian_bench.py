#!/usr/bin/env python3
"""The exact Hessian of the Lagrangian on the general NLP path (mpcqp_nlp_lagrangian) next to the evaluation it follows.

Kernel: device time from HIP events around REPS back-to-back launches, median of ROUNDS rounds after a warm-up, three legs that alternate:
mpcqp_nlp_eval alone, eval + lagrangian mode 0 (with the workspace), eval + lagrangian "dominant".  The model is the flagged one in all three legs
(the widened pattern is part of the feature's cost); `eval_unflagged` is the evaluation of the unflagged model's library for scale.
Loop: SQP ticks/s of DeviceSQPOptimizationSolver (alpha = 1, ITERS iterations per call, every call from the same start) with and without
options["exact_hessian"] = "dominant", alternating, median of ROUNDS calls after a warm-up call each; and the iterations either needs to a step
of 1e-3 (sqp_tol, at most MAX_ITERS) on the curved problem, the pendulum.
Workloads: the pendulum at horizon 20 (n = 62, ng = 56) and the skip-coupled double integrator (n = 32, ng = 26: linear constraints, the call is
a no-op) at batch 1, 256 and 4096.
usage: python tools/general_exact_hessian_bench.py [--out profiles/general_exact_hessian_bench.json] [--small]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from optimal_control_problem_amd import _lib  # noqa: E402
from optimal_control_problem_amd.general_nlp import GeneralNLP  # noqa: E402
from tests.support import general_problems as gp  # noqa: E402

REPS, ROUNDS, ITERS, MAX_ITERS = 50, 5, 4, 40
BATCHES = (1, 256, 4096)


def _timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _stat(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


def _models(name):
    """(unflagged, flagged, problem dict)"""
    if name == "skip_coupled":
        pr = gp.problem("skip_coupled")
        return pr["model"], GeneralNLP(30, 2, pr["cost"], pr["constraints"], exact_hessian=True), pr
    pr = dict(gp.pendulum(20), name="pendulum_N20")
    flagged = GeneralNLP(60, 2, lambda w: gp.pendulum_cost(w, 20), lambda w: gp.pendulum_constraints(w, 20), exact_hessian=True)
    return pr["model"], flagged, pr


def _point(pr, B):
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=7)
    if pr["model"].ng:
        lbg[0], ubg[0] = pr["lbg"], pr["ubg"]
    return x, dict(lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=p)


def kernel_leg(name, B, reps):
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    plain, flagged, pr = _models(name)
    x, arg = _point(pr, B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    d = {k: dev(v) for k, v in arg.items()}
    xd = dev(x)
    y = dev(np.random.default_rng(3).normal(0.0, 1.0, (B, flagged.m)))
    evs = {"plain": GeneralEvaluator(plain), "flagged": GeneralEvaluator(flagged)}
    outs = {k: ev.alloc(B) for k, ev in evs.items()}
    Cw = torch.zeros((B, evs["flagged"].nnzP), dtype=torch.float64, device="cuda"); shift = torch.zeros((B, flagged.n), dtype=torch.float64, device="cuda")

    def ev_(k):
        evs[k].eval(d["p"], xd, d["lbx"], d["ubx"], d["lbg"], d["ubg"], out=outs[k])

    def with_(mode):
        ev_("flagged")
        evs["flagged"].lagrangian(d["p"], xd, y, outs["flagged"]["P"], mode=mode, C=Cw, shift=shift)

    legs = {"eval_unflagged": lambda: ev_("plain"), "eval": lambda: ev_("flagged"), "eval_plus_mode0": lambda: with_(0),
            "eval_plus_dominant": lambda: with_("dominant")}
    for fn in legs.values():                                       # warm-up: loads the code objects
        fn()
    t = {k: [] for k in legs}
    for _ in range(ROUNDS):                                        # (alternating: other work shares the machine)
        for k, fn in legs.items():
            t[k].append(_timed(fn, reps))
    res = {k: _stat(v) for k, v in t.items()}
    res["mode0_over_eval"] = res["eval_plus_mode0"]["median_ms"] / res["eval"]["median_ms"]
    res["dominant_over_eval"] = res["eval_plus_dominant"]["median_ms"] / res["eval"]["median_ms"]
    res["flagged_eval_over_unflagged"] = res["eval"]["median_ms"] / res["eval_unflagged"]["median_ms"]
    res["nnzP"] = dict(unflagged=len(plain.Pi), flagged=len(flagged.Pi))
    for ev in evs.values():
        ev.close()
    return res


def loop_leg(name, B, rounds):
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    plain, flagged, pr = _models(name)
    x_start, arg = _point(pr, B)
    mk = lambda m, extra, iters, tol=0.0: DeviceSQPOptimizationSolver(m, dict(extra, max_iter=iters, alpha=1.0, skip_failed_steps=True, sqp_tol=tol),
                                                                     batch=B, evaluator=GeneralEvaluator(m))
    legs = {"cost_only": mk(plain, {}, ITERS), "dominant": mk(flagged, {"exact_hessian": "dominant"}, ITERS)}
    t = {k: [] for k in legs}
    for rep in range(rounds + 1):                                  # (the first round loads the code objects)
        for k, s in legs.items():
            s.setInitialGuess(x_start)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.getOptimalSolution(arg, to_host=False)
            torch.cuda.synchronize(); t[k].append(time.perf_counter() - t0)
    res = {}
    for k, s in legs.items():
        med = float(np.median(t[k][1:]))
        res[k] = dict(ms_per_call=med * 1e3, min_ms=min(t[k][1:]) * 1e3, max_ms=max(t[k][1:]) * 1e3, ticks_per_s=B * ITERS / med,
                      finite=bool(torch.isfinite(s.x).all()))
        s.close()
    res["dominant_over_cost_only"] = res["dominant"]["ticks_per_s"] / res["cost_only"]["ticks_per_s"]
    if name != "skip_coupled" and B <= 256:
        for k, (m, extra) in (("cost_only", (plain, {})), ("dominant", (flagged, {"exact_hessian": "dominant"}))):
            s = mk(m, extra, MAX_ITERS, 1e-3)
            s.setInitialGuess(x_start)
            s.getOptimalSolution(arg, to_host=False)
            res[k]["iterations_to_1e-3"] = int(s.iterations_done)
            res[k]["last_step_max"] = float(torch.nan_to_num(s.step_max, nan=float("inf")).max())
            s.close()
    return res


def recipe_leg(B=192):
    """the curved problem on which the option matters (examples/general_exact_hessian.py; tests/support/general_exact_hessian_cases.py): half the
    instances with p = 3, half with p = -2, starts [0.8, 0.5, 0.1] + 0.2 N(0, 1); iterations of the whole batch to a step of 1e-3 (at most MAX_ITERS),
    the share of instances whose last step is below it, and ticks/s of that call"""
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    from tests.support import general_exact_hessian_cases as ge
    arg = dict(p=np.array([[3.0]] * (B // 2) + [[-2.0]] * (B // 2)), lbx=np.full((B, 3), -5.0), ubx=np.full((B, 3), 5.0), lbg=np.zeros((B, 2)), ubg=np.zeros((B, 2)))
    x0 = np.array([0.8, 0.5, 0.1]) + 0.2 * np.random.default_rng(11).normal(size=(B, 3))
    res = {}
    for key, m, extra in (("cost_only", ge.model("recipe", False), {}), ("exact_mode0", ge.model("recipe"), {"exact_hessian": True}),
                          ("dominant", ge.model("recipe"), {"exact_hessian": "dominant"})):
        s = DeviceSQPOptimizationSolver(m, dict(extra, max_iter=MAX_ITERS, alpha=1.0, skip_failed_steps=True, sqp_tol=1e-3), batch=B, evaluator=GeneralEvaluator(m))
        t = []
        for rep in range(3):                                       # (the first call loads the code objects)
            s.setInitialGuess(x0)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.getOptimalSolution(arg, to_host=False)
            torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
        step = torch.nan_to_num(s.step_max, nan=float("inf"))
        ok = (s.status == 1) | (s.status == 2) | (s.status == 7)
        res[key] = dict(iterations=int(s.iterations_done), share_below_tol=float(((step < 1e-3) & ok).double().mean()),
                        share_qp_failed_last=float((~ok).double().mean()), ms_per_call=float(np.median(t[1:])) * 1e3,
                        ticks_per_s=B * int(s.iterations_done) / float(np.median(t[1:])))
        s.close()
    return dict(problem="recipe", batch=B, loop=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_exact_hessian_bench.json"))
    ap.add_argument("--small", action="store_true", help="batches 1 and 16, few repetitions: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    result = dict(lib_sha16=sha, reps=REPS, rounds=ROUNDS, sqp_iterations=ITERS,
                  note="kernel: HIP events around back-to-back launches, legs alternating, median / min / max over the rounds after a warm-up; "
                       "loop: ticks/s = batch * iterations / median seconds of one getOptimalSolution call", cases=[])
    result["recipe"] = recipe_leg()
    print(json.dumps(result["recipe"]), flush=True)
    for name in ("pendulum_N20", "skip_coupled"):
        for B in ((1, 16) if a.small else BATCHES):
            c = dict(problem=name, batch=B, kernel=kernel_leg(name, B, 5 if a.small else REPS), loop=loop_leg(name, B, 2 if a.small else ROUNDS))
            result["cases"].append(c)
            print(json.dumps(c), flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:                            # (kept after every case: a long run leaves what it has)
                json.dump(result, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
