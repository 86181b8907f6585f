#!/usr/bin/env python3
"""The per-instance merit line search of the general NLP path (mpcqp_nlp_linesearch) next to what it replaces.

Kernel: device time of one mpcqp_nlp_linesearch launch (K candidates, default 4; also K = 1 and K = 8) against one mpcqp_nlp_step + one
mpcqp_nlp_merit launch of the same build, from HIP events around REPS back-to-back launches on the first local system of the workload; both legs
restore x first, and that copy is timed alone and subtracted.  The two legs alternate, ROUNDS times; each figure is the median over the rounds and
the spread (min, max) is kept.  The eval kernel and the QP solve of the same system are timed the same way for scale: the kernel's share of a
tick is linesearch / (eval + QP + linesearch).
Loop: SQP ticks/s of DeviceSQPOptimizationSolver with and without options["line_search"] (alpha = 1, ITERS iterations per call, every call from
the same start), alternating, median of ROUNDS calls after one warm-up call each; the mean accepted alpha and the worst violation at the end.
Workloads: the two of tools/general_device_bench.py -- the skip-coupled double integrator (n = 32, ng = 26) and the pendulum at horizon 20
(n = 62, ng = 56) -- at batch 1, 256 and 4096.
usage: python tools/general_linesearch_bench.py [--out profiles/general_linesearch_bench.json] [--small]"""
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
from tests.support import general_problems as gp  # noqa: E402

REPS, ROUNDS, ITERS = 50, 5, 4
BATCHES = (1, 256, 4096)
CANDIDATES = (4, 1, 8)


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


def _problem(pr, B):
    m = pr["model"]
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=7)
    if m.ng:
        lbg[0], ubg[0] = pr["lbg"], pr["ubg"]                      # (no loose row here: every instance solves the same kind of QP)
    return m, x, dict(lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=p)


def kernel_leg(pr, B, reps):
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    m, x_start, arg = _problem(pr, B)
    sol = DeviceSQPOptimizationSolver(m, {"max_iter": 1, "alpha": 1.0, "line_search": True}, batch=B, evaluator=GeneralEvaluator(m))
    sol.setInitialGuess(x_start)
    x0 = sol.x.clone()
    sol.getOptimalSolution(arg, to_host=False)                     # leaves q, dw, y, status of the first QP on the device
    ev = sol.ev
    d = {k: sol._dev(arg[k], w) for k, w in (("p", m.np), ("lbx", m.nvar), ("ubx", m.nvar), ("lbg", m.ng), ("ubg", m.ng))}
    x = x0.clone(); mu = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = dict(sol._ls_out)

    def search(K):
        x.copy_(x0)
        ev.line_search(d["p"], x, d["lbx"], d["ubx"], sol.ls["q"], sol.dw, sol.y, status=sol.status, mu=mu, alpha0=1.0, candidates=K, out=out,
                       lbg=d["lbg"], ubg=d["ubg"])

    def pair():
        x.copy_(x0)
        ev.step(1.0, sol.dw, x, status=sol.status)
        ev.merit(d["p"], x, lbg=d["lbg"], ubg=d["ubg"])

    legs = {"copy": lambda: x.copy_(x0), "step_plus_merit": pair}
    legs.update({"linesearch_K%d" % K: (lambda K=K: search(K)) for K in CANDIDATES})
    legs["eval"] = lambda: ev.eval(d["p"], x0, d["lbx"], d["ubx"], d["lbg"], d["ubg"], out=sol.ls)
    t = {k: [] for k in legs}
    for _ in range(ROUNDS):                                        # (alternating: other work shares the machine)
        for k, fn in legs.items():
            t[k].append(_timed(fn, reps))
    qp = [_timed(lambda: sol.qp.solve(None), 3) for _ in range(3)]
    copy = float(np.median(t["copy"]))
    res = {k: _stat(np.array(v) - (copy if k != "copy" and k != "eval" else 0.0)) for k, v in t.items()}
    res["qp_solve"] = _stat(qp)
    ls, tick = res["linesearch_K4"]["median_ms"], res["eval"]["median_ms"] + res["qp_solve"]["median_ms"]
    res["linesearch_K4_over_pair"] = ls / res["step_plus_merit"]["median_ms"]
    res["linesearch_K4_share_of_tick"] = ls / (tick + ls)
    res["mean_alpha_first_iteration"] = float(sol.alpha_taken.mean())
    sol.close()
    return res


def loop_leg(pr, B):
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    m, x_start, arg = _problem(pr, B)
    legs = {}
    for key, extra in (("fixed_alpha", {}), ("line_search", {"line_search": True})):
        legs[key] = DeviceSQPOptimizationSolver(m, dict(extra, max_iter=ITERS, alpha=1.0, skip_failed_steps=True), batch=B, evaluator=GeneralEvaluator(m))
    t = {k: [] for k in legs}
    for rep in range(ROUNDS + 1):                                  # (the first round loads the code objects)
        for k, s in legs.items():
            s.setInitialGuess(x_start)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.getOptimalSolution(arg, to_host=False)
            torch.cuda.synchronize(); t[k].append(time.perf_counter() - t0)
    res = {}
    for k, s in legs.items():
        med = float(np.median(t[k][1:]))
        res[k] = dict(ms_per_call=med * 1e3, min_ms=min(t[k][1:]) * 1e3, max_ms=max(t[k][1:]) * 1e3, ticks_per_s=B * ITERS / med,
                      worst_gmax=float(torch.nan_to_num(s.gmax, nan=float("inf")).max()), finite=bool(torch.isfinite(s.x).all()))
    res["line_search"]["mean_alpha_last_iteration"] = float(legs["line_search"].alpha_taken.mean())
    res["line_search_over_fixed"] = res["line_search"]["ticks_per_s"] / res["fixed_alpha"]["ticks_per_s"]
    for s in legs.values():
        s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_linesearch_bench.json"))
    ap.add_argument("--small", action="store_true", help="batches 1 and 16, few repetitions: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    result = dict(lib_sha16=sha, reps=REPS, rounds=ROUNDS, sqp_iterations=ITERS,
                  note="kernel: HIP events around back-to-back launches, x restored before each (that copy timed alone and subtracted), legs alternating, "
                       "median / min / max over the rounds; loop: ticks/s = batch * iterations / median seconds of one getOptimalSolution call", cases=[])
    for pr in (gp.problem("skip_coupled"), dict(gp.pendulum(20), name="pendulum_N20")):
        for B in ((1, 16) if a.small else BATCHES):
            c = dict(problem=pr["name"], n=pr["model"].n, ng=pr["model"].ng, batch=B, kernel=kernel_leg(pr, B, 5 if a.small else REPS), loop=loop_leg(pr, B))
            result["cases"].append(c)
            print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
