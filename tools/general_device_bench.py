#!/usr/bin/env python3
"""SQP ticks/s of the general (non-stage) path: local system evaluated on the host (general_nlp.GeneralNLP: NumPy tapes, one complex-step
pass per column, arrays copied to the GPU for the QP) against the device evaluator (general_eval.GeneralEvaluator: mpcqp_nlp_*, the whole
iteration on the GPU).  The host leg is the code a problem on the general path runs without general_device=True, i.e. the yardstick.
Problems: the skip-coupled double integrator (n = 32, ng = 26) and the nonlinear pendulum of tests/support/general_problems.py at horizon 20
(n = 62, ng = 56).  Batches 1, 256 and 4096.  A tick = one getOptimalSolution call of ITERS SQP iterations for one instance; both legs start
every call from the same iterate, run in one process on the same build, interleaved; each cell is the median of five calls after one warm-up.
usage: python tools/general_device_bench.py [--out profiles/general_device_bench.json] [--small]"""
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

REPS, ITERS, ALPHA = 5, 2, 0.7
BATCHES = (1, 256, 4096)


def cell(pr, B):
    import torch
    from optimal_control_problem_amd.general_eval import GeneralEvaluator, compress
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, SQPOptimizationSolver
    m = pr["model"]
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=7)
    if m.ng:
        lbg[0], ubg[0] = pr["lbg"], pr["ubg"]                      # (no loose row here: every instance solves the same kind of QP)
    arg = dict(lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=p)
    opts = {"max_iter": ITERS, "alpha": ALPHA}
    legs = {"host": SQPOptimizationSolver(m, opts, batch=B),
            "device": DeviceSQPOptimizationSolver(m, opts, batch=B, evaluator=GeneralEvaluator(m))}
    t = {k: [] for k in legs}
    sol = {}
    for rep in range(REPS + 1):                                    # (the first round loads the code objects)
        for k, s in legs.items():
            s.setInitialGuess(x)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sol[k] = s.getOptimalSolution(arg)["x"]
            torch.cuda.synchronize(); t[k].append(time.perf_counter() - t0)
    c = compress(m)
    out = dict(problem=pr["name"], n=m.n, ng=m.ng, batch=B, sqp_iterations=ITERS, passes=c["hp"] + c["jp"], columns=int(len(m._hcols) + len(m._jcols)),
               max_abs_difference=float(np.nanmax(np.abs(sol["host"] - sol["device"]))))
    for k in legs:
        med = float(np.median(t[k][1:]))
        out[k] = dict(ms_per_call=med * 1e3, ticks_per_s=B / med)
    out["device_over_host"] = out["device"]["ticks_per_s"] / out["host"]["ticks_per_s"]
    legs["device"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_device_bench.json"))
    ap.add_argument("--small", action="store_true", help="batches 1 and 16: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    result = dict(lib_sha16=sha, note="ticks/s = batch / median seconds of one getOptimalSolution call (%d SQP iterations, alpha %.1f), median of %d, legs "
                  "interleaved in one process; host = GeneralNLP.local_system + QP on the GPU, device = mpcqp_nlp_* + QP on borrowed device arrays"
                  % (ITERS, ALPHA, REPS), cases=[])
    for pr in (gp.problem("skip_coupled"), dict(gp.pendulum(20), name="pendulum_N20")):
        for B in ((1, 16) if a.small else BATCHES):
            c = cell(pr, B)
            result["cases"].append(c)
            print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
