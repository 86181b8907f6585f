#!/usr/bin/env python3
"""What the soft twins of the iteration kernel cost against the plain instances (mpcqp_set_soft_rows).
One handle per workload -- quadrotor N=20 x 8192 (four waves), cart-pole N=100 x 16384 (eight waves) --, same process, the arms interleaved:
  plain      : no soft rows set -- the plain instance (the parent commit's kernel: its text is unchanged, profiles/soft_rows_kernel_resources.txt)
  all hard   : the soft twin with every w1 = 1e30 -- the same iterates bit for bit, so the difference is the twin's own cost per iteration
  state soft : the soft twin with the state boxes of frames 1 .. N-1 soft at (w1, w2) = (10, 100) -- another problem: its iteration count differs too
Per arm, the median of REPS solves: iteration-kernel ms (mpcqp_last_phase_ms: every launch behind the set-up kernel), set-up ms, mean ADMM iterations, and
iteration-kernel microseconds per QP and iteration.  The data are borrowed device tensors; the dispatch hint is off, so every solve runs in batch order.
usage: python tools/soft_rows_bench.py [--out profiles/soft_rows_bench.json] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from optimal_control_problem_amd import BatchQP, models  # noqa: E402

CASES = [("quadrotor", 20, 8192), ("cartpole", 100, 16384)]
REPS = 7
SOFT = (10.0, 100.0)


def bench(name, N, B):
    import torch
    mdl, ls, _ = models.make_workload(name, B, N=N)
    qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
    qp.set_dispatch_hint(False)
    dev = [torch.as_tensor(np.ascontiguousarray(v), device="cuda") for v in (ls.P, ls.q, ls.A, ls.l, ls.u)]
    hard = (torch.full((ls.m,), 1e30, dtype=torch.float64, device="cuda"), None)
    soft = tuple(torch.as_tensor(w, device="cuda") for w in mdl.soft_rows(state=SOFT))
    arms = {"plain": None, "all hard": hard, "state soft": soft}
    rows = {k: [] for k in arms}
    info = qp.plan_info()
    for rep in range(REPS + 2):      # (the first two rounds warm the code objects)
        for arm, w in arms.items():
            qp.set_soft_rows(*(w if w is not None else (None,)))
            qp.update(*dev); qp.solve(); qp.sync()
            r = qp.get(("status", "iters"))
            setup_ms, iter_ms = qp.last_phase_ms()
            rows[arm].append((setup_ms, iter_ms, float(r["iters"].mean()), int(np.isin(r["status"], (1, 2)).sum())))
    qp.close()
    out = dict(workload=name, N=N, batch=B, variant=info["variant"], lds_bytes=info["lds_bytes"], arms={})
    for arm, v in rows.items():
        a = np.array(v[2:], float)
        med = np.median(a, axis=0)
        out["arms"][arm] = dict(setup_ms=med[0], iteration_ms=med[1], iteration_ms_min=float(a[:, 1].min()), iteration_ms_max=float(a[:, 1].max()),
                                mean_admm_iterations=med[2], solved=int(med[3]), us_per_qp_iteration=1e3 * med[1] / (B * med[2]))
    p = out["arms"]["plain"]
    for arm in ("all hard", "state soft"):
        out["arms"][arm]["iteration_ms_over_plain"] = out["arms"][arm]["iteration_ms"] / p["iteration_ms"]
        out["arms"][arm]["us_per_qp_iteration_over_plain"] = out["arms"][arm]["us_per_qp_iteration"] / p["us_per_qp_iteration"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a rehearsal at batch 64")
    a = ap.parse_args()
    res = []
    for name, N, B in CASES:
        r = bench(name, N, 64 if a.small else B)
        res.append(r)
        for arm, v in r["arms"].items():
            print("%s N=%d x %d (variant %d) %-10s: iteration kernel %.3f ms [%.3f, %.3f], set-up %.3f ms, mean ADMM iterations %.1f, %.4f us per QP and iteration%s" % (
                name, N, r["batch"], r["variant"], arm, v["iteration_ms"], v["iteration_ms_min"], v["iteration_ms_max"], v["setup_ms"], v["mean_admm_iterations"],
                v["us_per_qp_iteration"], "" if arm == "plain" else "; over plain: %.3f (ms), %.3f (per iteration)" % (v["iteration_ms_over_plain"], v["us_per_qp_iteration_over_plain"])))
    print(json.dumps(dict(tool="soft_rows_bench", results=res)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="soft_rows_bench", reps=REPS, soft_weights=SOFT, results=res), f, indent=1)


if __name__ == "__main__":
    main()
