#!/usr/bin/env python3
"""What polishing buys and costs: quadrotor N=20 x 8192 and double integrator N=20 x 4096, cold start, batch-order dispatch, median of five solves.
  * polishing off at eps 1e-3, 1e-4, 1e-5, 1e-6: kernel ms per batch (mpcqp_last_kernel_ms)
  * polishing on at eps 1e-3: solve ms and polish ms (mpcqp_last_polish_ms) apart
  * per leg: the median host-recomputed residual (max of primal and dual, 64 sampled instances) and the number of polished instances
  * with --parent LIB (a build of the parent commit's libmpcqp.so): its kernel ms at eps 1e-3 and 1e-6 through tools/ab_lib.py (best of four there)
usage: python tools/polish_bench.py [--parent LIB] [--out profiles/polish_bench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from optimal_control_problem_amd import BatchQP, _lib, models  # noqa: E402

CASES = [("quadrotor", 20, 8192), ("double_integrator", 20, 4096)]
EPS = [1e-3, 1e-4, 1e-5, 1e-6]


def dense(ls, b):
    P = np.zeros((ls.n, ls.n)); A = np.zeros((ls.m, ls.n))
    P[ls.Pi, np.repeat(np.arange(ls.n), np.diff(ls.Pp))] = ls.P[b]
    A[ls.Ai, np.repeat(np.arange(ls.n), np.diff(ls.Ap))] = ls.A[b]
    return np.triu(P) + np.triu(P, 1).T, A


def residual(ls, mats, res, b):
    P, A = mats[b]
    x, y = res["x"][b], res["y"][b]
    ax = A @ x
    return max(np.abs(ax - np.clip(ax, ls.l[b], ls.u[b])).max(), np.abs(P @ x + ls.q[b] + A.T @ y).max())


def leg(ls, dev, mats, sample, eps, polish):
    import torch
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, eps_abs=eps, eps_rel=eps)
    qp.set_dispatch_hint(False)
    if polish:
        qp.set_polish(True)
    ms, pms = [], []
    for _ in range(7):
        qp.update(*dev); qp.solve(); qp.sync()
        ms.append(qp.last_kernel_ms())
        if polish:
            pms.append(qp.last_polish_ms())
    res = qp.get(); qp.close()
    torch.cuda.synchronize()
    out = dict(eps=eps, polish=bool(polish), solve_ms=float(np.median(ms[2:])), iters_mean=float(res["iters"].mean()), solved=int((res["status"] == 1).sum()),
               residual_median=float(np.median([residual(ls, mats, res, b) for b in sample])))
    if polish:
        out.update(polish_ms=float(np.median(pms[2:])), polished=int((res["polish_status"] == _lib.POLISH_SUCCESS).sum()),
                   rejected=int((res["polish_status"] == _lib.POLISH_FAILED).sum()), linsys_error=int((res["polish_status"] == _lib.POLISH_LINSYS_ERROR).sum()))
        out["total_ms"] = out["solve_ms"] + out["polish_ms"]
    return out


def parent_ms(lib, name, N, B, eps):
    env = dict(os.environ, AB_CASES="%s:%d:%d" % (name, N, B), AB_EPS=repr(eps))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_lib.py"), lib], capture_output=True, text=True, env=env, timeout=900)
    vals = [float(v) for v in re.findall(r"N=%d: ([0-9.]+) ms" % N, r.stdout)]
    if r.returncode != 0 or not vals:
        raise RuntimeError("ab_lib.py failed: " + r.stdout[-500:] + r.stderr[-500:])
    return min(vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish_bench.json"))
    a = ap.parse_args()
    import torch
    result = dict(note="kernel ms per batch, cold start, batch-order dispatch, median of five; residual = max(primal, dual) recomputed on the host, median of 64 instances",
                  cases=[])
    for name, N, B in CASES:
        _, ls, _ = models.make_workload(name, B, N=N)
        dev = [torch.as_tensor(v, device="cuda") for v in (ls.P, ls.q, ls.A, ls.l, ls.u)]
        sample = list(range(0, B, B // 64))
        mats = {b: dense(ls, b) for b in sample}
        case = dict(workload=name, N=N, batch=B, off=[leg(ls, dev, mats, sample, e, False) for e in EPS], on=leg(ls, dev, mats, sample, 1e-3, True))
        if a.parent:
            case["parent_off_ms"] = {"1e-3": parent_ms(a.parent, name, N, B, 1e-3), "1e-6": parent_ms(a.parent, name, N, B, 1e-6)}
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del dev
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
