#!/usr/bin/env python3
"""What keeping the scaling over a matrix update buys: full set-up (mpcqp_update) against mpcqp_update_matrices on the second linearisation of a workload.
One handle per workload -- quadrotor N=20 x 8192, quadrotor N=50 x 8192, cart-pole N=100 x 16384 --, same process, the two arms interleaved:
  full arm : update(QP2) -> solve                                  (the parent commit's path: its kernels are unchanged, tools/isa_guard.sh)
  kept arm : update(QP1) -> solve (untimed: it lays down D, E, c) -> update_matrices(QP2) -> solve
Per arm, the median of five: set-up ms and iteration ms (mpcqp_last_phase_ms), and the batch's total ADMM iterations.
Then QP/s of a five-iteration device SQP loop (DeviceSQPOptimizationSolver) with keep_scaling off and on, median of five calls each, interleaved.
QP2 = the linearisation at x_iterate + 0.7 dx, dx from the handle's own solve of QP1.
usage: python tools/keep_scaling_bench.py [--out profiles/keep_scaling_bench.json] [--small]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from optimal_control_problem_amd import BatchQP, _lib, models  # noqa: E402

CASES = [("quadrotor", 20, 8192), ("quadrotor", 50, 8192), ("cartpole", 100, 16384)]
REPS = 5


def data(ls):
    import torch
    return [torch.as_tensor(np.ascontiguousarray(v), device="cuda") for v in (ls.P, ls.q, ls.A, ls.l, ls.u)]


def solve_arms(name, N, B):
    mdl, qp1, meta = models.make_workload(name, B, N=N)
    qp = BatchQP(qp1.n, qp1.m, B, qp1.Pp, qp1.Pi, qp1.Ap, qp1.Ai)
    qp.set_dispatch_hint(False)
    qp.keep_workspace(True)
    d1 = data(qp1)
    qp.update(*d1); qp.solve(); first = qp.get()
    x = meta["x_iterate"] + 0.7 * np.nan_to_num(first["x"][:, mdl.np:])
    qp2 = mdl.local_system(meta["p"], x, meta["lbx"], meta["ubx"], meta["lbg"], meta["ubg"])
    d2 = data(qp2)
    out = dict(workload=name, N=N, batch=B, variant=qp.plan_info()["variant"])
    try:
        qp.update_matrices(*d2)
    except _lib.MpcqpError as e:
        if e.code != _lib.ERR_LIMIT:
            raise
        out["kept"] = None      # (this handle's kernel family has no such entry)
        qp.close()
        return out
    arms = {"full": [], "kept": []}
    for rep in range(REPS + 2):      # (the first two rounds warm the code objects)
        qp.update(*d2); qp.solve(); qp.sync()
        r = qp.get(("status", "iters")); arms["full"].append(qp.last_phase_ms() + (int(r["iters"].sum()), int((r["status"] == 1).sum())))
        qp.update(*d1); qp.solve(); qp.sync()
        qp.update_matrices(*d2); qp.solve(); qp.sync()
        r = qp.get(("status", "iters")); arms["kept"].append(qp.last_phase_ms() + (int(r["iters"].sum()), int((r["status"] == 1).sum())))
    qp.close()
    for k, v in arms.items():
        a = np.array(v[2:], float)
        out[k] = dict(setup_ms=float(np.median(a[:, 0])), solve_ms=float(np.median(a[:, 1])), admm_iterations=int(np.median(a[:, 2])), solved=int(np.median(a[:, 3])))
    return out


def sqp_arms(name, N, B):
    import torch
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, ls, meta = models.make_workload(name, B, N=N)
    arg = dict(lbx=meta["lbx"], ubx=meta["ubx"], lbg=meta["lbg"], ubg=meta["ubg"], p=meta["p"])
    solvers = {k: DeviceSQPOptimizationSolver(mdl, {"max_iter": 5, "alpha": 0.7, "keep_scaling": k == "kept"}, batch=B) for k in ("full", "kept")}
    t = {k: [] for k in solvers}
    its = {k: 0 for k in solvers}
    for rep in range(REPS + 2):
        for k, s in solvers.items():
            s.setInitialGuess(meta["x_iterate"]); s.admm_iterations = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.getOptimalSolution(arg, to_host=False)
            torch.cuda.synchronize(); t[k].append(time.perf_counter() - t0)
            its[k] = int(sum(int(a.sum()) for a in s.admm_iterations))
    out = {k: dict(qp_per_s=float(5 * B / np.median(t[k][2:])), admm_iterations=its[k], keeps=bool(solvers[k].keep_scaling)) for k in solvers}
    for s in solvers.values():
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_scaling_bench.json"))
    ap.add_argument("--small", action="store_true", help="batches of 256: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    result = dict(lib_sha16=sha, note="ms per batch, batch-order dispatch, device-resident inputs, median of five, arms interleaved in one process; "
                  "sqp: QP/s of a five-iteration device SQP loop, alpha 0.7 (the kept arm's first QP of every call after the first is a kept one as well)", cases=[])
    for name, N, B in CASES:
        if a.small:
            B = 256
        case = solve_arms(name, N, B)
        case["sqp"] = sqp_arms(name, N, B)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
