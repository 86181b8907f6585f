#!/usr/bin/env python3
"""SQP ticks/s of trajectory tracking (a reference state per frame) on three legs, interleaved in one process on one build:
  general_host      the facade's general host path (general_nlp.GeneralNLP: NumPy tapes over the whole vector, QPs on the GPU) -- what a problem
                    with a per-frame reference ran on before the tracking stage pattern existed; with general_device=True as well where the tape is
                    accepted (the refusal's reason is recorded otherwise)
  device_full       device evaluator (mpcqp_stage_create_tracking), full-form QP handle
  device_presolved  the same evaluator, handle from mpcqp_create_presolved (parameter rows and pinned first frame eliminated)
and, for orientation, single_reference: today's device loop on the same model with one shared reference state.
Workloads: quadrotor N = 20 on a figure-eight, cart-pole N = 100 with a moving set point; batches 1, 256, 4096.  A tick = one getOptimalSolution
call of ITERS SQP iterations for one instance; every call starts from the same iterate; each cell is the median of REPS calls after one warm-up
call.  Reported per leg: ms per call, ticks/s, the kernel family (mpcqp_plan_info variant) and the mean ADMM iterations per QP.
The host leg costs O(n) tape evaluations per iteration: --host-batches / --host-reps bound what it is run on (what was run is recorded).
usage: python tools/tracking_bench.py [--out profiles/tracking_bench.json] [--small] [--host-batches 1,256,4096] [--host-reps 5] [--workloads a,b] [--append]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from optimal_control_problem_amd import _lib, models  # noqa: E402
from optimal_control_problem_amd.ocp import Dynamics, OptimalControlProblem  # noqa: E402

REPS, ITERS, ALPHA = 5, 2, 0.7
BATCHES = (1, 256, 4096)


def reference(name, m, B):
    """[B, N, nx] reference states: a figure-eight at the instance's own phase (quadrotor), a set point sliding along the track (cart-pole)"""
    t = np.arange(m.N)[None, :] * m.dt
    ph = np.linspace(0.0, 2.0 * np.pi, B, endpoint=False)[:, None]
    r = np.zeros((B, m.N, m.nx))
    if name == "quadrotor":
        w, a = 1.5, 0.6
        r[..., 0] = a * np.sin(w * t + ph); r[..., 1] = 0.5 * a * np.sin(2.0 * (w * t + ph)); r[..., 2] = 0.5
        r[..., 6] = a * w * np.cos(w * t + ph); r[..., 7] = a * w * np.cos(2.0 * (w * t + ph))
    else:
        r[..., 0] = 0.5 * np.sin(0.8 * t + ph); r[..., 2] = 0.4 * np.cos(0.8 * t + ph)
    return r


def facade_problem(m, B, general_device):
    """the same problem through the facade's builders, kept off the stage pattern: the general model the parent of this feature compiled for it"""
    node = {"discretization_settings": {"dt": m.dt, "horizon": m.N},
            "solver_settings": {"verbose": False, "gen_code": False, "load_lib": False, "max_iter": 1000, "warm_start": True, "solve_method": "CUDA_SQP",
                                "SQP_settings": {"alpha": ALPHA, "step_num": ITERS}},
            "OCP_variables": [{"name": "state", "size": m.nx, "lower_bound": m.frame_bounds()[0][:m.nx].tolist(), "upper_bound": m.frame_bounds()[1][:m.nx].tolist()},
                              {"name": "input", "size": m.nu, "lower_bound": m.frame_bounds()[0][m.nx:].tolist(), "upper_bound": m.frame_bounds()[1][m.nx:].tolist()}]}

    class P(OptimalControlProblem):
        def deployConstraintsAndAddCost(self):
            cfg = self.OCPConfigPtr_
            ref = self.setReference(m.N * m.nx)
            for k in range(m.N):
                self.addVectorCost(m.Qk[k], cfg.getVariable(k, "state") - ref.frame(k))
                self.addVectorCost(m.Rk[k], cfg.getVariable(k, "input"))
            for k in range(m.N - 1):
                self.addEquationConstraint("dynamics", cfg.getVariable(k + 1, "state"), Dynamics(m.F, cfg.getVariable(k, "state"), cfg.getVariable(k, "input")))

        def _compile_stage_model(self):
            raise NotImplementedError("tracking_bench: general path on purpose")
    ocp = P(node, batch=B, general_device=general_device)
    ocp.deployConstraintsAndAddCost()
    ocp.genSolver()
    return ocp


def cell(name, N, B, host, host_reps):
    import torch
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    zoo = {"quadrotor": models.Quadrotor, "cartpole": models.CartPole}[name]
    single = zoo(N)
    m = type("Tracking" + zoo.__name__, (zoo,), {"per_frame_reference": True})(N)
    _, _, meta = models.make_workload(name, B, N=N)
    x = meta["x_iterate"]
    ref = reference(name, m, B)
    bounds = dict(lbx=meta["lbx"], ubx=meta["ubx"], lbg=meta["lbg"], ubg=meta["ubg"])
    opts = {"max_iter": ITERS, "alpha": ALPHA}
    legs = {"device_full": (DeviceSQPOptimizationSolver(m, opts, batch=B), dict(bounds, p=ref.reshape(B, -1))),
            "device_presolved": (DeviceSQPOptimizationSolver(m, dict(opts, presolve_fixed_rows=True), batch=B), dict(bounds, p=ref.reshape(B, -1))),
            "single_reference": (DeviceSQPOptimizationSolver(single, opts, batch=B), dict(bounds, p=ref[:, 0]))}
    out = dict(workload="%s_N%d" % (name, N), n=m.n, m=m.m, np=m.np, batch=B, sqp_iterations=ITERS)
    if host:
        t0 = time.perf_counter()
        ocp = facade_problem(m, B, general_device=True)
        out["general_host_setup_s"] = time.perf_counter() - t0
        out["general_device"] = ocp.generalDeviceReason_ or "accepted"
        if ocp.generalLibrary_ is not None:
            legs["general_device"] = (ocp.OSQPSolverPtr_, dict(bounds, p=ref.reshape(B, -1)))
            ocp = facade_problem(m, B, general_device=False)
        assert ocp.generalPath_
        legs["general_host"] = (ocp.OSQPSolverPtr_, dict(bounds, p=ref.reshape(B, -1)))
    reps = {k: (host_reps if k == "general_host" else REPS) for k in legs}
    t = {k: [] for k in legs}
    sol = {}
    for rep in range(REPS + 1):                                    # (the first round loads the code objects)
        for k, (s, arg) in legs.items():
            if rep > reps[k]:
                continue
            s.setInitialGuess(x)
            s.admm_iterations = []
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sol[k] = s.getOptimalSolution(arg)["x"]
            torch.cuda.synchronize(); t[k].append(time.perf_counter() - t0)
    for k, (s, arg) in legs.items():
        med = float(np.median(t[k][1:]))
        it = np.concatenate([np.asarray(a.cpu() if hasattr(a, "cpu") else a).ravel() for a in s.admm_iterations]) if s.admm_iterations else np.zeros(0)
        qp = getattr(s, "qp", None)
        out[k] = dict(ms_per_call=med * 1e3, ticks_per_s=B / med, calls_timed=len(t[k]) - 1, mean_admm_iterations=float(it.mean()) if it.size else None,
                      variant=int(qp.plan_info()["variant"]) if qp is not None else None, nfixed=int(qp.nfixed) if qp is not None else None)
    fin = lambda a: np.nan_to_num(a, nan=1e300)
    out["max_abs_presolved_minus_full"] = float(np.abs(fin(sol["device_presolved"]) - fin(sol["device_full"])).max())
    if "general_host" in sol:
        out["max_abs_full_minus_general_host"] = float(np.abs(fin(sol["device_full"]) - fin(sol["general_host"])).max())
    out["presolved_over_full"] = out["device_presolved"]["ticks_per_s"] / out["device_full"]["ticks_per_s"]
    out["presolved_over_single_reference"] = out["device_presolved"]["ticks_per_s"] / out["single_reference"]["ticks_per_s"]
    for k in ("device_full", "device_presolved", "single_reference", "general_device"):
        if k in legs:
            legs[k][0].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_bench.json"))
    ap.add_argument("--small", action="store_true", help="batches 1 and 16, short horizons: a rehearsal of the script, not a measurement")
    ap.add_argument("--host-batches", default=",".join(str(b) for b in BATCHES), help="batches on which the general host leg runs ('' = none)")
    ap.add_argument("--host-reps", type=int, default=REPS, help="timed calls of the general host leg (the device legs always take %d)" % REPS)
    ap.add_argument("--workloads", default="quadrotor,cartpole")
    ap.add_argument("--append", action="store_true", help="add the cases to an --out file written by the same library (workloads measured in separate runs)")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    hostb = {int(v) for v in a.host_batches.split(",") if v}
    result = dict(lib_sha16=sha, note="ticks/s = batch / median seconds of one getOptimalSolution call (%d SQP iterations, alpha %.1f) after one warm-up call, every call "
                  "from the same iterate, legs interleaved in one process; general_host timed over host_reps calls where it ran (calls_timed)" % (ITERS, ALPHA),
                  host_batches=sorted(hostb), host_reps=a.host_reps, cases=[])
    if a.append and os.path.exists(a.out):
        old = json.load(open(a.out))
        if old.get("lib_sha16") != sha:
            raise SystemExit("--append: %s was written by another library build" % a.out)
        result["cases"] = old["cases"]
        result["host_batches"] = "per case: a case has a general_host entry where the leg ran"; result["host_reps"] = "per case: calls_timed"
    for name in a.workloads.split(","):
        N = {"quadrotor": 20, "cartpole": 100}[name] if not a.small else {"quadrotor": 4, "cartpole": 6}[name]
        for B in ((1, 16) if a.small else BATCHES):
            c = cell(name, N, B, B in hostb, max(1, a.host_reps))
            result["cases"].append(c)
            print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
