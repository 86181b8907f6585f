#!/usr/bin/env python3
"""A move penalty (u_{k+1} - u_k)' S (u_{k+1} - u_k) as a link cost on the stage path (models.StageOCP.llink).

Kernel: time of one mpcqp_stage_eval, one mpcqp_stage_merit and one mpcqp_stage_linesearch (K = 4) launch of a generated library with the
penalty against the generated library of the same model without it, from HIP events around REPS back-to-back launches on the first local
system of the workload (cart-pole N=100 x 16384, the 12-state quadrotor N=20 x 8192, both through codegen).
Loop: ticks per second of DeviceSQPOptimizationSolver, 2 SQP iterations per tick (alpha = 1, ADMM warm start), with and without the penalty,
three runs each.
Baseline: the same model with the penalty as a user has it without this feature -- the facade's general path with general_device=True (cost and
constraints traced over the whole decision vector, mpcqp_nlp_*).  That path refuses the two workloads above (their tapes exceed
codegen.GENERAL_TAPE_CAP; the reason is recorded), so the two paths are compared through the same facade call at horizons the general device
path accepts: seconds per computeOptimalTrajectory (2 SQP iterations, host arrays in and out), median of 5, legs alternating.
usage: python tools/link_cost_bench.py [reps] [ticks]     prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from optimal_control_problem_amd import codegen, models
from optimal_control_problem_amd.ocp import Dynamics, LinkCost, OptimalControlProblem

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
TICKS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K = 4
WEIGHT = 0.5
WORKLOADS = (("cartpole", 100, 16384), ("quadrotor", 20, 8192))
FACADE_CASES = (("cartpole", 30, 4096), ("quadrotor", 8, 2048))     # horizons whose whole-vector tapes stay under GENERAL_TAPE_CAP


def du_penalty(s, u, sn, un):
    d = un - u
    return sum(WEIGHT * (d[..., i] * d[..., i]) for i in range(d.shape[-1]))


def model(name, N, penalty):
    base = {"cartpole": models.CartPole, "quadrotor": models.Quadrotor}[name]
    cls = type(base.__name__ + "Smooth", (base,), {"name": name + "_smooth", "llink": staticmethod(du_penalty)}) if penalty else base
    return cls(N, 0.02)


# ------------------------------------------------------------------------------------------------- kernels and the device loop
def _timed(fn, reps=REPS):
    import torch
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_leg(name, N, B, penalty):
    import torch
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl = model(name, N, penalty)
    _, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "line_search": {"candidates": K}}, batch=B, codegen=True)
    assert sol.ev.library is not None and sol.ev.link_cost == penalty
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.setInitialGuess(meta["x_iterate"])
    x0 = sol.x.clone()
    sol.getOptimalSolution(arg, to_host=False)                     # leaves q, dw, y, status of the first QP on the device
    ev = sol.ev
    x = x0.clone(); mu = torch.zeros(B, dtype=torch.float64, device="cuda")
    out = dict(sol._ls_out)

    def search():
        x.copy_(x0)
        ev.line_search(arg["p"], x, arg["lbx"], arg["ubx"], sol.ls["q"], sol.dw, sol.y, status=sol.status, mu=mu, alpha0=1.0, candidates=K, out=out)

    copy_ms = _timed(lambda: x.copy_(x0))
    res = {"eval_ms": _timed(lambda: ev.eval(arg["p"], x0, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"], out=sol.ls)),
           "merit_ms": _timed(lambda: ev.merit(arg["p"], x0)),
           "linesearch_ms": _timed(search) - copy_ms,               # the search restores x first; that copy is not its own
           "nnzP": ev.nnzP}
    sol.close()
    return res


def loop_leg(name, N, B, penalty):
    import torch
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl = model(name, N, penalty)
    _, _, meta = models.make_workload(name, B, N=N)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 2, "alpha": 1.0, "warm_start_admm": True}, batch=B, codegen=True)
    arg = {k: sol._dev(meta[k], w) for k, w in (("p", mdl.np), ("lbx", mdl.nvar), ("ubx", mdl.nvar), ("lbg", mdl.ng), ("ubg", mdl.ng))}
    sol.getOptimalSolution(arg, to_host=False); torch.cuda.synchronize()       # warm-up: the first tick pays the set-up
    runs = []
    for _ in range(3):
        sol.setInitialGuess(np.zeros(mdl.nvar))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(TICKS):
            sol.getOptimalSolution(arg, to_host=False)
        torch.cuda.synchronize()
        runs.append(TICKS / (time.perf_counter() - t0))
    sol.close()
    return runs


# ------------------------------------------------------------------------------------------------- the facade: stage path and general device path
def _node(mdl):
    lo, hi = mdl.frame_bounds()
    var = lambda nm, a, b: {"name": nm, "size": b - a, "lower_bound": [float(v) for v in lo[a:b]], "upper_bound": [float(v) for v in hi[a:b]]}
    return {"discretization_settings": {"dt": mdl.dt, "horizon": mdl.N},
            "solver_settings": {"verbose": False, "gen_code": True, "load_lib": False, "max_iter": 1000, "warm_start": True, "solve_method": "CUDA_SQP",
                                "SQP_settings": {"alpha": 1.0, "step_num": 2}},
            "OCP_variables": [var("state", 0, mdl.nx), var("input", mdl.nx, mdl.f)]}


class SmoothProblem(OptimalControlProblem):
    """tracking cost + move penalty on every stage + dynamics; general=True keeps it off the stage pattern, as before LinkCost was compiled"""
    plant = None; general = False

    def deployConstraintsAndAddCost(self):
        cfg = self.OCPConfigPtr_; N = cfg.getHorizon(); m = self.plant
        ref = self.setReference(m.nx)
        var = lambda k: (cfg.getVariable(k, "state"), cfg.getVariable(k, "input"))
        for k in range(N):
            self.addVectorCost(m.Q, var(k)[0] - ref)
            self.addVectorCost(m.R, var(k)[1])
            if k < N - 1:
                self.addScalarCost(LinkCost(du_penalty, *var(k), *var(k + 1)))
                self.addEquationConstraint("dynamics", var(k + 1)[0], Dynamics(m.F, *var(k)))

    def _compile_stage_model(self):
        if self.general:
            raise NotImplementedError("link costs are not compiled (the parent's facade)")
        return super()._compile_stage_model()


def facade_problem(name, N, B, general):
    plant = model(name, N, False)
    cls = type("P", (SmoothProblem,), {"plant": plant, "general": general})
    ocp = cls(_node(plant), batch=B, general_device=general)
    ocp.deployConstraintsAndAddCost()
    ocp.genSolver()
    return ocp


def general_refusal(name, N):
    """why general_device=True leaves this workload on the host loop (None: it takes it)"""
    ocp = facade_problem(name, N, 1, True)
    return ocp.generalDeviceReason_


def facade_leg(name, N, B):
    import torch
    _, _, meta = models.make_workload(name, B, N=N)
    frame, ref = meta["frame0"], meta["p"]
    legs = {"stage": facade_problem(name, N, B, False), "general_device": facade_problem(name, N, B, True)}
    assert legs["stage"].generalPath_ is False and legs["stage"].model_.link_cost
    if legs["general_device"].generalLibrary_ is None:
        return {"refused": legs["general_device"].generalDeviceReason_}
    times = {k: [] for k in legs}
    last = {}
    for k, ocp in legs.items():
        ocp.computeOptimalTrajectory(frame, ref)                   # warm-up: set-up and first use of the code objects
    for _ in range(5):
        for k, ocp in legs.items():
            ocp.firstTime_ = True                                  # every call starts from x = 0, like the first
            ocp.OSQPSolverPtr_.setInitialGuess(np.zeros(ocp.OCPConfigPtr_.getVariables()))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            last[k] = ocp.computeOptimalTrajectory(frame, ref)
            torch.cuda.synchronize(); times[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"batch": B, "sqp_iterations": 2, "stage": {"ms_per_call": 1e3 * med["stage"], "ticks_per_s": B / med["stage"], "runs_ms": [1e3 * v for v in times["stage"]]},
            "general_device": {"ms_per_call": 1e3 * med["general_device"], "ticks_per_s": B / med["general_device"], "runs_ms": [1e3 * v for v in times["general_device"]]},
            "stage_over_general_device": med["general_device"] / med["stage"],
            "max_abs_difference": float(np.abs(last["stage"] - last["general_device"]).max())}


if __name__ == "__main__":
    import torch
    res = {"reps": REPS, "ticks": TICKS, "sqp_iterations_per_tick": 2, "weight": WEIGHT, "device": torch.cuda.get_device_name(0),
           "general_tape_cap": codegen.GENERAL_TAPE_CAP, "kernel_ms": {}, "loop_ticks_per_s": {}, "general_device_refusal": {}, "facade": {}}
    for name, N, B in WORKLOADS:
        key = "%s_N%d_x%d" % (name, N, B)
        res["kernel_ms"][key] = {"plain": kernel_leg(name, N, B, False), "penalty": kernel_leg(name, N, B, True)}
        res["loop_ticks_per_s"][key] = {"plain": loop_leg(name, N, B, False), "penalty": loop_leg(name, N, B, True)}
        res["general_device_refusal"][key] = general_refusal(name, N)
    for name, N, B in FACADE_CASES:
        res["facade"]["%s_N%d_x%d" % (name, N, B)] = facade_leg(name, N, B)
    print(json.dumps(res))
