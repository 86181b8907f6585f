#!/usr/bin/env python3
"""A dynamically feasible start: options["initial_guess"] = "rollout" (DESIGN 6.27).

Both SQP loops start from x = 0, as the reference does, while the first frame is pinned to the measured state.  The first local system is then
linearised about a trajectory that jumps from the pinned frame to the origin; at cart-pole N = 100 its dynamics rows carry that defect and the QP is
primal infeasible.  With the option the fresh iterate is rolled out from the pinned frame with its input held (one mpcqp_stage_rollout on the
device): dx = 0 satisfies the dynamics rows, the QP can only be infeasible through the boxes, and it takes a tenth of the ADMM iterations.
usage: python examples/rollout_start_mpc.py [batch]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimal_control_problem_amd import _lib, models
from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
mdl, _, meta = models.make_workload("cartpole", B, N=100)
arg = {k: meta[k] for k in ("p", "lbx", "ubx", "lbg", "ubg")}

solved = {}
for name, opt in (("zero start", {}), ("rollout start", {"initial_guess": "rollout"})):
    sol = DeviceSQPOptimizationSolver(mdl, dict(opt, max_iter=1, alpha=1.0, skip_failed_steps=True), batch=B)
    sol.getOptimalSolution(arg)
    status = sol.status.cpu().numpy(); iters = sol.iters.cpu().numpy()
    solved[name] = int((status == 1).sum())
    names = sorted(set(_lib.STATUS.get(int(s), str(int(s))) for s in status))
    print("%s: first QP %s, ADMM iterations mean %.0f max %d" % (name, ", ".join(names), iters.mean(), iters.max()))
    if opt:
        print("  rollout: %d diverged, max box violation %.3g" % (int((sol.rollout_diverged >= 0).sum()), float(sol.rollout_box_viol.max())))
    sol.close()
print("solved from the rollout start: %d of %d (from the zero start: %d)" % (solved["rollout start"], B, solved["zero start"]))
