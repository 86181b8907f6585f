"""CPU: the per-instance merit line search (mpcqp_stage_linesearch) -- the wiring of the entry point, its NumPy statement
models.StageOCP.line_search on hand-made inputs, the host loop's recipe on the CPU oracle, and the conditions on the kernel cases that
tests/test_gpu_linesearch.py relies on, asserted here of the NumPy statement alone."""
import os
import re
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, codegen, models
from tests.support import advance_cases as ac
from tests.support import linesearch_cases as lc
from tests.support.oracle_backend import OracleCuCaQP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ wiring
def test_entry_point_is_declared_exported_and_bound(built):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"int mpcqp_stage_linesearch\(mpcqp_stage \*s, int batch, const mpcqp_stage_linesearch_args \*a, void \*stream\);", hdr)
    assert "SQPOptimizationSolver.cpp:171-177" in hdr
    body = hdr[hdr.index("typedef struct mpcqp_stage_linesearch_args"):hdr.index("} mpcqp_stage_linesearch_args;")]
    for field in ("p", "x", "lbx", "ubx", "q", "dw", "y", "status", "mu", "alpha_out", "accepted", "step_max", "f_out", "gmax_out", "phi",
                  "alpha0", "beta", "c1", "mu_min", "mu_factor", "candidates"):
        assert re.search(r"[ *,]%s[,;]" % field, body), field
    assert "mpcqp_stage_linesearch" in _lib.EXPORTS
    assert hasattr(C.CDLL(_lib.SO_PATH), "mpcqp_stage_linesearch")
    from optimal_control_problem_amd.stage_eval import LineSearchArgs
    # the ctypes struct mirrors the header: 15 pointers, 5 doubles, 1 int (padded to 8)
    assert C.sizeof(LineSearchArgs) == 15 * 8 + 5 * 8 + 8
    assert [n for n, _ in LineSearchArgs._fields_] == ["p", "x", "lbx", "ubx", "q", "dw", "y", "status", "mu", "alpha_out", "accepted", "step_max",
                                                      "f_out", "gmax_out", "phi", "alpha0", "beta", "c1", "mu_min", "mu_factor", "candidates"]


def test_generated_library_exports_linesearch(built):
    m = ac.pendulum()
    tape = codegen.trace(m.F, m.nx, m.nu)
    src = codegen.device_source(tape)
    assert "mpcqp_user_linesearch" in src and "stage_launch_linesearch<SmUser>" in src
    tape_t = codegen.trace(m.F, m.nx, m.nu, per_frame_reference=True)
    assert "stage_launch_linesearch<SmUser, SmUser::pref>" in codegen.device_source(tape_t)
    so = codegen.build_device_library(tape)            # hipcc --offload-arch=gfx950, no GPU needed
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "mpcqp_user_linesearch" in syms


def test_old_library_message_host_side():
    """the refusal for a library generated before this entry names the export and the remedy (the GPU test calls through such a handle)"""
    src = open(os.path.join(ROOT, "optimal_control_problem_amd", "csrc", "stage_eval.hip")).read()
    assert "the library does not export mpcqp_user_linesearch (generated before this entry); regenerate it" in src


# ------------------------------------------------------------------------------------------------ the rule by hand
# double integrator, N = 2, dt = 0.5: F(s, u) = [s0 + 0.5 s1 + 0.125 u, s1 + 0.5 u]; Q = diag(10, 1), R = 0.1; variables [p0 p1 | s0 v0 u0 s1 v1 u1]
def _di2():
    return models.DoubleIntegrator(2, 0.5)


def _hand(dx, B=1, x=None, **kw):
    m = _di2()
    x = np.zeros((B, 6)) if x is None else x
    lbx = np.full((B, 6), -np.inf); ubx = np.full((B, 6), np.inf)
    dw = np.concatenate([np.zeros((B, 2)), np.broadcast_to(np.asarray(dx, float), (B, 6))], axis=1)
    q = kw.pop("q", np.zeros((B, 8)))
    y = kw.pop("y", np.zeros((B, 14)))
    p = kw.pop("p", np.zeros((B, 2)))
    return m, m.line_search(p, x, lbx, ubx, q, dw, y, **kw), x


def test_only_the_third_candidate_passes():
    """x = 0, p = (1, 0): f(x) = 20 (two frames, 10 (0 - 1)^2 each), v = 0.  Along dx = (0, 0, 0, 4, 0, 0) the defect is |4 a| and the cost
    10 + 10 (4 a - 1)^2: phi(a) = 10 + 10 (4 a - 1)^2 + 4 a with mu = 1 -- 104, 22, 11, 13 for a = 1, 1/2, 1/4, 1/8.  With q' dx = -80 the threshold is
    20 - 1e-4 * 80 a, so 1 and 1/2 fail and 1/4 passes."""
    q = np.zeros((1, 8)); q[0, 5] = -20.0
    m, out, x = _hand([0, 0, 0, 4.0, 0, 0], q=q, p=np.array([[1.0, 0.0]]), candidates=4)
    assert np.array_equal(out["phis"][0], [20.0, 104.0, 22.0, 11.0, 13.0])
    assert out["accepted"][0] == 2 and out["alpha"][0] == 0.25 and out["D"][0] == -80.0
    assert np.array_equal(x[0], [0, 0, 0, 1.0, 0, 0]) and out["x"] is x
    assert out["step_max"][0] == 1.0 and out["f"][0] == 10.0 and out["gmax"][0] == 1.0
    assert np.array_equal(out["phi"][0], [20.0, 11.0]) and out["mu"][0] == 1.0


def test_ascent_direction_takes_the_last_candidate():
    """from the minimiser x = 0 of p = 0 every step raises the merit: no candidate passes, the last one is taken and reported as -1"""
    m, out, x = _hand([0, 0, 0, 1.0, 0, 0], candidates=4)
    assert out["accepted"][0] == -1 and out["alpha"][0] == 0.125 and out["D"][0] == 0.0
    assert np.array_equal(x[0], [0, 0, 0, 0.125, 0, 0])
    assert out["phi"][0, 1] == 10.0 * 0.125 ** 2 + 0.125 and out["gmax"][0] == 0.125
    # K = 1 with finite data always takes alpha0
    m, out, x = _hand([0, 0, 0, 1.0, 0, 0], candidates=1, alpha0=0.75)
    assert out["accepted"][0] == -1 and out["alpha"][0] == 0.75 and x[0, 3] == 0.75


def test_overflowing_step_leaves_x_untouched():
    x = np.array([[0.5, -0.25, 0.0, 0.25, 1.0, 0.0]])
    keep = x.copy()
    m, out, x = _hand([1e200, -1e200, 0, 1e200, 0, 1e200], x=x, candidates=8)
    assert out["accepted"][0] == -2 and out["alpha"][0] == 0.0 and out["step_max"][0] == 0.0
    assert np.array_equal(x, keep)
    v, g = m.violation(keep, np.full((1, 6), -np.inf), np.full((1, 6), np.inf))
    assert out["f"][0] == m.objective(np.zeros((1, 2)), keep)[0] and out["gmax"][0] == g[0]
    assert out["phi"][0, 0] == out["phi"][0, 1] == out["f"][0] + v[0]


def test_failed_status_keeps_x_and_mu():
    B = 3
    x = np.arange(18.0).reshape(B, 6) / 8.0
    keep = x.copy()
    dw = np.ones((B, 8)); y = np.full((B, 14), 5.0)
    dw[1] = np.nan; y[1] = np.nan
    mu = np.array([2.0, 3.0, 4.0])
    m = _di2()
    out = m.line_search(np.zeros((B, 2)), x, np.full((B, 6), -np.inf), np.full((B, 6), np.inf), np.zeros((B, 8)), dw, y, status=[1, 3, 7], mu=mu)
    assert np.array_equal(x[1], keep[1]) and mu[1] == 3.0
    assert out["accepted"][1] == -2 and out["alpha"][1] == 0.0 and out["step_max"][1] == 0.0
    assert np.isfinite(out["f"]).all() and np.isfinite(out["gmax"]).all() and np.isfinite(out["phi"]).all()
    assert out["f"][1] == m.objective(np.zeros((1, 2)), keep[1:2])[0]
    assert np.array_equal(mu[[0, 2]], [5.5, 5.5])                 # mu_factor * max |y| = 1.1 * 5
    assert (out["alpha"][[0, 2]] > 0).all() and not np.array_equal(x[0], keep[0])


def test_mu_is_monotone_across_calls():
    m = _di2()
    mu = np.zeros(2)
    args = lambda: (np.zeros((2, 2)), np.zeros((2, 6)), np.full((2, 6), -np.inf), np.full((2, 6), np.inf), np.zeros((2, 8)), np.zeros((2, 8)))
    y = np.zeros((2, 14)); y[0, 3] = -10.0; y[1, 0] = 100.0        # (y[1, 0] is a parameter row's multiplier: not counted)
    m.line_search(*args(), y, mu=mu)
    assert np.array_equal(mu, [11.0, 1.0])                         # max(mu_min, 1.1 * 10), mu_min
    m.line_search(*args(), 0.1 * y, mu=mu)
    assert np.array_equal(mu, [11.0, 1.0])                         # smaller multipliers do not lower it
    m.line_search(*args(), 2.0 * y, mu=mu, mu_min=3.0)
    assert np.array_equal(mu, [22.0, 3.0])


def test_box_terms_and_infinite_bounds():
    m = _di2()
    x = np.array([[0.0, 3.0, -2.0, 0.0, 0.0, 0.0]])
    lbx = np.array([[-np.inf, -2.0, -1.0, -np.inf, -np.inf, -np.inf]]); ubx = np.array([[np.inf, 2.0, 1.0, np.inf, np.inf, np.inf]])
    v, g = m.violation(x, lbx, ubx)
    # defects: s1 - F = (0, 0) - (0 + 1.5 - 0.25, 3 - 1) = (-1.25, -2); box: v0 over by 1, u0 under by 1
    assert v[0] == 1.25 + 2.0 + 1.0 + 1.0 and g[0] == 2.0


def test_refusals():
    m = _di2()
    a = (np.zeros((1, 2)), np.zeros((1, 6)), np.zeros((1, 6)), np.zeros((1, 6)), np.zeros((1, 8)), np.zeros((1, 8)), np.zeros((1, 14)))
    for kw in (dict(candidates=0), dict(candidates=9), dict(beta=0.0), dict(beta=1.0), dict(alpha0=0.0), dict(alpha0=-1.0), dict(c1=-0.1), dict(c1=1.0)):
        with pytest.raises(ValueError):
            m.line_search(*a, **kw)


# ------------------------------------------------------------------------------------------------ options of the loops
def test_loop_options(built):
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver, _line_search_options
    assert _line_search_options(None) is None and _line_search_options(False) is None
    assert _line_search_options(True) == {"candidates": 4, "beta": 0.5, "c1": 1e-4, "mu_min": 1.0, "mu_factor": 1.1}
    assert _line_search_options({"candidates": 6, "beta": 0.7})["candidates"] == 6
    with pytest.raises(ValueError):
        _line_search_options({"backtrack": 3})
    with pytest.raises(ValueError, match="stage OCP"):
        SQPOptimizationSolver(models.reference_test_cases()[1][0], {"max_iter": 1, "alpha": 1.0, "line_search": True}, batch=1, qp_solver=OracleCuCaQP(1))


# ------------------------------------------------------------------------------------------------ the host recipe on the oracle
@pytest.fixture(scope="module")
def recipe_runs(built):
    mdl, arg = lc.recipe()
    fixed = lc.host_loop(mdl, arg, {"alpha": 1.0}, OracleCuCaQP(lc.RECIPE_BATCH, nthreads=4))
    search = lc.host_loop(mdl, arg, {"alpha": 1.0, "line_search": True}, OracleCuCaQP(lc.RECIPE_BATCH, nthreads=4))
    return mdl, arg, fixed, search


def test_recipe_armijo_holds_where_accepted(recipe_runs):
    mdl, arg, _, (sol, log) = recipe_runs
    c1 = 1e-4
    x_old = np.zeros_like(log[0]["x"])
    seen = 0
    for it in log:
        ls = it["ls"]
        mu = ls["mu"]
        phi = lambda x: mdl.objective(arg["p"], x) + mu * mdl.violation(x, arg["lbx"], arg["ubx"])[0]
        p_old, p_new = phi(x_old), phi(it["x"])
        ok = ls["accepted"] >= 0
        seen += int(ok.sum())
        assert (p_new[ok] <= p_old[ok] + c1 * ls["alpha"][ok] * ls["D"][ok]).all()
        assert (ls["D"] <= 0.0).all()
        x_old = it["x"]
    assert seen >= 3 * lc.RECIPE_BATCH
    mus = np.array([it["ls"]["mu"] for it in log])
    assert (np.diff(mus, axis=0) >= 0.0).all()                       # the penalty persists and never decreases


def test_recipe_search_rescues_the_worst_instance(recipe_runs):
    """Measured on the CPU oracle, seed 5, after 4 iterations: the batch's worst max-norm violation is 30.69 with the fixed step alpha = 1 and
    0.1944 with the search (158 x); the median is 5.06e-4 in both runs; mean accepted alpha per iteration 1.0, 1.0, 1.0, 0.930.  Required: a
    margin of at least 2 x."""
    mdl, arg, (_, fixed), (_, search) = recipe_runs
    worst_fixed, worst_search = fixed[-1]["gmax"].max(), search[-1]["gmax"].max()
    print("worst gmax: fixed %.4g, search %.4g; median %.3g / %.3g; mean alpha %s" % (
        worst_fixed, worst_search, np.median(fixed[-1]["gmax"]), np.median(search[-1]["gmax"]), [round(float(l["alpha"].mean()), 3) for l in search]))
    assert np.isfinite(worst_search) and 2.0 * worst_search <= worst_fixed


def test_warm_start_uses_the_instance_step(built):
    """with warm_start_admm the QP start is (1 - alpha_b) dw per instance"""
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    mdl, arg = lc.recipe()

    class Spy(OracleCuCaQP):
        starts = []

        def setPrimalDualStart(self, x0, y0):
            Spy.starts.append(None if x0 is None else np.array(x0))
            super().setPrimalDualStart(x0, y0)

    sol = SQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "line_search": True, "warm_start_admm": True}, batch=lc.RECIPE_BATCH,
                                qp_solver=Spy(lc.RECIPE_BATCH, nthreads=4))
    sol.getOptimalSolution(arg)
    sol.alpha_taken = np.linspace(0.0, 1.0, lc.RECIPE_BATCH)          # pretend the search damped the instances differently
    dw = np.array(sol.last_qp_info["x"])
    sol.getOptimalSolution(arg)
    assert np.array_equal(Spy.starts[-1], (1.0 - np.linspace(0.0, 1.0, lc.RECIPE_BATCH))[:, None] * dw)


# ------------------------------------------------------------------------------------------------ conditions on the kernel cases
@pytest.fixture(scope="module")
def kernel_refs(built):
    return {(kind, which, K): lc.reference(lc.kernel_case(kind), which, K)[0] for kind in lc.KINDS for which in (0, 1) for K in lc.CANDIDATES}


def test_kernel_cases_cover_the_outcomes(kernel_refs):
    seen = set()
    for out in kernel_refs.values():
        seen |= set(int(a) for a in out["accepted"])
    assert -1 in seen and -2 in seen and len([a for a in seen if a >= 0]) >= 3, sorted(seen)
    # and the listed arrangement alone (scales 1, 3, 10 on ok instances) already spreads over three candidates
    seen0 = set()
    for (kind, which, K), out in kernel_refs.items():
        if which == 0:
            seen0 |= set(int(a) for a in out["accepted"])
    assert len([a for a in seen0 if a >= 0]) >= 3 and -2 in seen0, sorted(seen0)


def test_kernel_cases_have_no_undecided_instance(kernel_refs):
    for key, out in kernel_refs.items():
        assert not lc.undecided(out).any(), key


def test_kernel_cases_failed_instances(kernel_refs):
    for (kind, which, K), out in kernel_refs.items():
        case = lc.kernel_case(kind)
        _, _, status = lc.arrangement(case, which)
        bad = ~np.isin(status, lc.OK)
        assert bad.any() and (out["accepted"][bad] == -2).all() and (out["alpha"][bad] == 0.0).all()
        assert np.array_equal(out["x"][bad], case["x"][bad])
        assert np.isfinite(out["f"]).all() and np.isfinite(out["gmax"]).all() and np.isfinite(out["phi"]).all() and np.isfinite(out["mu"]).all()
        if K == 1:                                                   # finite data: alpha0 is always taken
            fin = ~bad & (np.abs(case["scales"][which]) < 1e100)
            assert (out["alpha"][fin] == 1.0).all()
