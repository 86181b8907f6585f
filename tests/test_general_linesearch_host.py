"""CPU: the per-instance merit line search of the general NLP path (mpcqp_nlp_linesearch) without a GPU -- the NumPy statement
(general_nlp.GeneralNLP.line_search) on hand-made inputs, the generated functor's host build (general_host_linesearch: the kernel's rule header
compiled by g++, a loop over the candidates) against the statement on the kernel cases, the runaway recipe on the CPU oracle, the gfx950
cross-build with and without the export, the host loop and the facade's YAML key.

Tolerances: the host build runs the emitted text of the same tapes the statement evaluates in NumPy; floats pass the project's evaluator bar,
1e-12 relative to max(1, |ref|) with non-finite values matching exactly (general_problems.close); `accepted` and `alpha` are compared exactly,
which the kernel cases allow because none of their instances is undecided (linesearch_cases.undecided) -- asserted here, not assumed."""
import subprocess

import numpy as np
import pytest
import yaml

from optimal_control_problem_amd import _lib, codegen
from optimal_control_problem_amd.general_nlp import GeneralNLP
from optimal_control_problem_amd.sqp import SQPOptimizationSolver
from tests.support import general_linesearch_cases as gl
from tests.support import general_problems as gp
from tests.support import linesearch_cases as lc
from tests.support.oracle_backend import OracleCuCaQP

INF = float("inf")


# ------------------------------------------------------------------------------------------------ the statement on hand-made inputs
def _toy():
    """nvar 2, np 1: f = (x0 - p)^2 + x1^2, one row g = x0 + x1"""
    return GeneralNLP(2, 1, lambda w: (w[1] - w[0]) ** 2 + w[2] ** 2, lambda w: [w[1] + w[2]])


def _toy_call(m, x, dx, y=None, status=None, mu=None, lbg=-INF, ubg=INF, lbx=-10.0, ubx=10.0, p=1.0, **kw):
    B = x.shape[0]
    x = np.array(x, float)
    w = np.concatenate([np.full((B, 1), p), x], axis=1)
    q = np.stack([np.zeros(B), 2.0 * (w[:, 1] - w[:, 0]), 2.0 * w[:, 2]], axis=1)
    dw = np.concatenate([np.zeros((B, 1)), np.asarray(dx, float)], axis=1)
    y = np.zeros((B, 4)) if y is None else np.asarray(y, float)
    out = m.line_search(np.full((B, 1), p), x, np.full((B, 2), lbx), np.full((B, 2), ubx), q, dw, y, status=status, mu=mu,
                        lbg=np.full((B, 1), lbg), ubg=np.full((B, 1), ubg), **kw)
    return out, x


def test_violation_measures():
    m = _toy()
    p = np.array([[1.0]]); x = np.array([[3.0, -12.0]])
    v, g = m.violation(p, x, np.array([[-10.0, -10.0]]), np.array([[2.0, INF]]), np.array([[-4.0]]), np.array([[INF]]))
    # row g = -9 below -4 by 5; x0 above 2 by 1; x1 below -10 by 2; the infinite bounds contribute 0
    assert v[0] == 5.0 + 1.0 + 2.0 and g[0] == 5.0
    v, g = m.violation(p, x, np.full((1, 2), -INF), np.full((1, 2), INF), np.array([[-INF]]), np.array([[INF]]))
    assert v[0] == 0.0 and g[0] == 0.0                                   # floor 0, general rows only
    c = gp.problem("cost_only")["model"]                                  # ng = 0: box terms only, gmax 0
    v, g = c.violation(np.ones((1, 1)), np.full((1, 5), 3.0), np.full((1, 5), -2.0), np.full((1, 5), 2.0), np.zeros((1, 0)), np.zeros((1, 0)))
    assert v[0] == 5.0 and g[0] == 0.0


def test_every_branch_of_accepted():
    m = _toy()
    x = np.array([[0.0, 2.0]] * 5)
    #  0: the Newton step is accepted at once; 1: a step four times too long is accepted at j = 2; 2: an ascent direction, K = 2: nothing accepted,
    #  the last candidate is finite (-1); 3: an overflowing step, nothing finite (-2); 4: the QP failed (-2), dx and y are NaN
    dx = np.array([[1.0, -2.0], [4.0, -8.0], [-1.0, 2.0], [1e200, 1e200], [np.nan, np.nan]])
    y = np.zeros((5, 4)); y[4] = np.nan
    status = np.array([1, 2, 7, 1, 3])
    out, xn = _toy_call(m, x, dx, y=y, status=status, candidates=4)
    assert list(out["accepted"][:2]) == [0, 2] and list(out["alpha"][:2]) == [1.0, 0.25]
    assert np.array_equal(xn[0], [1.0, 0.0]) and np.array_equal(xn[1], [1.0, 0.0])
    assert out["accepted"][3] == -2 and out["alpha"][3] == 0.0 and np.array_equal(xn[3], x[3])
    assert out["accepted"][4] == -2 and out["alpha"][4] == 0.0 and np.array_equal(xn[4], x[4]) and np.isnan(out["phis"][4, 1:]).all()
    assert np.isfinite(out["f"]).all() and np.isfinite(out["phi"]).all() and out["f"][4] == 5.0 and out["step_max"][4] == 0.0
    out2, xn2 = _toy_call(m, x[2:3], dx[2:3], candidates=2)
    assert out2["accepted"][0] == -1 and out2["alpha"][0] == 0.5 and np.array_equal(xn2[0], [-0.5, 3.0]) and out2["D"][0] == 0.0
    assert out2["f"][0] == m.objective(np.ones((1, 1)), xn2)[0] and out2["step_max"][0] == 1.0
    # the keys and shapes of models.StageOCP.line_search
    assert set(out) == {"x", "alpha", "accepted", "step_max", "f", "gmax", "phi", "mu", "D", "alphas", "phis"}
    assert out["phi"].shape == (5, 2) and out["phis"].shape == (5, 5) and list(out["alphas"]) == [1.0, 0.5, 0.25, 0.125]


def test_the_penalty_is_monotone_and_failed_instances_keep_theirs():
    m = _toy()
    x = np.array([[0.0, 2.0]] * 3); dx = np.array([[1.0, -2.0]] * 3)
    y = np.zeros((3, 4)); y[:, 0] = 1e6; y[0, 3] = -20.0; y[1, 2] = 3.0; y[2, 1] = 50.0      # (column 0 is the parameter's row: not looked at)
    mu = np.array([0.5, 40.0, 7.0])
    out, _ = _toy_call(m, x, dx, y=y, status=np.array([1, 1, 9]), mu=mu)
    assert np.allclose(mu, [22.0, 40.0, 7.0]) and mu[2] == 7.0 and np.allclose(out["mu"], [22.0, 40.0, 7.0])
    before = mu.copy()
    _toy_call(m, x, dx, y=np.zeros((3, 4)), status=np.array([1, 1, 1]), mu=mu)
    assert (mu >= before).all() and mu[2] == 7.0
    out, _ = _toy_call(m, x, dx, y=y, mu=None, mu_min=2.0, mu_factor=0.0)
    assert (out["mu"] == 2.0).all()
    # an infeasible start: the violation enters the merit and the slope
    out, _ = _toy_call(m, np.array([[0.0, 2.0]]), np.array([[1.0, -2.0]]), lbg=-INF, ubg=0.5, mu=np.array([3.0]))
    assert out["phis"][0, 0] == 5.0 + 3.0 * 1.5 and out["D"][0] == (-2.0 * 1.0 + 4.0 * -2.0) - 3.0 * 1.5 and out["gmax"][0] == 0.5


def test_refusals_of_the_statement():
    m = _toy()
    x = np.zeros((1, 2)); dx = np.ones((1, 2))
    for kw in (dict(candidates=0), dict(candidates=9), dict(beta=0.0), dict(beta=1.0), dict(alpha0=0.0), dict(alpha0=-1.0), dict(alpha0=INF),
               dict(c1=-0.1), dict(c1=1.0), dict(mu_min=-1.0), dict(mu_factor=INF)):
        with pytest.raises(ValueError):
            _toy_call(m, x, dx, **kw)
    with pytest.raises(ValueError, match="lbg"):
        m.line_search(np.ones((1, 1)), x, x - 1, x + 1, np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 4)))
    from optimal_control_problem_amd.models import StageOCP
    from optimal_control_problem_amd.sqp import _line_search_options
    assert _line_search_options(True) == StageOCP.LINE_SEARCH_DEFAULTS            # the defaults still come from the stage statement
    assert "mpcqp_nlp_linesearch" in _lib.EXPORTS and "mpcqp_nlp_has_linesearch" in _lib.EXPORTS


# ------------------------------------------------------------------------------------------------ the host build against the statement
@pytest.mark.parametrize("name", gl.PROBLEMS)
def test_kernel_cases_have_no_undecided_instance(name):
    """a condition on the inputs, not a tolerance: the exact comparison of `accepted` and `alpha` below and on the GPU rests on it"""
    case = gl.kernel_case(name)
    if name == "cost_only":
        assert (case["qp_status"] == 9).any() and case["model"].ng == 0          # NON_CVX instances, no general rows
    else:
        assert (case["qp_status"] == 1).all()
    for which in (0, 1):
        for K in (1, 4, 8):
            for mu0 in (None, MU0):
                ref, _ = gl.reference(case, which, K, mu0=mu0)
                assert not lc.undecided(ref).any(), (name, which, K)


MU0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])            # below, above and far above what the multipliers ask for


@pytest.mark.parametrize("K", gl.CANDIDATES)
@pytest.mark.parametrize("name", gl.PROBLEMS)
def test_host_build_matches_the_statement(built, name, K):
    case = gl.kernel_case(name)
    mdl = case["model"]
    for which in (0, 1):
        dw, y, status = gl.arrangement(case, which)
        for mu0 in (None, MU0):
            tag = (name, K, which, mu0 is not None)
            ref, mu_ref = gl.reference(case, which, K, mu0=mu0)
            got = gl.host_line_search(mdl, case["p"], case["x"], case["lbx"], case["ubx"], case["lbg"], case["ubg"], case["q"], dw, y, status=status,
                                      mu=mu0, candidates=K)
            assert np.array_equal(got["accepted"], ref["accepted"]) and np.array_equal(got["alpha"], ref["alpha"]), tag
            for k in gl.FLOATS + ("D",):
                assert gp.close(got[k], ref[k], gl.TOL), (tag, k)
            # (the merits of every candidate, a test output: NaN where a candidate was not evaluated or overflowed into inf - inf, in both alike)
            nan = np.isnan(ref["phis"])
            assert np.array_equal(np.isnan(got["phis"]), nan) and gp.close(np.where(nan, 0.0, got["phis"]), np.where(nan, 0.0, ref["phis"]), gl.TOL), tag
            bad = ~np.isin(status, lc.OK)
            assert (got["accepted"][bad] == -2).all() and (got["alpha"][bad] == 0.0).all(), tag
            assert np.array_equal(got["x"][bad].view(np.int64), case["x"][bad].view(np.int64)), tag        # bit for bit
            if mu0 is not None:
                assert np.array_equal(got["mu"][bad], mu0[bad]) and gp.close(got["mu"], mu_ref, gl.TOL), tag
                assert (got["mu"][~bad] >= mu0[~bad]).all(), tag


def test_cache_key_covers_the_rule_header(built, monkeypatch):
    import os
    seen = []
    real_open = open

    def spy(path, *a, **k):
        seen.append(os.path.basename(str(path)))
        return real_open(path, *a, **k)

    monkeypatch.setattr(codegen, "open", spy, raising=False)
    codegen.build_general_host_library(gp.problem("testcpp1")["model"])
    assert "general_linesearch.hpp" in seen and "general_kernels.hpp" in seen


@pytest.mark.parametrize("name", ["pendulum", "cost_only"])
def test_device_library_exports_the_entry_unless_told_not_to(built, name):
    m = gp.problem(name)["model"]
    with_ls = codegen.build_general_device_library(m)
    without = codegen.build_general_device_library(m, line_search=False)
    assert with_ls != without and with_ls == codegen.build_general_device_library(m, line_search=True)
    syms = lambda so: subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert "mpcqp_general_linesearch" in syms(with_ls) and "mpcqp_general_linesearch" not in syms(without)
    for sym in ("mpcqp_general_abi", "mpcqp_general_eval", "mpcqp_general_merit"):
        assert sym in syms(with_ls) and sym in syms(without)
    assert "linesearch" not in codegen.general_device_source(m, line_search=False)
    assert codegen.GENERAL_TAPE_CAP == 6000 and "GENERAL_ABI_VERSION 1" in open(codegen.CSRC + "/general_kernels.hpp").read()


# ------------------------------------------------------------------------------------------------ the recipe on the CPU oracle
@pytest.fixture(scope="module")
def recipe_logs(built):
    mdl, arg, x0 = gl.recipe()
    B = gl.RECIPE_BATCH
    _, searched = gl.host_loop(mdl, arg, x0, {"alpha": 1.0, "line_search": True}, OracleCuCaQP(B), gl.RECIPE_ITERS)
    _, fixed = gl.host_loop(mdl, arg, x0, {"alpha": 1.0}, OracleCuCaQP(B), gl.RECIPE_ITERS)
    return mdl, searched, fixed


def test_the_search_brings_every_instance_of_the_recipe_home(recipe_logs):
    mdl, searched, fixed = recipe_logs
    assert (mdl.n, mdl.ng) == (7, 2)
    home = gl.near_optimum(searched[-1]["x"]); lost = gl.near_optimum(fixed[-1]["x"])
    print("within 1e-2 of the optimum after %d iterations: %d of %d with the search, %d with alpha = 1; f max %.3f against %.3f"
          % (gl.RECIPE_ITERS, home.sum(), home.size, lost.sum(), searched[-1]["f"].max(), fixed[-1]["f"].max()))
    assert home.all()
    assert lost.sum() < 16
    for it in range(gl.PARITY_ITERS):
        assert not lc.undecided(searched[it]["ls"]).any(), it                 # what the device-loop parity test on the GPU rests on
    assert all((s["accepted"] >= -1).all() for s in searched)                  # every QP returned a point, every instance moved


def test_host_loop_options_on_a_general_nlp(built):
    """warm_start_admm with (1 - alpha_b) dx, skip_failed_steps and sqp_tol go through the shared loop code"""
    mdl, arg, x0 = gl.recipe()
    B = gl.RECIPE_BATCH
    sol = SQPOptimizationSolver(mdl, {"max_iter": 30, "alpha": 1.0, "line_search": {"candidates": 6}, "warm_start_admm": True, "skip_failed_steps": True,
                                      "sqp_tol": 1e-6}, batch=B, qp_solver=OracleCuCaQP(B))
    sol.setInitialGuess(x0)
    r = sol.getOptimalSolution(arg)
    assert sol.iterations_done < 30 and gl.near_optimum(r["x"]).all() and sol.line_search["candidates"] == 6
    assert sol.alpha_taken.shape == (B,) and sol.accepted.shape == (B,) and (sol._mu >= 1.0).all() and np.isfinite(sol.gmax).all()


# ------------------------------------------------------------------------------------------------ the facade
def _node(line_search):
    node = yaml.safe_load(gp.DI_YAML)["optimal_control_problem"]
    if line_search is not None:
        node["solver_settings"]["SQP_settings"]["line_search"] = line_search
    return node


def test_facade_passes_the_yaml_key_through(built):
    frame = np.array([[1.0, 0.0, 0.0], [0.5, -0.2, 0.0]]); ref = np.zeros((2, 2))
    out = {}
    for key, value in (("absent", None), ("false", False), ("true", True), ("map", {"candidates": 3, "beta": 0.25})):
        ocp = gp.SkipCoupledOCP(_node(value), batch=2, qp_solver=OracleCuCaQP(batch=2))
        ocp.deployConstraintsAndAddCost(); ocp.genSolver()
        sol = ocp.OSQPSolverPtr_
        assert ocp.generalPath_ and type(sol) is SQPOptimizationSolver
        if key in ("absent", "false"):
            assert sol.line_search is None
        elif key == "true":
            assert sol.line_search == {"candidates": 4, "beta": 0.5, "c1": 1e-4, "mu_min": 1.0, "mu_factor": 1.1}
        else:
            assert sol.line_search["candidates"] == 3 and sol.line_search["beta"] == 0.25 and sol.line_search["c1"] == 1e-4
        out[key] = ocp.computeOptimalTrajectory(frame, ref)
        if sol.line_search is not None:
            assert sol.accepted is not None and (sol.accepted >= -1).all()
    # the problem is a convex QP solved to 1e-3: the search may shorten the second, already tiny step, so the bar is the 5e-3 at which
    # tests/test_gpu_general_device.py holds facade results against their expected values
    assert np.abs(out["true"] - out["absent"]).max() < 5e-3 and np.abs(out["map"] - out["absent"]).max() < 5e-3
    assert np.array_equal(out["false"], out["absent"])
    # a stage problem takes the key as well (the host arm of a stage pattern)
    ocp = gp.DoubleIntegratorOCP(_node(True), batch=2, qp_solver=OracleCuCaQP(batch=2))
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    assert not ocp.generalPath_ and ocp.OSQPSolverPtr_.line_search is not None
    for bad in ("yes", 3, {"backtrack": 2}):
        with pytest.raises(ValueError):
            gp.SkipCoupledOCP(_node(bad), batch=1)
