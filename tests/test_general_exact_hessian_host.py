"""CPU: the exact Hessian of the Lagrangian on the general NLP path without a GPU -- GeneralNLP(..., exact_hessian=True), its NumPy
statement lagrangian_system with the DOMINANT safeguard, the generated host build general_host_lagrangian, the tables, the refusals, the recipe on
the CPU oracle, the facade key, the gfx950 cross-build and a sanitizer run of a stand-alone program.  These pin the inputs of
tests/test_gpu_general_exact_hessian.py.

Tolerances.  constraint_curvature against second central differences at 60 digits (step 1e-15: the reference's own error is ~1e-30): the project's
evaluator bar 1e-12 max(1, |ref|); measured distance 1.7e-16 (pendulum), 1.3e-16 (recipe), 0 (skip-coupled: no curvature).
Host build against the statement: the same bar; measured 8.9e-16 on P, 1.1e-16 on shift (the statement sums |C| over a whole column and subtracts
the diagonal, the walk skips it).  lambda_min(C + diag(shift)) >= -1e-12 ||C||_F: Gershgorin gives >= 0 in exact arithmetic; eigvalsh and the
rounding of R are a few ulp of ||C||.

The recipe on the CPU oracle, QPs solved to 1e-11, iterations to max|dx| < 1e-10 within 40 (three starts per p, seed 11):
    leg                      p = 3         p = -2
    cost-only                none, none, none   none, none, none
    exact, mode 0            10, 7, 7      not asserted (the oracle answers NON_CVX, lambda_min down to -19.7)
    dominant                 8, 7, 7       14, 18, 16
    dominant + line_search   8, 6, 7       21, 24, 24
The caps asserted below are these counts plus two."""
import os
import subprocess

import numpy as np
import pytest
import yaml

from optimal_control_problem_amd import codegen
from optimal_control_problem_amd.general_eval import colour_columns, compress
from optimal_control_problem_amd.general_nlp import GeneralNLP
from optimal_control_problem_amd.ocp import General, OptimalControlProblem
from optimal_control_problem_amd.sqp import SQPOptimizationSolver
from tests.support import general_exact_hessian_cases as ge
from tests.support import general_problems as gp
from tests.support import nlp_hp as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("CG", "ccol", "cslot", "ccols", "cptr", "clist", "cdiag", "lagrangian", "GnMulIn", "GnCurvOut", "cp =", "ncc")
CAPS = {"exact": (12, 9, 9), "dominant": (10, 9, 9, 16, 20, 18), "dominant_ls": (10, 8, 9, 23, 26, 26)}


def _callables(name):
    if name == "recipe":
        return ge.recipe_constraints
    if name == "pendulum":
        return gp.pendulum_constraints
    return gp.problem("skip_coupled")["constraints"]


# ------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("name", ge.NAMES)
def test_constraint_curvature_against_60_digits(name):
    c = ge.case(name); mdl = c["model"]
    cons = _callables(name)
    rows = [0, 1]
    for y in (c["y"], np.zeros_like(c["y"])):
        got = mdl.constraint_curvature(c["p"][rows], c["x"][rows], y[rows])
        assert got.shape == (2, mdl.n, mdl.n) and np.array_equal(got, got.transpose(0, 2, 1))
        assert not got[:, ~mdl.cm].any()                                                    # nothing outside the structure
        for i, b in enumerate(rows):
            with hp.mp.workdps(hp.DPS):
                lam = hp._mpfs(y[b, mdl.n:])
                fun = lambda z: sum((l * v for l, v in zip(lam, hp._list(cons(hp._vec(z))))), hp.mpf(0))
                _, _, H = hp.grad_hess(fun, hp._mpfs(c["p"][b]) + hp._mpfs(c["x"][b]), hp.mpf(hp.STEP))
                ref = np.array([[float(v) for v in row] for row in H])
            dist = (np.abs(got[i] - ref) / np.maximum(1.0, np.abs(ref))).max()
            print(name, "y = 0" if not y.any() else "random y", "instance", b, "distance", dist)
            assert dist <= ge.TOL
            if not y.any():
                assert not got[i].any()
    if name == "skip_coupled":
        assert not mdl.cm.any() and not mdl.constraint_curvature(c["p"], c["x"], c["y"]).any()


def test_flagged_pattern_and_zero_slots():
    for name in ge.NAMES:
        c = ge.case(name); mdl = c["model"]; plain = ge.model(name, False)
        cur, rows, cols = ge.slots(mdl)
        assert np.array_equal(mdl.hm, plain.hm | mdl.cm) and np.array_equal(mdl.cm, mdl.cm.T)
        has = mdl.cm.any(axis=0)
        assert np.array_equal(np.diag(mdl.cm), has)                                        # the safeguard's slot
        assert (mdl.Ap == plain.Ap).all() and (mdl.Ai == plain.Ai).all()
        # the slots the flag adds hold 0 after local_system; the others hold what the unflagged model gives
        Pplain = plain.local_system(c["p"], c["x"], c["lbx"], c["ubx"], c["lbg"], c["ubg"]).P
        added = ~plain.hm[rows, cols]
        assert not c["P"][:, added].any() and np.array_equal(c["P"][:, ~added], Pplain)
        assert int(added.sum()) == {"pendulum": 28, "recipe": 2, "skip_coupled": 0}[name]


def test_unflagged_model_is_what_it_was():
    for name in ("pendulum", "skip_coupled"):
        old = gp.problem(name)["model"]; new = ge.model(name, False)
        for attr in ("exact_hessian", "cm", "_cgtape", "_ccols"):
            assert not hasattr(new, attr)
        assert np.array_equal(old.Pp, new.Pp) and np.array_equal(old.Pi, new.Pi)
        assert codegen.general_device_source(new) == codegen.general_device_source(old)
        for src in (codegen.general_device_source(new), codegen.general_host_source(new)):
            body = src[src.index("namespace {"):]                                           # (the included headers are named above it)
            for word in NEW_NAMES:
                assert word not in body, word
        assert "compress_curvature" not in str(sorted(compress(new))) and "ccol" not in compress(new)
        with pytest.raises(ValueError, match="exact_hessian=True"):
            new.constraint_curvature(np.zeros((1, 2)), np.zeros((1, new.nvar)), np.zeros((1, new.m)))
        with pytest.raises(ValueError, match="exact_hessian=True"):
            new.lagrangian_system(np.zeros((1, 2)), np.zeros((1, new.nvar)), np.zeros((1, new.m)), np.zeros((1, len(new.Pi))))
    flagged = codegen.general_device_source(ge.model("pendulum"))
    assert "mpcqp_general_lagrangian" in flagged and "CG(" in flagged and "const double m0 = mul(0);" in flagged


def test_models_without_curvature_are_accepted():
    free = GeneralNLP(3, 1, ge.recipe_cost, None, exact_hessian=True)                     # ng = 0
    lin = ge.model("skip_coupled")
    for mdl, plain in ((free, GeneralNLP(3, 1, ge.recipe_cost, None)), (lin, ge.model("skip_coupled", False))):
        assert mdl.exact_hessian and not mdl.cm.any() and np.array_equal(mdl.Pi, plain.Pi) and np.array_equal(mdl.Pp, plain.Pp)
        c = compress(mdl)
        assert c["cp"] == 0 and len(c["ccols"]) == 0 and (c["ccol"] == -1).all()
        P = np.random.default_rng(0).normal(size=(3, len(mdl.Pi)))
        y = np.random.default_rng(1).normal(size=(3, mdl.m))
        for mode in (0, 1):
            Pn, shift = mdl.lagrangian_system(np.zeros((3, mdl.np)), np.zeros((3, mdl.nvar)), y, P, None, mode)
            assert ge_bits(Pn, P) and not shift.any()
            Ph, _, sh = ge.host_lagrangian(mdl, np.zeros((3, mdl.np)), np.zeros((3, mdl.nvar)), y, P, None, mode)
            assert ge_bits(Ph, P) and not sh.any()


def ge_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ------------------------------------------------------------------------------------------------ 2. tables
@pytest.mark.parametrize("name", ge.NAMES)
def test_colouring_and_slot_tables_of_the_curvature(name):
    mdl = ge.model(name)
    c = compress(mdl)
    cm, n = mdl.cm, mdl.n
    colour, cp = c["ccol"], c["cp"]
    assert (colour_columns(cm)[0] == colour).all() and c["cslot"].shape == (cp, n)
    assert ((colour >= 0) == cm.any(axis=0)).all() and (colour < cp).all() and set(colour[colour >= 0].tolist()) == set(range(cp))
    for k in range(cp):
        assert (cm[:, colour == k].sum(axis=1) <= 1).all()                                  # no two columns of a colour share a row
    # every non-negative slot names entry (r, the column of that colour with row r) in P's widened CSC; together they are the curvature's slots
    cur, rows, cols = ge.slots(mdl)
    where = {(int(r), int(cc)): s for s, (r, cc) in enumerate(zip(rows, cols))}
    got = {}
    for k in range(cp):
        for r in range(n):
            if c["cslot"][k, r] >= 0:
                (col,) = [j for j in np.nonzero(colour == k)[0] if cm[r, j]]
                assert where[(r, int(col))] == c["cslot"][k, r]
                got[(r, int(col))] = int(c["cslot"][k, r])
    assert sorted(got.values()) == np.nonzero(cur)[0].tolist() and len(got) == int(cm.sum())
    # the walk: ascending slots of each column with curvature, its diagonal among them
    assert (c["ccols"] == np.nonzero(cm.any(axis=0))[0]).all() and len(c["cptr"]) == len(c["ccols"]) + 1
    for i, j in enumerate(c["ccols"]):
        lst = c["clist"][c["cptr"][i]:c["cptr"][i + 1]]
        assert lst.tolist() == sorted(lst.tolist()) == [s for s in range(mdl.Pp[j], mdl.Pp[j + 1]) if cur[s]]
        assert c["cdiag"][i] in lst and rows[c["cdiag"][i]] == j and cols[c["cdiag"][i]] == j
    if name == "pendulum":
        print("pendulum: curvature colours", cp, "columns", len(c["ccols"]), "slots", len(c["clist"]))
        assert cp < len(c["ccols"])                                                         # compressed: fewer passes than columns


def test_tape_cap_counts_the_contracted_gradient():
    mdl, plain = ge.model("pendulum"), ge.model("pendulum", False)
    count = lambda t: sum(1 for i in t.live_nodes() if t.nodes[i][0] not in ("in", "const"))
    size = codegen.general_tape_size(mdl)
    assert size == codegen.general_tape_size(plain) + count(mdl._cgtape) and count(mdl._cgtape) > 0
    with pytest.raises(codegen.TapeTooLarge, match="%d operations" % size):
        codegen.emit_general(mdl, cap=size - 1)
    assert codegen.emit_general(mdl, cap=size)
    assert codegen.emit_general(plain, cap=size - count(mdl._cgtape))


# ------------------------------------------------------------------------------------------------ 3. statement and host build
@pytest.mark.parametrize("name", ge.NAMES)
def test_host_build_matches_the_statement(built, name):
    c = ge.case(name); mdl = c["model"]
    cur, rows, cols = ge.slots(mdl)
    Cd = mdl.constraint_curvature(c["p"], c["x"], c["y"])
    for mode in (0, 1):
        Pr, sr = mdl.lagrangian_system(c["p"], c["x"], c["y"], c["P"], None, mode)
        Ph, Cw, sh = ge.host_lagrangian(mdl, c["p"], c["x"], c["y"], c["P"], None, mode)
        print(name, "mode", mode, "P", np.abs(Ph - Pr).max(), "shift", np.abs(sh - sr).max())
        assert gp.close(Ph, Pr, ge.TOL) and gp.close(sh, sr, ge.TOL)
        assert gp.close(Cw[:, cur], Cd[:, rows, cols][:, cur], ge.TOL) and np.isnan(Cw[:, ~cur]).all()     # the workspace: C on its slots only
        # P' - P = C + diag(shift)
        D = ge.dense(mdl, Pr) - ge.dense(mdl, c["P"])
        want = Cd + np.stack([np.diag(v) for v in sr])
        assert np.abs(D - want).max() <= ge.TOL * max(1.0, np.abs(want).max())
        if mode == 0:
            assert not sr.any() and not sh.any()
            Pn, none, _ = ge.host_lagrangian(mdl, c["p"], c["x"], c["y"], c["P"], None, 0, workspace=False)
            assert none is None and ge_bits(Pn, Ph)                                         # the same bits with and without the workspace
        else:
            dg = np.arange(mdl.n)
            R = np.abs(Cd).sum(axis=1) - np.abs(Cd[:, dg, dg])
            dominant = Cd[:, dg, dg] >= R
            assert (sr >= 0.0).all() and not sr[dominant].any() and not sh[dominant].any()
            if name != "skip_coupled":
                assert sr.any() and dominant[:, mdl.cm.any(axis=0)].any()                   # both kinds of column occur


def test_dominant_shift_makes_the_addend_positive_semidefinite(built):
    rng = np.random.default_rng(3)
    for name in ("pendulum", "recipe"):
        c = ge.case(name); mdl = c["model"]
        worst, indefinite = 0.0, 0
        for draw in range(64):
            y = rng.normal(0.0, 3.0, (2, mdl.m))
            P0 = c["P"][:2]
            Ph, _, sh = ge.host_lagrangian(mdl, c["p"][:2], c["x"][:2], y, P0, None, 1)
            add = ge.dense(mdl, Ph) - ge.dense(mdl, P0)                                     # C + diag(shift) as the build applied it
            fro = np.sqrt((add ** 2).sum(axis=(1, 2)))
            lam = np.linalg.eigvalsh(add).min(axis=1)
            worst = min(worst, (lam / np.maximum(fro, 1e-300)).min())
            assert (lam >= -1e-12 * fro).all(), (name, draw, lam, fro)
            raw = np.linalg.eigvalsh(mdl.constraint_curvature(c["p"][:2], c["x"][:2], y)).min(axis=1)
            indefinite += int((raw < 0.0).sum())
        assert indefinite >= 32                                                             # the safeguard had something to do
        print(name, "worst lambda_min / ||.||_F over 64 draws", worst)


@pytest.mark.parametrize("name", ("pendulum", "recipe"))
def test_zero_multipliers_and_failed_instances_keep_every_bit(built, name):
    c = ge.case(name); mdl = c["model"]
    bad = ~np.isin(c["status"], ge.OK)
    assert bad.sum() == 2 and np.isnan(c["ynan"][bad]).all()
    P = c["P"].copy(); P[:, ::3] = -0.0                                                      # a signed zero is a bit pattern too
    for mode in (0, 1):
        for run in (lambda y, st: mdl.lagrangian_system(c["p"], c["x"], y, P, st, mode),
                    lambda y, st: (lambda r: (r[0], r[2]))(ge.host_lagrangian(mdl, c["p"], c["x"], y, P, st, mode))):
            Pz, sz = run(np.zeros_like(c["y"]), None)
            assert ge_bits(Pz, P) and not sz.any()
            Pf, sf = run(c["ynan"], c["status"])
            assert ge_bits(Pf[bad], P[bad]) and not sf[bad].any() and np.isfinite(Pf).all()
            Pa, sa = run(c["y"], None)
            assert ge_bits(Pf[~bad], Pa[~bad]) and ge_bits(sf[~bad], sa[~bad]) and not ge_bits(Pa[bad], P[bad])


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_option_refusals(built):
    from optimal_control_problem_amd import models
    from tests.support.oracle_backend import OracleCuCaQP
    opts = {"max_iter": 1, "alpha": 1.0}
    plain, mdl = ge.model("recipe", False), ge.model("recipe")
    with pytest.raises(ValueError, match=r"GeneralNLP\(\.\.\., exact_hessian=True\)"):
        SQPOptimizationSolver(plain, dict(opts, exact_hessian=True), batch=2, qp_solver=OracleCuCaQP(batch=2))
    with pytest.raises(ValueError, match="True or 'dominant'"):
        SQPOptimizationSolver(mdl, dict(opts, exact_hessian="project"), batch=2, qp_solver=OracleCuCaQP(batch=2))
    with pytest.raises(ValueError, match="convexify"):
        SQPOptimizationSolver(models.CartPole(3, 0.02), dict(opts, exact_hessian="dominant"), batch=2, qp_solver=OracleCuCaQP(batch=2))
    with pytest.raises(ValueError, match="mode must be"):
        mdl.lagrangian_system(np.zeros((1, 1)), np.zeros((1, 3)), np.zeros((1, 6)), np.zeros((1, 8)), None, 2)
    for value, mode in ((True, 0), ("dominant", 1)):
        sol = SQPOptimizationSolver(mdl, dict(opts, exact_hessian=value), batch=2, qp_solver=OracleCuCaQP(batch=2))
        assert sol.exact_hessian is True and sol._nlp_mode == mode and sol.lam.shape == (2, mdl.m) and not sol.lam.any()
    off = SQPOptimizationSolver(mdl, dict(opts, exact_hessian=False), batch=2, qp_solver=OracleCuCaQP(batch=2))
    assert off.exact_hessian is False and off.lam is None and off._nlp_mode is None


# ------------------------------------------------------------------------------------------------ 5. the recipe on the CPU oracle
@pytest.fixture(scope="module")
def recipe_logs(built):
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, arg, x0 = ge.recipe()
    legs = {"cost": {}, "exact": {"exact_hessian": True}, "dominant": {"exact_hessian": "dominant"},
            "dominant_ls": {"exact_hessian": "dominant", "line_search": True}}
    return {k: ge.host_loop(mdl, arg, x0, opt, OracleCuCaQP(6), ge.RECIPE_ITERS, qp_tol=1e-11) for k, opt in legs.items()}


def _converged(log):
    """iterations to a step below 1e-10 per instance (0: never), counting only iterations whose QP returned a point"""
    steps = np.array([np.where(np.isin(e["status"], ge.OK), e["step"], np.inf) for e in log])
    below = steps < ge.RECIPE_TOL
    return np.where(below.any(axis=0), below.argmax(axis=0) + 1, 0)


def test_recipe_on_the_cpu_oracle(recipe_logs):
    mdl = ge.model("recipe")
    its = {k: _converged(log) for k, (sol, log) in recipe_logs.items()}
    print("iterations to max|dx| < 1e-10 (0: not within 40):", {k: v.tolist() for k, v in its.items()})
    assert (its["cost"] == 0).all()                                                        # the cost-only Hessian does not get there in 40
    assert (its["exact"][:3] > 0).all() and (its["exact"][:3] <= CAPS["exact"]).all()      # p = 3 (p = -2 is not asserted: the QP may be NON_CVX)
    assert (its["dominant"] > 0).all() and (its["dominant"] <= CAPS["dominant"]).all()
    # every instance of a leg that converged sits at a feasible point, and the two exact legs agree at p = 3
    for k in ("dominant", "dominant_ls"):
        x = recipe_logs[k][1][-1]["x"]
        g = mdl.constraints(np.array([[3.0]] * 3 + [[-2.0]] * 3), x)
        assert np.abs(g).max() < 1e-9
    assert np.abs(recipe_logs["exact"][1][-1]["x"][:3] - recipe_logs["dominant"][1][-1]["x"][:3]).max() < 1e-8
    # the safeguard: lambda_min(P) >= lambda_min(hessian(f)) - 1e-12 ||C||_F in every iteration; the raw curvature goes indefinite at p = -2
    Hf = 2.0 * np.eye(4); Hf[0, 1] = Hf[1, 0] = -2.0                                       # hessian(f) over w = [p; x]: constant
    floor = np.linalg.eigvalsh(Hf).min()
    lows = []
    for e in recipe_logs["dominant"][1]:
        Pd = ge.dense(mdl, e["P"])
        fro = np.sqrt(((Pd - Hf) ** 2).sum(axis=(1, 2)))
        lam = np.linalg.eigvalsh(Pd).min(axis=1)
        assert (lam >= floor - 1e-12 * fro).all()
        lows.append(lam)
    raw = np.min([np.linalg.eigvalsh(ge.dense(mdl, e["P"])).min(axis=1) for e in recipe_logs["exact"][1]], axis=0)
    print("lambda_min(P): dominant", np.min(lows, axis=0), "mode 0", raw, "hessian(f)", floor)
    assert (raw[3:] < -1.0).all()


def test_host_loop_with_exact_hessian_and_line_search(recipe_logs):
    sol, log = recipe_logs["dominant_ls"]
    its = _converged(log)
    assert (its > 0).all() and (its <= CAPS["dominant_ls"]).all()
    assert sol.alpha_taken is not None and sol.shift.shape == (6, 4) and (sol.shift >= 0.0).all()
    # lam follows lam += alpha_b (y - lam): with the full step at the end it is the QP's multipliers
    assert np.abs(sol.lam - sol.last_qp_info["y"]).max() < 1e-6
    sol.setInitialGuess(np.zeros((6, 3)))
    assert not sol.lam.any()


# ------------------------------------------------------------------------------------------------ 6. the facade
class RecipeOCP(OptimalControlProblem):
    """the recipe through the builders: two frames of three, frame 0 pinned and appearing nowhere"""

    def deployConstraintsAndAddCost(self):
        self.setReference(1)
        self.addScalarCost(General(lambda X, p: (X[3] - p[0]) ** 2 + (X[4] - 1.0) ** 2 + (X[5] + 0.5) ** 2))
        self.addEquationConstraint("sphere", General(lambda X, p: [X[3] * X[3] + X[4] * X[4] + X[5] * X[5] - 1.0], 1))
        self.addEquationConstraint("saddle", General(lambda X, p: [X[3] * X[4] - 0.3 * X[5] - 0.2], 1))


def recipe_node(value, steps=12):
    node = yaml.safe_load(gp.TESTCPP_YAML % (steps, 3, "[-5.0, -5.0, -5.0]", "[5.0, 5.0, 5.0]"))["optimal_control_problem"]
    if value is not None:
        node["solver_settings"]["SQP_settings"]["exact_hessian"] = value
    return node


def test_facade_key(built):
    from tests.support.oracle_backend import OracleCuCaQP
    seen = {}
    for value in (None, False, True, "dominant"):
        ocp = RecipeOCP(recipe_node(value), batch=2, qp_solver=OracleCuCaQP(batch=2))
        ocp.deployConstraintsAndAddCost(); ocp.genSolver()
        sol = ocp.OSQPSolverPtr_
        on = value in (True, "dominant")
        assert ocp.generalPath_ and type(sol) is SQPOptimizationSolver and sol.exact_hessian is on
        assert getattr(ocp.model_, "exact_hessian", False) is on and sol._nlp_mode == {True: 0, "dominant": 1}.get(value if on else None)
        seen[value] = len(ocp.model_.Pi)
    assert seen[None] == seen[False] < seen[True] == seen["dominant"]
    with pytest.raises(ValueError, match="expected true, false or dominant"):
        RecipeOCP(recipe_node("project"), batch=1, qp_solver=OracleCuCaQP(batch=1))
    # a problem that lands on the stage path: the key names the gap
    node = gp.di_node(); node["solver_settings"]["SQP_settings"]["exact_hessian"] = True
    ocp = gp.DoubleIntegratorOCP(node, batch=1, qp_solver=OracleCuCaQP(batch=1))
    ocp.deployConstraintsAndAddCost()
    with pytest.raises(ValueError, match="6.18"):
        ocp.genSolver()
    # and the key turns the iteration count of the facade's own loop around: 12 iterations reach the optimum with it, not without
    ends = {}
    for value in (None, "dominant"):
        ocp = RecipeOCP(recipe_node(value), batch=1, qp_solver=OracleCuCaQP(batch=1))
        ocp.deployConstraintsAndAddCost(); ocp.genSolver()
        ocp.OSQPSolverPtr_.qpSolver_.setAbsoluteTolerance(1e-9)
        ocp.OSQPSolverPtr_.setInitialGuess(np.array([[0.8, 0.5, 0.1, 0.8, 0.5, 0.1]]))       # (at the facade's zero start the sphere row has no gradient)
        ocp.computeOptimalTrajectory(np.array([[0.8, 0.5, 0.1]]), np.array([[3.0]]))
        ends[value] = float(np.max(ocp.OSQPSolverPtr_.step_max))
    print("facade, last step of 12 iterations:", ends)
    assert ends["dominant"] < 1e-6 < ends[None]


# ------------------------------------------------------------------------------------------------ 7. the builds
def test_device_library_cross_compiles_and_exports(built):
    syms = {}
    for flagged in (True, False):
        so = codegen.build_general_device_library(ge.model("pendulum", flagged))
        syms[flagged] = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
        for sym in ("mpcqp_general_abi", "mpcqp_general_eval", "mpcqp_general_merit", "mpcqp_general_linesearch"):
            assert sym in syms[flagged]
    assert "mpcqp_general_lagrangian" in syms[True] and "mpcqp_general_lagrangian" not in syms[False]
    assert "GnUser" not in syms[True]
    lin = subprocess.check_output(["nm", "-D", "--defined-only", codegen.build_general_device_library(ge.model("skip_coupled"))], text=True)
    assert "mpcqp_general_lagrangian" in lin                                                # flagged without curvature: the export is there, a no-op


def test_standalone_program_under_the_sanitizers(built, tmp_path):
    """general_host_lagrangian of the pendulum's host source inside a program with its own main, built with -fsanitize=address,undefined: both modes,
    y = 0, a failed instance, NaN multipliers (tests/support/general_lagrangian_main.cpp checks the bit-level promises itself).  The sanitizer
    runtimes are linked statically: the program needs nothing from its environment"""
    src = tmp_path / "pendulum_host.cpp"
    src.write_text(codegen.general_host_source(ge.model("pendulum")))
    exe = tmp_path / "lagrangian_main"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", codegen.CSRC,
           '-DGEN_SRC="%s"' % src, "-o", str(exe), os.path.join(ROOT, "tests", "support", "general_lagrangian_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
