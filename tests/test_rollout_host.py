"""CPU: the dynamically feasible start (mpcqp_stage_rollout) -- its NumPy statement models.StageOCP.rollout, the recipe that motivates it on the CPU
oracle, options["initial_guess"] of the host SQP loop, and the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, codegen, models
from optimal_control_problem_amd.sqp import ROLLOUT_NEEDS_DYNAMICS, SQPOptimizationSolver
from optimal_control_problem_amd.stage_eval import model_tape
from tests.support import rollout_cases as rc
from tests.support.oracle_backend import OracleCuCaQP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = rc.bits


@pytest.mark.parametrize("N", rc.HORIZONS)
@pytest.mark.parametrize("name", rc.MODELS)
@pytest.mark.parametrize("mode", ["iterate", "hold"])
def test_rule(name, N, mode):
    mdl = rc.model(name, N)
    x, lbx, ubx = rc.inputs(mdl, 5)
    out = mdl.rollout(x, lbx, ubx, inputs=mode)
    assert (out["diverged"] == -1).all() and np.isfinite(out["x"]).all()
    rc.check_rule(mdl, x, lbx, ubx, mode, out["x"])                     # every step bitwise F on the statement's own output
    X = out["x"].reshape(5, N, mdl.f)
    assert np.array_equal(bits(X[0, 0]), bits(lbx[0, :mdl.f]))          # instance 0 is pinned: it comes out as pinned
    viol = np.fmax.reduce(np.fmax(lbx - out["x"], out["x"] - ubx), axis=1, initial=0.0)
    assert np.array_equal(out["box_viol"], viol)
    # without the pair the clip is the identity and nothing is reported
    free = mdl.rollout(x, inputs=mode)
    assert np.array_equal(bits(free["x"].reshape(5, N, mdl.f)[:, 0]), bits(x.reshape(5, N, mdl.f)[:, 0])) and (free["box_viol"] == 0.0).all()


def test_hold_copies_u0_bitwise():
    mdl = rc.model("quadrotor", 20)
    x, _, _ = rc.inputs(mdl, 4)
    X = mdl.rollout(x, inputs="hold")["x"].reshape(4, 20, mdl.f)
    for k in range(1, 20):
        assert np.array_equal(bits(X[:, k, mdl.nx:]), bits(X[:, 0, mdl.nx:]))


def test_frozen_rows_are_untouched():
    mdl = rc.model("cartpole", 3)
    x, lbx, ubx = rc.inputs(mdl, 6)
    frozen = np.array([0, 1, 0, 0, 1, 0], np.int32)
    out = mdl.rollout(x, lbx, ubx, frozen=frozen)
    ref = mdl.rollout(x, lbx, ubx)
    fz = frozen != 0
    assert np.array_equal(bits(out["x"][fz]), bits(x[fz])) and np.array_equal(bits(out["x"][~fz]), bits(ref["x"][~fz]))
    assert (out["diverged"][fz] == -1).all() and (out["box_viol"][fz] == 0.0).all()


def test_instance_parameter_rows_are_honoured():
    mdl = rc.model("cartpole", 20)
    x, lbx, ubx = rc.inputs(mdl, 2)
    x[1], lbx[1], ubx[1] = x[0], lbx[0], ubx[0]                         # the same instance twice ...
    rows = rc.cartpole_rows(2)
    shared = mdl.rollout(x, lbx, ubx)["x"]
    assert np.array_equal(bits(shared[0]), bits(shared[1]))
    mdl.set_instance_params(rows)                                       # ... with different masses
    out = mdl.rollout(x, lbx, ubx)
    mdl.set_instance_params(None)
    assert not np.array_equal(out["x"][0], out["x"][1]) and not np.array_equal(out["x"][0], shared[0])
    rc.check_rule(mdl, x, lbx, ubx, "iterate", out["x"], rows=rows)
    with pytest.raises(ValueError):
        mdl.set_instance_params(rows[:1]); mdl.rollout(x, lbx, ubx)
    mdl.set_instance_params(None)


def test_divergence_is_held_and_reported():
    mdl = rc.blowup(5)
    x = np.zeros((2, 5, 2)); x[1, 0, 0] = 1.0
    out = mdl.rollout(x.reshape(2, -1))
    X = out["x"].reshape(2, 5, 2)
    assert out["diverged"].tolist() == [-1, 1]
    assert (X[0] == 0.0).all()
    assert X[1, 1, 0] == 1e150 and (X[1, 2:, 0] == 1e150).all()
    assert np.isfinite(out["x"]).all()
    # a non-finite first frame the caller handed in is held and reported as step 0
    x[0, 0, 0] = np.inf
    out = mdl.rollout(x.reshape(2, -1))
    assert out["diverged"].tolist() == [0, 1] and (out["x"].reshape(2, 5, 2)[0, :, 0] == np.inf).all()


def test_arguments():
    mdl = rc.model("double_integrator", 3)
    x, lbx, ubx = rc.inputs(mdl, 2)
    with pytest.raises(ValueError):
        mdl.rollout(x, lbx, None)
    with pytest.raises(ValueError):
        mdl.rollout(x, lbx, ubx, inputs="zero")


def test_recipe_zero_start_is_infeasible_rollout_start_is_not(built):
    """cart-pole N = 100 from the workload's seed on the CPU oracle: the local system at x = 0 is primal infeasible in every instance, the one at
    the trajectory rolled out from the pinned frame with its input held is solved in every instance"""
    from oracle import oracle as orc
    mdl, meta = rc.recipe(4)
    pat = None
    got = {}
    zeros = np.zeros((4, mdl.nvar))
    start = mdl.rollout(zeros, meta["lbx"], meta["ubx"], inputs="hold")
    assert (start["box_viol"] == 0.0).all() and (start["diverged"] == -1).all()
    for key, x in (("zero", zeros), ("rollout", start["x"])):
        ls = mdl.local_system(meta["p"], x, meta["lbx"], meta["ubx"], meta["lbg"], meta["ubg"])
        pat = pat or orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
        got[key] = pat.solve(ls.P, ls.q, ls.A, ls.l, ls.u, orc.default_settings())
        print(key, "status", got[key]["status"].tolist(), "ADMM iterations", got[key]["iters"].tolist())
    assert got["zero"]["status"].tolist() == [3, 3, 3, 3]
    assert got["rollout"]["status"].tolist() == [1, 1, 1, 1]


def _loop(mdl, B, **opt):
    return SQPOptimizationSolver(mdl, dict({"max_iter": 2, "alpha": 1.0}, **opt), batch=B, qp_solver=OracleCuCaQP(B, nthreads=4))


@pytest.mark.parametrize("option,mode", [("rollout", "hold"), ("reshoot", "iterate")])
def test_host_loop_option_equals_the_composed_calls(built, option, mode):
    mdl = rc.model("cartpole", 20)
    B = 3
    x, lbx, ubx = rc.inputs(mdl, B)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(rc.clip(x.reshape(B, 20, mdl.f)[:, 0], *mdl.frame_bounds()))
    arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    guess = np.nan_to_num(x)
    a = _loop(mdl, B, initial_guess=option); a.setInitialGuess(guess)
    ra = a.getOptimalSolution(arg)
    b = _loop(mdl, B); b.setInitialGuess(mdl.rollout(guess, lbx, ubx, inputs=mode)["x"])
    rb = b.getOptimalSolution(arg)
    assert np.array_equal(bits(ra["x"]), bits(rb["x"])) and np.isfinite(ra["x"]).all()
    assert (a.rollout_diverged == -1).all() and a.rollout_box_viol.shape == (B,)
    # applied once: a second call continues from the stored iterate ...
    ra2, rb2 = a.getOptimalSolution(arg), b.getOptimalSolution(arg)
    assert np.array_equal(bits(ra2["x"]), bits(rb2["x"]))
    # ... and setInitialGuess re-arms it
    a.setInitialGuess(guess); b.setInitialGuess(mdl.rollout(guess, lbx, ubx, inputs=mode)["x"])
    assert np.array_equal(bits(a.getOptimalSolution(arg)["x"]), bits(b.getOptimalSolution(arg)["x"]))
    # without the option nothing changes: the loop from the raw guess is another one
    c = _loop(mdl, B); c.setInitialGuess(guess)
    assert c.initial_guess is None and not np.array_equal(c.getOptimalSolution(arg)["x"], ra["x"]) and c.rollout_diverged is None


def test_general_path_refuses_the_option_with_the_reason():
    from optimal_control_problem_amd.sqp import _initial_guess_option
    from tests.support.general_problems import problem
    mdl = problem("pendulum")["model"]                                  # a general_nlp.GeneralNLP
    dense = models.reference_test_cases()[0][0]                         # a DenseNLP of the reference's test.cpp: no dynamics either
    for bad in (mdl, dense):
        with pytest.raises(ValueError) as e:
            SQPOptimizationSolver(bad, {"max_iter": 1, "alpha": 1.0, "initial_guess": "rollout"}, batch=1, qp_solver=OracleCuCaQP(1))
        assert str(e.value) == ROLLOUT_NEEDS_DYNAMICS and "no notion of dynamics" in str(e.value)
    with pytest.raises(ValueError) as e:
        _initial_guess_option("rollout", rc.model("cartpole", 3), evaluator=object())      # an evaluator= without dynamics (general_eval.GeneralEvaluator)
    assert str(e.value) == ROLLOUT_NEEDS_DYNAMICS
    with pytest.raises(ValueError):
        _initial_guess_option("shoot", rc.model("cartpole", 3))
    assert _initial_guess_option(None, mdl) is None


def test_abi(built):
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert "int mpcqp_stage_rollout(mpcqp_stage *s, int batch, const mpcqp_stage_rollout_args *a, void *stream);" in header
    assert "mpcqp_stage_rollout" in _lib.EXPORTS
    assert (_lib.ROLLOUT_INPUTS_ITERATE, _lib.ROLLOUT_INPUTS_HOLD) == (0, 1)
    assert re.search(r"#define MPCQP_ROLLOUT_INPUTS_ITERATE 0\b", header) and re.search(r"#define MPCQP_ROLLOUT_INPUTS_HOLD\s+1\b", header)
    # the struct's fields in the header's order
    body = re.search(r"typedef struct mpcqp_stage_rollout_args \{(.*?)\} mpcqp_stage_rollout_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", body)
    assert names == [f[0] for f in _lib.RolloutArgs._fields_]
    L = _lib.lib()
    assert L.mpcqp_stage_rollout.argtypes[2]._type_ is _lib.RolloutArgs
    # null handle and null block are refused before anything touches a device
    assert L.mpcqp_stage_rollout(None, 1, None, None) == _lib.ERR_ARG


def test_generated_library_exports_the_launcher(built):
    tape = model_tape(rc.model("pendulum", 3))
    src = codegen.library_source(tape)
    assert src.count("mpcqp_user_rollout") == 1 and "stage_launch_rollout<SmUser>" in src
    # the launcher is a block behind the translation unit, whose own text does not move; the test-only switch leaves the block out
    assert src.startswith(codegen.device_source(tape)) and codegen.library_source(tape, rollout=False) == codegen.device_source(tape)
    assert "mpcqp_user_rollout" not in codegen.device_source(tape)
    so = codegen.build_device_library(tape)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T mpcqp_user_rollout$", syms, re.M)
    hip = open(os.path.join(ROOT, "optimal_control_problem_amd", "csrc", "stage_eval.hip")).read()
    assert "the library does not export mpcqp_user_rollout (generated before this entry); regenerate it" in hip
