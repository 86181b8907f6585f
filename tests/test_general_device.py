"""CPU: the general (non-stage) NLP's device evaluator without a GPU -- the colouring that compresses the Hessian and Jacobian passes, the
generated functor built for the host (the same emitted text, g++, a host loop over the passes with the same tables) against
GeneralNLP.local_system, the gfx950 cross-build, and the facade's wiring.

Tolerance of the host-build parity: forward-over-reverse duals against complex-step columns (symmetrised), relative to max(1, |ref|).
Measured maximum on the nonlinear problem (pendulum, 64 random points): 3.4e-16, below 1e-13, so the bar is the project's 1e-12 for
evaluator parity."""
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import codegen
from optimal_control_problem_amd.general_eval import colour_columns, compress, slot_table
from optimal_control_problem_amd.models import _csc_from_dense_mask
from tests.support import general_problems as gp

TOL = 1e-12


_close = gp.close


def _check_colouring(mask, colour, ncol, slot, colptr, first):
    mask = np.asarray(mask, bool)
    rows, cols = mask.shape
    # columns without entries have no colour, all others one in range
    assert ((colour >= 0) == mask.any(axis=0)).all() and (colour < ncol).all()
    assert set(colour[colour >= 0].tolist()) == set(range(ncol))
    # no two columns of a colour share a row
    for c in range(ncol):
        assert (mask[:, colour == c].sum(axis=1) <= 1).all()
    # the non-negative slots are a bijection onto the CSC positions of this block; each names entry (r, the column of that colour with row r)
    want = {}
    for j in range(cols):
        for e, r in enumerate(np.nonzero(mask[:, j])[0]):
            want[(int(colour[j]), int(r))] = int(colptr[j]) + first + e
    got = {(int(c), int(r)): int(slot[c, r]) for c in range(slot.shape[0]) for r in range(rows) if slot[c, r] >= 0}
    assert got == want and len(set(got.values())) == len(got) == int(mask.sum())


@pytest.mark.parametrize("name", gp.NAMES)
def test_colouring_of_the_problems(name):
    m = gp.problem(name)["model"]
    c = compress(m)
    assert c["hp"] == max(c["hcolours"], 1) and c["jp"] == (max(c["jcolours"], 1) if m.ng else 0)
    assert c["hslot"].shape == (c["hp"], m.n) and c["jslot"].shape == (c["jp"], m.ng)
    _check_colouring(m.hm, c["hcol"], c["hcolours"], c["hslot"][:c["hcolours"]], m.Pp, 0)
    assert sorted(c["hslot"][c["hslot"] >= 0].tolist()) == list(range(len(m.Pi)))          # all of P
    if m.ng:
        jm = m.am[m.n:]
        _check_colouring(jm, c["jcol"], c["jcolours"], c["jslot"][:c["jcolours"]], m.Ap, 1)
        ident = {int(m.Ap[j]) for j in range(m.n)}                                          # the identity entry leads its column
        assert all(m.Ai[s] == j for j, s in enumerate(sorted(ident)))
        assert sorted(c["jslot"][c["jslot"] >= 0].tolist()) == sorted(set(range(len(m.Ai))) - ident)
    else:
        assert (c["jcol"] == -1).all()
    if name == "skip_coupled":
        assert (m.n, m.ng, c["hcolours"], c["jcolours"]) == (32, 26, 11, 4)                  # against 32 + 30 columns
    if name.startswith("testcpp"):
        assert (c["hcol"][m.np:m.np + m.nvar // 2] == -1).all()                              # frame 0 appears nowhere


@pytest.mark.parametrize("seed", range(20))
def test_colouring_of_random_masks(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40)); rows = int(rng.integers(1, 40))
    dens = rng.choice([0.02, 0.1, 0.3, 0.8])
    sym = rng.random((n, n)) < dens
    sym = sym | sym.T
    sym[:, rng.integers(0, n)] = False; sym = sym & sym.T                                   # at least one empty column (and row)
    rect = rng.random((rows, n)) < dens
    rect[:, rng.integers(0, n)] = False
    for mask, first in ((sym, 0), (rect, 1)):
        colour, ncol = colour_columns(mask)
        full = np.vstack([np.eye(n, dtype=bool), mask]) if first else mask                  # A = [I; J]: one leading identity entry per column
        colptr, _ = _csc_from_dense_mask(full)
        _check_colouring(mask, colour, ncol, slot_table(mask, colour, ncol, colptr, first), colptr, first)


host_eval, violation = gp.host_eval, gp.violation


@pytest.mark.parametrize("name", gp.NAMES)
def test_host_build_of_the_generated_functor_matches_local_system(built, name):
    pr = gp.problem(name); m = pr["model"]
    B = 64 if name == "pendulum" else 6
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=5)
    ref = m.local_system(p, x, lbx, ubx, lbg, ubg)
    got = host_eval(m, p, x, lbx, ubx, lbg, ubg)
    worst = 0.0
    for k in ("P", "q", "A", "l", "u"):
        r = getattr(ref, k); fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(got[k]), fin) and np.array_equal(got[k][~fin], r[~fin])      # equal non-finite patterns, nothing left unwritten
        if fin.any():
            worst = max(worst, float((np.abs(got[k][fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))).max()))
    print("%s: max relative distance host build vs local_system %.3e" % (name, worst))
    for k in ("P", "q", "A", "l", "u"):
        assert _close(got[k], getattr(ref, k), TOL), k
    ident = np.array([int(m.Ap[j]) for j in range(m.n)])
    assert (got["A"][:, ident] == 1.0).all()                                                 # identity entries are exactly 1.0
    if m.ng:
        assert np.isneginf(got["l"][0, m.m - 1]) and np.isposinf(got["u"][0, m.m - 1])       # the loose row of instance 0 stays infinite
    assert _close(got["f"], m.objective(p, x), 1e-12)
    assert _close(got["gmax"], violation(m, p, x, lbg, ubg), 1e-11)


def test_emitted_shape_keeps_per_thread_storage_flat():
    """inputs are formed by the accessor where they are used, outputs go to the sink as they are produced: no array in the functor"""
    m = gp.problem("pendulum")["model"]
    src = codegen.emit_general(m)
    functor = src[:src.index("\n};\n")]
    bodies = functor[functor.index("template <class T"):]
    assert "= in(" in bodies and " out(" in bodies and "[" not in bodies and "]" not in bodies
    for fn in ("sm_sin", "sm_cos", "sm_tan", "sm_exp", "sm_log", "sm_sqrt", "sm_tanh", " / ", " * ", " + ", " - ", "= -"):
        assert fn in src, fn                                                                 # every operation the tracer knows
    assert src == codegen.emit_general(gp.pendulum()["model"])                               # deterministic
    # the stage flow's emission is what it was: the streaming form is opt-in
    from tests.test_codegen import pendulum_on_cart_with_drag
    stage = codegen.emit_functor(codegen.trace(pendulum_on_cart_with_drag, 3, 1))
    assert "= in(" not in stage and "out[0] =" in stage


@pytest.mark.parametrize("name", ["skip_coupled", "pendulum", "testcpp2", "cost_only"])
def test_device_library_cross_compiles_and_exports(built, name):
    m = gp.problem(name)["model"]
    so = codegen.build_general_device_library(m)
    assert os.path.exists(so) and so.endswith(".so") and so == codegen.build_general_device_library(m)      # cached by content
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for sym in ("mpcqp_general_abi", "mpcqp_general_dims", "mpcqp_general_tables", "mpcqp_general_eval", "mpcqp_general_merit"):
        assert sym in syms
    assert "GnUser" not in syms                                                              # internal linkage: libraries do not share tables


def test_cache_key_covers_the_general_kernel_header(built, tmp_path, monkeypatch):
    seen = []
    real_open = open

    def spy(path, *a, **k):
        seen.append(os.path.basename(str(path)))
        return real_open(path, *a, **k)

    monkeypatch.setattr(codegen, "open", spy, raising=False)
    codegen.build_general_host_library(gp.problem("testcpp1")["model"])
    assert "general_kernels.hpp" in seen and "stage_kernels.hpp" in seen


def test_tape_cap_refuses_with_a_reason():
    m = gp.problem("pendulum")["model"]
    size = codegen.general_tape_size(m)
    assert 0 < size <= codegen.GENERAL_TAPE_CAP
    with pytest.raises(codegen.TapeTooLarge, match="%d operations" % size):
        codegen.emit_general(m, cap=size - 1)
    assert codegen.emit_general(m, cap=size)


def test_facade_default_is_todays_object_graph(built):
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    ocp = gp.SkipCoupledOCP(gp.di_node(), batch=2, qp_solver=OracleCuCaQP(batch=2))
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    assert ocp.generalPath_ and ocp.generalDevice is False and type(ocp.OSQPSolverPtr_) is SQPOptimizationSolver
    assert ocp.generalDeviceReason_ is None and ocp.generalLibrary_ is None
    with pytest.raises(NotImplementedError, match="general path"):
        ocp.genCode()
    # an injected QP backend keeps the host loop even when the device form is asked for
    ocp = gp.SkipCoupledOCP(gp.di_node(), batch=2, qp_solver=OracleCuCaQP(batch=2), general_device=True)
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    assert type(ocp.OSQPSolverPtr_) is SQPOptimizationSolver
    with pytest.raises(NotImplementedError, match="general path"):
        ocp.genCode()


def test_facade_over_cap_tape_falls_back_to_the_host_loop_with_a_reason(built, monkeypatch):
    """needs no GPU: the refusal comes before anything touches the device, and the host loop's QP backend is only constructed here"""
    from optimal_control_problem_amd import sqp
    monkeypatch.setattr(codegen, "GENERAL_TAPE_CAP", 10)
    ocp = gp.SkipCoupledOCP(gp.di_node(), batch=1, general_device=True)
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    assert ocp.generalPath_ and type(ocp.OSQPSolverPtr_) is sqp.SQPOptimizationSolver
    assert "operations" in ocp.generalDeviceReason_ and ocp.generalLibrary_ is None
    with pytest.raises(codegen.TapeTooLarge):
        ocp.genCode()
