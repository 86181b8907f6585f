"""GPU: local-system evaluation of a general (non-stage) NLP on the device (mpcqp_nlp_*, csrc/general_kernels.hpp) against the host build
of the same generated functor, the arrays feeding the QP as borrowed device pointers, and the facade's general_device switch.

Tolerances: the device and the g++ build run the same emitted text with the same tables; they differ by compiler contraction and libm
only, so P, q, A, l, u pass the project's 1e-12 for evaluator parity (relative to max(1, |ref|)); identity entries, the damped update
and repeated evaluations are bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import general_problems as gp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_close = gp.close


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", gp.NAMES)
def test_eval_merit_step_match_the_host_build(built, name):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator, compress
    pr = gp.problem(name); m = pr["model"]
    ev = GeneralEvaluator(m)
    c = compress(m)
    assert (ev.nvar, ev.np, ev.ng, ev.n, ev.m, ev.nnzP, ev.nnzA, ev.passes) == (m.nvar, m.np, m.ng, m.n, m.m, len(m.Pi), len(m.Ai), c["hp"] + c["jp"])
    assert (ev.Pp == m.Pp).all() and (ev.Pi == m.Pi).all() and (ev.Ap == m.Ap).all() and (ev.Ai == m.Ai).all()
    ident = np.array([int(m.Ap[j]) for j in range(m.n)])
    for B in (1, 5, 67):                  # 67 instances x the passes: several 256-thread blocks, a partial last one, instances and passes mixed in a wave
        p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=B)
        ref = gp.host_eval(m, p, x, lbx, ubx, lbg, ubg)
        args = [_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)]
        out = ev.alloc(B)
        for t in out.values():
            t.fill_(float("nan"))                                  # every element must be written
        ev.eval(*args, out=out)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in ("P", "q", "A", "l", "u"):
            assert _close(got[k], ref[k], 1e-12), (k, B)
        assert (got["A"][:, ident] == 1.0).all()
        if m.ng:                                                   # instance 0 carries a row with -inf / +inf bounds
            assert np.isneginf(got["l"][0, m.m - 1]) and np.isposinf(got["u"][0, m.m - 1])
        again = ev.eval(*args)
        for k in ("P", "q", "A", "l", "u"):
            assert np.array_equal(again[k].cpu().numpy(), got[k], equal_nan=True), k       # one writer per element: the same bits
        f, g = ev.merit(args[0], args[1])
        assert _close(f.cpu().numpy(), m.objective(p, x), 1e-12)
        assert _close(g.cpu().numpy(), gp.violation(m, p, x, lbg, ubg), 1e-11)
        rng = np.random.default_rng(3)
        dw = rng.normal(size=(B, m.n)); xd = _dev(x)
        sm = ev.step(0.5, _dev(dw), xd)
        assert np.array_equal(xd.cpu().numpy(), x + 0.5 * dw[:, m.np:])
        assert np.array_equal(sm.cpu().numpy(), np.abs(0.5 * dw[:, m.np:]).max(axis=1))
        if B >= 5:      # with a status array, instances whose QP returned no point keep their iterate
            status = torch.ones(B, dtype=torch.int32, device="cuda"); status[0] = 3; status[B - 1] = 9; status[1] = 2; status[2] = 7
            before = xd.clone(); sm = ev.step(1.0, _dev(dw), xd, status=status)
            moved = (xd != before).any(dim=1).cpu().numpy()
            assert not moved[0] and not moved[B - 1] and moved[1:B - 1].all() and float(sm[0]) == 0.0
    ev.close()


def test_merit_uses_the_bounds_of_the_last_eval(built):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    pr = gp.problem("pendulum"); m = pr["model"]
    ev = GeneralEvaluator(m)
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, 4, seed=2)
    with pytest.raises(ValueError, match="bounds"):
        ev.merit(_dev(p), _dev(x))
    ev.eval(*[_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)])
    _, g1 = ev.merit(_dev(p), _dev(x))
    ev.eval(*[_dev(a) for a in (p, x, lbx, ubx, lbg - 1.0, ubg + 1.0)])
    _, g2 = ev.merit(_dev(p), _dev(x))
    assert _close(g1.cpu().numpy(), gp.violation(m, p, x, lbg, ubg), 1e-11)
    assert _close(g2.cpu().numpy(), gp.violation(m, p, x, lbg - 1.0, ubg + 1.0), 1e-11) and (g2 < g1).any()
    ev.close()


def test_a_captured_graph_replays_eval_step_and_merit(built):
    """nothing is allocated inside a call: eval, step and merit on caller-owned buffers capture into a HIP graph and replay"""
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    pr = gp.problem("pendulum"); m = pr["model"]
    ev = GeneralEvaluator(m)
    B = 9
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=4)
    args = [_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)]
    want = {k: v.clone() for k, v in ev.eval(*args).items()}
    out = ev.alloc(B)
    L = _lib.lib()
    f = torch.zeros(B, dtype=torch.float64, device="cuda"); g = torch.zeros(B, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream(); gr = torch.cuda.CUDAGraph()
    ptrs = [t.data_ptr() for t in args] + [out[k].data_ptr() for k in ("P", "q", "A", "l", "u")]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            _lib.check(L.mpcqp_nlp_eval(ev._h, B, *ptrs, s.cuda_stream))
            _lib.check(L.mpcqp_nlp_merit(ev._h, B, ptrs[0], ptrs[1], ptrs[4], ptrs[5], f.data_ptr(), g.data_ptr(), s.cuda_stream))
        for t in out.values():
            t.zero_()
        gr.replay(); s.synchronize()
    for k in ("P", "q", "A", "l", "u"):
        assert torch.equal(out[k], want[k]), k
    f0, g0 = ev.merit(args[0], args[1])
    assert torch.equal(f, f0) and torch.equal(g, g0)
    ev.close()


@pytest.mark.parametrize("name", ["skip_coupled", "pendulum"])
def test_eval_feeds_the_qp_without_leaving_the_device(built, name):
    """device-evaluated QP data -> mpcqp_update on borrowed device pointers -> solve: the statuses, iteration counts and solution of the
    host-evaluated data through the host path"""
    from optimal_control_problem_amd.batch_qp import BatchQP, solve_local_system
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    pr = gp.problem(name); m = pr["model"]
    B = 8
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=11)
    ls = m.local_system(p, x, lbx, ubx, lbg, ubg)
    ev = GeneralEvaluator(m)
    out = ev.eval(*[_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)])
    qp = BatchQP(ev.n, ev.m, B, ev.Pp, ev.Pi, ev.Ap, ev.Ai)
    qp.update(out["P"], out["q"], out["A"], out["l"], out["u"]); qp.solve(); got = qp.get(); qp.close()
    ref = solve_local_system(ls)
    assert (got["status"] == ref["status"]).all() and (got["status"] == 1).all()
    assert (got["iters"] == ref["iters"]).all()
    assert np.abs(got["x"] - ref["x"]).max() < 1e-7
    ev.close()


@pytest.mark.parametrize("idx", range(7))
def test_facade_testcpp_cases_on_the_device(built, idx):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, SQPOptimizationSolver
    od, xd, expect = gp.testcpp_through_builders(idx, True)
    oh, xh, _ = gp.testcpp_through_builders(idx, False)
    assert od.generalPath_ and oh.generalPath_ and od.generalDeviceReason_ is None
    assert type(od.OSQPSolverPtr_) is DeviceSQPOptimizationSolver and type(oh.OSQPSolverPtr_) is SQPOptimizationSolver
    assert np.abs(xd - xh).max() < 1e-6 and np.abs(xd[0] - expect).max() < 5e-3
    so = od.genCode()
    assert so.endswith(".so") and os.path.exists(so) and so == od.OSQPSolverPtr_.ev.library
    with pytest.raises(NotImplementedError, match="general path"):
        oh.genCode()


def test_facade_without_a_reference_vector_on_the_device(built):
    """np = 0 through the whole device loop: no setReference(), the parameter arrays have no elements"""
    import yaml
    from optimal_control_problem_amd.ocp import General, OptimalControlProblem

    class P(OptimalControlProblem):
        def deployConstraintsAndAddCost(self):
            self.addScalarCost(General(lambda X, p: (X[2] - 1.0) ** 2 + (X[3] + 2.0) ** 2 + X[2] * X[3]))
            self.addInequalityConstraint("sum", [-np.inf], General(lambda X, p: [X[2] + X[3]], 1), [0.5])

    node = yaml.safe_load(gp.TESTCPP_YAML % (10, 2, "[-10.0, -10.0]", "[10.0, 10.0]"))["optimal_control_problem"]
    ocp = P(node, batch=2, general_device=True)
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    assert ocp.generalPath_ and ocp.model_.np == 0 and type(ocp.OSQPSolverPtr_.ev).__name__ == "GeneralEvaluator"
    x = ocp.computeOptimalTrajectory(np.zeros((2, 2)), np.zeros((2, 0)))
    assert np.abs(x[:, 2:] - np.array([8.0 / 3, -10.0 / 3])).max() < 5e-3


def test_facade_skip_coupling_on_the_device(built):
    B = 4
    frame = np.array([[1.0, 0.0, 0.0], [0.5, -0.2, 0.0], [-1.0, 0.3, 0.0], [0.2, 0.1, 0.0]]); ref = np.zeros((B, 2))
    out = []
    for flag in (True, False):
        ocp = gp.SkipCoupledOCP(gp.di_node(), batch=B, general_device=flag)
        ocp.deployConstraintsAndAddCost(); ocp.genSolver()
        assert ocp.generalPath_ and type(ocp.OSQPSolverPtr_).__name__ == ("DeviceSQPOptimizationSolver" if flag else "SQPOptimizationSolver")
        out.append(ocp.computeOptimalTrajectory(frame, ref))
    assert np.abs(out[0] - out[1]).max() < 1e-6
    du2 = out[0].reshape(B, 10, 3)[:, 2:, 2] - out[0].reshape(B, 10, 3)[:, :-2, 2]
    assert np.abs(du2).max() <= gp.SkipCoupledOCP.d + 5e-3


def test_stage_problem_forced_onto_the_general_device_path_equals_the_stage_device_path(built):
    B = 3
    frame = np.array([[1.0, 0.0, 0.0], [0.5, -0.2, 0.0], [-1.0, 0.3, 0.0]]); ref = np.zeros((B, 2))
    stage = gp.DoubleIntegratorOCP(gp.di_node(), batch=B, device_resident=True)
    stage.deployConstraintsAndAddCost(); stage.genSolver()
    assert not stage.generalPath_ and type(stage.OSQPSolverPtr_).__name__ == "DeviceSQPOptimizationSolver"
    forced = gp.DoubleIntegratorOCP(gp.di_node(), batch=B, general_device=True)
    forced.deployConstraintsAndAddCost(); forced._compile_stage_model = lambda: (_ for _ in ()).throw(NotImplementedError("forced"))
    forced.genSolver()
    assert forced.generalPath_ and type(forced.OSQPSolverPtr_.ev).__name__ == "GeneralEvaluator"
    xa = stage.computeOptimalTrajectory(frame, ref); xb = forced.computeOptimalTrajectory(frame, ref)
    assert np.abs(xa - xb).max() < 1e-6


_WRONG_ABI = """
extern "C" {
int mpcqp_general_abi() { return 0x7fff; }
void mpcqp_general_dims(int *) {}
void mpcqp_general_tables(int *, int *, int *, int *, int *, int *, int *, int *) {}
int mpcqp_general_eval() { return 0; }
int mpcqp_general_merit() { return 0; }
}
"""


def test_errors_leave_the_handle_usable(built, tmp_path):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator, _bind
    L = _bind(_lib.lib())
    src = tmp_path / "wrong_abi.cpp"; so = tmp_path / "wrong_abi.so"
    src.write_text(_WRONG_ABI)
    subprocess.check_call(["g++", "-shared", "-fPIC", "-o", str(so), str(src)])
    h = C.c_void_p()
    assert L.mpcqp_nlp_create(str(so).encode(), -1, C.byref(h)) == _lib.ERR_ARG and not h.value          # another ABI number
    assert L.mpcqp_nlp_create(str(tmp_path / "missing.so").encode(), -1, C.byref(h)) == _lib.ERR_ARG and not h.value
    assert L.mpcqp_nlp_create(None, -1, C.byref(h)) == _lib.ERR_ARG
    pr = gp.problem("pendulum"); m = pr["model"]
    ev = GeneralEvaluator(m)
    B = 3
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=1)
    args = [_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)]
    good = ev.eval(*args)
    want = {k: v.clone() for k, v in good.items()}
    ptrs = [t.data_ptr() for t in args] + [good[k].data_ptr() for k in ("P", "q", "A", "l", "u")]
    assert L.mpcqp_nlp_eval(ev._h, 0, *ptrs, None) == _lib.ERR_ARG                                        # batch 0
    assert L.mpcqp_nlp_eval(ev._h, B, *ptrs[:6], None, *ptrs[7:], None) == _lib.ERR_ARG                   # a null output pointer
    assert L.mpcqp_nlp_eval(None, B, *ptrs, None) == _lib.ERR_ARG
    assert L.mpcqp_nlp_merit(ev._h, 0, ptrs[0], ptrs[1], ptrs[4], ptrs[5], None, None, None) == _lib.ERR_ARG
    assert L.mpcqp_nlp_step(ev._h, B, 1.0, None, ptrs[1], None, None, None) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="dimension mismatch"):
        ev.eval(args[0], args[1][:, :-1].contiguous(), *args[2:])
    again = ev.eval(*args)                                                                                # the handle is still usable
    for k in ("P", "q", "A", "l", "u"):
        assert torch.equal(again[k], want[k]), k
    ev.close()
