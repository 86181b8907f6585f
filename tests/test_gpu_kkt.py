"""GPU: the optimality-residual kernel (mpcqp_stage_kkt / mpcqp_nlp_kkt) against its NumPy statement kkt.kkt_residuals, the launch
properties (position, batch, frozen rows, repeatability), and options["kkt_tol"] of the device loop against the host loop and the C++ program.

The kernel adds the entries of a column in storage order with every product and sum rounded, as the statement does, so all four residuals and the
verdict are compared bit for bit; stat and scale are held to the rounding bar of tests/test_kkt_host.py on top (0 <= the bar)."""
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd.kkt import kkt_residuals
from tests.support import general_problems as gp
from tests.support import kkt_cases as kc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 3, 65, 257)
# double integrator N = 2: n - col0 = 6, m = 10 (the group of 16, n - col0 below it) and N = 3; cart-pole N = 20: n - col0 = 100, m = 180;
# quadrotor N = 20: n = 332, m = 560 (several columns and rows per lane, the group of 64)
SHAPES = [("double_integrator", 2), ("double_integrator", 3), ("cartpole", 20), ("quadrotor", 20)]
TOL = 1e-3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _launch(ev, d, tol, frozen=None, out=None):
    ls = {k: _dev(d[k]) for k in ("q", "A", "l", "u")}
    res, conv = ev.kkt(ls, _dev(d["y"]), tol, out=out, frozen=frozen)
    torch.cuda.synchronize()
    return res.cpu().numpy(), conv.cpu().numpy()


def _ref(mdl, d, tol):
    return kkt_residuals(mdl.Ap, mdl.Ai, d["q"], d["A"], d["l"], d["u"], d["y"], mdl.np, tol)


_SYSTEMS = {}


def system(name, N):
    """(model, evaluator, arrays of 257 instances, the statement's (res, converged) on them): computed once, shared, never changed"""
    key = (name, N)
    if key not in _SYSTEMS:
        from optimal_control_problem_amd.stage_eval import StageEvaluator
        mdl, ls, y = kc.zoo_system(name, N, max(BATCHES))
        y[::5] *= 1e-4                                    # every fifth instance with small multipliers ...
        d = dict(q=ls.q.copy(), A=ls.A, l=ls.l.copy(), u=ls.u.copy(), y=y)
        d["q"][::5] *= 1e-5; d["l"][::5] = np.minimum(d["l"][::5], 0.0); d["u"][::5] = np.maximum(d["u"][::5], 0.0)     # ... and feasible: some converge
        _SYSTEMS[key] = (mdl, StageEvaluator(mdl), d, _ref(mdl, d, TOL))
    return _SYSTEMS[key]


@pytest.mark.parametrize("name,N", SHAPES)
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_equals_the_statement(built, name, N, B):
    mdl, ev, d, (rres, rconv) = system(name, N)
    part = {k: v[:B] for k, v in d.items()}
    res, conv = _launch(ev, part, TOL)
    assert np.array_equal(bits(res[:, 1]), bits(rres[:B, 1])) and np.array_equal(bits(res[:, 2]), bits(rres[:B, 2]))
    assert np.array_equal(conv != 0, rconv[:B])
    # stat and scale: within the rounding bar 2 (k + 2) 2^-53 max_j sum |terms_j|; the same order of additions makes the difference 0
    bar = kc.rounding_bar(mdl.Ap, mdl.Ai, part["q"], part["A"], part["y"], mdl.np)
    print("%s N=%d B=%d: largest |stat - statement| %.3e, |scale - statement| %.3e, smallest bar %.3e" % (
        name, N, B, np.abs(res[:, 0] - rres[:B, 0]).max(), np.abs(res[:, 3] - rres[:B, 3]).max(), bar.min()))
    assert (np.abs(res[:, 0] - rres[:B, 0]) <= bar).all() and (np.abs(res[:, 3] - rres[:B, 3]) <= bar).all()
    assert np.array_equal(bits(res), bits(rres[:B]))
    if B == max(BATCHES):
        assert 0 < rconv.sum() < B                        # both verdicts occur


def test_width_32_equals_the_statement(built):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    mdl, ls, y = kc.zoo_system("double_integrator", 6, 5)      # n - col0 = 18, m = 30: the group of 32, which no shape above takes
    assert 16 < max(mdl.n - mdl.np, mdl.m) <= 32
    ev = StageEvaluator(mdl)
    d = dict(q=ls.q, A=ls.A, l=ls.l, u=ls.u, y=y)
    res, conv = _launch(ev, d, TOL)
    rres, rconv = _ref(mdl, d, TOL)
    assert np.array_equal(bits(res), bits(rres)) and np.array_equal(conv != 0, rconv)
    ev.close()


def test_branch_instances_at_the_first_last_and_a_middle_position(built):
    """the hand-built branches on the double integrator's pattern, every one of them at position 0, at the middle and at the last position of a
    batch of 257 (whose last block holds that one instance), between instances of the shared system: three branches per launch, one at each
    position, three rotations of every triple -- and all of them alone in order first"""
    mdl, ev, d, (sres, sconv) = system("double_integrator", 2)
    br, verdict = kc.branch_instances(mdl.Ap, mdl.Ai, mdl.n, mdl.m, mdl.np, kc.TOL)
    K, B = len(verdict), 257
    rres, rconv = _ref(mdl, br, kc.TOL)
    for want, got in zip(verdict, rconv):
        assert want is None or want == bool(got)
    res, conv = _launch(ev, br, kc.TOL)
    assert np.array_equal(bits(res), bits(rres)) and np.array_equal(conv != 0, rconv)
    _, fconv = _ref(mdl, {k: v[:B] for k, v in d.items()}, kc.TOL)      # the neighbours' verdicts at this tolerance
    fres = sres[:B]
    places = (0, B // 2, B - 1)
    checked = set()
    for first in range(0, K, 3):
        triple = [(first + t) % K for t in range(3)]
        for rot in range(3):
            at = {places[(t + rot) % 3]: k for t, k in enumerate(triple)}
            full = {key: d[key][:B].copy() for key in d}
            for where, k in at.items():
                for key in full:
                    full[key][where] = br[key][k]
            res, conv = _launch(ev, full, kc.TOL)
            for where, k in at.items():
                assert np.array_equal(bits(res[where]), bits(rres[k])) and bool(conv[where]) == bool(rconv[k]), (k, where)
                checked.add((k, where))
            rest = np.array([b for b in range(B) if b not in at])          # a branch next door changes no other instance
            assert np.array_equal(bits(res[rest]), bits(fres[rest])) and np.array_equal(conv[rest] != 0, fconv[rest])
    assert checked == {(k, where) for k in range(K) for where in places}   # K x 3 placements, every one compared


def test_position_and_batch_do_not_matter(built):
    """instance 0 of a batch-1 launch gives the bits it gives inside batch 257, at position 0 and at position 200"""
    for name, N in (("double_integrator", 2), ("quadrotor", 20)):
        mdl, ev, d, (rres, _) = system(name, N)
        one, c1 = _launch(ev, {k: v[:1] for k, v in d.items()}, TOL)
        big, cb = _launch(ev, d, TOL)
        moved = {k: np.roll(v, 200, axis=0) for k, v in d.items()}
        rolled, cr = _launch(ev, moved, TOL)
        assert np.array_equal(bits(one[0]), bits(big[0])) and c1[0] == cb[0]
        assert np.array_equal(bits(one[0]), bits(rolled[200])) and c1[0] == cr[200]


def test_frozen_rows_are_untouched_and_the_launch_repeats(built):
    mdl, ev, d, (rres, rconv) = system("cartpole", 20)
    B = 65
    part = {k: v[:B].copy() for k, v in d.items()}
    frozen = np.zeros(B, np.int32); frozen[[0, 7, 63, 64]] = [1, -1, 5, 1]
    part["y"][7] = np.nan                                 # a frozen instance is not read: its NaN stays out
    guard = 123.25
    out = (torch.full((B, 4), guard, dtype=torch.float64, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"))
    res, conv = _launch(ev, part, TOL, frozen=_dev(frozen, torch.int32), out=out)
    live = frozen == 0
    assert (res[~live] == guard).all() and (conv[~live] == 77).all()
    assert np.array_equal(bits(res[live]), bits(rres[:B][live])) and np.array_equal(conv[live] != 0, rconv[:B][live])
    again = (torch.full((B, 4), guard, dtype=torch.float64, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"))
    res2, conv2 = _launch(ev, part, TOL, frozen=_dev(frozen, torch.int32), out=again)
    assert np.array_equal(bits(res), bits(res2)) and np.array_equal(conv, conv2)
    # the verdicts as their own frozen mask, as the device loop launches it: converged rows keep their bits, the others are written again
    mask = torch.as_tensor(rconv[:B].astype(np.int32), device="cuda")
    keep = torch.full((B, 4), guard, dtype=torch.float64, device="cuda")
    res3, conv3 = _launch(ev, {k: v[:B] for k, v in d.items()}, TOL, frozen=mask, out=(keep, mask))
    assert (res3[rconv[:B]] == guard).all() and np.array_equal(conv3 != 0, rconv[:B])
    assert np.array_equal(bits(res3[~rconv[:B]]), bits(rres[:B][~rconv[:B]]))


def test_tolerance_dict_and_refusals(built):
    from optimal_control_problem_amd import _lib
    mdl, ev, d, _ = system("double_integrator", 3)
    part = {k: v[:3] for k, v in d.items()}
    tol = {"stat": 1e-1, "feas": 1e-6, "compl": 10.0}
    res, conv = _launch(ev, part, tol)
    rres, rconv = _ref(mdl, part, tol)
    assert np.array_equal(bits(res), bits(rres)) and np.array_equal(conv != 0, rconv)
    with pytest.raises(ValueError, match="dimension mismatch"):
        ev.kkt({k: _dev(part[k]) for k in ("q", "A", "l", "u")}, _dev(part["y"][:, :-1]), TOL)
    import ctypes as C
    from optimal_control_problem_amd.kkt import KktArgs
    a = KktArgs()
    assert _lib.lib().mpcqp_stage_kkt(ev._h, 3, C.byref(a), None) == _lib.ERR_ARG        # null pointers
    assert _lib.lib().mpcqp_stage_kkt(ev._h, 0, C.byref(a), None) == _lib.ERR_ARG
    assert _lib.lib().mpcqp_stage_kkt(None, 3, C.byref(a), None) == _lib.ERR_ARG


def test_general_evaluator(built):
    """mpcqp_nlp_kkt on a generated general problem without parameters (np = 0: every column counts)"""
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    pr = gp.problem("testcpp1")
    mdl = pr["model"]
    B = 65
    p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=4)
    ev = GeneralEvaluator(mdl)
    assert ev.np == 0
    ls = ev.eval(*[_dev(a) for a in (p, x, lbx, ubx, lbg, ubg)])
    y = np.random.default_rng(8).normal(0.0, 2.0, size=(B, mdl.m))
    y[::4] = 0.0
    res, conv = ev.kkt(ls, _dev(y), 3.0)
    host = {k: v.cpu().numpy() for k, v in ls.items()}
    rres, rconv = kkt_residuals(mdl.Ap, mdl.Ai, host["q"], host["A"], host["l"], host["u"], y, 0, 3.0)
    assert np.array_equal(bits(res.cpu().numpy()), bits(rres)) and np.array_equal(conv.cpu().numpy() != 0, rconv)
    assert 0 < rconv.sum() < B
    ev.close()


# ------------------------------------------------------------------------------------------------ the loops
@pytest.fixture(scope="module")
def device_recipe(built):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, arg = kc.recipe()
    dev = DeviceSQPOptimizationSolver(mdl, kc.recipe_options(), batch=kc.RECIPE_BATCH)
    out = dev.getOptimalSolution(arg)
    rep = dict(x=out["x"], converged=dev.converged.cpu().numpy(), converged_at=dev.converged_at.cpu().numpy(), iterations_done=dev.iterations_done,
               history=[h.cpu().numpy() for h in dev.kkt_history], now=dev.kkt(arg))
    dev.close()
    return mdl, arg, rep


def test_device_loop_equals_host_loop_on_the_recipe(device_recipe):
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    mdl, arg, rep = device_recipe
    host = SQPOptimizationSolver(mdl, kc.recipe_options(), batch=kc.RECIPE_BATCH)
    rh = host.getOptimalSolution(arg)
    assert np.array_equal(rep["converged_at"], host.converged_at) and rep["converged_at"].tolist() == [1, 1, 1, 2, 2, 2, 3, 6]
    assert rep["converged"].all() and host.converged.all()
    assert rep["iterations_done"] == host.iterations_done == 6 and len(rep["history"]) == len(host.kkt_history) == 6
    scale = 1.0 + np.abs(rh["x"]).max()
    assert np.abs(rep["x"] - rh["x"]).max() <= 1e-6 * scale          # the bar of tests/test_gpu_stage_eval.py test_device_sqp_equals_host_sqp
    # a frozen row of the history keeps its bits
    for b, at in enumerate(rep["converged_at"]):
        for h in rep["history"][at:]:
            assert np.array_equal(bits(h[b]), bits(rep["history"][at - 1][b]))
    assert bool(rep["now"]["converged"].all())
    host.qpSolver_.close()


def test_cpp_program_equals_the_python_loop(device_recipe):
    mdl, arg, rep = device_recipe
    exe = os.path.join(ROOT, "tests", "support", "stagesqp_kkt_test")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.splitlines() if ln.strip()}
    assert int(out["iterations_done"][0]) == rep["iterations_done"]
    assert [int(v) for v in out["converged_at"]] == rep["converged_at"].tolist()
    assert [int(v) for v in out["converged"]] == rep["converged"].astype(int).tolist()
    x = np.array([float(v) for v in out["x"]]).reshape(rep["x"].shape)
    assert np.array_equal(bits(x), bits(rep["x"]))                   # the same kernels in the same order
    res = np.array([float(v) for v in out["res"]]).reshape(-1, 4)
    assert np.array_equal(bits(res), bits(rep["history"][-1]))


def test_without_the_option_nothing_changes(built):
    """no kkt_tol: no check, no report, the fixed iteration count"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, arg = kc.recipe()
    dev = DeviceSQPOptimizationSolver(mdl, {"max_iter": 3, "alpha": 1.0}, batch=kc.RECIPE_BATCH)
    dev.getOptimalSolution(arg)
    assert dev.iterations_done == 3 and dev.kkt_history == [] and dev.converged is None and dev.kkt_tol is None
    now = dev.kkt(arg, 1.0)                               # the check on demand works without the option
    assert tuple(now["res"].shape) == (kc.RECIPE_BATCH, 4) and bool(torch.isfinite(now["res"]).all())
    dev.close()


def test_combinations(built):
    """kkt_tol next to line_search, warm_start_admm, keep_scaling, presolve_fixed_rows and sqp_tol: the loop converges on the recipe and stops early.
    (exact_hessian and convexify need a generated library: tests/test_kkt_host.py runs them through the host loop, whose lines the device loop shares)"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, arg = kc.recipe()
    for extra in ({"line_search": True, "warm_start_admm": True}, {"keep_scaling": True, "sqp_tol": 1e-12}, {"presolve_fixed_rows": True, "skip_failed_steps": True}):
        dev = DeviceSQPOptimizationSolver(mdl, kc.recipe_options(**extra), batch=kc.RECIPE_BATCH)
        dev.getOptimalSolution(arg)
        assert bool(dev.converged.all()) and dev.iterations_done == int(dev.converged_at.max()) < kc.RECIPE_MAX_ITER, extra
        assert bool(dev.kkt(arg)["converged"].all()), extra
        dev.close()


def test_constant_matrices_and_damping(built):
    """kkt_tol next to constant_matrices (the double integrator: P and A do not depend on the iterate, so every QP after the first replaces q, l, u
    on the kept workspace), damped with alpha = 0.5 so that the instances need several iterations: the device loop freezes every instance in the
    iteration in which the host loop (full set-ups) does.
    Every residual halves per iteration; on the CPU oracle the check of iteration 7 gives stat / max(1, scale) 0.0078 for everyone, feas 0.0023 ..
    0.0196 rising with the start position and compl 0.0078 .. 0.0195.  1.25e-2 lies at least 10 % away from every deciding figure (0.0113 | 0.0141
    in feas at iteration 7, 0.0099 in compl and 0.0098 in feas at iteration 8): converged_at = 7 7 7 7 7 8 8 8"""
    from optimal_control_problem_amd import models
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, SQPOptimizationSolver
    B = 8
    mdl = models.DoubleIntegrator(20, 0.05)
    frame0 = np.zeros((B, 3)); frame0[:, 0] = np.linspace(0.05, 2.5, B); frame0[:, 1] = 0.3
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    opt = {"max_iter": 30, "alpha": 0.5, "kkt_tol": 1.25e-2}
    host = SQPOptimizationSolver(mdl, opt, batch=B)
    dev = DeviceSQPOptimizationSolver(mdl, dict(opt, constant_matrices=True), batch=B)
    rh = host.getOptimalSolution(arg); rd = dev.getOptimalSolution(arg)
    at = dev.converged_at.cpu().numpy()
    print("converged_at", at, host.converged_at)
    assert bool(dev.converged.all()) and host.converged.all() and np.array_equal(at, host.converged_at)
    assert at.tolist() == [7, 7, 7, 7, 7, 8, 8, 8] and dev.iterations_done == host.iterations_done == 8
    # x is not held to the 1e-6 of the recipe's parity test: the host loop sets every QP up in full, the kept workspace runs other ADMM iterations
    # from another rho and scaling (include/mpcqp.h, mpcqp_update_vectors), and both end anywhere within the QPs' 1e-3.  Both points are first-order
    # points at the tolerance, which the check on demand confirms on the device loop's
    assert bool(dev.kkt(arg)["converged"].all()) and host.kkt(arg)["converged"].all()
    assert np.isfinite(rd["x"]).all() and np.isfinite(rh["x"]).all()
    host.qpSolver_.close(); dev.close()


def test_step_with_a_status_of_ones_is_the_step_without_one(built):
    """what the loop's mask relies on: mpcqp_stage_step with status = MPCQP_SOLVED for everyone moves x exactly as with no status, NaN steps included"""
    mdl, ev, d, _ = system("cartpole", 20)
    B = 65
    rng = np.random.default_rng(5)
    dw = rng.normal(size=(B, ev.n)); dw[3] = np.nan
    x0 = rng.normal(size=(B, ev.nvar))
    xa, xb = _dev(x0), _dev(x0)
    sa = ev.step(0.7, _dev(dw), xa)
    sb = ev.step(0.7, _dev(dw), xb, status=torch.ones(B, dtype=torch.int32, device="cuda"))
    assert np.array_equal(bits(xa.cpu().numpy()), bits(xb.cpu().numpy())) and np.array_equal(bits(sa.cpu().numpy()), bits(sb.cpu().numpy()))


def test_closed_loop_mpc_passes_the_option_through(built):
    """ClosedLoopMPC hands its options to the device loop: with kkt_tol and up to 6 iterations per tick, a tick of the (linear) double integrator
    solves one QP, finds every instance converged at the check of iteration 1 and applies what the tick of a fixed 6 iterations applies, to 1e-3"""
    from optimal_control_problem_amd import models
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    B = 8
    mdl = models.DoubleIntegrator(20, 0.05)
    frame0 = np.zeros((B, 3)); frame0[:, 0] = np.linspace(-1.0, 1.0, B); frame0[:, 1] = 0.2
    out = {}
    for key, extra in (("fixed", {}), ("kkt", {"kkt_tol": 1e-2})):
        mpc = ClosedLoopMPC(mdl, dict(extra, max_iter=6), batch=B)
        mpc.reset(frame0)
        done, applied = [], []
        for _ in range(3):
            r = mpc.tick()
            done.append(mpc.sol.iterations_done); applied.append(r["applied"].cpu().numpy().copy())
        out[key] = (done, np.stack(applied), mpc.sol)
    assert out["fixed"][0] == [6, 6, 6] and out["fixed"][2].kkt_tol is None
    sol = out["kkt"][2]
    assert out["kkt"][0] == [1, 1, 1] and bool(sol.converged.all()) and bool((sol.converged_at == 1).all()) and len(sol.kkt_history) == 1
    # (every QP ends within its termination tolerance 1e-3 (1 + max|x|), max|x| about 2, of its optimum, and the two loops differ by such QPs over three ticks)
    assert np.abs(out["kkt"][1] - out["fixed"][1]).max() < 1e-2
    sol.close(); out["fixed"][2].close()
