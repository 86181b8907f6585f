"""GPU: per-frame references on the device (mpcqp_stage_create_tracking, the PF = true instances of csrc/stage_kernels.hpp) against the NumPy
statement (models.StageOCP with per_frame_reference), and the device-resident SQP loop -- full-form handle and presolved handle -- against the
host loop over the CPU oracle.

Tolerances are those of tests/test_gpu_stage_eval.py: 1e-12 relative to max(1, |ref|) (forward-mode duals on the device, complex step on the
host, same operation order, different libm), gmax 1e-11; identity entries exactly 1.0, parameter rows l = u = 0 exactly.  A traced stage cost
and per-frame diagonal weights exclude each other (mpcqp_stage_set_weights refuses a handle with its own cost), so the generated library comes in
two kinds: traced cost + terminal cost + path constraint, and diagonal per-frame weights + path constraint + link constraint."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems
from tests.support.oracle_backend import OracleCuCaQP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOO = {"double_integrator": models.DoubleIntegrator, "quadrotor": models.Quadrotor, "cartpole": models.CartPole}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _close(a, b, tol):
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin])
    return (np.abs(a[fin] - b[fin]) <= tol * np.maximum(1.0, np.abs(b[fin]))).all()


def tracking(cls):
    return type("Tracking" + cls.__name__, (cls,), {"per_frame_reference": True})


def _lcost(s, u, r):
    e = s - r
    return 3.0 * e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + 0.5 * e[..., 0] * e[..., 1] + 0.2 * u[..., 0] * u[..., 0] + 0.1 * np.cos(s[..., 1]) * u[..., 0] * u[..., 0] \
        + 0.05 * np.sin(r[..., 0]) * u[..., 0]


def _lterm(s, u, r):
    e = s - r
    return 20.0 * e[..., 0] * e[..., 0] + 4.0 * e[..., 1] * e[..., 1] + 0.3 * u[..., 0] * u[..., 0] + np.exp(0.1 * e[..., 0] * e[..., 1])


class Pendulum(models.StageOCP):
    nx = 2; nu = 1; name = "tracking_pendulum"
    nh = 1; h_lo = [-1.5]; h_hi = [1.5]

    def __init__(self, N, dt=0.05, Q=(4.0, 1.0), R=(0.3,)):
        super().__init__(N, dt, Q, R)

    def F(self, s, u):
        h = self.dt
        return np.stack([s[..., 0] + h * s[..., 1], s[..., 1] + h * (u[..., 0] - np.sin(s[..., 0]))], axis=-1)

    def hfun(self, s, u):
        return np.stack([s[..., 1] + 0.5 * u[..., 0]], axis=-1)

    def frame_bounds(self):
        return np.array([-3.0, -4.0, -2.0]), np.array([3.0, 4.0, 2.0])


class CostPendulum(Pendulum):
    """traced stage cost + terminal cost + path constraint"""
    per_frame_reference = True
    lcost = staticmethod(_lcost); lterm = staticmethod(_lterm)


class WeightedPendulum(Pendulum):
    """diagonal per-frame weights + path constraint + link constraint (rate limit on the input)"""
    per_frame_reference = True
    nk = 1; k_lo = [-0.4]; k_hi = [0.4]

    def __init__(self, N, dt=0.05):
        ramp = np.linspace(1.0, 3.0, N)[:, None]
        super().__init__(N, dt, ramp * np.array([4.0, 1.0]), 0.3 * ramp)

    def kfun(self, s, u, sn, un):
        return np.stack([un[..., 0] - u[..., 0]], axis=-1)


def _point(m, B, seed=3):
    """iterate, references and bounds of B instances: first frame pinned, every instance its own Jacobians"""
    rng = np.random.default_rng(seed)
    if m.name in ZOO:
        _, _, meta = models.make_workload(m.name, B, N=m.N)
        x = meta["x_iterate"]; frame0 = meta["frame0"]
    else:
        x = rng.normal(0.0, 0.4, size=(B, m.nvar)); frame0 = x[:, :m.f].copy()
    lbx, ubx, lbg, ubg = m.stacked_bounds(frame0)
    s, _ = m.frames(x)
    p = (s + rng.normal(0.0, 0.3, size=s.shape)).reshape(B, -1)          # a different reference state on every frame
    return p, x, lbx, ubx, lbg, ubg


def _check_eval(m, B, codegen=None):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    ev = StageEvaluator(m, codegen=codegen)
    args = _point(m, B)
    ref = m.local_system(*args)
    assert (ev.np, ev.n, ev.m, ev.nnzP, ev.nnzA) == (m.N * m.nx, ref.n, ref.m, len(ref.Pi), len(ref.Ai))
    assert (ev.Pp == ref.Pp).all() and (ev.Pi == ref.Pi).all() and (ev.Ap == ref.Ap).all() and (ev.Ai == ref.Ai).all()
    dargs = [_dev(a) for a in args]
    out = ev.eval(*dargs)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("P", "q", "A", "l", "u"):
        assert _close(got[k], getattr(ref, k), 1e-12), k
    if not m.general_cost:
        assert np.array_equal(got["P"], ref.P)                           # constants: 2 Q_k, -2 Q_k, 2 R_k
    assert np.array_equal(got["A"][:, m._A_id], np.ones((B, m.n)))       # identity entries are exactly 1.0
    assert np.array_equal(got["A"][:, m._A_next[1:].ravel()], np.ones((B, (m.N - 1) * m.nx)))
    assert not got["l"][:, :m.np].any() and not got["u"][:, :m.np].any() and not np.signbit(got["l"][:, :m.np]).any()      # p rows: l = u = 0 exactly
    f, g = ev.merit(dargs[0], dargs[1])
    assert _close(f.cpu().numpy(), m.objective(args[0], args[1]), 1e-12)
    viol = np.abs(m.constraints(args[1])).max(axis=1)
    if m.nh:
        lo, hi = m.path_bounds(); hv = m.path_values(args[1]).reshape(B, m.N, m.nh)
        viol = np.maximum(viol, np.maximum(lo - hv, hv - hi).reshape(B, -1).max(axis=1))
    if m.nk:
        lo, hi = m.link_bounds(); kv = m.link_values(args[1]).reshape(B, m.N - 1, m.nk)
        viol = np.maximum(viol, np.maximum(lo - kv, kv - hi).reshape(B, -1).max(axis=1))
    assert _close(g.cpu().numpy(), viol, 1e-11)
    # the same input twice: the same bits (one writer per element, no atomics)
    again = ev.eval(*dargs)
    for k in ("P", "q", "A", "l", "u"):
        assert torch.equal(out[k], again[k]), k
    f2, g2 = ev.merit(dargs[0], dargs[1])
    assert torch.equal(f, f2) and torch.equal(g, g2)
    # the damped update skips the larger parameter block
    rng = np.random.default_rng(1)
    dw = rng.normal(size=(B, m.n)); x = _dev(args[1])
    ev.step(0.5, _dev(dw), x)
    assert np.array_equal(x.cpu().numpy(), args[1] + 0.5 * dw[:, m.np:])
    ev.close()


@pytest.mark.parametrize("name,N,B", [("double_integrator", 2, 1), ("double_integrator", 20, 67),
                                      ("quadrotor", 3, 5),            # cooperative mapping: 48 + 48 threads per instance straddle a wave and a 256-thread block
                                      ("quadrotor", 20, 17),
                                      ("cartpole", 13, 9)])           # f = 5: one thread per column, n = 117
def test_zoo_eval_and_merit_match_the_numpy_statement(built, name, N, B):
    _check_eval(tracking(ZOO[name])(N), B)


@pytest.mark.parametrize("N", [3, 6])
@pytest.mark.parametrize("cls", [CostPendulum, WeightedPendulum])
def test_generated_library_eval_and_merit(built, cls, N):
    _check_eval(cls(N), 7)


def test_zoo_tracking_with_per_frame_weights(built):
    class M(tracking(models.CartPole)):
        def __init__(self, N):
            ramp = np.linspace(1.0, 2.0, N)[:, None]
            models.StageOCP.__init__(self, N, 0.02, ramp * np.array([1.0, 10.0, 0.1, 0.1]), 0.01 * ramp)
    _check_eval(M(6), 4)


@functools.lru_cache(maxsize=None)
def _libraries():
    from optimal_control_problem_amd import codegen as cg
    m = Pendulum(4)
    mk = lambda flag: cg.build_device_library(cg.trace(m.F, m.nx, m.nu, m.hfun, m.nh, m.h_lo, m.h_hi, per_frame_reference=flag))
    return mk(False), mk(True)


def test_entry_points_refuse_the_wrong_kind_of_library(built):
    from optimal_control_problem_amd import _lib
    from optimal_control_problem_amd.stage_eval import StageDesc, _bind
    L = _bind(_lib.lib())
    plain, pref = _libraries()
    assert plain != pref
    d = StageDesc()
    assert L.mpcqp_stage_default(0, 4, C.byref(d)) == 0
    d.dt = 0.05; d.device = -1
    for entry, lib, want in ((L.mpcqp_stage_create_user, plain, _lib.OK), (L.mpcqp_stage_create_user, pref, _lib.ERR_ARG),
                             (L.mpcqp_stage_create_tracking, pref, _lib.OK), (L.mpcqp_stage_create_tracking, plain, _lib.ERR_ARG)):
        h = C.c_void_p()
        assert entry(C.byref(d), lib.encode(), C.byref(h)) == want
        assert bool(h.value) == (want == _lib.OK)
        if h.value:
            dims = np.zeros(8, np.int32)
            assert L.mpcqp_stage_dims(h, dims.ctypes.data) == 0 and dims[2] == (8 if entry is L.mpcqp_stage_create_tracking else 2)
            L.mpcqp_stage_destroy(h)


class ReducedOracleCuCaQP(OracleCuCaQP):
    """the oracle on the presolved QP: the rows named are eliminated as mpcqp_create_presolved does (tests/support/problems.reduce_qp), the oracle
    solves what remains, x comes back in the caller's dimensions"""

    def __init__(self, rows, **kw):
        super().__init__(**kw)
        self.rows = list(rows)

    def solve(self):
        full = self.ls
        red, free, kept, fvars, xfix = problems.reduce_qp(full, self.rows)
        self.ls = red
        super().solve()
        self.ls = full
        x = np.zeros((full.batch, full.n)); x[:, free] = self.res["x"]; x[:, fvars] = xfix
        self.res = dict(self.res, x=x)
        return True


def _figure_eight(m, B, tick):
    t = (tick + np.arange(m.N)) * m.dt
    ph = np.linspace(0.0, 1.0, B)[:, None]
    r = np.zeros((B, m.N, 12))
    r[..., 0] = 0.5 * np.sin(1.5 * t + ph); r[..., 1] = 0.25 * np.sin(3.0 * t + ph); r[..., 2] = 0.2
    return r.reshape(B, -1)


@pytest.mark.parametrize("presolve", [False, True])
def test_device_loop_equals_the_host_loop_over_the_oracle(built, presolve):
    """quadrotor N = 10, B = 8, 3 SQP iterations, alpha 0.5, the reference moving from one call to the next.  presolve: the handle comes from
    mpcqp_create_presolved (the N nx parameter rows and the pinned first frame found and eliminated) and lands on an on-chip kernel family; its
    yardstick is the host loop with the oracle on the same reduced QP, compared on the free variables."""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, SQPOptimizationSolver
    B = 8
    m = tracking(models.Quadrotor)(10)
    p, x0, lbx, ubx, lbg, ubg = _point(m, B)
    opt = {"max_iter": 3, "alpha": 0.5, "presolve_fixed_rows": presolve}
    fixed = list(range(m.np + m.f))
    host = SQPOptimizationSolver(m, opt, batch=B, qp_solver=ReducedOracleCuCaQP(fixed, batch=B, nthreads=8) if presolve else OracleCuCaQP(batch=B, nthreads=8))
    dev = DeviceSQPOptimizationSolver(m, opt, batch=B)
    assert (dev.qp is None) == presolve                              # the presolved handle is created from the first system's bounds
    host.setInitialGuess(x0); dev.setInitialGuess(x0)
    for tick in range(2):
        arg = dict(lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=_figure_eight(m, B, tick))
        rh = host.getOptimalSolution(arg); rd = dev.getOptimalSolution(arg)
        assert np.isfinite(rd["x"]).all()
        free = slice(m.f, None) if presolve else slice(None)
        err = np.abs(rd["x"][:, free] - rh["x"][:, free]).max(); scale = 1.0 + np.abs(rh["x"]).max()
        print("presolve %s tick %d: max|x_dev - x_host| %.3e (bar %.3e)" % (presolve, tick, err, 1e-6 * scale))
        assert err <= 1e-6 * scale
        assert _close(rd["f"], rh["f"], 1e-6)
    info = dev.qp.plan_info()
    print("presolve %s: variant %d, n %d, nfixed %d" % (presolve, info["variant"], info["n"], dev.qp.nfixed))
    if presolve:
        assert dev.qp.nfixed == m.np + m.f and info["variant"] >= 200
        assert np.array_equal(rd["x"][:, :m.f], x0[:, :m.f])         # the pinned frame never moves
    else:
        assert dev.qp.nfixed == 0
    dev.close()


def test_presolved_loop_forwards_warm_start_and_kept_scaling(built):
    """warm start, carried rho and keep_scaling through the reduced handle: the loop runs, stays finite and ends where the cold loop ends (within the
    QP tolerance: a different ADMM run on the same QPs)"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B = 4
    m = tracking(models.Quadrotor)(10)
    p, x0, lbx, ubx, lbg, ubg = _point(m, B)
    arg = dict(lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=_figure_eight(m, B, 0))
    out = []
    for extra in ({}, {"warm_start_admm": True, "carry_rho": True, "keep_scaling": True}):
        dev = DeviceSQPOptimizationSolver(m, dict({"max_iter": 4, "alpha": 0.5, "presolve_fixed_rows": True}, **extra), batch=B)
        dev.setInitialGuess(x0)
        out.append(dev.getOptimalSolution(arg)["x"])
        assert np.isfinite(out[-1]).all() and (dev.status.cpu().numpy() == 1).all()
        dev.close()
    assert np.abs(out[0] - out[1]).max() <= 2e-2 * (1.0 + np.abs(out[0]).max())


def test_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "tracking_mpc.py"), "16", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "tracking stage pattern True, np = 240" in r.stdout and "position error" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
