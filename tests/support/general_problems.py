"""Problems for the general (non-stage) device evaluator: GeneralNLP models with evaluation points and bounds.

(a) the seven NLPs of the reference's test/test.cpp as models.reference_test_cases() states them, over a two-frame decision vector
    whose frame 0 appears nowhere (the facade pins it, reference src/OptimalControlProblem.cpp:93-96): np = 0 in six of them, ng = 0 in
    three, variables without any derivative in all;
(b) the skip-coupled double integrator of tests/test_ocp_facade.py (n = 32, ng = 26): linear, a constraint between frames k and k + 2;
(c) a pendulum with sin / cos dynamics, horizon 6: a different cost function on every frame (exp, a quotient, sqrt, integer powers, log,
    tan, tanh), a term over all inputs, a constraint coupling frames k and k + 2, two parameters -- every operation the tracer knows;
(d) a cost-only problem (constraints=None, ng = 0) with a parameter and a variable that appears nowhere."""
import functools

import numpy as np
import yaml

from optimal_control_problem_amd import models
from optimal_control_problem_amd.general_nlp import GeneralNLP
from optimal_control_problem_amd.ocp import Dynamics, General, OptimalControlProblem

INF = float("inf")
_TESTCPP_COST_CENTRES = {0: [0, 0], 1: [3, -2], 2: [2, 3], 3: [0, 0], 4: [1, 2, 3], 6: [3, 4]}


def _testcpp(idx):
    mdl, arg, expect = models.reference_test_cases()[idx]
    nx, npar = mdl.nx, mdl.np

    def cost(w):
        X = w[npar:]
        if idx == 5:
            return (X[nx] - w[0]) ** 2 + X[nx + 1] ** 2
        c = _TESTCPP_COST_CENTRES[idx]
        return sum((X[nx + i] - float(c[i])) ** 2 for i in range(nx))

    cons = None
    if idx in (0, 2):
        cons = lambda w: [w[npar + nx] + w[npar + nx + 1] - 1.0]
    elif idx == 3:
        cons = lambda w: [w[npar + nx], w[npar + nx + 1]]
    elif idx == 4:
        cons = lambda w: [w[npar + nx] + w[npar + nx + 1] + w[npar + nx + 2] - 5.0]
    model = GeneralNLP(2 * nx, npar, cost, cons)
    lbx = np.concatenate([np.zeros(nx), np.asarray(arg["lbx"], float)]); ubx = np.concatenate([np.zeros(nx), np.asarray(arg["ubx"], float)])
    return dict(name="testcpp%d" % (idx + 1), model=model, lbx=lbx, ubx=ubx, lbg=np.asarray(arg["lbg"], float), ubg=np.asarray(arg["ubg"], float),
                p0=np.asarray(arg["p"], float), scale=1.0)


def _skip_coupled():
    N, h, d = 10, 0.05, 0.05

    def cost(w):
        p, X = w[:2], w[2:]
        f = 0.0
        for k in range(N):
            s = X[3 * k:3 * k + 2] - p
            f = f + 10.0 * (s[0] * s[0]) + 1.0 * (s[1] * s[1]) + 0.1 * (X[3 * k + 2] * X[3 * k + 2])
        return f

    def cons(w):
        X = w[2:]
        out = []
        for k in range(N - 1):
            s, u, sn = X[3 * k:3 * k + 2], X[3 * k + 2], X[3 * k + 3:3 * k + 5]
            out += [sn[0] - (s[0] + h * s[1] + 0.5 * h * h * u), sn[1] - (s[1] + h * u)]
        for k in range(N - 2):
            out.append(X[3 * (k + 2) + 2] - X[3 * k + 2])
        return out

    model = GeneralNLP(3 * N, 2, cost, cons)
    lbx = np.tile([-INF, -2.0, -1.0], N); ubx = np.tile([INF, 2.0, 1.0], N)
    lbg = np.concatenate([np.zeros(2 * (N - 1)), -d * np.ones(N - 2)]); ubg = np.concatenate([np.zeros(2 * (N - 1)), d * np.ones(N - 2)])
    return dict(name="skip_coupled", model=model, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p0=np.zeros(2), scale=0.5, cost=cost, constraints=cons)


PENDULUM_N = 6


def pendulum_cost(w, N=PENDULUM_N):
    """p = [target angle, damping]; frame k = [theta, omega, u].  The first six frames carry six different functions; longer horizons
    (the measurement tool) repeat them"""
    p, X = w[:2], w[2:]
    f = 0.0
    usum = 0.0
    for k in range(N):
        th, om, u = X[3 * k], X[3 * k + 1], X[3 * k + 2]
        e = th - p[0]
        kind = k % 6
        if kind == 0:
            f = f + e ** 2 + 0.1 * u ** 2 + 0.5 * om ** 2
        elif kind == 1:
            f = f + np.exp(0.3 * e) - 0.3 * e + om * om + 0.1 * u ** 2
        elif kind == 2:
            f = f + 2.0 * e ** 2 / (1.0 + 0.1 * om ** 2) + om ** 2 + 0.1 * u * u
        elif kind == 3:
            f = f + 3.0 * np.sqrt(1.0 + e ** 2 + om ** 2) + 0.1 * np.square(u)
        elif kind == 4:
            f = f + e ** 4 + e ** 2 + 0.01 * om ** 3 + om ** 2 + 0.1 * u ** 2 + 0.05 * np.log(1.0 + u * u)
        else:
            f = f + 5.0 * e ** 2 + om ** 2 + 0.01 * np.tan(0.2 * u) ** 2 + 0.1 * np.tanh(om) ** 2 + 0.1 * (-u) * (-u) + 1.0 / (2.0 + e ** 2)
        usum = usum + u
    return f + 0.01 * usum ** 2 + 0.02 * (p[1] * p[1])


def pendulum_constraints(w, N=PENDULUM_N, h=0.1):
    p, X = w[:2], w[2:]
    out = []
    for k in range(N - 1):
        th, om, u = X[3 * k], X[3 * k + 1], X[3 * k + 2]
        out += [X[3 * k + 3] - (th + h * om), X[3 * k + 4] - (om + h * (-9.81 * np.sin(th) - p[1] * om + u * np.cos(th)))]
    for k in range(N - 2):                                    # frames k and k + 2: a slew limit on the input, tightened by the swing between them
        out.append(X[3 * (k + 2) + 2] - X[3 * k + 2] + 0.05 * np.negative(X[3 * (k + 1) + 1]) * X[3 * k + 2])
    return out


def pendulum(N=PENDULUM_N):
    model = GeneralNLP(3 * N, 2, lambda w: pendulum_cost(w, N), lambda w: pendulum_constraints(w, N))
    lbx = np.tile([-INF, -8.0, -3.0], N); ubx = np.tile([INF, 8.0, 3.0], N)
    lbg = np.concatenate([np.zeros(2 * (N - 1)), -0.5 * np.ones(N - 2)]); ubg = np.concatenate([np.zeros(2 * (N - 1)), np.full(N - 2, INF)])
    return dict(name="pendulum", model=model, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p0=np.array([0.4, 0.3]), scale=0.3)


def _cost_only():
    def cost(w):
        p, x = w[0], w[1:]
        return (x[0] - p) ** 2 + 100.0 * (x[1] - x[0] ** 2) ** 2 + np.exp(0.5 * x[2]) * np.cos(x[3]) + x[2] ** 2 + x[3] ** 2      # x[4] appears nowhere

    model = GeneralNLP(5, 1, cost, None)
    return dict(name="cost_only", model=model, lbx=-2.0 * np.ones(5), ubx=np.array([2.0, 2.0, INF, 2.0, 2.0]), lbg=np.zeros(0), ubg=np.zeros(0),
                p0=np.array([1.0]), scale=0.5)


@functools.lru_cache(maxsize=None)
def problems():
    """[(a) x 7, (b), (c), (d)] as dicts: name, model, lbx, ubx, lbg, ubg (one instance), p0, scale"""
    return [_testcpp(i) for i in range(7)] + [_skip_coupled(), pendulum(), _cost_only()]


def problem(name):
    return next(pr for pr in problems() if pr["name"] == name)


NAMES = ["testcpp%d" % (i + 1) for i in range(7)] + ["skip_coupled", "pendulum", "cost_only"]


def point(pr, B, seed=0):
    """a batch of evaluation points: p, x, lbx, ubx, lbg, ubg as [B, .] arrays (bounds tiled; instance 0 of a problem with general rows gets
    one loose row -inf / +inf)"""
    m = pr["model"]
    rng = np.random.default_rng(seed)
    p = np.tile(pr["p0"], (B, 1)) + rng.normal(0.0, 0.1, (B, m.np))
    x = rng.normal(0.0, pr["scale"], (B, m.nvar))
    t = lambda a: np.tile(np.asarray(a, float), (B, 1))
    lbg, ubg = t(pr["lbg"]), t(pr["ubg"])
    if m.ng:
        lbg[0, m.ng - 1] = -INF; ubg[0, m.ng - 1] = INF
    return p, x, t(pr["lbx"]), t(pr["ubx"]), lbg, ubg


# ---------------------------------------------------------------------------------------------------- checkers
def close(a, b, tol):
    """elementwise |a - b| <= tol * max(1, |b|), with infinities required to match exactly (tests/test_gpu_stage_eval.py)"""
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin])
    return (np.abs(a[fin] - b[fin]) <= tol * np.maximum(1.0, np.abs(b[fin]))).all()


def host_eval(model, p, x, lbx, ubx, lbg, ubg):
    """the generated functor's g++ build over a batch: dict P, q, A, l, u, f, gmax (outputs start as NaN: every element must be written)"""
    import ctypes as C
    from optimal_control_problem_amd import codegen as _codegen
    L = C.CDLL(_codegen.build_general_host_library(model))
    d = np.zeros(9, np.int32); L.general_host_dims(C.c_void_p(d.ctypes.data))
    assert [int(v) for v in d[:7]] == [model.nvar, model.np, model.ng, model.n, model.m, len(model.Pi), len(model.Ai)]
    tabs = [np.zeros(k, np.int32) for k in (model.n + 1, len(model.Pi), model.n + 1, len(model.Ai))]
    L.general_host_tables(*[C.c_void_p(t.ctypes.data) for t in tabs], None, None, None, None)
    for got, want in zip(tabs, (model.Pp, model.Pi, model.Ap, model.Ai)):
        assert np.array_equal(got, want)                                                    # the patterns match exactly
    B = x.shape[0]
    out = dict(P=np.full((B, len(model.Pi)), np.nan), q=np.full((B, model.n), np.nan), A=np.full((B, len(model.Ai)), np.nan),
               l=np.full((B, model.m), np.nan), u=np.full((B, model.m), np.nan), f=np.full(B, np.nan), gmax=np.full(B, np.nan))
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    for b in range(B):
        w = np.ascontiguousarray(np.concatenate([p[b], x[b]]))
        ins = [np.ascontiguousarray(a[b]) for a in (lbx, ubx, lbg, ubg)]
        outs = [np.zeros_like(out[k][b]) + np.nan for k in ("P", "q", "A", "l", "u")]
        L.general_host_eval(ptr(w), *[ptr(a) for a in ins], *[ptr(a) for a in outs])
        for k, a in zip(("P", "q", "A", "l", "u"), outs):
            out[k][b] = a
        f = np.zeros(1); g = np.zeros(1)
        L.general_host_merit(ptr(w), ptr(ins[2]), ptr(ins[3]), ptr(f), ptr(g))
        out["f"][b] = f[0]; out["gmax"][b] = g[0]
    return out


def violation(model, p, x, lbg, ubg):
    """max-norm violation of lbg <= g(p, x) <= ubg per instance (0 when feasible or without general rows)"""
    g = model.constraints(p, x)
    v = np.maximum(lbg - g, g - ubg)
    return np.maximum(v.max(axis=1), 0.0) if model.ng else np.zeros(x.shape[0])


# ---------------------------------------------------------------------------------------------------- through the facade
TESTCPP_YAML = """
optimal_control_problem:
  discretization_settings: {dt: 0.1, horizon: 2}
  solver_settings:
    verbose: false
    gen_code: false
    load_lib: false
    max_iter: 1000
    warm_start: true
    solve_method: CUDA_SQP
    SQP_settings: {alpha: 1.0, step_num: %d}
  OCP_variables:
    - name: "x"
      size: %d
      lower_bound: %s
      upper_bound: %s
"""


def _fmt(b):
    return "[" + ", ".join(".inf" if v == np.inf else "-.inf" if v == -np.inf else repr(float(v)) for v in b) + "]"


def testcpp_through_builders(idx, general_device, batch=1, qp_solver=None, step_num=10):
    """tests/test_ocp_facade.py states the seven NLPs through the OptimalControlProblem builders; the same here with the general_device switch.
    Returns (the facade object, solution of frame 1, expected)"""
    mdl, arg, expect = models.reference_test_cases()[idx]
    nx, npar = mdl.nx, mdl.np

    class Problem(OptimalControlProblem):
        def deployConstraintsAndAddCost(self):
            self.setReference(max(npar, 1))
            if idx == 5:
                self.addScalarCost(General(lambda X, p: (X[nx] - p[0]) ** 2 + X[nx + 1] ** 2))
            else:
                c = _TESTCPP_COST_CENTRES[idx]
                self.addScalarCost(General(lambda X, p: sum((X[nx + i] - float(c[i])) ** 2 for i in range(nx))))
            lbg, ubg = np.asarray(arg["lbg"], float), np.asarray(arg["ubg"], float)
            if idx in (0, 2):
                self.addInequalityConstraint("sum", lbg, General(lambda X, p: [X[nx] + X[nx + 1] - 1.0], 1), ubg)
            elif idx == 3:
                self.addInequalityConstraint("each", lbg, General(lambda X, p: [X[nx], X[nx + 1]], 2), ubg)
            elif idx == 4:
                self.addInequalityConstraint("sum", lbg, General(lambda X, p: [X[nx] + X[nx + 1] + X[nx + 2] - 5.0], 1), ubg)
            else:
                self.addInequalityConstraint("none", [-np.inf], General(lambda X, p: [X[nx]], 1), [np.inf])

    node = yaml.safe_load(TESTCPP_YAML % (step_num, nx, _fmt(arg["lbx"]), _fmt(arg["ubx"])))["optimal_control_problem"]
    ocp = Problem(node, batch=batch, qp_solver=qp_solver, general_device=general_device)
    ocp.deployConstraintsAndAddCost(); ocp.genSolver()
    p = np.asarray(arg["p"], float) if npar else np.zeros(1)
    x = ocp.computeOptimalTrajectory(np.zeros((batch, nx)), np.tile(p, (batch, 1)))
    return ocp, x[:, nx:], np.asarray(expect, float)


DI_YAML = """
optimal_control_problem:
  discretization_settings: {dt: 0.05, horizon: 10}
  solver_settings:
    verbose: false
    gen_code: false
    load_lib: false
    max_iter: 1000
    warm_start: true
    solve_method: CUDA_SQP
    SQP_settings: {alpha: 1.0, step_num: 2}
  OCP_variables:
    - {name: "state", size: 2, lower_bound: [-.inf, -2.0], upper_bound: [.inf, 2.0]}
    - {name: "input", size: 1, lower_bound: [-1.0], upper_bound: [1.0]}
"""


class DoubleIntegratorOCP(OptimalControlProblem):
    def deployConstraintsAndAddCost(self):
        cfg = self.OCPConfigPtr_
        h = cfg.getDt()

        def F(s, u):
            return np.stack([s[..., 0] + h * s[..., 1] + 0.5 * h * h * u[..., 0], s[..., 1] + h * u[..., 0]], axis=-1)

        ref = self.setReference(2)
        for k in range(cfg.getHorizon()):
            self.addVectorCost([10.0, 1.0], cfg.getVariable(k, "state") - ref)
            self.addVectorCost([0.1], cfg.getVariable(k, "input"))
        for k in range(cfg.getHorizon() - 1):
            self.addEquationConstraint("dynamics", cfg.getVariable(k + 1, "state"), Dynamics(F, cfg.getVariable(k, "state"), cfg.getVariable(k, "input")))


class SkipCoupledOCP(DoubleIntegratorOCP):
    d = 0.05

    def deployConstraintsAndAddCost(self):
        super().deployConstraintsAndAddCost()
        cfg = self.OCPConfigPtr_
        for k in range(cfg.getHorizon() - 2):
            self.addInequalityConstraint("skip", [-self.d], cfg.getVariable(k + 2, "input") - cfg.getVariable(k, "input"), [self.d])


def di_node():
    return yaml.safe_load(DI_YAML)["optimal_control_problem"]
