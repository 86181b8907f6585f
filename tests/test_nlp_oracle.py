"""Rows a1 / a2 / f1 against the oracle's restatement of the reference formulation (oracle/nlp_oracle.py: plain callables + central
differences, no code shared with the product): the host path's local system (models.StageOCP, general_nlp.GeneralNLP) on the CPU, the
device evaluator (mpcqp_stage_eval) under -m gpu.  The cost and the dynamics defects are written out here, stage by stage, from the
model's discrete map -- the formulation under test (w = [p; x], rows [p; x; g], shifted bounds, the 2Q Hessian of sum w e^2) is the
reference's src/sqp_solver/SQPOptimizationSolver.cpp:47-120.

This file covers the three zoo models with diagonal weights, one shared reference and dynamics rows only, by central differences in double at
1e-5.  Everything added since -- path and link rows, per-frame weights, bounds and references, lcost / lterm / llink, theta, stage data,
convexification, the line search, the hand-over, the general device path -- is held at 1e-12 against a 60-digit restatement in
tests/test_nlp_hp_host.py (the statement) and tests/test_gpu_nlp_hp.py (the kernels); see DESIGN 6.17."""
import numpy as np
import pytest

from optimal_control_problem_amd import models
from oracle import nlp_oracle

CASES = [("double_integrator", 5), ("quadrotor", 3), ("cartpole", 4)]


def _callables(mdl):
    nx, nu, N, f = mdl.nx, mdl.nu, mdl.N, mdl.f

    def cost(w):
        p, x = w[:nx], w[nx:].reshape(N, f)
        return float(sum(np.sum(mdl.Qk[k] * (x[k, :nx] - p) ** 2) + np.sum(mdl.Rk[k] * x[k, nx:] ** 2) for k in range(N)))

    def cons(w):
        x = w[nx:].reshape(N, f)
        return np.concatenate([x[k + 1, :nx] - np.asarray(mdl.F(x[k, :nx][None, :], x[k, nx:][None, :]))[0] for k in range(N - 1)])
    return cost, cons


def _dense(ls, b):
    Pd, Ad = ls.dense(b)
    return np.triu(Pd) + np.triu(Pd, 1).T, Ad


def _check(ls, b, ref, tol=1e-5):
    P, q, A, l, u = ref
    Pd, Ad = _dense(ls, b)
    for name, got, want in (("P", Pd, P), ("q", ls.q[b], q), ("A", Ad, A), ("l", ls.l[b], l), ("u", ls.u[b], u)):
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), name
        scale = 1.0 + np.abs(want[fin]).max()
        assert np.abs(got[fin] - want[fin]).max() <= tol * scale, (name, np.abs(got[fin] - want[fin]).max(), scale)


@pytest.mark.parametrize("name,N", CASES)
def test_host_local_system_equals_the_oracle_formulation(name, N):
    mdl, ls, meta = models.make_workload(name, 2, N=N)
    rng = np.random.default_rng(5)
    p = meta["p"] + rng.normal(0.0, 0.2, meta["p"].shape)
    ls = mdl.local_system(p, meta["x_iterate"], meta["lbx"], meta["ubx"], meta["lbg"], meta["ubg"])
    cost, cons = _callables(mdl)
    for b in range(2):
        _check(ls, b, nlp_oracle.local_system_dense(cost, cons, p[b], meta["x_iterate"][b], meta["lbx"][b], meta["ubx"][b], meta["lbg"][b], meta["ubg"][b]))


def test_general_nlp_equals_the_oracle_formulation():
    """the general path of the facade (general_nlp.GeneralNLP: tapes + complex step) on a small non-stage NLP with a parameter"""
    from optimal_control_problem_amd.general_nlp import GeneralNLP
    f = lambda w: (w[1] - w[0]) ** 2 + w[2] * w[2] + np.sin(w[1]) * w[3] + 0.5 * w[3] * w[3]
    g = lambda w: [w[1] * w[2] - 1.0, np.exp(w[3]) + w[0]]
    m = GeneralNLP(3, 1, f, g)
    rng = np.random.default_rng(1)
    p = rng.normal(size=(2, 1)); x = rng.normal(size=(2, 3))
    lbx = np.full((2, 3), -4.0); ubx = np.full((2, 3), 5.0); lbg = np.array([[0.0, -np.inf]] * 2); ubg = np.array([[0.0, 3.0]] * 2)
    ls = m.local_system(p, x, lbx, ubx, lbg, ubg)
    fo = lambda w: float(f(w)); go = lambda w: np.array([float(v) for v in g(w)])
    for b in range(2):
        _check(ls, b, nlp_oracle.local_system_dense(fo, go, p[b], x[b], lbx[b], ubx[b], lbg[b], ubg[b]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,N", CASES)
def test_device_evaluator_equals_the_oracle_formulation(built, name, N):
    import torch
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    B = 3
    mdl, ls0, meta = models.make_workload(name, B, N=N)
    rng = np.random.default_rng(7)
    p = meta["p"] + rng.normal(0.0, 0.2, meta["p"].shape)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    ev = StageEvaluator(mdl)
    out = ev.eval(dev(p), dev(meta["x_iterate"]), dev(meta["lbx"]), dev(meta["ubx"]), dev(meta["lbg"]), dev(meta["ubg"]))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ev.close()
    ls = models.LocalSystem(ls0.n, ls0.m, ls0.Pp, ls0.Pi, ls0.Ap, ls0.Ai, got["P"], got["q"], got["A"], got["l"], got["u"], mdl.np)
    cost, cons = _callables(mdl)
    for b in range(B):
        _check(ls, b, nlp_oracle.local_system_dense(cost, cons, p[b], meta["x_iterate"][b], meta["lbx"][b], meta["ubx"][b], meta["lbg"][b], meta["ubg"][b]))
