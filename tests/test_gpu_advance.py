"""GPU: the hand-over between two MPC ticks (mpcqp_stage_advance, csrc/stage_kernels.hpp stage_advance_kernel) against its NumPy statement
(models.StageOCP.advance), its refusals, the closed loop built on it (mpc.ClosedLoopMPC) and a plain C client.

Tolerances: whatever is a copy, a zero or the pin is compared bit for bit; what passes through F (the new state, the rollout tail) and the stage
cost to 1e-12 max(1, |ref|) -- the bound tests/test_gpu_stage_eval.py applies to values that pass through F and to the merit: same operation
order, different libm."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from tests.support import advance_cases as ac

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-12
OK = (1, 2, 7)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _close(a, b):
    return bool((np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))).all())


def _model(kind, N):
    if kind == "double_integrator":
        return models.DoubleIntegrator(N, 0.05)
    if kind == "quadrotor":
        return models.Quadrotor(N, 0.02)
    if kind == "cartpole":
        return models.CartPole(N, 0.02)
    if kind == "generated_rows":
        return ac.pendulum_rows(N)
    return ac.TrackingIntegrator(N, 0.05)


def _trajectory(mdl, B, rng):
    X = rng.normal(0.0, 0.3, size=(B, mdl.N, mdl.f))
    if mdl.name == "quadrotor":
        X[:, :, mdl.nx:] += mdl.hover_thrust
    return X.reshape(B, -1)


# (kind, N, B, r_new): N = 2 is the smallest horizon; N = 70 > 64 frames, so the lanes stride more than once; the generated model has
# nh = nk = 1, so all five row blocks are non-empty; the tracking model runs with and without a new last reference
CASES = [("double_integrator", 3, 5, False), ("quadrotor", 2, 3, False), ("cartpole", 70, 2, False), ("generated_rows", 4, 6, False),
         ("tracking", 4, 6, True), ("tracking", 4, 6, False)]


@pytest.mark.parametrize("kind,N,B,with_r_new", CASES)
def test_advance_matches_numpy(built, kind, N, B, with_r_new):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    mdl = _model(kind, N)
    ev = StageEvaluator(mdl)
    assert (ev.n, ev.m, ev.np) == (mdl.n, mdl.m, mdl.np)
    rng = np.random.default_rng(11)
    nx, f, pf = mdl.nx, mdl.f, mdl.pref
    status = np.array(ac.STATUS6[:B], np.int32)
    ok = np.isin(status, OK)
    x = _trajectory(mdl, B, rng)
    lbx = rng.normal(size=(B, mdl.nvar)); ubx = lbx + 1.0
    lbx[:, -1] = -np.inf; ubx[:, -2] = np.inf
    p = rng.normal(size=(B, mdl.np))
    dw = rng.normal(size=(B, mdl.n)); y = rng.normal(size=(B, mdl.m))
    dw[~ok] = np.nan; y[~ok] = np.nan
    s_meas = rng.normal(size=(B, nx)); w = rng.normal(0.0, 0.01, size=(B, nx))
    r_new = rng.normal(size=(B, nx)) if with_r_new else None
    try:
        for tail in ("repeat", "rollout"):
            for mode in ("simulated", "measured", "disturbed"):
                kw = {"measured": dict(s_meas=s_meas), "disturbed": dict(w=w)}.get(mode, {})
                ref = mdl.advance(x, lbx, ubx, status=status, tail=tail, p=p, r_new=r_new, dw=dw, y=y, **kw)
                d = dict(x_out=_nan(B, mdl.nvar), dw_out=_nan(B, mdl.n), y_out=_nan(B, mdl.m), applied=_nan(B, f), stage_cost=_nan(B))
                dl, du = _dev(lbx), _dev(ubx)
                if pf:
                    d["p_out"] = _nan(B, mdl.np)
                ev.advance(_dev(x), d["x_out"], dl, du, status=_dev(status, torch.int32), tail=tail, dw_in=_dev(dw), dw_out=d["dw_out"], y_in=_dev(y),
                           y_out=d["y_out"], applied=d["applied"], stage_cost=d["stage_cost"], r_new=None if r_new is None else _dev(r_new),
                           **({"p_in": _dev(p), "p_out": d["p_out"]} if pf else {"p": _dev(p)}), **{k: _dev(v) for k, v in kw.items()})
                torch.cuda.synchronize()
                got = {k.replace("_out", ""): v.cpu().numpy() for k, v in d.items()}
                got["lbx"] = dl.cpu().numpy(); got["ubx"] = du.cpu().numpy()
                tag = (tail, mode)
                G = got["x"].reshape(B, N, f); R = ref["x"].reshape(B, N, f)
                # frame 0: the state through F unless measured, the input a copy
                assert (_bits if mode == "measured" else _close)(G[:, 0, :nx], R[:, 0, :nx]), tag
                assert _bits(G[:, 0, nx:], R[:, 0, nx:]) and _bits(G[:, 1:N - 1], R[:, 1:N - 1]), tag
                assert (_bits if tail == "repeat" else _close)(G[:, N - 1, :nx], R[:, N - 1, :nx]) and _bits(G[:, N - 1, nx:], R[:, N - 1, nx:]), tag
                # the pin is frame 0 of x_out bit for bit; nothing else in lbx / ubx moved
                for k, old in (("lbx", lbx), ("ubx", ubx)):
                    assert _bits(got[k][:, :f], G[:, 0]) and _bits(got[k][:, f:], old[:, f:]), (tag, k)
                for k in ("dw", "y", "applied") + (("p",) if pf else ()):
                    assert _bits(got[k], ref[k]), (tag, k)
                assert _close(got["stage_cost"], ref["stage_cost"]), tag
                for k, v in got.items():
                    fin = np.isfinite(v) | np.isinf(np.broadcast_to(ref[k], v.shape))
                    assert not np.isnan(v[ok]).any() and fin[ok].all(), (tag, k)
                assert not np.isnan(got["dw"]).any() and not np.isnan(got["y"]).any(), tag       # the failed instances restart from zeros
                # two runs on the same input give the same bits
                if tail == "rollout" and mode == "simulated":
                    x2 = _nan(B, mdl.nvar)
                    ev.advance(_dev(x), x2, _dev(lbx), _dev(ubx), status=_dev(status, torch.int32), tail=tail,
                               **({"p_in": _dev(p), "p_out": _nan(B, mdl.np)} if pf else {}))
                    assert _bits(x2.cpu().numpy(), got["x"])
    finally:
        ev.close()


def test_advance_errors(built):
    """every refusal of include/mpcqp.h; the outputs stay as they were"""
    from optimal_control_problem_amd.stage_eval import AdvanceArgs, StageEvaluator, _bind
    L = _bind(_lib.lib())
    B = 3
    plain = StageEvaluator(models.DoubleIntegrator(3, 0.05)); track = StageEvaluator(ac.TrackingIntegrator(3, 0.05))
    try:
        for ev in (plain, track):
            t = {k: _nan(B, w) for k, w in (("x_out", ev.nvar), ("dw_out", ev.n), ("y_out", ev.m), ("p_out", ev.np))}
            t.update({k: torch.ones((B, w), dtype=torch.float64, device="cuda") for k, w in
                      (("x_in", ev.nvar), ("lbx", ev.nvar), ("ubx", ev.nvar), ("dw_in", ev.n), ("y_in", ev.m), ("p_in", ev.np), ("p", ev.nx),
                       ("r_new", ev.nx), ("s_meas", ev.nx), ("w", ev.nx))})
            t["stage_cost"] = _nan(B)
            base = ["x_in", "x_out", "lbx", "ubx"] + (["p_in", "p_out"] if ev is track else [])

            def call(names, handle=ev._h, batch=B, tail=1, alias=None):
                a = AdvanceArgs()
                for k in names:
                    setattr(a, k, t[k].data_ptr())
                for dst, src in (alias or {}).items():
                    setattr(a, dst, t[src].data_ptr())
                a.tail = tail
                return L.mpcqp_stage_advance(handle, batch, C.byref(a), None)

            assert call(base + ["dw_in", "dw_out", "y_in", "y_out"], batch=0) == _lib.ERR_ARG
            assert call(base, handle=None) == _lib.ERR_ARG and call(base, batch=-1) == _lib.ERR_ARG
            assert L.mpcqp_stage_advance(ev._h, B, None, None) == _lib.ERR_ARG
            for missing in ("x_in", "x_out", "lbx", "ubx"):
                assert call([k for k in base if k != missing]) == _lib.ERR_ARG, missing
            assert call(base, alias={"x_out": "x_in"}) == _lib.ERR_ARG
            assert call(base + ["dw_in"], alias={"dw_out": "dw_in"}) == _lib.ERR_ARG
            assert call(base + ["y_in"], alias={"y_out": "y_in"}) == _lib.ERR_ARG
            for half in ("dw_in", "dw_out", "y_in", "y_out"):
                assert call(base + [half]) == _lib.ERR_ARG, half
            assert call(base + ["w", "s_meas"]) == _lib.ERR_ARG
            assert call(base, tail=2) == _lib.ERR_ARG and call(base, tail=-1) == _lib.ERR_ARG
            if ev is track:
                assert call([k for k in base if k != "p_in"]) == _lib.ERR_ARG and call([k for k in base if k != "p_out"]) == _lib.ERR_ARG
                assert call(base, alias={"p_out": "p_in"}) == _lib.ERR_ARG
                assert call(base + ["p"]) == _lib.ERR_ARG
            else:
                assert call(base + ["p_in", "p_out"]) == _lib.ERR_ARG and call(base + ["p_in"]) == _lib.ERR_ARG
                assert call(base + ["r_new"]) == _lib.ERR_ARG
                assert call(base + ["stage_cost"]) == _lib.ERR_ARG         # no reference to measure the cost against
            torch.cuda.synchronize()
            for k in ("x_out", "dw_out", "y_out", "p_out", "stage_cost"):
                assert torch.isnan(t[k]).all(), k
            for k in ("lbx", "ubx", "x_in"):
                assert (t[k] == 1.0).all(), k
            assert call(base) == _lib.OK                                   # and the same block without the fault is taken
            torch.cuda.synchronize()
            assert not torch.isnan(t["x_out"]).any()
    finally:
        plain.close(); track.close()


def test_closed_loop_equals_composed_loop(built):
    """measured plant + repeated tail: advance is pure data movement, so ClosedLoopMPC must reproduce, bit for bit, a loop composed here from
    DeviceSQPOptimizationSolver.getOptimalSolution and torch slicing"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, _, meta = models.make_workload("double_integrator", 16)
    B, N, nx, f, n = 16, mdl.N, mdl.nx, mdl.f, mdl.n
    opts = {"max_iter": 1, "alpha": 1.0, "warm_start_admm": True, "skip_failed_steps": True}
    ticks = 5
    sol = DeviceSQPOptimizationSolver(mdl, opts, batch=B)
    mpc = ClosedLoopMPC(mdl, opts, batch=B, tail="repeat", shift=True)
    try:
        arg = {k: _dev(meta[k]) for k in ("lbx", "ubx", "lbg", "ubg", "p")}
        want = []; measured = []
        for _ in range(ticks):
            sol.getOptimalSolution(arg, to_host=False)
            X = sol.x.view(B, N, f)
            okm = ((sol.status == 1) | (sol.status == 2) | (sol.status == 7)).unsqueeze(1)
            frame = X[:, 0].cpu().numpy()
            meas = _dev(mdl.F(frame[:, :nx], frame[:, nx:]))           # the plant, in NumPy
            measured.append(meas)
            xn = torch.cat([meas, torch.where(okm, X[:, 1, nx:], X[:, 0, nx:]), X[:, 2:].reshape(B, -1), X[:, N - 1]], dim=1).contiguous()
            arg["lbx"][:, :f] = xn[:, :f]; arg["ubx"][:, :f] = xn[:, :f]
            zf = torch.zeros((B, f), dtype=torch.float64, device="cuda"); zx = torch.zeros((B, nx), dtype=torch.float64, device="cuda")
            dwn = torch.cat([sol.dw[:, :nx], sol.dw[:, nx + f:], zf], dim=1)
            yn = torch.cat([sol.y[:, :nx], sol.y[:, nx + f:n], zf, sol.y[:, n + nx:], zx], dim=1)
            want.append((xn.clone(), sol.status.clone(), sol.iters.clone()))
            sol.x = xn
            sol.dw = torch.where(okm, dwn, torch.zeros_like(dwn)).contiguous(); sol.y = torch.where(okm, yn, torch.zeros_like(yn)).contiguous()
        mpc.reset(meta["frame0"])
        for t in range(ticks):
            out = mpc.tick(measured=measured[t])
            xw, sw, iw = want[t]
            assert torch.equal(out["status"], sw) and torch.equal(out["iters"], iw), t
            assert _bits(mpc.x.cpu().numpy(), xw.cpu().numpy()), t
            assert _bits(mpc.lbx.cpu().numpy()[:, :f], xw.cpu().numpy()[:, :f])
        assert (want[-1][2] > 0).all()
    finally:
        sol.close(); mpc.close()


@pytest.mark.parametrize("kind", ["quadrotor", "pendulum"])
def test_closed_loop_simulated(built, kind):
    """the plant is the model's own map, applied on the device: after every tick the new first state is F (NumPy) of the frame that was applied"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    B = 8
    if kind == "quadrotor":
        mdl, _, meta = models.make_workload("quadrotor", B, N=10)
        frame0 = meta["frame0"]
    else:
        mdl = ac.pendulum(20)
        frame0 = np.concatenate([np.random.default_rng(0).uniform(-1, 1, (B, 2)), np.zeros((B, 1))], axis=1)
    nx, f = mdl.nx, mdl.f
    mpc = ClosedLoopMPC(mdl, {"warm_start_admm": True}, batch=B, tail="rollout")
    try:
        mpc.reset(frame0)
        for t in range(4):
            out = mpc.tick()
            applied = out["applied"].cpu().numpy()
            x = mpc.x.cpu().numpy()
            assert np.isin(out["status"].cpu().numpy(), OK).all(), t
            assert _close(x[:, :nx], mdl.F(applied[:, :nx], applied[:, nx:])), t
            assert _bits(mpc.lbx.cpu().numpy()[:, :f], x[:, :f]) and _bits(mpc.ubx.cpu().numpy()[:, :f], x[:, :f]), t
            assert np.isfinite(x).all()
    finally:
        mpc.close()


def test_closed_loop_recipe(built):
    """the recipe tests/test_advance_host.py fixes on the CPU oracle: every instance ends nearer the origin than it began, no tick is infeasible"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl, frame0 = ac.recipe()
    mpc = ClosedLoopMPC(mdl, dict(ac.RECIPE_OPTIONS), batch=ac.RECIPE_BATCH, tail="rollout")
    try:
        mpc.reset(frame0)
        failed = torch.zeros(ac.RECIPE_BATCH, dtype=torch.int32, device="cuda")
        for _ in range(ac.RECIPE_TICKS):
            st = mpc.tick()["status"]
            failed += ((st != 1) & (st != 2) & (st != 7)).to(torch.int32)
        assert int(failed.sum()) == 0
        end = mpc.x.cpu().numpy()[:, :mdl.nx]
        assert (np.linalg.norm(end, axis=1) < np.linalg.norm(frame0[:, :mdl.nx], axis=1)).all()
    finally:
        mpc.close()


C_EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "advance_c_test")


def test_advance_from_plain_c(built):
    r = subprocess.run([C_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "advance from C ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    X = ac.HAND_X
    m = models.DoubleIntegrator(3, 0.5)
    lbx = -100.0 + np.arange(18.0).reshape(2, 9); ubx = 100.0 + np.arange(18.0).reshape(2, 9)
    dw = 0.5 + np.arange(22.0).reshape(2, 11); y = -0.25 * np.arange(30.0).reshape(2, 15)
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] in ("x", "lbx", "ubx", "dw", "y"):
            got[(w[0], int(w[1]), int(w[2]))] = np.array([float(v) for v in w[3:]])
    assert len(got) == 5 * 2 * 2
    for ti, tail in enumerate(("repeat", "rollout")):
        ref = m.advance(X, lbx, ubx, status=[1, 3], tail=tail, dw=dw, y=y)
        for k in ("x", "lbx", "ubx", "dw", "y"):
            for b in range(2):
                g = got[(k, ti, b)]
                assert g.shape == ref[k][b].shape and _close(g, ref[k][b]), (tail, k, b)
                if k in ("dw", "y"):
                    assert _bits(g, ref[k][b])
