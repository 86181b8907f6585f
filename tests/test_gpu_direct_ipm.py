"""GPU: the interior-point direct solve (mpcqp_stage_riccati_solve_ipm; csrc/stage_riccati_ipm.hpp stage_direct_ipm_kernel) against its NumPy
statement (models.StageOCP.direct_qp_ipm) on the batches whose margins tests/test_direct_ipm_host.py checks, its bitwise promises, a block whose
groups finish in different iterations, and the layers built on it: StageEvaluator.riccati_solve_ipm, options["direct_qp"]["interior_point"] of the
device loop against the host loop, ClosedLoopMPC, a captured graph, the example.

Tolerances.  w, z and y of accepted instances are compared with the statement at di.DEVICE_BAR_W / di.DEVICE_BAR_Y = max(1e-12, 16 e_np) relative to
max(1, max |ref|), e_np the statement's rounding sensitivity (6.0e-9 and 2.0e-8, see tests/support/direct_ipm_cases.py for why they are that large):
the device runs the statement's operations with fused multiply-adds.  Iteration-0 acceptances are compared at direct_qp's bars.  direct and
iters_used are compared exactly, res at the larger of its tolerance and the bar."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import direct_ipm_cases as di
from tests.support import direct_qp_cases as dc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = di.bits
KEYS = di.KEYS
_EV = {}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _ev(mdl):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    if id(mdl) not in _EV:
        _EV[id(mdl)] = (mdl, StageEvaluator(mdl))
    return _EV[id(mdl)][1]


def _batches(f):
    from optimal_control_problem_amd.stage_eval import riccati_groups_per_block
    G = riccati_groups_per_block(f)
    return [B for B in (1, G - 1, G, G + 1, 2 * G + 1) if B >= 1]


def _run(ev, d, guard=0, frozen=None, **kw):
    """riccati_solve_ipm on NaN-filled outputs with `guard` rows around them; iters_used prefilled with -1, direct with -7"""
    B = d["P"].shape[0]
    full = lambda w: torch.full((B + 2 * guard, w), float("nan"), dtype=torch.float64, device="cuda")
    W, Y, Z, R = full(ev.n), full(ev.m), full(ev.m), full(3)
    direct = torch.full((B + 2 * guard,), -7, dtype=torch.int32, device="cuda")
    used = torch.full((B + 2 * guard,), -1, dtype=torch.int32, device="cuda")
    s = slice(guard, guard + B)
    out = {"w": W[s], "y": Y[s], "z": Z[s], "direct": direct[s], "iters_used": used[s], "res": R[s]}
    kw = dict(dict(feas_tol=di.FEAS_TOL, comp_tol=di.COMP_TOL, stat_tol=di.STAT_TOL, iters=di.ITERS), **kw)
    ev.riccati_solve_ipm({k: _dev(d[k]) for k in KEYS}, out=out, frozen=None if frozen is None else _dev(frozen, torch.int32), **kw)
    torch.cuda.synchronize()
    return {"w": W.cpu().numpy(), "y": Y.cpu().numpy(), "z": Z.cpu().numpy(), "direct": direct.cpu().numpy(), "iters_used": used.cpu().numpy(),
            "res": R.cpu().numpy()}


def _check(got, st, frozen, tag, guard=0):
    w, y, z, direct, used, res = st
    B = len(direct)
    s = slice(guard, guard + B)
    want = np.where(frozen != 0, -7, direct)                 # a frozen instance's verdict slot is not written
    assert np.array_equal(got["direct"][s], want), (tag, got["direct"][s], want)
    assert np.array_equal(got["iters_used"][s], used), (tag, got["iters_used"][s], used)
    acc = direct == 1
    for k in ("w", "y", "z"):
        assert np.isnan(got[k][s][~acc]).all() and np.isfinite(got[k][s][acc]).all(), (tag, k)
    assert np.array_equal(np.isnan(got["res"][s]), np.isnan(res)), tag
    if guard:
        for k in ("w", "y", "z", "res"):
            assert np.isnan(got[k][:guard]).all() and np.isnan(got[k][guard + B:]).all(), (tag, k)
        assert (got["direct"][[0, -1]] == -7).all() and (got["iters_used"][[0, -1]] == -1).all(), tag
    worst = 0.0
    for sel, bw, by in ((acc & (used == 0), dc.DEVICE_BAR_W, dc.DEVICE_BAR_Y), (acc & (used > 0), di.DEVICE_BAR_W, di.DEVICE_BAR_Y)):
        if sel.any():
            ew, ey, ez = di.rel_err(got["w"][s][sel], w[sel]), di.rel_err(got["y"][s][sel], y[sel]), di.rel_err(got["z"][s][sel], z[sel])
            assert ew <= bw and ez <= bw and ey <= by, (tag, ew, ey, ez)
            worst = max(worst, ew / bw, ez / bw, ey / by)
    a1 = acc & (used > 0)
    if a1.any():
        r = got["res"][s][a1]
        assert (r[:, 0] <= di.FEAS_TOL).all() and (r[:, 1] <= di.COMP_TOL).all() and (r[:, 2] <= di.STAT_TOL).all(), tag
        assert np.abs(r[:, 1] - res[a1][:, 1]).max() <= di.DEVICE_BAR_Y * di.COMP_TOL * 10, tag
    return worst


@pytest.mark.parametrize("N", di.HORIZONS)
@pytest.mark.parametrize("kind", di.MODELS)
def test_parity(built, kind, N):
    """the case batch (every role) repeated to batches around the groups per block, with and without reg; and iterations spent at iters = 5"""
    mdl = di.model(kind, N)
    ev = _ev(mdl)
    worst = 0.0
    for reg in (0.0, 0.05):
        for iters in (di.ITERS, 5) if reg == 0.0 else (di.ITERS,):
            st0 = di.statement(kind, N, reg, iters)
            for B in _batches(mdl.f):
                _, d, frozen, roles = di.tiled(kind, N, B, reg)
                idx = np.arange(B) % len(st0[3])
                st = tuple(a[idx] for a in st0)
                got = _run(ev, d, guard=1, frozen=frozen, reg=reg, iters=iters)
                worst = max(worst, _check(got, st, frozen, (kind, N, B, reg, iters), guard=1))
    print(kind, N, "worst error / bar", worst)


@pytest.mark.parametrize("kind", ("cartpole", "quadrotor", "linear13x4"))
def test_bitwise_promises(built, kind):
    """a repeat launch gives the same bits; an instance alone gives the bits it has at any position of a batch of 11; an instance accepted in
    iteration 0 has the bits of riccati_solve"""
    N, B = 20, 11
    mdl = di.model(kind, N)
    ev = _ev(mdl)
    _, d, frozen, roles = di.tiled(kind, N, B)
    ref = _run(ev, d, frozen=frozen)
    again = _run(ev, d, frozen=frozen)
    assert (ref["direct"] == 1).sum() >= 5 and (ref["iters_used"] >= 1).sum() >= 5
    for k in ("w", "y", "z", "direct", "iters_used", "res"):
        assert _same(ref[k], again[k]), k
    for b in (0, 1, 2, 4, 8):
        one = _run(ev, {k: v[b:b + 1] for k, v in d.items()}, frozen=frozen[b:b + 1])
        for k in ("w", "y", "z", "res", "direct", "iters_used"):
            assert _same(one[k][0], ref[k][b]), (k, b)
    plain = ev.riccati_solve({k: _dev(d[k]) for k in KEYS}, feas_tol=di.FEAS_TOL)
    torch.cuda.synchronize()
    r0 = (ref["direct"] == 1) & (ref["iters_used"] == 0)
    assert r0.any() and np.array_equal(plain["direct"].cpu().numpy() == 1, r0 & (frozen == 0))
    for k in ("w", "y", "z"):
        assert _same(plain[k].cpu().numpy()[r0], ref[k][r0]), k


def test_groups_of_one_block_finish_in_different_iterations(built):
    """16 double integrators in one block: accepted in iteration 0 and after different numbers of iterations, one that spends them all, an
    ineligible and a frozen one, side by side.  A group that is done walks the barriers of the other groups' iterations: its neighbours' results
    are those they have alone, bit for bit."""
    mdl, d, frozen = di.mixed_block()
    ev = _ev(mdl)
    tr = []
    st = mdl.direct_qp_ipm(*(d[k] for k in KEYS), frozen=frozen, trace=tr)
    direct, used = st[3], st[4]
    print("verdicts", direct, "iterations", used)
    assert di.margins(mdl, d, tr, direct, used).min() >= di.MARGIN
    assert ((direct == 1) & (used == 0)).any() and len(set(used[(direct == 1) & (used > 0)])) >= 3 and ((direct == 0) & (used == di.ITERS)).any()
    assert (direct == -1).any() and (frozen != 0).any()
    got = _run(ev, d, guard=1, frozen=frozen)
    _check(got, st, frozen, "mixed", guard=1)
    for b in range(len(direct)):
        one = _run(ev, {k: v[b:b + 1] for k, v in d.items()}, frozen=frozen[b:b + 1])
        for k in ("w", "y", "z", "res", "direct", "iters_used"):
            assert _same(one[k][0], got[k][1 + b]), (k, b)


def _device_loop(option, **more):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, arg, x0 = di.recipe()
    opt = dict({"max_iter": di.RECIPE_ITERS, "alpha": 1.0}, **more)
    if option is not None:
        opt["direct_qp"] = option
    sol = DeviceSQPOptimizationSolver(mdl, opt, batch=di.RECIPE_B)
    sol.setInitialGuess(x0)
    out = sol.getOptimalSolution(arg)
    return sol, np.array(out["x"], float), arg


def test_device_loop_is_the_host_loop(built):
    """the state-bound recipe of tests/test_direct_ipm_host.py: the device loop with "interior_point" equals the host loop with it to the bar of the
    parity test (the model is linear: every iteration's x + dw is one QP solution); verdicts and iteration counts are the same in every SQP
    iteration; every QP is accepted, none by direct_qp alone or with "active_set" """
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    sol, x, arg = _device_loop({"interior_point": True})
    try:
        mdl, _, x0 = di.recipe()
        host = SQPOptimizationSolver(mdl, {"max_iter": di.RECIPE_ITERS, "alpha": 1.0, "direct_qp": {"interior_point": True}}, batch=di.RECIPE_B,
                                     qp_solver=OracleCuCaQP(di.RECIPE_B, nthreads=4))
        host.setInitialGuess(x0)
        xh = np.array(host.getOptimalSolution(arg)["x"], float)
        hd = np.array([h.cpu().numpy() for h in sol.direct_history]); hh = np.array(host.direct_history)
        rd = np.array([h.cpu().numpy() for h in sol.direct_iters_history]); rh = np.array(host.direct_iters_history)
        print("device verdicts\n", hd, "\ndevice iterations\n", rd, "\nhost iterations\n", rh)
        assert np.array_equal(hd, hh) and np.array_equal(rd, rh) and (hd == 1).all() and (rd >= 1).all()
        err = np.abs(x - xh).max()
        print("|x_device - x_host| %.3e" % err)
        assert err <= di.DEVICE_BAR_W * (1.0 + np.abs(xh).max())
        its = np.array([i.cpu().numpy() for i in sol.admm_iterations])
        assert (its == 0).all() and (sol.status.cpu().numpy() == 1).all()
    finally:
        sol.close()
    for option in (True, {"active_set": True}):
        other, _, _ = _device_loop(option)
        try:
            assert all((h.cpu().numpy() == 0).all() for h in other.direct_history) and other.direct_iters_history == [] and other.direct_ipm is None
        finally:
            other.close()


def _composed(mdl, frame0, ticks, option):
    """the ticks of ClosedLoopMPC composed by hand from getOptimalSolution and ev.advance"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B, f = frame0.shape[0], mdl.f
    opt = {"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True, "warm_start_admm": True, "direct_qp": option}
    sol = DeviceSQPOptimizationSolver(mdl, opt, batch=B)
    ev = sol.ev
    lbx, ubx, lbg, ubg = [_dev(v) for v in mdl.stacked_bounds(frame0)]
    p = torch.zeros((B, ev.np), dtype=torch.float64, device="cuda")
    mk = lambda w: torch.zeros((B, w), dtype=torch.float64, device="cuda")
    x2, dw2, y2 = mk(ev.nvar), mk(ev.n), mk(ev.m)
    applied = mk(f); cost = torch.zeros(B, dtype=torch.float64, device="cuda")
    sol.setInitialGuess(np.zeros(ev.nvar))
    log = []
    try:
        for _ in range(ticks):
            sol.getOptimalSolution({"p": p, "lbx": lbx, "ubx": ubx, "lbg": lbg, "ubg": ubg}, to_host=False)
            ev.advance(sol.x, x2, lbx, ubx, status=sol.status, tail="rollout", p=p, dw_in=sol.dw, dw_out=dw2, y_in=sol.y, y_out=y2,
                       applied=applied, stage_cost=cost)
            sol.x, x2 = x2, sol.x
            sol.dw, dw2 = dw2, sol.dw
            sol.y, y2 = y2, sol.y
            sol._start_clean = True
            torch.cuda.synchronize()
            log.append(dict(applied=applied.cpu().numpy().copy(), x=sol.x.cpu().numpy().copy(), y=sol.y.cpu().numpy().copy(),
                            direct=sol.direct_history[-1].cpu().numpy().copy(), iters=sol.direct_iters_history[-1].cpu().numpy().copy()))
        return log
    finally:
        sol.close()


def _riding_start(mdl, B):
    frame0 = np.zeros((B, mdl.f))
    frame0[:, 0] = np.linspace(3.0, 4.0, B)
    frame0[:, 1] = -np.linspace(1.6, 1.9, B)
    return frame0


def test_closed_loop_with_the_option_is_the_composed_loop(built):
    """ClosedLoopMPC with "interior_point" is bitwise the loop composed from the calls (nothing is carried between ticks); the first ticks, whose
    plans ride the velocity limit, are accepted"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl = di.model("double_integrator", 20)
    B, ticks = 5, 4
    frame0 = _riding_start(mdl, B)
    ref = _composed(mdl, frame0, ticks, {"interior_point": True})
    mpc = ClosedLoopMPC(mdl, {"direct_qp": {"interior_point": True}, "warm_start_admm": True}, batch=B)
    try:
        mpc.reset(frame0)
        for i in range(ticks):
            out = mpc.tick()
            torch.cuda.synchronize()
            assert _same(out["applied"].cpu().numpy(), ref[i]["applied"]) and _same(mpc.x.cpu().numpy(), ref[i]["x"]), i
            assert _same(mpc.sol.y.cpu().numpy(), ref[i]["y"]), i
            assert np.array_equal(mpc.sol.direct_history[-1].cpu().numpy(), ref[i]["direct"]), i
            assert np.array_equal(mpc.sol.direct_iters_history[-1].cpu().numpy(), ref[i]["iters"]), i
        h = np.array([r["direct"] for r in ref]); r = np.array([r["iters"] for r in ref])
        print("closed loop verdicts per tick\n", h, "\niterations\n", r)
        assert (h[0] == 1).all() and (r[0] >= 1).all()
    finally:
        mpc.close()


def test_without_interior_point_the_new_entry_is_not_called(built, monkeypatch):
    """options["direct_qp"] = True, {"active_set": True} and no direct_qp at all are bitwise what they are with the new entry point replaced by a
    function that fails the test: the device loop and ClosedLoopMPC"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    mdl = di.model("double_integrator", 20)
    frame0 = _riding_start(mdl, 5)

    def loops():
        res = []
        for option in (True, {"active_set": True}, None):
            sol, x, _ = _device_loop(option)
            res.append(x); sol.close()
            mpc = ClosedLoopMPC(mdl, dict({"warm_start_admm": True}, **({"direct_qp": option} if option else {})), batch=5)
            mpc.reset(frame0)
            for _ in range(3):
                out = mpc.tick()
            torch.cuda.synchronize()
            res.append(mpc.x.cpu().numpy().copy()); res.append(out["applied"].cpu().numpy().copy())
            assert mpc.sol.direct_ipm is None and mpc.sol.direct_iters_history == []
            mpc.close()
        return res

    ref = loops()

    def boom(*a, **k):
        raise AssertionError("a loop without interior_point launched mpcqp_stage_riccati_solve_ipm")

    monkeypatch.setattr(StageEvaluator, "riccati_solve_ipm", boom)
    for a, b in zip(loops(), ref):
        assert _same(a, b)


def test_captured_graph_replays_after_a_first_plain_call(built):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    N, B = 20, 9
    mdl = di.model("cartpole", N)
    ev = StageEvaluator(mdl)                           # a fresh handle: neither tables nor workspace yet
    try:
        _, d, frozen, roles = di.tiled("cartpole", N, B)
        ls = {k: _dev(d[k]) for k in KEYS}
        fz = _dev(frozen, torch.int32)
        mk = lambda w: torch.zeros((B, w), dtype=torch.float64, device="cuda")
        out = {"w": mk(ev.n), "y": mk(ev.m), "z": mk(ev.m), "direct": torch.zeros(B, dtype=torch.int32, device="cuda"),
               "iters_used": torch.zeros(B, dtype=torch.int32, device="cuda"), "res": mk(3)}
        s = torch.cuda.Stream(); g0 = torch.cuda.CUDAGraph(); g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g0, stream=s):
                out["direct"].fill_(-5)
                with pytest.raises(_lib.MpcqpError) as e:      # the first call would allocate: refused under capture, with the reason
                    ev.riccati_solve_ipm(ls, frozen=fz, out=out, stream=s.cuda_stream)
            assert e.value.code == _lib.ERR_STATE and "capturing" in str(e.value)
            ev.riccati_solve_ipm(ls, frozen=fz, out=out, stream=s.cuda_stream)
            s.synchronize()
            ref = {k: v.cpu().numpy().copy() for k, v in out.items()}
            assert (ref["direct"] == 1).any() and (ref["iters_used"] >= 1).any()
            with torch.cuda.graph(g, stream=s):
                ev.riccati_solve_ipm(ls, frozen=fz, out=out, stream=s.cuda_stream)
            for k in ("w", "y", "z", "res"):
                out[k].fill_(-1.0)
            out["direct"].fill_(-7); out["iters_used"].fill_(-7)
            g.replay(); s.synchronize()
        acc = ref["direct"] == 1
        written = np.isin(ref["direct"], (0, 1)) & (frozen == 0)
        for k in ("w", "y", "z"):
            assert _same(out[k].cpu().numpy()[acc], ref[k][acc]), k
            assert (out[k].cpu().numpy()[~acc] == -1.0).all(), k
        assert np.array_equal(out["direct"].cpu().numpy()[frozen == 0], ref["direct"][frozen == 0]) and (out["direct"].cpu().numpy()[frozen != 0] == -7).all()
        assert np.array_equal(out["iters_used"].cpu().numpy()[written], ref["iters_used"][written]) and (out["iters_used"].cpu().numpy()[~written] == -7).all()
        assert _same(out["res"].cpu().numpy()[written], ref["res"][written]) and (out["res"].cpu().numpy()[~written] == -1.0).all()
        # a larger batch than any plain call has seen would grow the workspace: refused under capture as well, then served by a plain call
        B2 = B + 3
        _, d2, frozen2, _ = di.tiled("cartpole", N, B2)
        ls2 = {k: _dev(d2[k]) for k in KEYS}
        g1 = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g1, stream=s):
                out["direct"].fill_(-5)
                with pytest.raises(_lib.MpcqpError) as e:
                    ev.riccati_solve_ipm(ls2, stream=s.cuda_stream)
            assert e.value.code == _lib.ERR_STATE and "capturing" in str(e.value)
            s.synchronize()
        got = _run(ev, d2, frozen=frozen2)
        st0 = di.statement("cartpole", N)
        idx = np.arange(B2) % len(st0[3])
        _check(got, tuple(a[idx] for a in st0), frozen2, "after the refused capture")
    finally:
        ev.close()


def test_refusals(built):
    import ctypes as C
    from optimal_control_problem_amd import stage_eval as se
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, DIRECT_QP_REFUSES
    from tests.support import convexify_cases as cc
    N = 3
    mdl = di.model("double_integrator", N)
    ev = _ev(mdl)
    d = dc.local_qp(mdl, 2)
    ls = {k: _dev(d[k]) for k in KEYS}
    for kw in (dict(feas_tol=-1.0), dict(reg=float("nan")), dict(comp_tol=-1.0), dict(comp_tol=float("nan")), dict(stat_tol=-1.0), dict(stat_tol=float("nan")),
               dict(iters=0), dict(iters=51), dict(iters=1.5)):
        with pytest.raises(ValueError):
            ev.riccati_solve_ipm(ls, **kw)
    L = se._bind(_lib.lib())
    good = ev.riccati_solve_ipm(ls)

    def args(**kw):
        a = _lib.RiccatiSolveIpmArgs()
        for k in KEYS:
            setattr(a, k, ls[k].data_ptr())
        a.w, a.y, a.direct, a.iters = good["w"].data_ptr(), good["y"].data_ptr(), good["direct"].data_ptr(), 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.mpcqp_stage_riccati_solve_ipm(ev._h, 2, C.byref(args()), None) == _lib.OK      # iters_used, res and z are optional
    for kw in (dict(P=None), dict(q=None), dict(A=None), dict(l=None), dict(u=None), dict(w=None), dict(y=None), dict(direct=None),
               dict(feas_tol=-1e-9), dict(feas_tol=float("nan")), dict(reg=-1.0), dict(comp_tol=-1e-9), dict(comp_tol=float("nan")),
               dict(stat_tol=-1e-9), dict(stat_tol=float("nan")), dict(iters=0), dict(iters=51), dict(iters=-1)):
        assert L.mpcqp_stage_riccati_solve_ipm(ev._h, 2, C.byref(args(**kw)), None) == _lib.ERR_ARG, kw
    assert L.mpcqp_stage_riccati_solve_ipm(ev._h, 0, C.byref(args()), None) == _lib.ERR_ARG
    assert L.mpcqp_stage_riccati_solve_ipm(ev._h, 2, None, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    link = cc.case("bump_link")["model"]
    evl = se.StageEvaluator(link)
    try:
        z = lambda w: torch.zeros((1, w), dtype=torch.float64, device="cuda")
        with pytest.raises(_lib.MpcqpError) as e:
            evl.riccati_solve_ipm({"P": z(evl.nnzP), "q": z(evl.n), "A": z(evl.nnzA), "l": z(evl.m), "u": z(evl.m)})
        assert e.value.code == _lib.ERR_LIMIT and "link cost" in str(e.value)
    finally:
        evl.close()
    on = {"interior_point": True}
    for key, why in DIRECT_QP_REFUSES.items():
        with pytest.raises(ValueError) as e:
            DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "direct_qp": on, key: True if key != "soft_rows" else {"state": (1.0, 0.0)}}, batch=1)
        assert str(e.value) == why
    with pytest.raises(ValueError) as e:
        DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "direct_qp": on}, batch=1, evaluator=object())
    assert "stage OCPs" in str(e.value)
    for bad in (dict(on, iters=51), dict(on, active_set=True), {"iters": 3}):
        with pytest.raises(ValueError):
            DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "direct_qp": bad}, batch=1)


def test_state_bound_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "state_bound_mpc.py"), "4", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    m = re.search(r"accepted share with interior_point: first tick (\S+) %, smallest (\S+) %", r.stdout)
    assert m and float(m.group(1)) == 100.0 and float(m.group(2)) == 100.0, r.stdout[-2000:]
    m = re.search(r"accepted share with direct_qp alone: first tick (\S+) %; with active_set: first tick (\S+) %", r.stdout)
    assert m and float(m.group(1)) == 0.0 and float(m.group(2)) == 0.0, r.stdout[-2000:]
    m = re.search(r"largest difference of an applied frame to the loop without direct_qp: (\S+)", r.stdout)
    # the loop beside it solves every QP to eps = 1e-3: the applied frames differ by no more than a few of those tolerances (examples/direct_qp_mpc.py's bar)
    assert m and float(m.group(1)) < 1e-2, r.stdout[-2000:]
