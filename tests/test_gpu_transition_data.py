"""GPU: transition data -- the stage data in F / cdyn, kfun and llink (models.StageOCP.transition_data; the sm_tdata branches of stage_eval_kernel,
stage_merit_kernel, stage_linesearch_kernel, stage_advance_kernel, stage_rollout_kernel and stage_lagrangian_kernel in csrc/stage_kernels.hpp) against
the NumPy statement, against the handle without a stored set, the SQP loop, the closed loop and the example.

Tolerances are those of tests/test_gpu_stage_data.py: bit for bit for copies, pins, zeros and untouched data; 1e-12 max(1, |ref|) for whatever passes
through the generated functions; for the Lagrangian Hessian those of tests/test_gpu_exact_hessian.py (1e-12 max(1, |ref|) for the add, 1e-12 max(1,
||H_k^L||_F) behind the eigen-solve); 1e-6 (1 + max |x|) per iteration for the device loop against the host loop.  The CPU side
(tests/test_transition_data_host.py) pins the inputs: no line-search decision sits on its threshold, every QP of the recipe ends solved on the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import transition_data_cases as tdc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])
TAILS = ("rollout", "repeat")
INPUTS = ("iterate", "hold")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _close(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))).all())


@pytest.fixture(scope="module")
def evaluators(built):
    """one evaluator (one generated library) per kind for the whole module; every test leaves it with nothing set"""
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    evs = {}
    yield lambda kind: evs[kind] if kind in evs else evs.setdefault(kind, StageEvaluator(tdc.kernel_case(kind)["model"]))
    for ev in evs.values():
        ev.close()


class _rows:
    """the case's rows (data, and parameters where the model has them) on the evaluator for the duration of a block"""

    def __init__(self, ev, case, d="case", idx=None):
        idx = slice(None) if idx is None else idx
        self.ev, self.theta = ev, None if case["theta"] is None else case["theta"][idx]
        self.d = case["d"][idx] if isinstance(d, str) else d

    def __enter__(self):
        self.ev.set_stage_data(self.d)
        if self.theta is not None:
            self.ev.set_instance_params(self.theta)

    def __exit__(self, *exc):
        self.ev.set_stage_data(None)
        if self.theta is not None:
            self.ev.set_instance_params(None)
        return False


def _run(ev, case, idx=None, K=4, alpha0=1.0):
    """every kernel that calls a transition function on fresh device copies of the case's instances idx (default: all), NaN-filled outputs; returns
    host arrays by name.  Whatever the evaluator holds is in force."""
    mdl = case["model"]
    idx = np.arange(tdc.BATCH) if idx is None else np.asarray(idx)
    B = len(idx)
    h = {k: case[k][idx] for k in ("p", "x", "lbx", "ubx", "lbg", "ubg", "dw", "y", "status", "w")}
    h["q"] = case["ls"].q[idx]
    out = ev.alloc(B)
    for v in out.values():
        v.fill_(float("nan"))
    ev.eval(_dev(h["p"]), _dev(h["x"]), _dev(h["lbx"]), _dev(h["ubx"]), _dev(h["lbg"]), _dev(h["ubg"]), out=out)
    f, g = ev.merit(_dev(h["p"]), _dev(h["x"]))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["f"] = f.cpu().numpy(); got["gmax"] = g.cpu().numpy()
    if mdl.exact_hessian:
        st = _dev(h["status"], torch.int32)
        for mode in (None, "project"):
            P = out["P"].clone()
            touched = torch.full((B,), -77, dtype=torch.int32, device="cuda"); lam = _nan(B, mdl.N)
            ev.lagrangian(_dev(h["p"]), _dev(h["x"]), _dev(h["y"]), P, status=st, mode=mode, eps=1e-6, touched=touched, lam_min=lam)
            tag = "lag" if mode is None else "lag_project"
            got[tag] = P.cpu().numpy(); got[tag + "_touched"] = touched.cpu().numpy(); got[tag + "_lam"] = lam.cpu().numpy()
    lo = {k: _nan(B) for k in ("alpha", "step_max", "f", "gmax")}
    lo["accepted"] = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    phi = _nan(B, 2); xs = _dev(h["x"]); mu = _dev(MU0[idx])
    ev.line_search(_dev(h["p"]), xs, _dev(h["lbx"]), _dev(h["ubx"]), _dev(h["q"]), _dev(h["dw"]), _dev(h["y"]), status=_dev(h["status"], torch.int32), mu=mu,
                   alpha0=alpha0, candidates=K, out=lo, phi=phi)
    for k, v in lo.items():
        got["ls_" + k] = v.cpu().numpy()
    got["ls_phi"] = phi.cpu().numpy(); got["ls_x"] = xs.cpu().numpy(); got["ls_mu"] = mu.cpu().numpy()
    fm, gm = ev.merit(_dev(h["p"]), xs)                 # the merit kernel at the search's new x
    got["ls_merit_f"] = fm.cpu().numpy(); got["ls_merit_gmax"] = gm.cpu().numpy()
    for tail in TAILS:
        d = dict(x_out=_nan(B, mdl.nvar), dw_out=_nan(B, mdl.n), y_out=_nan(B, mdl.m), applied=_nan(B, mdl.f), stage_cost=_nan(B))
        dl, du = _dev(h["lbx"]), _dev(h["ubx"])
        if mdl.pref:
            d["p_out"] = _nan(B, mdl.np)
        ev.advance(_dev(h["x"]), d["x_out"], dl, du, status=_dev(h["status"], torch.int32), tail=tail, w=_dev(h["w"]), dw_in=_dev(h["dw"]), dw_out=d["dw_out"],
                   y_in=_dev(h["y"]), y_out=d["y_out"], applied=d["applied"], stage_cost=d["stage_cost"],
                   **({"p_in": _dev(h["p"]), "p_out": d["p_out"]} if mdl.pref else {"p": _dev(h["p"])}))
        for k, v in d.items():
            got["adv_%s_%s" % (tail, k.replace("_out", ""))] = v.cpu().numpy()
        got["adv_%s_lbx" % tail] = dl.cpu().numpy(); got["adv_%s_ubx" % tail] = du.cpu().numpy()
    for inputs in INPUTS:
        xo = _nan(B, mdl.nvar)
        r = ev.rollout(_dev(h["x"]), xo, _dev(h["lbx"]), _dev(h["ubx"]), inputs=inputs, diverged=torch.full((B,), -99, dtype=torch.int32, device="cuda"),
                       box_viol=_nan(B))
        xin = _dev(h["x"])
        ev.rollout(xin, None, _dev(h["lbx"]), _dev(h["ubx"]), inputs=inputs)                  # in place
        got["roll_%s_x" % inputs] = xo.cpu().numpy(); got["roll_%s_inplace" % inputs] = xin.cpu().numpy()
        got["roll_%s_diverged" % inputs] = r["diverged"].cpu().numpy(); got["roll_%s_viol" % inputs] = r["box_viol"].cpu().numpy()
    torch.cuda.synchronize()
    return got


def _same_bits(a, b, tag, keys=None):
    for k in (keys or a):
        if a[k].dtype.kind == "f":
            assert _bits(a[k], b[k]), (tag, k, np.abs(a[k] - b[k])[np.isfinite(a[k] - b[k])].max(initial=0.0))
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


def _hnorm(c):
    """||H_k^L||_F [B, N] of the case under its rows: the scale of what passes through the eigen-solve (tests/support/exact_hessian_cases.bar_cvx)"""
    mdl = c["model"]
    mdl.set_stage_data(c["d"])
    try:
        _, hess = mdl.cost_derivatives(c["p"], c["x"])
        C = mdl.constraint_curvature(c["x"], c["y"])
    finally:
        mdl.set_stage_data(None)
    hess = hess.copy()
    hess[:, :, :mdl.f, :mdl.f] += C
    return np.linalg.norm(hess, axis=(2, 3))


# ------------------------------------------------------------------------------------------------ 1. kernels against the statement
@pytest.mark.parametrize("kind", tdc.KINDS)
def test_kernels_match_the_statement(evaluators, kind):
    """every frame of every instance with its own row, batch 7, failed instances among them"""
    ev = evaluators(kind)
    c = tdc.kernel_case(kind)
    mdl = c["model"]
    B, N, nx, f = tdc.BATCH, mdl.N, mdl.nx, mdl.f
    assert ev.transition_data and ev.nsd == mdl.nsd == 2 and ev.param_count == mdl.ntheta
    assert (ev.n, ev.m, ev.np, ev.nnzP, ev.nnzA) == (mdl.n, mdl.m, mdl.np, len(mdl.Pi), len(mdl.Ai))
    assert np.array_equal(ev.Pi, mdl.Pi) and np.array_equal(ev.Ai, mdl.Ai)
    with _rows(ev, c):
        got = _run(ev, c)
    ls = tdc.statement(c, "local_system")
    for k in ("P", "q", "A", "l", "u"):
        assert _close(got[k], getattr(ls, k)), (kind, k, np.abs(got[k] - getattr(ls, k))[np.isfinite(getattr(ls, k))].max())
    ident = np.concatenate([mdl._A_id, mdl._A_next[1:].ravel()])
    assert (got["A"][:, ident] == 1.0).all()
    fr, gr = tdc.statement(c, "merit")
    assert _close(got["f"], fr) and _close(got["gmax"], gr), kind
    mu = MU0.copy()
    se = tdc.statement(c, "line_search", mu=mu)
    print(kind, "accepted", got["ls_accepted"], "alpha", got["ls_alpha"])
    assert np.array_equal(got["ls_accepted"], se["accepted"]) and np.array_equal(got["ls_alpha"], se["alpha"]), kind
    stay = se["alpha"] == 0.0
    assert _bits(got["ls_x"][stay], c["x"][stay]) and _close(got["ls_x"], se["x"]), kind
    bad = ~np.isin(c["status"], tdc.OK)
    assert _bits(got["ls_mu"][bad], MU0[bad]) and _close(got["ls_mu"], mu), kind
    for k in ("f", "gmax", "phi", "step_max"):
        assert np.isfinite(got["ls_" + k]).all() and _close(got["ls_" + k], se[k]), (kind, k)
    for tail in TAILS:
        ref = tdc.statement(c, "advance", tail=tail)
        tag = (kind, tail)
        pre = "adv_%s_" % tail
        G = got[pre + "x"].reshape(B, N, f); R = ref["x"].reshape(B, N, f)
        assert _close(G[:, 0, :nx], R[:, 0, :nx]), tag
        assert _bits(G[:, 0, nx:], R[:, 0, nx:]) and _bits(G[:, 1:N - 1], R[:, 1:N - 1]), tag
        assert (_bits if tail == "repeat" else _close)(G[:, N - 1, :nx], R[:, N - 1, :nx]) and _bits(G[:, N - 1, nx:], R[:, N - 1, nx:]), tag
        for k, old in (("lbx", c["lbx"]), ("ubx", c["ubx"])):
            assert _bits(got[pre + k][:, :f], G[:, 0]) and _bits(got[pre + k][:, f:], old[:, f:]), (tag, k)
        for k in ("dw", "y", "applied") + (("p",) if mdl.pref else ()):
            assert _bits(got[pre + k], ref[k]), (tag, k)
        assert _close(got[pre + "stage_cost"], ref["stage_cost"]), tag
    for inputs in INPUTS:
        ref = tdc.statement(c, "rollout", inputs=inputs)
        G = got["roll_%s_x" % inputs].reshape(B, N, f); R = ref["x"].reshape(B, N, f)
        assert _bits(G[:, 0], R[:, 0]) and _bits(G[:, :, nx:], R[:, :, nx:]) and _close(G[:, 1:, :nx], R[:, 1:, :nx]), (kind, inputs)
        assert np.array_equal(got["roll_%s_diverged" % inputs], ref["diverged"]) and _close(got["roll_%s_viol" % inputs], ref["box_viol"]), (kind, inputs)
    if mdl.exact_hessian:
        ref, _, _ = tdc.statement(c, "lagrangian", P=ls.P)
        assert (np.abs(got["lag"] - ref) <= TOL * np.maximum(1.0, np.abs(ref))).all(), kind
        assert (got["lag_touched"] == -77).all() and np.isnan(got["lag_lam"]).all()
        assert _bits(got["lag"][bad], got["P"][bad]) and not _bits(got["lag"][0], got["P"][0])
        rp, rt, rl = tdc.statement(c, "lagrangian", P=ls.P, mode="project")
        bar = TOL * np.maximum(1.0, _hnorm(c))
        assert np.array_equal(got["lag_project_touched"], rt) and (rt > 0).any(), (kind, got["lag_project_touched"], rt)
        assert (np.abs(got["lag_project_lam"] - rl)[~bad] <= bar[~bad]).all() and np.isnan(got["lag_project_lam"][bad]).all()
        assert (np.abs(got["lag_project"] - rp).max(axis=1) <= bar.max(axis=1)).all(), kind
        assert _bits(got["lag_project"][bad], got["P"][bad])
    # the data show: the statement without them is another system, in the dynamics
    plain = tdc.statement(c, "local_system", d=None)
    blk = mdl._A_blk.ravel()
    assert tdc.gap(plain.A[:, blk], ls.A[:, blk]) > 1e-3 and tdc.gap(plain.l[:, tdc.dynamics_rows(mdl)], ls.l[:, tdc.dynamics_rows(mdl)]) > 1e-3


@pytest.mark.parametrize("kind", tdc.KINDS)
def test_the_data_matter(evaluators, kind):
    """two instances with the same x, p and bounds and different rows: the dynamics blocks of A and the dynamics rows of l, u differ by more than
    1e-3, as the statement says they do"""
    ev = evaluators(kind)
    mdl, d, p, x, lbx, ubx, lbg, ubg = tdc.matters_case(kind)
    mdl.set_stage_data(d)
    try:
        ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
    finally:
        mdl.set_stage_data(None)
    ev.set_stage_data(d)
    try:
        out = {k: v.cpu().numpy() for k, v in ev.eval(_dev(p), _dev(x), _dev(lbx), _dev(ubx), _dev(lbg), _dev(ubg)).items()}
    finally:
        ev.set_stage_data(None)
    blk = mdl._A_blk.ravel(); rows = tdc.dynamics_rows(mdl)
    for k in ("A", "l", "u"):
        assert _close(out[k], getattr(ls, k)), (kind, k)
    assert tdc.gap(out["A"][0, blk], out["A"][1, blk]) > 1e-3
    assert tdc.gap(out["l"][0, rows], out["l"][1, rows]) > 1e-3 and tdc.gap(out["u"][0, rows], out["u"][1, rows]) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. defaults, single instances, in place
@pytest.mark.parametrize("kind", tdc.KINDS)
def test_defaults_and_single_instances(evaluators, kind):
    """the defaults set explicitly are the handle without a set, bit for bit; every instance alone at batch 1 is its row of the batch run; the
    rollout in place is the rollout out of place"""
    ev = evaluators(kind)
    c = tdc.kernel_case(kind)
    mdl = c["model"]
    with _rows(ev, c, d=None):
        unset = _run(ev, c)
    with _rows(ev, c, d=tdc.constant_rows(mdl)):
        explicit = _run(ev, c)
    _same_bits(unset, explicit, (kind, "defaults"))
    with _rows(ev, c):
        batch = _run(ev, c)
        again = _run(ev, c)
    _same_bits(batch, again, (kind, "two runs"))
    blk = mdl._A_blk.ravel()
    assert not _bits(batch["A"][:, blk], unset["A"][:, blk]) and not _bits(batch["roll_iterate_x"], unset["roll_iterate_x"])
    for inputs in INPUTS:
        assert _bits(batch["roll_%s_x" % inputs], batch["roll_%s_inplace" % inputs]), (kind, inputs)
    for b in range(tdc.BATCH):
        with _rows(ev, c, idx=slice(b, b + 1)):
            one = _run(ev, c, idx=[b])
        _same_bits({k: v[b:b + 1] for k, v in batch.items()}, one, (kind, "alone", b))


# ------------------------------------------------------------------------------------------------ 3. the search's invariants
@pytest.mark.parametrize("kind", tdc.KINDS)
def test_search_invariants(evaluators, kind):
    """f_out of the search is the merit kernel's f at the new x, and candidates = 1 is mpcqp_stage_step"""
    ev = evaluators(kind)
    c = tdc.kernel_case(kind)
    with _rows(ev, c):
        got = _run(ev, c)
        diff = np.abs(got["ls_f"] - got["ls_merit_f"]).max()
        print(kind, "max |f_out - merit f| %.3e" % diff)
        # alpha0 = 1, beta = 0.5: every alpha is a power of two, so x + alpha dx is the same number in the search and in the stored x
        assert _bits(got["ls_f"], got["ls_merit_f"]), (kind, diff)
        assert _close(got["ls_gmax"], got["ls_merit_gmax"]), kind
        for alpha0 in (1.0, 0.3):
            one = _run(ev, c, K=1, alpha0=alpha0)
            xs = _dev(c["x"])
            sm = ev.step(alpha0, _dev(c["dw"]), xs, status=_dev(c["status"], torch.int32))
            assert _bits(one["ls_x"], xs.cpu().numpy()) and _bits(one["ls_step_max"], sm.cpu().numpy()), (kind, alpha0)
            ok = np.isin(c["status"], tdc.OK)
            assert (one["ls_alpha"][ok] == alpha0).all() and (one["ls_alpha"][~ok] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 4. the shift
@pytest.mark.parametrize("kind", ["pendulum2", "pendulum3", "pendulum70"])
def test_kernels_after_a_shift(evaluators, kind):
    """after one and after two mpcqp_stage_shift_data calls the kernels compute what they compute with the shifted set handed over afresh"""
    ev = evaluators(kind)
    c = tdc.kernel_case(kind)
    ev.set_stage_data(c["d"])
    try:
        ev.shift_stage_data(_dev(c["d_new"]))
        once = _run(ev, c)
        ev.shift_stage_data()
        twice = _run(ev, c)
        want1 = tdc.shift_reference(c["d"], c["d_new"])
        ev.set_stage_data(want1)
        _same_bits(_run(ev, c), once, (kind, "one shift"))
        ev.set_stage_data(tdc.shift_reference(want1))
        _same_bits(_run(ev, c), twice, (kind, "two shifts"))
        assert not _bits(once["A"], twice["A"]) or c["model"].N == 2
    finally:
        ev.set_stage_data(None)


# ------------------------------------------------------------------------------------------------ 5. the loop
@pytest.mark.parametrize("search", [False, True])
def test_device_loop_equals_host_loop(built, search):
    """the non-uniform-grid recipe (N = 10 x 4, three iterations): the device loop with the grid's rows against the host loop over the CPU oracle with
    the rows on the statement, per iteration"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, d, arg, x0 = tdc.recipe()
    B = d.shape[0]
    host, log = tdc.host_loop(mdl, d, arg, x0, OracleCuCaQP(batch=B, nthreads=4), line_search=search)
    dev = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": tdc.RECIPE_ALPHA, "line_search": search or None}, batch=B)
    try:
        assert dev.ev.transition_data
        dev.setStageData(d)
        dev.setInitialGuess(x0)
        for it in range(tdc.RECIPE_ITERS):
            rd = dev.getOptimalSolution(arg)
            ref = log[it]
            scale = 1.0 + np.abs(ref["x"]).max()
            err = np.abs(rd["x"] - ref["x"]).max()
            print(search, it, "max |x_dev - x_host| %.3e" % err, "scale %.3e" % scale, "status", dev.status.cpu().numpy())
            assert np.array_equal(dev.status.cpu().numpy(), ref["status"]), (search, it)
            assert err <= 1e-6 * scale, (search, it, err)
            assert np.abs(rd["f"] - ref["f"]).max() <= 1e-6 * (1.0 + np.abs(ref["f"]).max())
            if search:
                assert np.array_equal(dev.alpha_taken.cpu().numpy(), ref["alpha"]), it
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 6. the closed loop
@pytest.mark.parametrize("shift_data", [True, False])
def test_closed_loop_equals_composed_ticks(built, shift_data):
    """ClosedLoopMPC over four ticks against a loop composed from getOptimalSolution, evaluator.advance and -- with shift_data=True only --
    evaluator.shift_stage_data on a second solver: x, bounds, status and iterations of every tick bit for bit"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, d, arg, x0 = tdc.recipe()
    B, N = d.shape[0], mdl.N
    frame0 = arg["lbx"][:, :mdl.f]
    mpc = ClosedLoopMPC(mdl, dict(tdc.LOOP_OPTIONS), batch=B, tail="rollout", shift_data=shift_data)
    sol = DeviceSQPOptimizationSolver(mdl, dict(tdc.LOOP_OPTIONS, skip_failed_steps=True), batch=B)
    try:
        mpc.set_stage_data(d); sol.setStageData(d)
        mpc.reset(frame0, reference=arg["p"], x0=x0)
        sol.setInitialGuess(x0)
        if not shift_data:
            with pytest.raises(ValueError, match="shift_data=False"):
                mpc.tick(d_new=d[:, -1])
        lbx, ubx = _dev(arg["lbx"]), _dev(arg["ubx"])
        x2 = _nan(B, mdl.nvar)
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(tdc.LOOP_TICKS):
            dn = d[:, -1] * tdc.RECIPE_GROWTH ** (t + 1)
            sol.getOptimalSolution({"p": arg["p"], "lbx": lbx, "ubx": ubx, "lbg": arg["lbg"], "ubg": arg["ubg"]}, to_host=False)
            status, iters = sol.status.cpu().numpy().copy(), sol.iters.cpu().numpy().copy()
            sol.ev.advance(sol.x, x2, lbx, ubx, status=sol.status, tail="rollout", p=_dev(arg["p"]), stream=stream)
            if shift_data:
                sol.ev.shift_stage_data(_dev(dn), stream=stream)
            sol.x, x2 = x2, sol.x
            out = mpc.tick(d_new=dn) if shift_data else mpc.tick()
            assert np.array_equal(out["status"].cpu().numpy(), status) and np.array_equal(out["iters"].cpu().numpy(), iters), t
            assert np.isin(status, tdc.OK).all(), (t, status)
            assert _bits(mpc.x.cpu().numpy(), sol.x.cpu().numpy()), t
            assert _bits(mpc.lbx.cpu().numpy(), lbx.cpu().numpy()), t
        # what the handle holds afterwards: the grid where it was, or moved up by four frames
        want = d
        if shift_data:
            for t in range(tdc.LOOP_TICKS):
                want = tdc.shift_reference(want, d[:, -1] * tdc.RECIPE_GROWTH ** (t + 1))
        f1 = mpc.ev.merit(mpc.p, mpc.x)[0].cpu().numpy()
        mpc.ev.set_stage_data(want)
        assert _bits(f1, mpc.ev.merit(mpc.p, mpc.x)[0].cpu().numpy())
    finally:
        mpc.close(); sol.close()


# ------------------------------------------------------------------------------------------------ 7. the example
def test_nonuniform_grid_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "nonuniform_grid_mpc.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-800:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith(("non-uniform", "uniform"))]
    print(r.stdout)
    assert len(lines) == 2 and all("frames" in ln and "final cost" in ln and "worst violation" in ln for ln in lines)
    frames = [int(ln.split("frames")[0].split()[-1]) for ln in lines]
    assert frames[0] * 2 < frames[1]
