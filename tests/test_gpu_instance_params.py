"""GPU: per-instance plant parameters (mpcqp_stage_set_instance_params; the PP instances of stage_eval_kernel, stage_merit_kernel,
stage_advance_kernel and stage_linesearch_kernel in csrc/stage_kernels.hpp) against the NumPy statement (models.StageOCP.set_instance_params),
against the shared instances of the same build, the refusals, the two SQP loops, the closed loop, the C++ loop and the example.

Tolerances are the project's: bit for bit for copies, pins, zeros and untouched data; 1e-12 max(1, |ref|) for whatever passes through F (the bar of
tests/test_gpu_stage_eval.py); 1e-6 (1 + max |x|) per iteration for the device loop against the host loop (the bar of tests/test_gpu_linesearch.py).
The CPU side (tests/test_instance_params_host.py) pins the inputs: no line-search decision of the kernel cases sits on its threshold, every QP of
the loop recipes ends solved on the oracle, the instances of the `matters` cases differ by more than 1e-3."""
import os
import subprocess
import sys

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from tests.support import instance_params_cases as ipc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])
ADVANCES = (("rollout", "simulated"), ("repeat", "disturbed"), ("rollout", "measured"), ("rollout", "disturbed"), ("repeat", "simulated"))


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
    """one evaluator (one generated library) per kind for the whole module; every test leaves it without rows"""
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    evs = {}
    yield lambda kind: evs[kind] if kind in evs else evs.setdefault(kind, StageEvaluator(ipc.kernel_case(kind)["model"]))
    for ev in evs.values():
        ev.close()


def _run(ev, case, idx=None, B=None):
    """the four kernels on fresh device copies of the case's instances idx (default: all), NaN-filled outputs; returns host arrays by name.  Whatever
    rows the evaluator holds are in force."""
    mdl = case["model"]
    idx = np.arange(ipc.BATCH if B is None else B) if idx is None else np.asarray(idx)
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
    # line search, K = 4, with a persistent penalty
    lo = {k: _nan(B) for k in ("alpha", "step_max", "f", "gmax")}
    lo["accepted"] = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    phi = _nan(B, 2); xs = _dev(h["x"]); mu = _dev(MU0[idx])
    ev.line_search(_dev(h["p"]), xs, _dev(h["lbx"]), _dev(h["ubx"]), _dev(h["q"]), _dev(h["dw"]), _dev(h["y"]), status=_dev(h["status"], torch.int32), mu=mu,
                   alpha0=1.0, candidates=4, out=lo, phi=phi)
    for k, v in lo.items():
        got["ls_" + k] = v.cpu().numpy()
    got["ls_phi"] = phi.cpu().numpy(); got["ls_x"] = xs.cpu().numpy(); got["ls_mu"] = mu.cpu().numpy()
    # advance
    s_meas = h["x"][:, mdl.f:mdl.f + mdl.nx] * 0.5 + 0.125
    for tail, mode in ADVANCES:
        kw = {"measured": dict(s_meas=s_meas), "disturbed": dict(w=h["w"])}.get(mode, {})
        d = dict(x_out=_nan(B, mdl.nvar), dw_out=_nan(B, mdl.n), y_out=_nan(B, mdl.m), applied=_nan(B, mdl.f), stage_cost=_nan(B))
        dl, du = _dev(h["lbx"]), _dev(h["ubx"])
        if mdl.pref:
            d["p_out"] = _nan(B, mdl.np)
        ev.advance(_dev(h["x"]), d["x_out"], dl, du, status=_dev(h["status"], torch.int32), tail=tail, dw_in=_dev(h["dw"]), dw_out=d["dw_out"], y_in=_dev(h["y"]),
                   y_out=d["y_out"], applied=d["applied"], stage_cost=d["stage_cost"],
                   **({"p_in": _dev(h["p"]), "p_out": d["p_out"]} if mdl.pref else {"p": _dev(h["p"])}), **{k: _dev(v) for k, v in kw.items()})
        for k, v in d.items():
            got["adv_%s_%s_%s" % (tail, mode, k.replace("_out", ""))] = v.cpu().numpy()
        got["adv_%s_%s_lbx" % (tail, mode)] = dl.cpu().numpy(); got["adv_%s_%s_ubx" % (tail, mode)] = du.cpu().numpy()
    torch.cuda.synchronize()
    got["s_meas"] = s_meas
    return got


def _same_bits(a, b, tag, keys=None):
    for k in (keys or a):
        if a[k].dtype.kind == "f":
            assert _bits(a[k], b[k]), (tag, k, np.abs(a[k] - b[k])[np.isfinite(a[k] - b[k])].max(initial=0.0))
        else:
            assert np.array_equal(a[k], b[k]), (tag, k)


# ------------------------------------------------------------------------------------------------ 1. kernels against the statement
@pytest.mark.parametrize("kind", ipc.KINDS)
def test_kernels_match_the_statement(evaluators, kind):
    """every instance with its own row, the unused columns NaN, batch 7"""
    ev = evaluators(kind)
    c = ipc.kernel_case(kind)
    mdl = c["model"]
    B, N, nx, f = ipc.BATCH, mdl.N, mdl.nx, mdl.f
    assert ev.param_count == mdl.ntheta and (ev.n, ev.m, ev.np) == (mdl.n, mdl.m, mdl.np)
    ev.set_instance_params(ipc.padded(c["theta"]))
    ev.set_instance_params(ipc.padded(c["plant"]), plant=True)
    try:
        got = _run(ev, c)
    finally:
        ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    ls = ipc.statement(c, "local_system")
    for k in ("P", "q", "A", "l", "u"):
        assert _close(got[k], getattr(ls, k)), (kind, k)
    fr, gr = ipc.statement(c, "merit")
    assert _close(got["f"], fr) and _close(got["gmax"], gr), kind
    mu = MU0.copy()
    se = ipc.statement(c, "line_search", mu=mu)
    print(kind, "accepted", got["ls_accepted"], "alpha", got["ls_alpha"])
    assert np.array_equal(got["ls_accepted"], se["accepted"]) and np.array_equal(got["ls_alpha"], se["alpha"]), kind
    stay = se["alpha"] == 0.0
    assert _bits(got["ls_x"][stay], c["x"][stay]) and _close(got["ls_x"], se["x"]), kind
    bad = ~np.isin(c["status"], ipc.OK)
    assert _bits(got["ls_mu"][bad], MU0[bad]) and _close(got["ls_mu"], mu), kind
    for k in ("f", "gmax", "phi", "step_max"):
        assert np.isfinite(got["ls_" + k]).all() and _close(got["ls_" + k], se[k]), (kind, k)
    for tail, mode in ADVANCES:
        kw = {"measured": dict(s_meas=got["s_meas"]), "disturbed": dict(w=c["w"])}.get(mode, {})
        ref = ipc.statement(c, "advance", plant=True, tail=tail, **kw)
        tag = (kind, tail, mode)
        pre = "adv_%s_%s_" % (tail, mode)
        G = got[pre + "x"].reshape(B, N, f); R = ref["x"].reshape(B, N, f)
        assert (_bits if mode == "measured" else _close)(G[:, 0, :nx], R[:, 0, :nx]), tag
        assert _bits(G[:, 0, nx:], R[:, 0, nx:]) and _bits(G[:, 1:N - 1], R[:, 1:N - 1]), tag
        assert (_bits if tail == "repeat" else _close)(G[:, N - 1, :nx], R[:, N - 1, :nx]) and _bits(G[:, N - 1, nx:], R[:, N - 1, nx:]), tag
        for k, old in (("lbx", c["lbx"]), ("ubx", c["ubx"])):
            assert _bits(got[pre + k][:, :f], G[:, 0]) and _bits(got[pre + k][:, f:], old[:, f:]), (tag, k)
        for k in ("dw", "y", "applied") + (("p",) if mdl.pref else ()):
            assert _bits(got[pre + k], ref[k]), (tag, k)
        assert _close(got[pre + "stage_cost"], ref["stage_cost"]), tag


# ------------------------------------------------------------------------------------------------ 2. the parameter matters
@pytest.mark.parametrize("kind", ipc.KINDS)
def test_the_parameter_matters(evaluators, kind):
    """two instances with the same x, p and bounds and different rows: the dynamics blocks of A and gmax differ as the statement says they do"""
    ev = evaluators(kind)
    mdl, th, p, x, lbx, ubx, lbg, ubg = ipc.matters_case(kind)
    mdl.set_instance_params(th)
    try:
        ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
        gr = mdl.violation(x, lbx, ubx)[1]
    finally:
        mdl.set_instance_params()
    ev.set_instance_params(ipc.padded(th))
    try:
        out = ev.eval(_dev(p), _dev(x), _dev(lbx), _dev(ubx), _dev(lbg), _dev(ubg))
        g = ev.merit(_dev(p), _dev(x))[1].cpu().numpy()
    finally:
        ev.set_instance_params(None)
    A = out["A"].cpu().numpy()
    blk = mdl._A_blk.ravel()
    assert np.abs(A[0, blk] - A[1, blk]).max() > 1e-3 and abs(g[0] - g[1]) > 1e-3, kind
    assert _close(A, ls.A) and _close(g, gr), kind
    rest = np.setdiff1d(np.arange(A.shape[1]), blk)
    assert _bits(A[0, rest], A[1, rest]) and _bits(out["P"].cpu().numpy()[0], out["P"].cpu().numpy()[1])


# ------------------------------------------------------------------------------------------------ 3. shared values given per instance
@pytest.mark.parametrize("kind", ipc.KINDS)
def test_shared_values_per_instance_are_the_plain_handle(evaluators, kind):
    """every row equal to the handle's shared parameters: all outputs of the four kernels are those of the handle without the call, bit for bit; and
    after theta = NULL the handle is the plain one again"""
    ev = evaluators(kind)
    c = ipc.kernel_case(kind)
    plain = _run(ev, c)
    shared = np.tile(np.asarray(c["model"].theta, float), (ipc.BATCH, 1))
    ev.set_instance_params(ipc.padded(shared))
    try:
        model_only = _run(ev, c)
        ev.set_instance_params(ipc.padded(shared), plant=True)
        both = _run(ev, c)
        ev.set_instance_params(None)
        plant_only = _run(ev, c)
    finally:
        ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    for tag, got in (("model", model_only), ("both", both), ("plant", plant_only)):
        _same_bits(plain, got, (kind, tag))
    # other rows, then NULL: the plain handle again
    ev.set_instance_params(ipc.padded(c["theta"])); ev.set_instance_params(ipc.padded(c["plant"]), plant=True)
    moved = _run(ev, c)
    ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    assert not _bits(moved["A"], plain["A"]) and not _bits(moved["adv_rollout_simulated_x"], plain["adv_rollout_simulated_x"])
    _same_bits(plain, _run(ev, c), (kind, "after NULL"))


# ------------------------------------------------------------------------------------------------ 4. permutation
@pytest.mark.parametrize("kind", ipc.KINDS)
def test_permuting_the_instances_permutes_the_outputs(evaluators, kind):
    ev = evaluators(kind)
    c = ipc.kernel_case(kind)
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    ev.set_instance_params(ipc.padded(c["theta"])); ev.set_instance_params(ipc.padded(c["plant"]), plant=True)
    try:
        base = _run(ev, c)
        again = _run(ev, c)
        ev.set_instance_params(ipc.padded(c["theta"])[perm]); ev.set_instance_params(ipc.padded(c["plant"])[perm], plant=True)
        got = _run(ev, c, idx=perm)
    finally:
        ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    _same_bits(base, again, (kind, "two runs"))
    _same_bits({k: v[perm] for k, v in base.items()}, got, (kind, "permuted"))


# ------------------------------------------------------------------------------------------------ 5. plant against model
@pytest.mark.parametrize("kind", ["quadrotor3", "cartpole70", "pendulum3"])
def test_plant_rows_move_the_plant_step_only(evaluators, kind):
    ev = evaluators(kind)
    c = ipc.kernel_case(kind)
    mdl = c["model"]
    B, N, nx, f = ipc.BATCH, mdl.N, mdl.nx, mdl.f
    ev.set_instance_params(ipc.padded(c["theta"]))
    try:
        model_only = _run(ev, c)
        ev.set_instance_params(ipc.padded(c["plant"]), plant=True)
        both = _run(ev, c)
    finally:
        ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    differs = ipc.SCALES != np.roll(ipc.SCALES, 3)                  # instances whose plant row is another row than their model row
    for tail, mode in (("rollout", "simulated"), ("rollout", "disturbed"), ("repeat", "simulated"), ("repeat", "disturbed")):
        kw = dict(w=c["w"]) if mode == "disturbed" else {}
        pre = "adv_%s_%s_" % (tail, mode)
        tag = (kind, tail, mode)
        G = both[pre + "x"].reshape(B, N, f); M = model_only[pre + "x"].reshape(B, N, f)
        # the first state follows the plant row ... (expected values: the statement with and without the plant rows)
        rp = ipc.statement(c, "advance", plant=True, tail=tail, **kw)["x"].reshape(B, N, f)
        rm = ipc.statement(c, "advance", tail=tail, **kw)["x"].reshape(B, N, f)
        sp, sm, tail_ref = rp[:, 0, :nx], rm[:, 0, :nx], rm[:, N - 1, :nx]
        assert _bits(rp[:, N - 1], rm[:, N - 1])
        assert _close(G[:, 0, :nx], sp) and _close(M[:, 0, :nx], sm), tag
        assert (np.abs(sp - sm).max(axis=1)[differs] > 1e-6).all() and (np.abs(G[:, 0, :nx] - M[:, 0, :nx]).max(axis=1)[differs] > 1e-6).all(), tag
        assert _bits(both[pre + "lbx"][:, :f], G[:, 0]) and _bits(both[pre + "ubx"][:, :f], G[:, 0]), tag
        # ... the rollout tail the model row, and nothing else knows about the plant set
        if tail == "rollout":
            assert _close(G[:, N - 1, :nx], tail_ref), tag
        assert _bits(G[:, 0, nx:], M[:, 0, nx:]) and _bits(G[:, 1:], M[:, 1:]), tag
        _same_bits(model_only, both, tag, keys=[pre + k for k in ("dw", "y", "applied", "stage_cost")])
    # a measured state: the plant set is not read
    _same_bits(model_only, both, (kind, "measured"), keys=[k for k in both if k.startswith("adv_rollout_measured_")])
    _same_bits(model_only, both, (kind, "other kernels"), keys=[k for k in both if not k.startswith("adv_")])


# ------------------------------------------------------------------------------------------------ 6. refusals
def _merit_works(ev, B=2):
    f, g = ev.merit(torch.zeros((B, ev.np), dtype=torch.float64, device="cuda"), torch.zeros((B, ev.nvar), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    return bool(torch.isfinite(f).all())


def test_refusals_leave_the_handle_usable(built, evaluators):
    from optimal_control_problem_amd.stage_eval import StageEvaluator, _bind
    L = _bind(_lib.lib())
    rows = np.ones((4, 8))
    ptr = rows.ctypes.data
    # the double integrator, and a library generated without parameters: MPCQP_ERR_ARG with a message that says why
    for mdl, word in ((models.DoubleIntegrator(3, 0.05), "no parameters"), (ipc.plain_pendulum(), "generated without parameters")):
        ev = StageEvaluator(mdl)
        try:
            assert ev.param_count == 0 and L.mpcqp_stage_param_count(ev._h) == 0
            for which in (0, 1):
                rc = L.mpcqp_stage_set_instance_params(ev._h, which, 4, ptr, _lib.MEM_HOST)
                assert rc == _lib.ERR_ARG and word in L.mpcqp_strerror(rc).decode(), (mdl.name, L.mpcqp_strerror(rc))
            with pytest.raises(_lib.MpcqpError):
                ev.set_instance_params(np.ones((4, 1)))
            assert _merit_works(ev)
        finally:
            ev.close()
    ev = evaluators("cartpole70")
    assert L.mpcqp_stage_param_count(ev._h) == 4 and evaluators("quadrotor2").param_count == 7 and evaluators("pendulum3").param_count == 2
    assert L.mpcqp_stage_param_count(None) == 0
    c = ipc.kernel_case("cartpole70")
    try:
        # a bad `which`, batch <= 0 with rows, a bad mem, a null handle
        for which in (-1, 2):
            assert L.mpcqp_stage_set_instance_params(ev._h, which, 4, ptr, _lib.MEM_HOST) == _lib.ERR_ARG
        for batch in (0, -3):
            assert L.mpcqp_stage_set_instance_params(ev._h, 0, batch, ptr, _lib.MEM_HOST) == _lib.ERR_ARG
        assert L.mpcqp_stage_set_instance_params(ev._h, 0, 4, ptr, 7) == _lib.ERR_ARG
        assert L.mpcqp_stage_set_instance_params(None, 0, 4, ptr, _lib.MEM_HOST) == _lib.ERR_ARG
        assert _merit_works(ev)
        # a launch above the stored batch: refused on all four entries, nothing written; a smaller one uses the first rows
        ev.set_instance_params(ipc.padded(c["theta"])[:4])
        with pytest.raises(_lib.MpcqpError) as e:
            _run(ev, c)
        assert e.value.code == _lib.ERR_ARG and "larger than the stored" in str(e.value)
        B = ipc.BATCH
        p, x = _dev(c["p"]), _dev(c["x"])
        with pytest.raises(_lib.MpcqpError):
            ev.merit(p, x)
        xo = _nan(B, ev.nvar)
        with pytest.raises(_lib.MpcqpError):
            ev.advance(x, xo, _dev(c["lbx"]), _dev(c["ubx"]))
        with pytest.raises(_lib.MpcqpError):
            ev.line_search(p, x, _dev(c["lbx"]), _dev(c["ubx"]), _dev(c["ls"].q), _dev(c["dw"]), _dev(c["y"]))
        torch.cuda.synchronize()
        assert torch.isnan(xo).all() and _bits(x.cpu().numpy(), c["x"])
        ev.set_instance_params(None)
        ev.set_instance_params(ipc.padded(c["plant"])[:4], plant=True)          # the plant set is a stored batch of its own: advance alone minds it
        assert _merit_works(ev, B)
        with pytest.raises(_lib.MpcqpError):
            ev.advance(x, xo, _dev(c["lbx"]), _dev(c["ubx"]))
        ev.set_instance_params(None, plant=True)
        ev.set_instance_params(ipc.padded(c["theta"]))
        full = _run(ev, c)
        first = _run(ev, c, idx=np.arange(3))
        _same_bits({k: v[:3] for k, v in full.items()}, first, "first rows")
        # rows handed over in device memory are the rows handed over from the host
        ev.set_instance_params(_dev(ipc.padded(c["theta"])))
        _same_bits(full, _run(ev, c), "device rows")
        ev.set_instance_params(_dev(c["theta"]))                                # [B, count]: the wrapper pads
        _same_bits(full, _run(ev, c), "padded by the wrapper")
    finally:
        ev.set_instance_params(None); ev.set_instance_params(None, plant=True)
    # tracing an hfun that reads self.theta
    bad = ipc.param_pendulum(cls=ipc.ThetaInPath)
    with pytest.raises(ValueError, match="hfun reads self.theta"):
        StageEvaluator(bad)


# ------------------------------------------------------------------------------------------------ 7. loops
@pytest.mark.parametrize("search", [False, True])
@pytest.mark.parametrize("name", ipc.RECIPES)
def test_device_loop_equals_host_loop(built, name, search):
    """the two recipes: the device loop with the rows against the host loop over the CPU oracle with the rows on the statement, per iteration"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, th, arg = ipc.recipe(name)
    B = th.shape[0]
    host, log = ipc.host_loop(mdl, th, arg, OracleCuCaQP(batch=B, nthreads=4), line_search=search)
    dev = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": ipc.RECIPE_ALPHA, "line_search": search or None}, batch=B)
    try:
        dev.setInstanceParams(th)
        for it in range(ipc.RECIPE_ITERS):
            rd = dev.getOptimalSolution(arg)
            ref = log[it]
            scale = 1.0 + np.abs(ref["x"]).max()
            err = np.abs(rd["x"] - ref["x"]).max()
            print(name, search, it, "max |x_dev - x_host| %.3e" % err, "status", dev.status.cpu().numpy())
            assert np.array_equal(dev.status.cpu().numpy(), ref["status"]), (name, search, it)
            assert err <= 1e-6 * scale, (name, search, it, err)
            assert np.abs(rd["f"] - ref["f"]).max() <= 1e-6 * (1.0 + np.abs(ref["f"]).max())
            if search:
                assert np.array_equal(dev.alpha_taken.cpu().numpy(), ref["alpha"]), (name, it)
        # the rows show: the instances ended at different trajectories, as on the host
        X = rd["x"].reshape(B, mdl.N, mdl.f)
        assert np.abs(X[0, 1, :mdl.nx] - X[-1, 1, :mdl.nx]).max() > 1e-2
        with pytest.raises(ValueError):
            dev.setInstanceParams(th[:-1])
    finally:
        dev.close()


def test_closed_loop_fleet_equals_composed_ticks(built):
    """ClosedLoopMPC, cart-pole N = 10 x 3, four ticks, plant length x {0.6, 1, 1.5} under a nominal controller, against the same ticks composed from
    getOptimalSolution (a second solver, started at every tick from the loop's own state: same inputs, same bits) and the NumPy advance with the
    plant rows, at 1e-12 per tick"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, frame0, plant = ipc.fleet()
    B, nx, f = 3, mdl.nx, mdl.f
    mpc = ClosedLoopMPC(mdl, dict(ipc.FLEET_OPTIONS), batch=B, tail="rollout")
    sol = DeviceSQPOptimizationSolver(mdl, dict(ipc.FLEET_OPTIONS, skip_failed_steps=True), batch=B)
    try:
        with pytest.raises(ValueError):
            mpc.set_instance_params(plant=plant[:2])
        mpc.set_instance_params(plant=plant)
        mpc.reset(frame0)
        ends = []
        for t in range(ipc.FLEET_TICKS):
            lbx, ubx = mpc.lbx.cpu().numpy(), mpc.ubx.cpu().numpy()
            sol.setInitialGuess(mpc.x.clone())
            sol.getOptimalSolution({"p": mpc.p.clone(), "lbx": mpc.lbx.clone(), "ubx": mpc.ubx.clone(), "lbg": mpc.lbg.clone(), "ubg": mpc.ubg.clone()}, to_host=False)
            status = sol.status.cpu().numpy()
            mdl.set_instance_params(None, plant)
            try:
                ref = mdl.advance(sol.x.cpu().numpy(), lbx, ubx, status=status, tail="rollout", p=np.zeros((B, nx)))
            finally:
                mdl.set_instance_params()
            out = mpc.tick()
            assert np.array_equal(out["status"].cpu().numpy(), status) and np.isin(status, ipc.OK).all(), t
            assert _close(mpc.x.cpu().numpy(), ref["x"]), (t, np.abs(mpc.x.cpu().numpy() - ref["x"]).max())
            assert _close(mpc.lbx.cpu().numpy(), ref["lbx"]) and _close(mpc.ubx.cpu().numpy(), ref["ubx"]), t
            assert _bits(out["applied"].cpu().numpy(), ref["applied"]) and _close(out["stage_cost"].cpu().numpy(), ref["stage_cost"]), t
            ends.append(mpc.x.cpu().numpy()[:, :nx].copy())
        # the plants are different plants: the nominal controller sees three different measured states
        assert np.abs(ends[-1][0] - ends[-1][2]).max() > 1e-3 and np.abs(ends[-1][0] - ends[-1][1]).max() > 1e-3
        # and with the nominal row the plant is the plain one, bit for bit
        mpc.set_instance_params(plant=np.tile(mdl.theta, (B, 1)))
        mpc.reset(frame0)
        mpc.tick(); a = mpc.x.cpu().numpy().copy()
        mpc.set_instance_params()
        mpc.reset(frame0)
        mpc.tick()
        assert _bits(a, mpc.x.cpu().numpy())
    finally:
        mpc.close(); sol.close()


CPP_EXE = os.path.join(ROOT, "tests", "support", "stagesqp_params_test")


def test_cpp_stage_sqp_with_instance_params(built):
    """cpp/StageSQP.hpp with setInstanceParams against the Python device loop on the cart-pole recipe (tests/support/stagesqp_params_test.cpp)"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    r = subprocess.run([CPP_EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "StageSQP instance params ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr)
    xs = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "x":
            xs[int(w[1])] = np.array([float(v) for v in w[2:]])
    mdl, th, arg = ipc.recipe("cartpole")
    B = th.shape[0]
    x_cpp = np.stack([xs[b] for b in range(B)])
    dev = DeviceSQPOptimizationSolver(mdl, {"max_iter": ipc.RECIPE_ITERS, "alpha": ipc.RECIPE_ALPHA}, batch=B)
    try:
        dev.setInstanceParams(th)
        rd = dev.getOptimalSolution(arg)
        assert x_cpp.shape == rd["x"].shape
        assert np.abs(x_cpp - rd["x"]).max() <= 1e-6 * (1.0 + np.abs(rd["x"]).max())
        dev.setInstanceParams(None)
        dev.setInitialGuess(np.zeros(mdl.nvar))
        plain = dev.getOptimalSolution(arg)
        assert np.abs(x_cpp - plain["x"]).max() > 1e-2          # (the program did hand its rows over)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 8. the example
def test_fleet_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fleet_mpc.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-800:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("plant ")]
    assert len(lines) == 8
    costs = np.array([float(ln.split("closed-loop cost")[1].split()[0]) for ln in lines])
    assert np.isfinite(costs).all() and len(np.unique(costs)) == 8
