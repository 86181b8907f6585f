"""GPU: the feedback gains along the plan (mpcqp_stage_riccati, mpcqp_stage_feedback; csrc/stage_riccati.hpp) against their NumPy statements
(models.StageOCP.riccati_gains / feedback), their bitwise promises and refusals, and the layers built on them: StageEvaluator.riccati / feedback,
DeviceSQPOptimizationSolver.feedbackGains, ClosedLoopMPC(feedback=...).hold, a captured graph, and the recipe of tests/test_riccati_host.py.

Tolerances.  K and V are compared with the statement at rc.DEVICE_BAR = max(1e-12, 16 e_np) relative to max(1, max |ref|), e_np the statement's own
error against 60 digits (tests/test_riccati_host.py measures it: 1.7e-15, so the bar is 1e-12): the device runs the statement's operations in another
summation order and with fused multiply-adds.  `failed` is compared exactly.  The feedback kernel rounds every product and sum on its own, in the
statement's order (fp contraction is off in that kernel), so it is compared bit for bit."""
import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import riccati_cases as rc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

bits = rc.bits
KINDS = ("double_integrator", "cartpole", "quadrotor", "linear13x4", "linear16x8")      # f = 3, 5, 16 (a full group of 16), 17, 24
_EV = {}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _ev(name, N):
    """one evaluator per (model, horizon), shared by the tests of this file and closed with the process"""
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    if (name, N) not in _EV:
        _EV[(name, N)] = StageEvaluator(rc.model(name, N))
    return _EV[(name, N)]


def _batches(f):
    from optimal_control_problem_amd.stage_eval import riccati_groups_per_block
    G = riccati_groups_per_block(f)
    return (1, G - 1, G, G + 1, 2 * G + 1)


def _run(ev, d, fill=float("nan"), **kw):
    """riccati on NaN-filled outputs: dict of NumPy K, V, failed"""
    B = d["P"].shape[0]
    K = torch.full((B, ev.horizon, ev.nu, ev.nx), fill, dtype=torch.float64, device="cuda")
    V = torch.full((B, ev.horizon, ev.nx, ev.nx), fill, dtype=torch.float64, device="cuda")
    failed = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    for key in ("x", "lbx", "ubx"):
        if key in kw:
            kw[key] = _dev(kw[key])
    if "frozen" in kw:
        kw["frozen"] = _dev(kw["frozen"], torch.int32)
    ev.riccati(_dev(d["P"]), _dev(d["A"]), K=K, V=V, failed=failed, **kw)
    torch.cuda.synchronize()
    return {"K": K.cpu().numpy(), "V": V.cpu().numpy(), "failed": failed.cpu().numpy()}


@pytest.mark.parametrize("N", rc.HORIZONS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity(built, kind, N):
    mdl, ev = rc.model(kind, N), _ev(kind, N)
    assert (ev.library is not None) == kind.startswith("linear")
    worst = 0.0
    for B in _batches(mdl.f):
        if B < 1:
            continue
        for data in ("local", "random"):
            d = rc.local_data(mdl, B) if data == "local" else rc.random_data(mdl, B)
            for kw in ({}, dict(x=d["x"], lbx=d["lbx"], ubx=d["ubx"], clamp_tol=1e-9, reg=1e-3) if data == "local" else dict(reg=0.5)):
                got = _run(ev, d, **dict(kw))
                ref = mdl.riccati_gains(d["P"], d["A"], **kw)
                tag = (kind, N, B, data, sorted(kw))
                assert np.array_equal(got["failed"], ref["failed"]) and (got["failed"] == -1).all(), tag
                assert np.isfinite(got["K"]).all() and np.isfinite(got["V"]).all(), tag
                eK, eV = rc.rel_err(got["K"], ref["K"]), rc.rel_err(got["V"], ref["V"])
                worst = max(worst, eK, eV)
                assert eK <= rc.DEVICE_BAR and eV <= rc.DEVICE_BAR, (tag, eK, eV)
                assert _same(got["V"], got["V"].transpose(0, 1, 3, 2)), tag              # symmetric bit for bit
                if "x" in kw:
                    assert (got["K"][:, 0] == 0.0).all(), tag                            # the pinned first frame
    print(kind, N, "worst error / bar", worst / rc.DEVICE_BAR)


@pytest.mark.parametrize("kind", ("quadrotor", "linear13x4"))
def test_bitwise_promises(built, kind):
    """a repeat launch; an instance alone = the instance at any position of a larger batch; frozen rows and guard rows keep their NaN; the frames above
    a failed one are the unmodified run's; a clamped row is exactly 0"""
    N = 20
    mdl, ev = rc.model(kind, N), _ev(kind, N)
    B = 11
    d = rc.local_data(mdl, B)
    ref = _run(ev, d)
    again = _run(ev, d)
    assert _same(ref["K"], again["K"]) and _same(ref["V"], again["V"])
    for b in (0, 3, 4, 10):
        one = _run(ev, {"P": d["P"][b:b + 1], "A": d["A"][b:b + 1]})
        assert _same(one["K"][0], ref["K"][b]) and _same(one["V"][0], ref["V"][b]), b
    # frozen rows, and guard rows around the outputs
    frozen = np.zeros(B, np.int32); frozen[[2, 7, 10]] = (1, -3, 9)
    K = torch.full((B + 2, N, ev.nu, ev.nx), float("nan"), dtype=torch.float64, device="cuda")
    V = torch.full((B + 2, N, ev.nx, ev.nx), float("nan"), dtype=torch.float64, device="cuda")
    fl = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    ev.riccati(_dev(d["P"]), _dev(d["A"]), frozen=_dev(frozen, torch.int32), K=K[1:B + 1], V=V[1:B + 1], failed=fl[1:B + 1])
    torch.cuda.synchronize()
    Kh, Vh, fh = K.cpu().numpy(), V.cpu().numpy(), fl.cpu().numpy()
    fz = np.concatenate([[True], frozen != 0, [True]])
    assert np.isnan(Kh[fz]).all() and np.isnan(Vh[fz]).all() and (fh[fz] == -7).all()
    assert _same(Kh[~fz], ref["K"][frozen == 0]) and _same(Vh[~fz], ref["V"][frozen == 0]) and (fh[~fz] == -1).all()
    # failure: an indefinite (then a NaN) diagonal slot in frame k of two instances
    ps, _ = mdl._riccati_slots()
    # (the linear model's B' V B exceeds 1 on the diagonal, so -1 would leave its Q_uu positive definite: its slot is set to -1000)
    for bad in (-1.0 if kind == "quadrotor" else -1000.0, float("nan")):
        k = 11
        P = d["P"].copy()
        P[[1, 6], ps[k, mdl.nx + 1, mdl.nx + 1]] = bad
        got = _run(ev, {"P": P, "A": d["A"]})
        st = mdl.riccati_gains(P, d["A"])
        assert np.array_equal(got["failed"], st["failed"]) and got["failed"].tolist() == [k if b in (1, 6) else -1 for b in range(B)]
        for b in (1, 6):
            assert (got["K"][b, :k + 1] == 0.0).all() and (got["V"][b, :k + 1] == 0.0).all()
            assert _same(got["K"][b, k + 1:], ref["K"][b, k + 1:]) and _same(got["V"][b, k + 1:], ref["V"][b, k + 1:])
        keep = [b for b in range(B) if b not in (1, 6)]
        assert _same(got["K"][keep], ref["K"][keep]) and _same(got["V"][keep], ref["V"][keep])
    # clamp: an input on its bound in frame 7
    k, i = 7, mdl.nu - 1
    ubx = d["ubx"].copy()
    ubx[:, k * mdl.f + mdl.nx + i] = d["x"][:, k * mdl.f + mdl.nx + i]
    got = _run(ev, d, x=d["x"], lbx=d["lbx"], ubx=ubx)
    assert (got["K"][:, k, i] == 0.0).all() and (got["K"][:, 0] == 0.0).all() and np.abs(ref["K"][:, k, i]).max() > 0.0
    assert _same(got["K"][:, k + 1:], ref["K"][:, k + 1:])


def test_feedback_kernel_is_the_statement_bit_for_bit(built):
    N = 3
    mdl, ev = rc.model("quadrotor", N), _ev("quadrotor", N)
    nx, nu, f = mdl.nx, mdl.nu, mdl.f
    for B in (1, 63, 64, 65, 300):                     # one thread per (instance, input): across the 256-thread workgroup
        rng = np.random.default_rng(B)
        K = rng.normal(0.0, 0.1, size=(B, N, nu, nx))
        traj = rng.normal(size=(B, mdl.nvar)); plan = 0.3 * rng.normal(size=(B, mdl.nvar))
        lbx = traj - 1.0; ubx = traj + 1.0
        lbx[:, f + nx:2 * f] = -0.4; ubx[:, f + nx:2 * f] = 0.4          # frame 1's input box: some corrections are clipped
        s, sn, un = traj[:, :nx], plan[:, f:f + nx], plan[:, f + nx:2 * f]
        ref = mdl.feedback(K, 1, s, sn, un, lo=lbx[:, f + nx:2 * f], hi=ubx[:, f + nx:2 * f], x=traj, lbx=lbx, ubx=ubx)
        assert B == 1 or ((np.abs(ref["u"]) == 0.4).any() and (np.abs(ref["u"]) < 0.4).any())
        tx, tp, tl, tu = _dev(traj), _dev(plan), _dev(lbx), _dev(ubx)
        du = torch.full((B, nu), float("nan"), dtype=torch.float64, device="cuda")
        # the rows are views into the trajectory and bound arrays: no copies
        ev.feedback(_dev(K), 1, tx[:, :nx], tp[:, f:f + nx], tp[:, f + nx:2 * f], tx, lo=tl[:, f + nx:2 * f], hi=tu[:, f + nx:2 * f], lbx=tl, ubx=tu, du=du)
        torch.cuda.synchronize()
        assert _same(tx.cpu().numpy(), ref["x"]) and _same(tl.cpu().numpy(), ref["lbx"]) and _same(tu.cpu().numpy(), ref["ubx"]), B
        assert _same(du.cpu().numpy(), ref["du"]), B
        # without the box and the pins
        tx2 = _dev(traj)
        ev.feedback(_dev(K), 2, _dev(s), _dev(sn), _dev(un), tx2)
        torch.cuda.synchronize()
        assert _same(tx2.cpu().numpy(), mdl.feedback(K, 2, s, sn, un, x=traj)["x"]), B


def _problem(mdl, B, seed=5):
    rng = np.random.default_rng(seed)
    frame0 = np.zeros((B, mdl.f))
    frame0[:, :mdl.nx] = rng.uniform(-0.05, 0.05, size=(B, mdl.nx))
    return frame0


def test_feedback_gains_of_the_solver(built):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl = rc.model("double_integrator", 20)
    B = 6
    frame0 = _problem(mdl, B)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 2, "alpha": 1.0}, batch=B)
    try:
        with pytest.raises(RuntimeError):
            sol.feedbackGains()
        sol.getOptimalSolution(arg)
        g = sol.feedbackGains()
        ref = sol.ev.riccati(sol.ls)
        gc = sol.feedbackGains(arg, clamp_tol=1e-9)
        refc = sol.ev.riccati(sol.ls, x=sol.x, lbx=_dev(lbx), ubx=_dev(ubx), clamp_tol=1e-9)
        torch.cuda.synchronize()
        for a, b in ((g, ref), (gc, refc)):
            assert _same(a["K"].cpu().numpy(), b["K"].cpu().numpy()) and _same(a["V"].cpu().numpy(), b["V"].cpu().numpy())
            assert (a["failed"].cpu().numpy() == -1).all()
        assert (gc["K"][:, 0].cpu().numpy() == 0.0).all() and np.abs(g["K"][:, 0].cpu().numpy()).max() > 0.0
        # against the statement on the same system
        st = mdl.riccati_gains(sol.ls["P"].cpu().numpy(), sol.ls["A"].cpu().numpy())
        assert rc.rel_err(g["K"].cpu().numpy(), st["K"]) <= rc.DEVICE_BAR
    finally:
        sol.close()


def test_general_path_refuses_feedback_gains():
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    fake = DeviceSQPOptimizationSolver.__new__(DeviceSQPOptimizationSolver)
    fake.ev = object(); fake._have_start = True          # an evaluator= of the general path has no riccati
    with pytest.raises(ValueError) as e:
        fake.feedbackGains()
    assert "general evaluator" in str(e.value)


def _composed(mdl, frame0, steps, dist, feedback):
    """the ticks and holds of ClosedLoopMPC composed by hand from getOptimalSolution, ev.riccati, ev.advance and ev.feedback"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B, nx, f = frame0.shape[0], mdl.nx, mdl.f
    sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 1.0, "skip_failed_steps": True}, batch=B)
    assert not sol.warm_start_admm
    ev = sol.ev
    lbx, ubx, lbg, ubg = [_dev(v) for v in mdl.stacked_bounds(frame0)]
    p = torch.zeros((B, ev.np), dtype=torch.float64, device="cuda")
    x2 = torch.zeros((B, ev.nvar), dtype=torch.float64, device="cuda")
    applied = torch.zeros((B, f), dtype=torch.float64, device="cuda"); cost = torch.zeros(B, dtype=torch.float64, device="cuda")
    du = torch.zeros((B, ev.nu), dtype=torch.float64, device="cuda")
    sol.setInitialGuess(np.zeros(ev.nvar))
    g, age, log = None, 0, []
    try:
        for step, w in zip(steps, dist):
            wd = None if w is None else _dev(w)
            if step == "tick":
                sol.getOptimalSolution({"p": p, "lbx": lbx, "ubx": ubx, "lbg": lbg, "ubg": ubg}, to_host=False)
                if feedback:
                    g = ev.riccati(sol.ls, x=sol.x, lbx=lbx, ubx=ubx, V=False)
                ev.advance(sol.x, x2, lbx, ubx, status=sol.status, w=wd, tail="rollout", p=p, applied=applied, stage_cost=cost)
                age = 0
            else:
                ev.advance(sol.x, x2, lbx, ubx, status=None, w=wd, tail="rollout", p=p, applied=applied, stage_cost=cost)
                ev.feedback(g["K"], age + 1, x2[:, :nx], sol.x[:, f:f + nx], sol.x[:, f + nx:2 * f], x2, lo=lbx[:, f + nx:2 * f],
                            hi=ubx[:, f + nx:2 * f], lbx=lbx, ubx=ubx, du=du)
                age += 1
            sol.x, x2 = x2, sol.x
            torch.cuda.synchronize()
            log.append(dict(applied=applied.cpu().numpy().copy(), x=sol.x.cpu().numpy().copy(), lbx=lbx.cpu().numpy().copy(),
                            cost=cost.cpu().numpy().copy(), du=du.cpu().numpy().copy()))
        return log, (None if g is None else {k: v.cpu().numpy() for k, v in g.items() if v is not None})
    finally:
        sol.close()


def test_closed_loop_tick_hold_hold_tick_is_the_composed_loop(built):
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl = rc.model("double_integrator", 20)
    B = 5
    frame0 = _problem(mdl, B)
    rng = np.random.default_rng(8)
    steps = ("tick", "hold", "hold", "tick")
    dist = (None, rng.normal(0.0, 0.02, size=(B, mdl.nx)), None, rng.normal(0.0, 0.02, size=(B, mdl.nx)))
    ref, g = _composed(mdl, frame0, steps, dist, True)
    mpc = ClosedLoopMPC(mdl, batch=B, feedback=True)
    try:
        mpc.reset(frame0)
        with pytest.raises(RuntimeError):
            mpc.hold()                                 # no plan yet
        for i, (step, w) in enumerate(zip(steps, dist)):
            out = mpc.tick(disturbance=w) if step == "tick" else mpc.hold(disturbance=w)
            torch.cuda.synchronize()
            assert _same(out["applied"].cpu().numpy(), ref[i]["applied"]) and _same(mpc.x.cpu().numpy(), ref[i]["x"]), (i, step)
            assert _same(mpc.lbx.cpu().numpy(), ref[i]["lbx"]) and _same(out["stage_cost"].cpu().numpy(), ref[i]["cost"]), (i, step)
            if step == "hold":
                assert _same(out["du"].cpu().numpy(), ref[i]["du"]), i
            assert mpc.age == (0, 1, 2, 0)[i]
        assert _same(mpc.K.cpu().numpy(), g["K"]) and (mpc.gain_failed.cpu().numpy() == -1).all()
        assert np.abs(ref[1]["du"]).max() > 0.0        # the disturbed hold was corrected
    finally:
        mpc.close()


def test_closed_loop_without_the_option_is_unchanged(built, monkeypatch):
    """five ticks without feedback= are bitwise the ticks composed from getOptimalSolution and ev.advance -- the parent's tick -- and launch neither of
    the new kernels: both entry points are replaced by a function that fails the test"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    mdl = rc.model("double_integrator", 20)
    B = 5
    frame0 = _problem(mdl, B)
    steps, dist = ("tick",) * 5, (None,) * 5
    ref, _ = _composed(mdl, frame0, steps, dist, False)

    def boom(*a, **k):
        raise AssertionError("a tick without feedback= launched a Riccati or feedback kernel")

    monkeypatch.setattr(StageEvaluator, "riccati", boom); monkeypatch.setattr(StageEvaluator, "feedback", boom)
    mpc = ClosedLoopMPC(mdl, batch=B)
    try:
        assert mpc.feedback is None and not hasattr(mpc, "K")
        mpc.reset(frame0)
        for i in range(5):
            out = mpc.tick()
            torch.cuda.synchronize()
            assert _same(out["applied"].cpu().numpy(), ref[i]["applied"]) and _same(mpc.x.cpu().numpy(), ref[i]["x"]), i
        with pytest.raises(ValueError) as e:
            mpc.hold()
        assert "feedback=True" in str(e.value)
    finally:
        mpc.close()


def test_hold_refusals(built):
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl = rc.model("double_integrator", 3)
    frame0 = _problem(mdl, 2)
    mpc = ClosedLoopMPC(mdl, batch=2, feedback={"clamp_tol": 1e-9, "reg": 1e-6}, shift=False)
    try:
        mpc.reset(frame0); mpc.tick()
        with pytest.raises(ValueError) as e:
            mpc.hold()
        assert "shift=False" in str(e.value)
    finally:
        mpc.close()
    mpc = ClosedLoopMPC(mdl, batch=2, feedback=True)
    try:
        mpc.reset(frame0); mpc.tick()
        mpc.hold()                                     # N = 3: frame 1 is the only one a hold may use
        with pytest.raises(ValueError) as e:
            mpc.hold()
        assert "exhausted" in str(e.value)
        mpc.tick(); mpc.hold()                         # a tick resets the age
    finally:
        mpc.close()


def test_captured_graph_replays_after_a_first_plain_call(built):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    N = 20
    mdl = rc.model("cartpole", N)
    ev = StageEvaluator(mdl)                           # a fresh handle: its slot tables are not built yet
    try:
        B, nx, f = 9, mdl.nx, mdl.f
        d = rc.local_data(mdl, B)
        P, A = _dev(d["P"]), _dev(d["A"])
        K = torch.zeros((B, N, ev.nu, ev.nx), dtype=torch.float64, device="cuda"); V = torch.zeros((B, N, ev.nx, ev.nx), dtype=torch.float64, device="cuda")
        fl = torch.zeros(B, dtype=torch.int32, device="cuda")
        rng = np.random.default_rng(4)
        traj, plan = _dev(rng.normal(size=(B, ev.nvar))), _dev(rng.normal(size=(B, ev.nvar)))
        s = torch.cuda.Stream(); g0 = torch.cuda.CUDAGraph(); g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g0, stream=s):
                fl.fill_(-5)
                with pytest.raises(_lib.MpcqpError) as e:      # the first call would allocate: refused under capture, with the reason
                    ev.riccati(P, A, K=K, V=V, failed=fl, stream=s.cuda_stream)
            assert e.value.code == _lib.ERR_STATE and "capturing" in str(e.value)
            ev.riccati(P, A, K=K, V=V, failed=fl, stream=s.cuda_stream)
            ev.feedback(K, 1, traj[:, :nx], plan[:, f:f + nx], plan[:, f + nx:2 * f], traj, stream=s.cuda_stream)
            s.synchronize()
            ref = (K.cpu().numpy().copy(), V.cpu().numpy().copy(), traj.cpu().numpy().copy())
            with torch.cuda.graph(g, stream=s):
                ev.riccati(P, A, K=K, V=V, failed=fl, stream=s.cuda_stream)
                ev.feedback(K, 1, traj[:, :nx], plan[:, f:f + nx], plan[:, f + nx:2 * f], traj, stream=s.cuda_stream)
            K.fill_(-1.0); V.fill_(-1.0); fl.fill_(-7); traj[:, nx:f] = -1.0
            g.replay(); s.synchronize()
        assert _same(K.cpu().numpy(), ref[0]) and _same(V.cpu().numpy(), ref[1]) and _same(traj.cpu().numpy(), ref[2])
        assert (fl.cpu().numpy() == -1).all()
    finally:
        ev.close()


def test_recipe_on_the_device(built):
    """the recipe of tests/test_riccati_host.py on the device loop: solve, then four holds with an impulse on the first; in EVERY instance the
    plant ends nearer the plan with the gains than with open-loop holds"""
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    mdl, frame0, w = rc.recipe()
    B, nx, f = rc.RECIPE_B, mdl.nx, mdl.f
    dev = {}
    for gains in (True, False):
        sol = DeviceSQPOptimizationSolver(mdl, {"max_iter": rc.RECIPE_SQP_ITERS, "alpha": 1.0}, batch=B)
        try:
            ev = sol.ev
            lbx, ubx, lbg, ubg = [_dev(v) for v in mdl.stacked_bounds(frame0)]
            arg = {"p": torch.zeros((B, ev.np), dtype=torch.float64, device="cuda"), "lbx": lbx, "ubx": ubx, "lbg": lbg, "ubg": ubg}
            sol.getOptimalSolution(arg, to_host=False)
            plan = sol.x.clone()
            g = sol.feedbackGains(arg)
            x, x2 = sol.x.clone(), torch.zeros_like(sol.x)
            for h in range(rc.RECIPE_HOLDS):
                ev.advance(x, x2, lbx, ubx, status=None, w=_dev(w) if h == 0 else None, tail="rollout", p=arg["p"])
                if gains:
                    ev.feedback(g["K"], h + 1, x2[:, :nx], x[:, f:f + nx], x[:, f + nx:2 * f], x2, lo=lbx[:, f + nx:2 * f], hi=ubx[:, f + nx:2 * f],
                                lbx=lbx, ubx=ubx)
                x, x2 = x2, x
            torch.cuda.synchronize()
            assert (g["failed"].cpu().numpy() == -1).all()
            dev[gains] = rc.recipe_deviation(plan.cpu().numpy(), x.cpu().numpy(), rc.RECIPE_HOLDS)
        finally:
            sol.close()
    print("deviation with gains", dev[True], "open loop", dev[False], "ratio", dev[True] / dev[False])
    assert (dev[True] < dev[False]).all() and (dev[True] / dev[False]).max() < 0.5


def test_refusals(built):
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    from tests.support import convexify_cases as cc
    N = 3
    mdl, ev = rc.model("double_integrator", N), _ev("double_integrator", N)
    d = rc.local_data(mdl, 2)
    P, A, x, lbx, ubx = [_dev(d[k]) for k in ("P", "A", "x", "lbx", "ubx")]
    K = torch.zeros((2, N, ev.nu, ev.nx), dtype=torch.float64, device="cuda")
    for kw in (dict(x=x), dict(x=x, lbx=lbx), dict(lbx=lbx, ubx=ubx)):
        with pytest.raises(ValueError):
            ev.riccati(P, A, **kw)
    for kw in (dict(clamp_tol=-1.0), dict(reg=-1.0), dict(reg=float("nan"))):
        with pytest.raises(_lib.MpcqpError) as e:
            ev.riccati(P, A, **kw)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        ev.riccati(P)                                  # P without A
    with pytest.raises(ValueError):
        ev.riccati(P[:, :-1].contiguous(), A)
    with pytest.raises(ValueError):
        ev.riccati(P, A, K=K[:, :2].contiguous())
    # the feedback launch
    z = torch.zeros((2, ev.nx), dtype=torch.float64, device="cuda"); u = torch.zeros((2, ev.nu), dtype=torch.float64, device="cuda")
    for k in (-1, N):
        with pytest.raises(_lib.MpcqpError) as e:
            ev.feedback(K, k, z, z, u, x)
        assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        ev.feedback(K, 0, z, z, u, x, lo=u)
    with pytest.raises(ValueError):
        ev.feedback(K, 0, z, z, u, x, lbx=lbx)
    with pytest.raises(ValueError):
        ev.feedback(K, 0, x[:, ::2][:, :ev.nx], z, u, x)      # rows that are not contiguous
    # a link cost couples neighbouring frames: refused with the reason
    link = cc.case("bump_link")["model"]
    evl = StageEvaluator(link)
    try:
        with pytest.raises(_lib.MpcqpError) as e:
            evl.riccati(torch.zeros((1, evl.nnzP), dtype=torch.float64, device="cuda"), torch.zeros((1, evl.nnzA), dtype=torch.float64, device="cuda"))
        assert e.value.code == _lib.ERR_LIMIT and "link cost" in str(e.value)
    finally:
        evl.close()
