"""CPU: the exact Lagrangian Hessian -- the NumPy statement (models.StageOCP.constraint_curvature, lagrangian_system) against a 60-digit restatement,
the pattern, the generated source, the refusals, the generated functors FG / HG through a stand-alone host program, and the SQP recipe on the CPU oracle.
These pin the inputs of tests/test_gpu_exact_hessian.py.

The restatement takes second central differences of y'c(w) in mpmath arithmetic, frame by frame, with the scalar machinery of tests/support/nlp_hp.py
(its callbacks-on-one-frame and its differencing; nothing of the package's tapes).  Bars: mode = None at 1e-12 relative to max(1, |ref|), what DESIGN
6.17 uses for P; what passes through the eigen-solve at 1e-12 max(1, ||H_k^L||_F), DESIGN 6.16's."""
import os
import subprocess

import numpy as np
import pytest
from mpmath import mp, mpf

from optimal_control_problem_amd import _lib, codegen, models
from tests.support import exact_hessian_cases as ec
from tests.support import nlp_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
_REF = {}


def restated(name):
    """dict C [B, N, f, f] (float64 of the 60-digit values), HL [B, N, nl, nl] = frame Hessian of the cost + C, and per mode the corrections
    D [B, N, nl, nl] (zero where untouched), lam_min [B, N]: second central differences of y'c over [s_k; u_k], and of the frame term over [s; u; r]"""
    if name in _REF:
        return _REF[name]
    c = ec.case(name)
    mdl = c["model"]
    st = nlp_hp.Stage(mdl, theta=c["theta"], sdata=c["d"])
    N, nx, f, nh, n = mdl.N, mdl.nx, mdl.f, mdl.nh, mdl.n
    nl = f + nx
    Bn = c["x"].shape[0]
    C = np.zeros((Bn, N, f, f)); HL = np.zeros((Bn, N, nl, nl))
    D = {m: np.zeros((Bn, N, nl, nl)) for m in ec.MODES}
    lam_min = np.zeros((Bn, N))
    with mp.workdps(st.dps):
        h = mpf(st.step)
        e = mpf(ec.EPS)
        for b in range(Bn):
            m = st._model(b)
            w = st._w(c["p"], c["x"], b)
            y = nlp_hp._mpfs(c["y"][b])
            for k in range(N):
                z = [w[i] for i in st._x_idx(k)]

                def yc(v, k=k):
                    """the terms of y'c that depend on frame k: the dynamics rows of stage k (s_{k+1} held) and the path rows of frame k"""
                    acc = mpf(0)
                    if k < N - 1:
                        nxt = [w[i] for i in st._x_idx(k + 1)[:nx]]
                        for i, g in enumerate(st._dyn(m, list(v) + nxt)):
                            acc += y[n + k * nx + i] * g
                    if nh:
                        for i, g in enumerate(st._path(m, b, k, list(v))):
                            acc += y[n + (N - 1) * nx + k * nh + i] * g
                    return acc

                _, _, Hc = nlp_hp.grad_hess(yc, z, h)
                zl = [w[i] for i in st._frame_idx(k)]
                _, _, Hf = st._frame_hess(m, b, k, zl, h)
                H = [[Hf[r][q] + (Hc[r][q] if r < f and q < f else mpf(0)) for q in range(nl)] for r in range(nl)]
                C[b, k] = nlp_hp._f64(Hc); HL[b, k] = nlp_hp._f64(H)
                if not mdl.convexify:
                    continue
                E, Q = mp.eigsy(mp.matrix(H))
                lam = [E[j] for j in range(nl)]
                lam_min[b, k] = float(min(lam))
                if not min(lam) < e:
                    continue
                for mode in ec.MODES:
                    add = [[mpf(0)] * nl for _ in range(nl)]
                    for j in range(nl):
                        if lam[j] < e:
                            t = max(abs(lam[j]) if mode == "mirror" else lam[j], e) - lam[j]
                            for r in range(nl):
                                for q in range(nl):
                                    add[r][q] += t * Q[r, j] * Q[q, j]
                    D[mode][b, k] = nlp_hp._f64(add)
    _REF[name] = dict(C=C, HL=HL, D=D, lam_min=lam_min)
    return _REF[name]


def scatter(mdl, blocks, nb):
    """dense [n, n] of frame blocks [N, nb, nb] over [s; u] (nb = f) or [s; u; r] (nb = nl) at their indices of w"""
    out = np.zeros((mdl.n, mdl.n))
    for k in range(mdl.N):
        idx = [mdl.np + k * mdl.f + i for i in range(mdl.f)] + [(k * mdl.nx if mdl.pref else 0) + i for i in range(mdl.nx)]
        idx = idx[:nb]
        out[np.ix_(idx, idx)] += blocks[k]
    return out


def dense_P(mdl, Pv):
    D = np.zeros((mdl.n, mdl.n))
    for j in range(mdl.n):
        D[mdl.Pi[mdl.Pp[j]:mdl.Pp[j + 1]], j] = Pv[mdl.Pp[j]:mdl.Pp[j + 1]]
    return D


# ------------------------------------------------------------------------------------------------ 1. the inputs
@pytest.mark.parametrize("name", ec.CASES)
def test_case_inputs(name):
    c = ec.case(name)
    y = c["y"]
    assert (y > 0).any() and (y < 0).any() and (y == 0.0).any()
    assert not np.isin(c["status"][3], models.StageOCP.STATUS_OK) and np.isin(np.delete(c["status"], 3), models.StageOCP.STATUS_OK).all()
    assert np.abs(c["C"]).max() > 0.1
    if name == "pend2":      # frame 0 is the only one with dynamics curvature, the last frame has path curvature only
        mdl = c["model"]
        y0 = y.copy(); y0[:, mdl.n + mdl.ngd:] = 0.0
        Cd = ec.with_data(c, lambda: mdl.constraint_curvature(c["x"], y0))
        assert np.abs(Cd[:, 0]).max() > 1e-3 and not Cd[:, 1].any()
    if name in ec.CONVEXIFY_CASES:      # no eigenvalue of H_k^L sits near eps: the touched counts do not depend on rounding
        lam = np.linalg.eigvalsh(0.5 * (c["HL"] + np.swapaxes(c["HL"], 2, 3)))[..., 0]
        assert (np.abs(lam - ec.EPS) >= 1e-6 * np.maximum(1.0, c["hnorm"])).all()


def test_cvx_case_has_indefinite_and_positive_frames():
    """the curvature makes frames of `cvx` indefinite though its cost is convex everywhere, and leaves others positive: checked here, on the statement"""
    c = ec.case("cvx")
    lam_cost = np.linalg.eigvalsh(c["hess"])[..., 0]
    lam = np.linalg.eigvalsh(0.5 * (c["HL"] + np.swapaxes(c["HL"], 2, 3)))[..., 0]
    assert (lam_cost > ec.EPS).all()
    ok = np.isin(c["status"], models.StageOCP.STATUS_OK)
    assert (lam[ok] < -1.0).any() and (lam[ok] > ec.EPS).any()
    assert ((lam[0] < ec.EPS).any() and (lam[0] > ec.EPS).any())      # one instance holds both kinds
    assert (lam[4] > ec.EPS).all()                                   # and one instance stays convex in every frame
    _, touched, _ = ec.statement(c, "project")
    assert np.array_equal(touched, np.where(ok, (lam < ec.EPS).sum(axis=1), 0))


# ------------------------------------------------------------------------------------------------ 2. the statement against the restatement
@pytest.mark.parametrize("name", ec.CASES)
def test_statement_matches_the_restatement(name):
    c = ec.case(name)
    mdl = c["model"]
    ref = restated(name)
    dC = np.abs(c["C"] - ref["C"]) / ec.bar_add(ref["C"])
    print(name, "max |C - ref| / bar", dC.max())
    assert (dC <= 1.0).all()
    ok = np.isin(c["status"], models.StageOCP.STATUS_OK)
    P0 = c["ls"].P
    Pn, touched, lam_min = ec.statement(c)
    assert not touched.any() and np.isnan(lam_min).all()
    for b in range(P0.shape[0]):
        if not ok[b]:
            assert np.array_equal(Pn[b].view(np.int64), P0[b].view(np.int64))       # no point: every bit of P
            continue
        want = dense_P(mdl, P0[b]) + scatter(mdl, ref["C"][b], mdl.f)
        assert (np.abs(dense_P(mdl, Pn[b]) - want) <= ec.bar_add(want)).all(), (name, b)
    # without a status every instance takes its curvature
    Pa, _, _ = ec.statement(c, status=False)
    assert not np.array_equal(Pa[3], P0[3]) and np.array_equal(Pa[ok], Pn[ok])
    if name not in ec.CONVEXIFY_CASES:
        with pytest.raises(ValueError, match="convexify = True"):
            ec.statement(c, "project")
        return
    per_frame, per_inst = ec.bar_cvx(c)
    for mode in ec.MODES:
        Pm, touched, lam_min = ec.statement(c, mode)
        want_touched = np.where(ok, (ref["lam_min"] < ec.EPS).sum(axis=1), 0)
        assert np.array_equal(touched, want_touched), (name, mode)
        assert (np.abs(lam_min[ok] - ref["lam_min"][ok]) <= per_frame[ok]).all() and np.isnan(lam_min[~ok]).all()
        for b in range(P0.shape[0]):
            if not ok[b]:
                assert np.array_equal(Pm[b].view(np.int64), P0[b].view(np.int64))
                continue
            want = dense_P(mdl, P0[b]) + scatter(mdl, ref["C"][b], mdl.f) + scatter(mdl, ref["D"][mode][b], mdl.f + mdl.nx)
            err = np.abs(dense_P(mdl, Pm[b]) - want).max()
            assert err <= per_inst[b], (name, mode, b, err, per_inst[b])
            # a frame the convexification does not touch holds the bits mode = None gives
            src = mdl._P_src
            for k in np.nonzero(~(ref["lam_min"][b] < ec.EPS))[0]:
                own = src[(src[:, 0] == k) & (src[:, 1] < mdl.f) & (src[:, 2] < mdl.f)][:, 3]
                assert np.array_equal(Pm[b, own], Pn[b, own])


def test_statement_against_the_whole_system_restatement():
    """pend2 once more against d2(f + y'c)/dw2 differenced over the whole of w (n = 8): cost, curvature and their places in P in one reference"""
    c = ec.case("pend2")
    mdl = c["model"]
    st = nlp_hp.Stage(mdl)
    assert st.whole
    Pn, _, _ = ec.statement(c, status=False)
    with mp.workdps(st.dps):
        h = mpf(st.step)
        for b in range(c["x"].shape[0]):
            m = st._model(b)
            y = nlp_hp._mpfs(c["y"][b])
            w = st._w(c["p"], c["x"], b)

            def lagrangian(z):
                cw = list(z) + st._g(m, b, z)
                return st._f(m, b, z) + sum((yi * ci for yi, ci in zip(y, cw)), mpf(0))

            _, _, H = nlp_hp.grad_hess(lagrangian, w, h)
            want = nlp_hp._f64(H)
            assert (np.abs(dense_P(mdl, Pn[b]) - want) <= ec.bar_add(want)).all(), b


@pytest.mark.parametrize("name", ec.CASES)
def test_zero_multipliers_leave_every_bit(name):
    c = ec.case(name)
    Pz, _, _ = ec.statement(c, y=np.zeros_like(c["y"]), status=False)
    assert np.array_equal(Pz, c["ls"].P)


# ------------------------------------------------------------------------------------------------ 3. pattern and generated source
def _twin(mdl):
    cls = ec.unflagged(type(mdl))
    return cls(mdl.N, mdl.dt, mdl.Q, mdl.R)


@pytest.mark.parametrize("name", ec.CASES)
def test_pattern_holds_the_curvature_and_is_symmetric(name):
    c = ec.case(name)
    mdl = c["model"]
    f = mdl.f
    # structurally nonzero entries, seen numerically on random multipliers at random points
    rng = np.random.default_rng(5)
    seen = np.zeros((f, f), bool)
    for _ in range(3):
        Cr = ec.with_data(c, lambda: mdl.constraint_curvature(rng.normal(size=c["x"].shape), rng.normal(size=c["y"].shape)))
        seen |= (Cr != 0.0).any(axis=(0, 1))
    assert np.array_equal(seen, mdl.curvature_mask), (seen, mdl.curvature_mask)
    assert (mdl.cost_mask[:f, :f] >= mdl.curvature_mask).all() and np.array_equal(mdl.cost_mask, mdl.cost_mask.T)
    S = dense_P(mdl, np.ones(len(mdl.Pi))) != 0
    assert np.array_equal(S, S.T)
    for k in range(mdl.N):
        idx = [mdl.np + k * f + i for i in range(f)]
        assert (S[np.ix_(idx, idx)] >= mdl.curvature_mask).all()
    twin = _twin(mdl)
    assert len(mdl.Pi) >= len(twin.Pi) and not hasattr(twin, "curvature_mask")


def _tape(mdl, **kw):
    k = {}
    if mdl.per_frame_reference: k["per_frame_reference"] = True
    if mdl.link_cost: k["llink"] = mdl.llink
    if mdl.nsd: k.update(nsd=mdl.nsd, sdata0=mdl.sdata, model=mdl)
    if mdl.ntheta: k.update(ntheta=mdl.ntheta, theta0=mdl.theta, model=mdl)
    if mdl.nk: k.update(kfun=mdl.kfun, nk=mdl.nk, k_lo=mdl.k_lo, k_hi=mdl.k_hi)
    h_lo, h_hi = mdl.path_bounds() if mdl.nh else (None, None)
    return codegen.trace(mdl.F, mdl.nx, mdl.nu, mdl.hfun if mdl.nh else None, mdl.nh, h_lo[0] if mdl.nh else None, h_hi[0] if mdl.nh else None,
                         lcost=mdl.lcost, lterm=mdl.lterm, convexify=bool(mdl.convexify), **k, **kw)


@pytest.mark.parametrize("name", ("pend3", "pend_theta", "pend_sd", "pend_theta_sd", "pend_pf", "nohfun", "klin", "llink"))
def test_generated_source_and_pattern_without_the_flag_are_unchanged(name):
    mdl = ec.case(name)["model"]
    twin = _twin(mdl)
    plain, off = _tape(twin), _tape(twin, exact_hessian=False)
    assert codegen.device_source(plain) == codegen.device_source(off) and codegen.host_source(plain) == codegen.host_source(off)
    src = codegen.device_source(plain)
    for word in ("lagrangian", "exact", "FG", "HG", "curv_mask"):
        assert word not in src, word
    flagged = _tape(mdl, exact_hessian=True)
    fs = codegen.device_source(flagged)
    assert "mpcqp_user_lagrangian(" in fs and ("mpcqp_user_ntheta" in fs) == (mdl.ntheta > 0) and ("mpcqp_user_nsd" in fs) == (mdl.nsd > 0)
    assert ("HG(" in fs) == (mdl.nh > 0) and "FG(" in fs
    assert np.array_equal(flagged.exact["mask"], mdl.curvature_mask) and np.array_equal(flagged.cost["mask"], mdl.cost_mask)
    # the unflagged model's pattern is the one it always had: cost mask without the curvature
    ref_mask = codegen.hessian_mask(twin._gtape) | np.eye(twin.f + twin.nx, dtype=bool)
    assert np.array_equal(twin.cost_mask, codegen.closed_mask(ref_mask) if twin.convexify else ref_mask)


def test_header_and_exports():
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    for nm in ("mpcqp_stage_has_exact_hessian", "mpcqp_stage_lagrangian"):
        assert nm + "(" in header and nm in _lib.EXPORTS
    assert "typedef struct mpcqp_stage_lagrangian_args" in header and "hessian(f, w)" in header
    assert models.StageOCP.exact_hessian is False


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    with pytest.raises(ValueError, match="nonlinear link constraint"):
        ec._pend(ec.NonlinearLink, 3)
    lin = ec.case("klin")["model"]
    with pytest.raises(ValueError, match="nonlinear link constraint"):
        codegen.trace(lin.F, 2, 1, lin.hfun, 2, [-1.0, -1.0], [1.0, 1.0], lcost=lin.lcost, kfun=ec.NonlinearLink.kfun.__get__(lin), nk=1, k_lo=[-1.0], k_hi=[1.0],
                      exact_hessian=True)
    with pytest.raises(ValueError, match="needs a stage cost"):
        codegen.trace(models.DoubleIntegrator(4).F, 2, 1, exact_hessian=True)

    class Diagonal(ec.Pendulum):
        lcost = None; convexify = False

    with pytest.raises(ValueError, match="needs a stage cost"):
        ec._pend(Diagonal, 3)
    plain = _twin(ec.case("pend3")["model"])
    c = ec.case("pend3")
    with pytest.raises(ValueError, match="exact_hessian = True"):
        plain.constraint_curvature(c["x"], c["y"])
    with pytest.raises(ValueError, match="exact_hessian = True"):
        plain.lagrangian_system(c["p"], c["x"], c["y"], c["ls"].P)
    for kw in (dict(mode="reflect"), dict(mode="project", eps=0.0), dict(mode="mirror", eps=float("inf"))):
        with pytest.raises(ValueError):
            c["model"].lagrangian_system(c["p"], c["x"], c["y"], c["ls"].P, **kw)
    opts = {"max_iter": 1, "alpha": 1.0, "exact_hessian": True}
    with pytest.raises(ValueError, match="exact_hessian = True"):
        SQPOptimizationSolver(plain, opts, batch=2, qp_solver=OracleCuCaQP(batch=2))
    with pytest.raises(ValueError, match="exact_hessian = True"):
        SQPOptimizationSolver(models.CartPole(3, 0.02), opts, batch=2, qp_solver=OracleCuCaQP(batch=2))
    sol = SQPOptimizationSolver(plain, dict(opts, exact_hessian=False), batch=2, qp_solver=OracleCuCaQP(batch=2))
    assert sol.exact_hessian is False and sol.lam is None


# ------------------------------------------------------------------------------------------------ 5. the generated functors, on the host
@pytest.mark.parametrize("name", ("pend3", "pend_theta", "pend_sd", "nohfun", "wide7"))
def test_generated_functors_match_the_statement(built, tmp_path, name):
    c = ec.case(name)
    mdl = c["model"]
    lib = codegen.build_host_library(_tape(mdl, exact_hessian=True))
    Bn, N, nx, nu, nh, n = c["x"].shape[0], mdl.N, mdl.nx, mdl.nu, mdl.nh, mdl.n
    X = c["x"].reshape(Bn, N, mdl.f)
    rows = ["%d %d %d %d %d %d" % (Bn * N, nx, nu, nh, mdl.ntheta, mdl.nsd)]
    for b in range(Bn):
        for k in range(N):
            lam = c["y"][b, n + k * nx:n + (k + 1) * nx] if k < N - 1 else np.zeros(nx)
            mu = c["y"][b, n + mdl.ngd + k * nh:n + mdl.ngd + (k + 1) * nh]
            vals = np.concatenate([c["theta"][b] if mdl.ntheta else [], X[b, k], lam, mu, c["d"][b, k] if mdl.nsd else []])
            rows.append("%d " % (k < N - 1) + " ".join(float(v).hex() for v in vals))
    inp = tmp_path / "frames.txt"
    inp.write_text("\n".join(rows) + "\n")
    r = subprocess.run([os.path.join(ROOT, "tests", "support", "exact_hessian_host"), lib, str(inp)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().split("\n")]).reshape(Bn, N, mdl.f, mdl.f)
    err = np.abs(got - c["C"]) / ec.bar_add(c["C"])
    print(name, "max |functor - statement| / bar", err.max())
    assert (err <= 1.0).all()
    assert np.array_equal(got != 0.0, np.broadcast_to(mdl.curvature_mask, got.shape) & (got != 0.0))      # nothing outside the structure


# ------------------------------------------------------------------------------------------------ 6. the SQP recipe on the CPU oracle
def _iterations_to(log, tol):
    for i, it in enumerate(log):
        if np.isfinite(it["step"]).all() and it["step"].max() < tol:
            return i + 1
    return None


def test_recipe_needs_fewer_iterations_with_the_exact_hessian(built):
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, arg, x0 = ec.recipe()
    nB = x0.shape[0]
    assert (mdl.N, mdl.dt, nB, ec.RECIPE_ALPHA, ec.RECIPE_TOL) == (10, 0.2, 4, 1.0, 1e-8)
    sol0, off = ec.host_loop(mdl, arg, x0, OracleCuCaQP(batch=nB, nthreads=4), ec.RECIPE_MAX, exact=False, qp_tol=1e-11)
    sol1, on = ec.host_loop(mdl, arg, x0, OracleCuCaQP(batch=nB, nthreads=4), ec.RECIPE_MAX, exact=True, qp_tol=1e-11)
    assert all(np.isin(it["status"], (1, 2, 7)).all() for it in off + on)
    n_off, n_on = _iterations_to(off, ec.RECIPE_TOL), _iterations_to(on, ec.RECIPE_TOL)
    print("iterations to max|dx| < %g: %s without the option, %s with it" % (ec.RECIPE_TOL, n_off, n_on))
    print("steps without:", ["%.1e" % it["step"].max() for it in off[:n_off or len(off)]])
    print("steps with:   ", ["%.1e" % it["step"].max() for it in on[:n_on or len(on)]])
    assert n_on is not None and (n_off is None or n_on < n_off)
    # the first QP is the reference's: lam starts at zero
    assert np.array_equal(on[0]["x"], off[0]["x"])
    # both arrive at the same point, and the estimate holds the QP's multipliers there
    assert np.abs(on[-1]["x"] - off[-1]["x"]).max() < 1e-5
    assert np.abs(sol1.lam - sol1.last_qp_info["y"]).max() < 1e-6 and np.abs(sol1.lam[:, mdl.n:]).max() > 1e-3
    sol1.setInitialGuess(x0)
    assert not sol1.lam.any()
