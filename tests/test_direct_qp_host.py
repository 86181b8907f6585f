"""The direct solve of the stage QP on the host: models.StageOCP.direct_qp, the NumPy statement of mpcqp_stage_riccati_solve, against a
60-digit KKT restatement written from the header; the optimality certificate of every accepted instance; the masks; the host SQP loop with
options["direct_qp"]; refusals and the ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from tests.support import direct_qp_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("local", "random", "random_mix", "random_free")
KEYS = ("P", "q", "A", "l", "u")
# the certificate's bar: what the polish path is held to (README)
CERT_BAR = 1e-10


def _same(a, b):
    return np.array_equal(dc.bits(a), dc.bits(b))


def _solve(mdl, d, **kw):
    return mdl.direct_qp(*(d[k] for k in KEYS), **kw)


@pytest.mark.parametrize("N", dc.HORIZONS)
@pytest.mark.parametrize("name", dc.MODELS)
def test_statement_against_60_digits(name, N):
    """w, y, z of the statement against the restatement, on local systems at drawn iterates and on random data whose unread slots are NaN; pinned,
    mixed and free inputs in frame 0.  No case exceeds the recorded E_NP (tests/support/direct_qp_cases.py)."""
    mdl = dc.model(name, N)
    for kind in KINDS:
        d, ref = dc.reference(name, N, kind)
        w, y, z, direct = _solve(mdl, d, feas_tol=dc.REF_FEAS_TOL)
        assert (direct == 1).all() and all(r["direct"] == 1 for r in ref), (kind, direct)
        for b, r in enumerate(ref):
            ew, ey, ez = dc.rel_err(w[b], r["w"]), dc.rel_err(y[b], r["y"]), dc.rel_err(z[b], r["z"])
            print("%s N=%d %s b=%d  e_w %.2e  e_y %.2e  e_z %.2e" % (name, N, kind, b, ew, ey, ez))
            assert ew <= dc.E_NP_W and ez <= dc.E_NP_W and ey <= dc.E_NP_Y, (kind, b, ew, ey, ez)


@pytest.mark.parametrize("name", dc.MODELS)
def test_optimality_certificate(name, built):
    """on every instance accepted at feas_tol = 0: stationarity, bound violation and the multipliers of slack rows within 1e-10 (worst seen: stat
    4.0e-16, viol 1.1e-16, slack rows exactly 0); on the local systems the CPU oracle at its default settings reports status 1 and agrees with w
    to its own tolerance.  That tolerance is one on residuals: the oracle stops when |A x - z| <= eps_abs + eps_rel max(|A x|, |z|) and
    |P x + q + A'y| <= eps_abs + eps_rel max(|P x|, |A'y|, |q|) (infinity norms, unscaled).  On an accepted instance the active rows are the
    equalities, on which z = l exactly, and the ADMM's multiplier of a row it does not clip is exactly 0: so the oracle's (x, y) solves the
    equality-constrained KKT system up to a right-hand side no larger than those two thresholds, and |x - w|_inf <= |K^-1|_inf times the larger
    of them, K the KKT matrix (direct_mp reports the norm)."""
    from oracle import oracle as orc
    seen = 0
    for N in dc.HORIZONS:
        mdl = dc.model(name, N)
        for kind in KINDS:
            d, mp_ref = dc.reference(name, N, kind)
            w, y, z, direct = _solve(mdl, d)
            acc = np.flatnonzero(direct == 1)
            for b in acc:
                st, vi, sl = dc.certificate(mdl, d, w[b], y[b], b)
                print("%s N=%d %s b=%d  stat %.2e  viol %.2e  slack-row |y| %.2e" % (name, N, kind, b, st, vi, sl))
                assert st <= CERT_BAR and vi <= CERT_BAR and sl <= CERT_BAR
                seen += 1
            if kind == "local" and len(acc):
                pat = orc.Pattern(mdl.n, mdl.m, mdl.Pp, mdl.Pi, mdl.Ap, mdl.Ai)
                st_ = orc.default_settings()
                ref = pat.solve(*(d[k][acc] for k in KEYS), st_)
                assert (ref["status"] == 1).all()
                for i, b in enumerate(acc):
                    Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, d["P"][b], mdl.n, mdl.n)
                    Ad, _ = dc.dense_from_csc(mdl.Ap, mdl.Ai, d["A"][b], mdl.m, mdl.n)
                    xo, yo = ref["x"][i], ref["y"][i]
                    nrm = lambda v: float(np.abs(v).max())
                    eps = max(st_.eps_abs + st_.eps_rel * max(nrm(Ad @ xo), nrm(ref["z"][i])),
                              st_.eps_abs + st_.eps_rel * max(nrm(Pd @ xo), nrm(Ad.T @ yo), nrm(d["q"][b])))
                    tol = mp_ref[b]["kinv_norm"] * eps
                    err = np.abs(ref["x"][i] - w[b]).max()
                    print("%s N=%d b=%d  |x_oracle - w| %.2e  (tolerance %.2e)" % (name, N, b, err, tol))
                    # a sanity check only: on a badly conditioned system (cart-pole N = 20: |K^-1| = 1e4) this bound is wide, and the proof that w
                    # is the optimum is the certificate above
                    assert err <= tol
                    # the comparison that scales: (w, y, z) meets the oracle's own stopping test, with room of a factor 1e6
                    r_prim, r_dual = nrm(Ad @ w[b] - z[b]), nrm(Pd @ w[b] + d["q"][b] + Ad.T @ y[b])
                    e_prim = st_.eps_abs + st_.eps_rel * max(nrm(Ad @ w[b]), nrm(z[b]))
                    e_dual = st_.eps_abs + st_.eps_rel * max(nrm(Pd @ w[b]), nrm(Ad.T @ y[b]), nrm(d["q"][b]))
                    assert r_prim <= 1e-6 * e_prim and r_dual <= 1e-6 * e_dual, (r_prim, e_prim, r_dual, e_dual)
                    assert (d["l"][b] <= z[b]).all() and (z[b] <= d["u"][b]).all()
    assert seen > 0


@pytest.mark.parametrize("name", ("double_integrator", "cartpole"))
def test_masks(name):
    """a batch the restatement accepts in part, every verdict with a margin of at least 1e-6 of the bound's scale; direct equals the restatement's;
    rejected, ineligible, failed and frozen instances report no w, y, z"""
    mdl, d, ref = dc.mask_batch(name)
    want = np.array([r["direct"] for r in ref])
    margins = np.array([r["margin"] for r in ref])
    print(name, "restatement", want, "margins", margins)
    assert (want == 1).any() and (want == 0).any()
    assert (np.abs(margins) >= 1e-6).all()
    w, y, z, direct = _solve(mdl, d)
    assert (direct == want).all()
    out = direct != 1
    assert np.isnan(w[out]).all() and np.isnan(y[out]).all() and np.isnan(z[out]).all()
    assert np.isfinite(w[~out]).all() and np.isfinite(y[~out]).all() and np.isfinite(z[~out]).all()
    b = int(np.flatnonzero(want == 1)[0])
    for how in dc.SPOILS:
        o, code = dc.spoiled(mdl, d, b, how)
        w1, y1, z1, d1 = _solve(mdl, o)
        assert d1[0] == code, (how, d1)
        assert np.isnan(w1).all() and np.isnan(y1).all() and np.isnan(z1).all()
        if code == -1:
            assert dc.direct_mp(mdl, *(o[k][0] for k in KEYS))["direct"] == -1
    # frozen: no verdict, no result; the others are what they are without the mask
    fz = np.zeros(len(want), np.int32); fz[b] = 1
    w2, y2, z2, d2 = _solve(mdl, d, frozen=fz)
    assert d2[b] == 0 and np.isnan(w2[b]).all()
    keep = fz == 0
    assert (d2[keep] == direct[keep]).all() and np.array_equal(w2[keep], w[keep], equal_nan=True) and np.array_equal(y2[keep], y[keep], equal_nan=True)
    # a batch of one is the instance's row of the batch, bit for bit
    w3, y3, z3, d3 = _solve(mdl, {k: v[b:b + 1] for k, v in d.items()})
    assert _same(w3[0], w[b]) and _same(y3[0], y[b]) and _same(z3[0], z[b])


@pytest.mark.parametrize("name", ("double_integrator", "quadrotor", "linear16x8"))
def test_frame_zero(name):
    """N = 2: the frame-0 step is the only solve of the recursion.  A pinned input is its value exactly and carries a multiplier; a free input
    carries none and makes its column stationary; reg moves the free inputs only"""
    mdl = dc.model(name, 2)
    npp, nx, f = mdl.np, mdl.nx, mdl.f
    for kind, pins in (("random", "all"), ("random_mix", "mix"), ("random_free", "none")):
        d, ref = dc.reference(name, 2, kind)
        w, y, z, direct = _solve(mdl, d, feas_tol=dc.REF_FEAS_TOL)
        assert (direct == 1).all()
        pin = d["l"][:, npp + nx:npp + f] == d["u"][:, npp + nx:npp + f]
        assert pin.all() if pins == "all" else (not pin.any() if pins == "none" else (pin.any() or mdl.nu == 1) and not pin.all())
        du = w[:, npp + nx:npp + f]; yu = y[:, npp + nx:npp + f]
        assert _same(du[pin], d["l"][:, npp + nx:npp + f][pin])
        assert (yu[~pin] == 0.0).all()
        assert _same(w[:, npp:npp + nx], d["l"][:, npp:npp + nx])
        if not pin.all():
            w2, y2, _, d2 = _solve(mdl, d, feas_tol=dc.REF_FEAS_TOL, reg=0.5)
            assert (d2 == 1).all()
            assert _same(w2[:, npp + nx:npp + f][pin], du[pin])
            assert (np.abs(w2[:, npp + nx:npp + f][~pin]) < np.abs(du[~pin])).any()
            r = dc.direct_mp(mdl, *(d[k][0] for k in KEYS), feas_tol=dc.REF_FEAS_TOL, reg=0.5)
            assert dc.rel_err(w2[0], r["w"]) <= dc.E_NP_W and dc.rel_err(y2[0], r["y"]) <= dc.E_NP_Y


TIGHT = 1e-9      # the oracle's eps_abs = eps_rel in the tight comparisons: its QP solutions are then exact to about |K^-1| 1e-9


def _host_loop(which, direct, backend=None, iters=None, eps=None):
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, arg, x0 = dc.recipe(which)
    opt = {"max_iter": dc.RECIPE_ITERS if iters is None else iters, "alpha": 1.0}
    if direct:
        opt["direct_qp"] = True
    sol = SQPOptimizationSolver(mdl, opt, batch=dc.RECIPE_B, qp_solver=backend or OracleCuCaQP(dc.RECIPE_B, nthreads=4))
    if eps is not None:      # (the loop's constructor has set the reference's 1e-3)
        sol.qpSolver_.setAbsoluteTolerance(eps); sol.qpSolver_.setRelativeTolerance(eps); sol.qpSolver_.setMaxIteration(200000)
    sol.setInitialGuess(x0)
    out = sol.getOptimalSolution(arg)
    return sol, np.array(out["x"], float)


def _system_at(which, x):
    mdl, arg, _ = dc.recipe(which)
    return mdl, mdl.local_system(arg["p"], x, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"])


def _kkt_bar(which, x, eps):
    """what a QP solver that stops at residuals eps_abs = eps_rel = eps may be away from the exact solution of the QP at x, in the infinity norm and
    at worst over the batch: |K^-1|_inf (eps + eps S), K the equality-constrained KKT matrix (the active set of an accepted instance), S the
    largest of the norms the two stopping thresholds scale with, taken at the exact solution"""
    mdl, ls = _system_at(which, x)
    w, y, z, direct = mdl.direct_qp(ls.P, ls.q, ls.A, ls.l, ls.u)
    assert (direct == 1).all()
    worst = 0.0
    for b in range(x.shape[0]):
        Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, ls.P[b], mdl.n, mdl.n)
        Ad, _ = dc.dense_from_csc(mdl.Ap, mdl.Ai, ls.A[b], mdl.m, mdl.n)
        S = max(np.abs(v).max() for v in (Ad @ w[b], z[b], Pd @ w[b], Ad.T @ y[b], ls.q[b]))
        kn = dc.direct_mp(mdl, ls.P[b], ls.q[b], ls.A[b], ls.l[b], ls.u[b])["kinv_norm"]
        worst = max(worst, kn * (eps + eps * S))
    return worst


def _last_qp_is_the_direct_solve(which, sol):
    """the step, multipliers, status and iteration count the loop reports for its last QP are the direct solve's on the system at the iterate before
    the last step (the loop of one iteration less ends there: the host loop is deterministic), bit for bit"""
    prev, xp = _host_loop(which, True, iters=dc.RECIPE_ITERS - 1)
    mdl, ls = _system_at(which, xp)
    w, y, z, direct = mdl.direct_qp(ls.P, ls.q, ls.A, ls.l, ls.u)
    info = sol.last_qp_info
    assert np.array_equal(direct, sol.direct_history[-1]) and (direct == 1).all()
    assert _same(np.asarray(info["x"], float), w) and _same(np.asarray(info["y"], float), y) and _same(np.asarray(info["z"], float), z)
    assert _same(np.asarray(sol._last_solution, float), w)
    assert (np.asarray(info["status"]) == 1).all() and (np.asarray(info["iters"]) == 0).all()
    assert _same(sol.result_["x"], xp + w[:, mdl.np:])


def test_host_loop_near_the_origin(built):
    """every instance accepted in every iteration.  x against the loop without the option, twice: at the reference's settings within the QPs' own
    tolerance eps_abs + eps_rel max(1, |x|_inf) = 2e-3 (measured 1.3e-7); and with the other loop's oracle at eps 1e-9, where its QP solutions are
    exact to _kkt_bar: the model is linear, so the last iterate is the last QP's solution added to the iterate before it, and the difference of the two
    loops is at most that bar for the QP at either loop's previous iterate (measured 3.7e-13 against a bar of 2.7e-5).  What the loop reports for its last QP is the direct solve, bit for bit."""
    sol, x = _host_loop("near", True)
    plain, x0 = _host_loop("near", False)
    assert len(sol.direct_history) == dc.RECIPE_ITERS and all((h == 1).all() for h in sol.direct_history)
    assert plain.direct_history == []
    tol = 1e-3 + 1e-3 * max(1.0, np.abs(x0).max())
    err = np.abs(x - x0).max()
    print("near: |x_direct - x_plain| %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol
    tight, xt = _host_loop("near", False, eps=TIGHT)
    assert (np.asarray(tight.last_qp_info["status"]) == 1).all()
    bar = _kkt_bar("near", _host_loop("near", True, iters=dc.RECIPE_ITERS - 1)[1], TIGHT)
    err = np.abs(x - xt).max()
    print("near: |x_direct - x_plain at eps 1e-9| %.3e (bar %.3e)" % (err, bar))
    assert err <= bar and bar < 1e-4
    assert all((np.asarray(it) == 0).all() for it in sol.admm_iterations)
    _last_qp_is_the_direct_solve("near", sol)


def test_host_loop_from_far_out(built):
    """the first iterations want more input than the box allows and are rejected (the backend solves them); later ones are accepted.  x against the loop
    without the option with both loops' oracles at eps 1e-9: every QP of either loop is then exact to _kkt_bar, the two loops run the same Newton iteration
    up to that, and near its solution the SQP map contracts, so the iterates differ by at most the bar per iteration (measured 5.1e-7 against a bar of 4.3e-4;
    at the reference's 1e-3 the two loops end 1.6e-2 apart, which is what an ADMM point at that tolerance is away from the optimum of these QPs)"""
    sol, x = _host_loop("far", True)
    h = np.array(sol.direct_history)
    print("far: verdicts per iteration\n", h)
    assert (h[0] == 0).all()
    assert (h[-1] == 1).all()
    assert ((h == 0) | (h == 1)).all()
    its = np.array([np.asarray(i) for i in sol.admm_iterations])
    assert (its[h == 1] == 0).all() and (its[h == 0] > 0).all()
    _last_qp_is_the_direct_solve("far", sol)
    st, xs = _host_loop("far", True, eps=TIGHT)
    pt, xp = _host_loop("far", False, eps=TIGHT)
    ht = np.array(st.direct_history)
    assert (ht[0] == 0).all() and (ht[-1] == 1).all() and (np.asarray(pt.last_qp_info["status"]) == 1).all()
    bar = dc.RECIPE_ITERS * _kkt_bar("far", _host_loop("far", True, iters=dc.RECIPE_ITERS - 1, eps=TIGHT)[1], TIGHT)
    err = np.abs(xs - xp).max()
    print("far: |x_direct - x_plain|, both at eps 1e-9: %.3e (bar %.3e)" % (err, bar))
    assert err <= bar and bar < 1e-2


def test_host_loop_uses_set_skip_where_the_backend_has_it(built):
    """a backend with setSkip is handed the accepted instances; its rows for them are replaced whatever it returns"""
    from tests.support.oracle_backend import OracleCuCaQP

    class Skipping(OracleCuCaQP):
        masks = None

        def setSkip(self, skip):
            type(self).masks = (self.masks or []) + [None if skip is None else np.array(skip)]

        def getSolutionAsDM(self):
            x = np.array(super().getSolutionAsDM(), float)
            if self.masks and self.masks[-1] is not None:
                x[self.masks[-1] != 0] = np.nan      # what a handle that never solved an instance may hold
            return x

    sol, x = _host_loop("far", True, backend=Skipping(dc.RECIPE_B, nthreads=4))
    ref, x0 = _host_loop("far", True)
    assert len(Skipping.masks) == dc.RECIPE_ITERS
    for m, h in zip(Skipping.masks, sol.direct_history):
        assert (m is None and not (h == 1).any()) or np.array_equal(m != 0, h == 1)
    assert np.isfinite(x).all() and _same(x, x0)


def test_refusals():
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver, DIRECT_QP_REFUSES, _direct_qp_option
    from tests.support.oracle_backend import OracleCuCaQP
    mdl = dc.model("double_integrator", 3)
    d = dc.local_qp(mdl, 2)
    for kw in (dict(feas_tol=-1.0), dict(feas_tol=np.nan), dict(reg=-1e-3), dict(reg=np.nan)):
        with pytest.raises(ValueError):
            _solve(mdl, d, **kw)
    with pytest.raises(ValueError):
        mdl.direct_qp(d["P"][:, :-1], d["q"], d["A"], d["l"], d["u"])
    from tests.support import convexify_cases as cc
    link = cc.case("bump_link")["model"]
    with pytest.raises(ValueError) as e:
        link.direct_qp(np.zeros((1, len(link.Pi))), np.zeros((1, link.n)), np.zeros((1, len(link.Ai))), np.zeros((1, link.m)), np.zeros((1, link.m)))
    assert "link cost" in str(e.value)
    base = {"max_iter": 1, "alpha": 1.0}
    for bad in (1, "yes", {"tol": 1.0}, {"reg": -1.0}, {"feas_tol": -1e-9}, {"feas_tol": np.nan}):
        with pytest.raises(ValueError):
            SQPOptimizationSolver(mdl, dict(base, direct_qp=bad), batch=1, qp_solver=OracleCuCaQP(1))
    for key, why in DIRECT_QP_REFUSES.items():
        with pytest.raises(ValueError) as e:
            _direct_qp_option(dict(base, direct_qp=True, **{key: True}), mdl)
        assert str(e.value) == why and key in why
    with pytest.raises(ValueError) as e:
        SQPOptimizationSolver(mdl, dict(base, direct_qp=True, carry_rho=True), batch=1, qp_solver=OracleCuCaQP(1))
    assert "carry_rho" in str(e.value)
    with pytest.raises(ValueError) as e:
        _direct_qp_option(dict(base, direct_qp=True), link)
    assert "link cost" in str(e.value)
    with pytest.raises(ValueError) as e:
        _direct_qp_option(dict(base, direct_qp=True), mdl, evaluator=object())
    assert "stage OCPs" in str(e.value)
    with pytest.raises(ValueError) as e:
        _direct_qp_option(dict(base, direct_qp=True), models.reference_test_cases()[1][0])
    assert "stage OCPs" in str(e.value)
    assert _direct_qp_option(dict(base), mdl) is None and _direct_qp_option(dict(base, direct_qp=False), mdl) is None
    assert _direct_qp_option(dict(base, direct_qp={"feas_tol": 1e-9}), mdl) == (1e-9, 0.0)


def test_abi(built):
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert "int mpcqp_stage_riccati_solve(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_args *a, void *stream);" in header
    assert "mpcqp_stage_riccati_solve" in _lib.EXPORTS
    import ctypes as C
    from optimal_control_problem_amd import stage_eval as se
    cname, cls = "mpcqp_stage_riccati_solve_args", se.RiccatiSolveArgs
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\b([a-z_0-9A-Z]+)\s*[,;]", body)
    assert names == [f[0] for f in cls._fields_], (names, [f[0] for f in cls._fields_])
    assert C.sizeof(cls) == 12 * 8 and cls.feas_tol.offset == 40 and cls.reg.offset == 48 and cls.frozen.offset == 56 and cls.direct.offset == 88
    L = se._bind(_lib.lib())
    assert L.mpcqp_stage_riccati_solve(None, 1, None, None) == _lib.ERR_ARG
    assert b"stage handle is null" in L.mpcqp_strerror(_lib.ERR_ARG)
    hpp = open(os.path.join(ROOT, "optimal_control_problem_amd", "csrc", "stage_riccati.hpp")).read()
    assert hpp.count("static_assert(G * tile * 8 <= 48 * 1024") == 2
    assert "static_assert(G == R::G" in hpp
