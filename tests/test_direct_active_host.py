"""The direct solve with active input bounds on the host: models.StageOCP.direct_qp_active, the NumPy statement of
mpcqp_stage_riccati_solve_active, against an independent restatement written from the header (one dense KKT solve per round, 60 digits); the margins
of every decision; the cases the rule must cover; the QP's own KKT certificate on every accepted instance; the host SQP loop with
options["direct_qp"]["active_set"]; refusals and the ABI.  No GPU."""
import os
import re

import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import direct_active_cases as da
from tests.support import direct_qp_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("P", "q", "A", "l", "u")
CERT_BAR = 1e-10      # the bar of DESIGN 6.30
REGS = (0.0, 0.05)


def _same(a, b):
    return np.array_equal(da.bits(a), da.bits(b))


def _solve(mdl, d, **kw):
    return mdl.direct_qp_active(*(d[k] for k in KEYS), **kw)


def _agree(ref, direct, act, used, roles):
    for b, r in enumerate(ref):
        if r is None:
            continue
        assert r["direct"] == direct[b], (roles[b], r["direct"], direct[b])
        if r["direct"] >= 0:
            assert np.array_equal(r["act"], act[b]) and r["rounds_used"] == used[b], (roles[b], r["rounds_used"], used[b])


@pytest.mark.parametrize("N", da.HORIZONS)
@pytest.mark.parametrize("name", da.MODELS)
def test_statement_against_60_digits(name, N):
    """w, y, z of every accepted instance of the case batch against the restatement at 60 digits; direct, act and rounds_used equal to it.  No case
    exceeds the recorded E_NP (tests/support/direct_active_cases.py)."""
    mdl, d, guess, frozen, roles = da.case_batch(name, N)
    ref = da.restated(name, N, digits=60)
    w, y, z, direct, act, used = _solve(mdl, d, act=guess, frozen=frozen)
    _agree(ref, direct, act, used, roles)
    seen = 0
    for b, r in enumerate(ref):
        if r is None or r["direct"] != 1:
            continue
        ew, ey, ez = da.rel_err(w[b], r["w"]), da.rel_err(y[b], r["y"]), da.rel_err(z[b], r["z"])
        print("%s N=%d %s round %d  e_w %.2e  e_y %.2e  e_z %.2e" % (name, N, roles[b], used[b], ew, ey, ez))
        assert ew <= da.E_NP_W and ez <= da.E_NP_W and ey <= da.E_NP_Y, (roles[b], ew, ey, ez)
        seen += used[b] >= 1
    assert seen >= 3


@pytest.mark.parametrize("reg", REGS)
@pytest.mark.parametrize("N", da.HORIZONS)
@pytest.mark.parametrize("name", da.MODELS)
def test_margins_and_verdicts(name, N, reg):
    """every primal and dual decision of every round of every instance of the case batch is at least 1e-6 of its scale away from its threshold in the
    restatement, none left out; direct, act and rounds_used of the statement equal the restatement's, at rounds = 4 and at rounds = 1"""
    mdl, d, guess, frozen, roles = da.case_batch(name, N, reg)
    for rounds in (4, 1):
        ref = da.restated(name, N, reg, rounds=rounds)
        margins = [r["margin"] for r in ref if r is not None and r["direct"] >= 0]
        print(name, N, reg, rounds, "smallest margin %.2e" % min(margins))
        assert len(margins) == len(roles) - 3 and min(margins) >= da.MARGIN
        w, y, z, direct, act, used = _solve(mdl, d, reg=reg, rounds=rounds, act=guess, frozen=frozen)
        _agree(ref, direct, act, used, roles)
        out = direct != 1
        assert np.isnan(w[out]).all() and np.isnan(y[out]).all() and np.isnan(z[out]).all()
        assert np.isfinite(w[~out]).all() and np.isfinite(y[~out]).all() and np.isfinite(z[~out]).all()


@pytest.mark.parametrize("N", da.HORIZONS)
@pytest.mark.parametrize("name", da.MODELS)
def test_cases_cover_the_rule(name, N):
    mdl, d, guess, frozen, roles = da.case_batch(name, N)
    ref = da.restated(name, N)
    at = {role: b for b, role in enumerate(roles)}
    w, y, z, direct, act, used = _solve(mdl, d, act=guess, frozen=frozen)
    npp, nx, f, nu = mdl.np, mdl.nx, mdl.f, mdl.nu
    pin0 = d["l"][:, npp + nx:npp + f] == d["u"][:, npp + nx:npp + f]
    # accepted in round 0, with the bits of direct_qp
    b = at["round0"]
    w0, y0, z0, d0 = mdl.direct_qp(*(d[k] for k in KEYS))
    assert direct[b] == 1 and used[b] == 0 and d0[b] == 1 and not act[b].any()
    assert _same(w[b], w0[b]) and _same(y[b], y0[b]) and _same(z[b], z0[b])
    # accepted in round 1 with held inputs (the tight boxes; which of the two depends on the model)
    r1 = [b for b in (at["tight"], at["tight2"], at["all_held"]) if direct[b] == 1 and used[b] == 1 and act[b].any()]
    assert r1
    for b in r1:      # a held input sits on its bound exactly and carries a multiplier of the right sign; a free one carries none
        for k in range(N):
            s = slice(npp + k * f + nx, npp + (k + 1) * f)
            a = act[b, k]
            assert _same(w[b, s][a > 0], d["u"][b, s][a > 0]) and _same(w[b, s][a < 0], d["l"][b, s][a < 0])
            assert (y[b, s][a > 0] >= 0).all() and (y[b, s][a < 0] <= 0).all()
            free = (a == 0) & ~(pin0[b] if k == 0 else np.zeros(nu, bool))
            assert (y[b, s][free] == 0).all()
    # a wrong guess is released
    b = at["wrong_guess"]
    named = guess[b] != 0
    assert named.any() and direct[b] == 1
    if used[b] >= 2:
        assert (act[b][named] != guess[b][named]).any()
    # hopeless rows
    for role in ("hopeless_state", "hopeless_path", "hopeless_link"):
        if role in at:
            assert direct[at[role]] == 0 and ref[at[role]]["direct"] == 0 and np.isnan(w[at[role]]).all()
    assert ("hopeless_path" in at) == (mdl.nh > 0) and ("hopeless_link" in at) == (mdl.nk > 0)
    # every input of every frame held (nu = 1: the integrators and the cart-pole; nu >= 2: the others)
    b = at["all_held"]
    assert not pin0[b].any() and direct[b] == 1 and (act[b] == 1).all()
    # a hold in the last frame
    if N == 2:
        assert any(act[b, N - 1].any() for b in r1)
    # an infinite bound named in the guess is ignored
    b = at["inf_guess"]
    k, i = np.argwhere(guess[b] != 0)[0]
    assert np.isinf(d["l"][b, npp + k * f + nx + i]) and guess[b, k, i] == -1 and act[b, k, i] != -1 and used[b] >= 1 and direct[b] == 1
    # rounds spent: with one round, an instance that needs two
    w1, y1, z1, direct1, act1, used1 = _solve(mdl, d, rounds=1, act=guess, frozen=frozen)
    spent = (direct == 1) & (used >= 2)
    assert (direct1[spent] == 0).all() and (used1[spent] == 1).all() and np.isnan(w1[spent]).all()
    # ineligible, failed and frozen instances write nothing: act is the guess that came in, rounds_used -1
    mark = np.where(guess == 0, 1, guess).astype(np.int32)
    _, _, _, direct2, act2, used2 = _solve(mdl, d, act=mark, frozen=frozen)
    for role, code in (("ineligible", -1), ("failed", -2), ("frozen", 0)):
        b = at[role]
        assert direct2[b] == code and used2[b] == -1 and np.array_equal(act2[b], mark[b]) and np.isnan(w[b]).all()
    # the pinned inputs of frame 0 are not part of the set: their entries stay what came in
    b = at["tight"]
    assert (act2[b, 0][pin0[b]] == 1).all()


def test_the_cases_contain_a_released_guess_and_spent_rounds():
    """over the whole set (the per-case test asserts what every case has): a wrong guess released and accepted in round >= 2, rounds spent, a hold in
    the last frame at N = 2"""
    released = spent = 0
    for name in da.MODELS:
        for N in da.HORIZONS:
            mdl, d, guess, frozen, roles = da.case_batch(name, N)
            w, y, z, direct, act, used = _solve(mdl, d, act=guess, frozen=frozen)
            b = roles.index("wrong_guess")
            released += int(direct[b] == 1 and used[b] >= 2 and (act[b][guess[b] != 0] == 0).any())
            _, _, _, direct1, _, used1 = _solve(mdl, d, rounds=1, act=guess, frozen=frozen)
            spent += int(((direct1 == 0) & (used1 == 1) & (direct == 1)).sum())
    print("released guesses", released, "instances with rounds spent", spent)
    assert released >= 6 and spent >= 6


@pytest.mark.parametrize("name", da.MODELS)
def test_optimality_certificate(name, built):
    """on every accepted instance: stationarity, bound violation, multiplier signs and complementarity of the QP's own KKT conditions within 1e-10 of
    max(1, |P|_max |w|_inf, |q|_inf).  As a sanity check the CPU oracle at eps 1e-9 agrees with w within |K^-1|_inf times its two stopping thresholds,
    K the KKT matrix of the accepting round (its active set is the QP's: the certificate says so)."""
    from oracle import oracle as orc
    seen = 0
    for N in da.HORIZONS:
        mdl, d, guess, frozen, roles = da.case_batch(name, N)
        ref = da.restated(name, N)
        w, y, z, direct, act, used = _solve(mdl, d, act=guess, frozen=frozen)
        for b in np.flatnonzero(direct == 1):
            st, vi, sg, co = da.kkt_certificate(mdl, d, w[b], y[b], b)
            print("%s N=%d %s  stat %.2e  viol %.2e  sign %.2e  compl %.2e" % (name, N, roles[b], st, vi, sg, co))
            assert max(st, vi, sg, co) <= CERT_BAR
            seen += 1
        if N == 20:
            continue
        acc = [b for b in np.flatnonzero(direct == 1) if roles[b] in ("tight", "wrong_guess", "tight2")]
        dd = {k: np.where(np.isnan(d[k][acc]), 0.0, d[k][acc]) for k in KEYS}      # unread slots: any value
        # (the identity and s_{k+1} entries of A are unread and NaN in random data: they are 1)
        dd["A"] = np.where(np.isnan(d["A"][acc]), 1.0, d["A"][acc])
        Psym = []
        for b in acc:
            Pd, S = dc.dense_from_csc(mdl.Pp, mdl.Pi, d["P"][b], mdl.n, mdl.n)
            Pd = np.nan_to_num(np.where(np.isnan(Pd), Pd.T, Pd), nan=0.0)
            Psym.append(np.array([Pd[mdl.Pi[e], j] for j in range(mdl.n) for e in range(mdl.Pp[j], mdl.Pp[j + 1])]))
        dd["P"] = np.array(Psym)
        pat = orc.Pattern(mdl.n, mdl.m, mdl.Pp, mdl.Pi, mdl.Ap, mdl.Ai)
        st_ = orc.default_settings()
        st_.eps_abs = st_.eps_rel = 1e-9; st_.max_iter = 200000
        out = pat.solve(*(dd[k] for k in KEYS), st_)
        assert (out["status"] == 1).all()
        for i, b in enumerate(acc):
            Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, dd["P"][i], mdl.n, mdl.n)
            Ad, _ = dc.dense_from_csc(mdl.Ap, mdl.Ai, dd["A"][i], mdl.m, mdl.n)
            xo, yo = out["x"][i], out["y"][i]
            nrm = lambda v: float(np.abs(v).max())      # noqa: E731
            eps = max(st_.eps_abs + st_.eps_rel * max(nrm(Ad @ xo), nrm(out["z"][i])),
                      st_.eps_abs + st_.eps_rel * max(nrm(Pd @ xo), nrm(Ad.T @ yo), nrm(d["q"][b])))
            tol = ref[b]["kinv_norm"] * eps
            err = np.abs(xo - w[b]).max()
            print("%s N=%d %s  |x_oracle - w| %.2e  (tolerance %.2e)" % (name, N, roles[b], err, tol))
            assert err <= tol
    assert seen > 0


def _host_loop(option, eps=None):
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, arg, x0 = da.recipe()
    opt = {"max_iter": da.RECIPE_ITERS, "alpha": 1.0}
    if option is not None:
        opt["direct_qp"] = option
    sol = SQPOptimizationSolver(mdl, opt, batch=da.RECIPE_B, qp_solver=OracleCuCaQP(da.RECIPE_B, nthreads=4))
    if eps is not None:
        sol.qpSolver_.setAbsoluteTolerance(eps); sol.qpSolver_.setRelativeTolerance(eps); sol.qpSolver_.setMaxIteration(200000)
    sol.setInitialGuess(x0)
    out = sol.getOptimalSolution(arg)
    return sol, np.array(out["x"], float)


def _kkt_bar(eps):
    """what a QP solver that stops at residuals eps_abs = eps_rel = eps may be away from the exact solution of the recipe's QP, in the infinity norm
    and at worst over the batch: |K^-1|_inf (eps + eps S), K the KKT matrix with the QP's active set as equalities (the accepting round's), S the
    largest of the norms the two stopping thresholds scale with, at the exact solution -- the bar of tests/test_direct_qp_host.py.  The model is
    linear and its cost quadratic: x + dw is the same point for every iterate x, so the QP at the start stands for every QP of the loop."""
    mdl, arg, x0 = da.recipe()
    ls = mdl.local_system(arg["p"], x0, arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"])
    w, y, z, direct, act, used = mdl.direct_qp_active(ls.P, ls.q, ls.A, ls.l, ls.u)
    assert (direct == 1).all()
    worst = 0.0
    for b in range(x0.shape[0]):
        Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, ls.P[b], mdl.n, mdl.n)
        Ad, _ = dc.dense_from_csc(mdl.Ap, mdl.Ai, ls.A[b], mdl.m, mdl.n)
        S = max(np.abs(v).max() for v in (Ad @ w[b], z[b], Pd @ w[b], Ad.T @ y[b], ls.q[b]))
        r = da.active_mp(mdl, ls.P[b], ls.q[b], ls.A[b], ls.l[b], ls.u[b], digits=None)
        assert r["direct"] == 1 and np.array_equal(r["act"], act[b])
        worst = max(worst, r["kinv_norm"] * (eps + eps * S))
    return worst


def test_host_loop_on_the_bound_riding_recipe(built):
    """|u| <= 1 saturates over the first part of every plan: direct_qp alone accepts nothing, with "active_set" every QP is accepted within the default 4 rounds
    (measured: 3 to 4 rounds for the first QP, 1 to 3 for the later ones, which start from the set handed on).  x ends within the QP tolerance of the loop without the option, at the
    reference's eps 1e-3 and with that loop's oracle at eps 1e-8: what a solver that stops at residuals eps may be away from the QP's solution
    (_kkt_bar: |K^-1|_inf is 8e5 on these QPs, so the bar is wide -- 1.6e3 and 1.6e-2; measured 1.2e-2 and 1.3e-5, about 1e3 eps, which is where
    an ADMM point at that tolerance lies on these QPs: the difference is the other loop's)."""
    sol, x = _host_loop({"active_set": True})
    alone, xa = _host_loop(True)
    plain, x0 = _host_loop(None)
    h = np.array(sol.direct_history); r = np.array(sol.direct_rounds_history)
    print("verdicts\n", h, "\nrounds\n", r, "\nwithout active_set\n", np.array(alone.direct_history))
    assert (np.array(alone.direct_history) == 0).all() and alone.direct_rounds_history == []
    assert h.shape == (da.RECIPE_ITERS, da.RECIPE_B) and (h == 1).all() and (r >= 1).all() and (r <= 4).all()
    assert plain.direct_history == [] and plain.direct_rounds_history == []
    mdl = sol.model
    u = x.reshape(da.RECIPE_B, mdl.N, mdl.f)[:, :, mdl.nx:]
    assert (np.abs(u).max(axis=(1, 2)) == 1.0).all()      # riding the bound, exactly on it
    for eps, (other, xo) in ((1e-3, (plain, x0)), (1e-8, _host_loop(None, eps=1e-8))):
        assert (np.asarray(other.last_qp_info["status"]) == 1).all()
        bar = _kkt_bar(eps)
        err = np.abs(x - xo).max()
        print("|x_active - x_plain at eps %.0e| %.3e (bar %.3e)" % (eps, err, bar))
        assert err <= bar
    assert all((np.asarray(it) == 0).all() for it in sol.admm_iterations)


def test_refusals():
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver, DIRECT_QP_REFUSES, _direct_qp_option, _direct_active_option
    from tests.support.oracle_backend import OracleCuCaQP
    mdl = dc.model("double_integrator", 3)
    d = dc.local_qp(mdl, 2)
    for kw in (dict(feas_tol=-1.0), dict(reg=np.nan), dict(dual_tol=-1e-9), dict(dual_tol=np.nan), dict(rounds=0), dict(rounds=9), dict(rounds=2.5)):
        with pytest.raises(ValueError):
            _solve(mdl, d, **kw)
    with pytest.raises(ValueError):
        mdl.direct_qp_active(d["P"][:, :-1], d["q"], d["A"], d["l"], d["u"])
    from tests.support import convexify_cases as cc
    link = cc.case("bump_link")["model"]
    with pytest.raises(ValueError) as e:
        link.direct_qp_active(np.zeros((1, len(link.Pi))), np.zeros((1, link.n)), np.zeros((1, len(link.Ai))), np.zeros((1, link.m)), np.zeros((1, link.m)))
    assert "link cost" in str(e.value)
    base = {"max_iter": 1, "alpha": 1.0}
    for bad in ({"active_set": 1.5}, {"active_set": True, "rounds": 0}, {"active_set": True, "rounds": 9}, {"active_set": True, "rounds": 2.5},
                {"active_set": True, "dual_tol": -1.0}, {"active_set": True, "dual_tol": np.nan}, {"rounds": 3}, {"dual_tol": 1e-9},
                {"active_set": False, "rounds": 3}, {"active_set": True, "round": 3}):
        with pytest.raises(ValueError):
            SQPOptimizationSolver(mdl, dict(base, direct_qp=bad), batch=1, qp_solver=OracleCuCaQP(1))
    on = {"active_set": True}
    # the refusals of direct_qp apply unchanged, with their reasons
    for key, why in DIRECT_QP_REFUSES.items():
        with pytest.raises(ValueError) as e:
            _direct_qp_option(dict(base, direct_qp=on, **{key: True}), mdl)
        assert str(e.value) == why
    with pytest.raises(ValueError) as e:
        _direct_qp_option(dict(base, direct_qp=on), link)
    assert "link cost" in str(e.value)
    with pytest.raises(ValueError) as e:
        _direct_qp_option(dict(base, direct_qp=on), mdl, evaluator=object())
    assert "stage OCPs" in str(e.value)
    assert _direct_active_option(dict(base)) is None and _direct_active_option(dict(base, direct_qp=True)) is None
    assert _direct_active_option(dict(base, direct_qp={"feas_tol": 1e-9})) is None
    assert _direct_active_option(dict(base, direct_qp={"active_set": False})) is None
    assert _direct_active_option(dict(base, direct_qp=on)) == (4, 0.0)
    assert _direct_active_option(dict(base, direct_qp={"active_set": True, "rounds": 8, "dual_tol": 1e-9})) == (8, 1e-9)
    assert _direct_qp_option(dict(base, direct_qp={"active_set": True, "feas_tol": 1e-9}), mdl) == (1e-9, 0.0)


def test_abi(built):
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert "int mpcqp_stage_riccati_solve_active(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_active_args *a, void *stream);" in header
    assert "mpcqp_stage_riccati_solve_active" in _lib.EXPORTS
    assert "#define MPCQP_ACTIVE_MAX_ROUNDS %d" % _lib.ACTIVE_MAX_ROUNDS in header
    import ctypes as C
    from optimal_control_problem_amd import stage_eval as se
    cname, cls = "mpcqp_stage_riccati_solve_active_args", _lib.RiccatiSolveActiveArgs
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?\b([a-z_0-9A-Z]+)\s*[,;]", body)
    assert names == [f[0] for f in cls._fields_], (names, [f[0] for f in cls._fields_])
    # the leading fields are those of mpcqp_stage_riccati_solve_args, at the same offsets
    for fld in ("P", "q", "A", "l", "u", "feas_tol", "reg", "frozen", "w", "y", "z", "direct"):
        assert getattr(cls, fld).offset == getattr(se.RiccatiSolveArgs, fld).offset
    assert C.sizeof(cls) == 17 * 8 and cls.rounds.offset == 96 and cls.dual_tol.offset == 104 and cls.act_in.offset == 112 and cls.rounds_used.offset == 128
    L = se._bind(_lib.lib())
    assert L.mpcqp_stage_riccati_solve_active(None, 1, None, None) == _lib.ERR_ARG
    assert b"stage handle is null" in L.mpcqp_strerror(_lib.ERR_ARG)
    hpp = open(os.path.join(ROOT, "optimal_control_problem_amd", "csrc", "stage_riccati_active.hpp")).read()
    assert "using C = stage_dir<W, FM>;" in hpp and "__syncthreads_and(!open)" in hpp
