"""CPU: the NumPy statement (models.StageOCP, general_nlp.GeneralNLP) against the independent high-precision restatement
(tests/support/nlp_hp.py; cases in tests/support/hp_cases.py), and the reference against itself.  tests/test_gpu_nlp_hp.py holds the kernels
against the same references.

The reference works with 60 digits and the step 1e-15 (truncation and rounding both ~1e-30).  Measured here, on one case per term kind
(`hp_cases.TERM_KINDS`) and before the rounding to float64: with 120 digits and the step 1e-16 no value the reference returns -- P, q, A, l, u, f,
the violations of every row, the convexified P and lam_min -- moves by more than 1.7e-27 max(1, |ref|) (allowed: 1e-16).  So the reference
contributes nothing to a comparison at the project's bar, 1e-12 max(1, |ref|).  The statement's largest measured distances: P 3.2e-14
(`every4`, an instance far outside its bounds), A 5.6e-15, q 2.9e-15, l and u 2.1e-15, f, l1, gmax and the line search's phi 4.4e-16, the hand-over
3.7e-15; the convexified P 3.2e-3 and lam_min 4.5e-4 of their bar 1e-12 max(1, ||H_k||_F).

Differencing is over the whole of w for n <= 20 and term by term above it (cartpole3_pfw, quadrotor2, quadrotor2_pfw, link_smooth_tracking,
link_general_tracking, link_quadrotor, every4, every_pf3, every_pf4, bump_pf, quad_dense, wide: whole-vector differencing of n = 44 .. 56 costs
tens of seconds an instance); each test prints which.  The two routes agree to 1e-16 where both run
(test_whole_vector_and_term_by_term_differencing_agree).  The general problems are always differenced over the whole of w."""
import numpy as np
import pytest
from mpmath import mp

from tests.support import convexify_cases as cc
from tests.support import general_problems as gp
from tests.support import hp_cases as hc
from tests.support import nlp_hp as hp

TOL = hc.TOL
SELF = 1e-16


def _statement_system(c):
    with hc.rows_on_statement(c) as mdl:
        ls = mdl.local_system(*hc.args(c))
    return dict(P=ls.P, q=ls.q, A=ls.A, l=ls.l, u=ls.u)


# ------------------------------------------------------------------------------------------------ 0. the scalar
def test_the_scalar_computes_in_the_working_precision_and_leaves_it_unchanged():
    before = mp.dps
    S = hc.restatement("di2")
    S.merit(*[hc.case("di2")[k][:1] for k in ("p", "x", "lbx", "ubx")])
    assert mp.dps == before
    with mp.workdps(50):
        x = hp.HP(0.3)
        a = np.empty((), object); a[()] = x
        third = hp.HP(1.0) / 3
        assert abs(third.v * 3 - 1) < mp.mpf(10) ** -48                      # not a double's third
        for got, want in ((np.float64(2.0) * x, 2 * x.v), (x * np.float64(2.0), 2 * x.v), (a * x, x.v * x.v), (x * a, x.v * x.v), (2 - a, 2 - x.v),
                          (x ** 3, x.v ** 3), (a ** 2, x.v ** 2), (1.0 / x, 1 / x.v), (-x, -x.v), (np.negative(x), -x.v), (np.square(x), x.v ** 2)):
            assert isinstance(got, hp.HP) and got.v == want
        for name in ("sin", "cos", "tan", "exp", "log", "sqrt", "tanh"):
            want = getattr(mp, name)(x.v)
            assert getattr(np, name)(x).v == want and getattr(np, name)(a).v == want
        v = np.stack([x, a * 2.0], axis=-1)
        assert v.shape == (2,) and v[..., 1][()].v == 2 * x.v and (v + 0.5 * v)[0].v == x.v + x.v / 2


# ------------------------------------------------------------------------------------------------ 1. the reference against itself
@pytest.mark.parametrize("name", hc.TERM_KINDS)
def test_reference_self_accuracy(name):
    """twice the digits and a tenth of the step: no value moves by more than 1e-16 max(1, |ref|).  Compared before the rounding to float64 (raw):
    the reference's own error is what is measured, and a value on a float64 rounding tie -- the exact gradient of a quadratic is one often --
    would move by a whole ulp, 1.1e-16, on an error of 1e-30"""
    c = hc.case(name)
    sl = slice(1, 3) if c["kind"] == "convexify" else slice(0, 2)          # (a convex and a non-convex instance)
    one = {k: (None if c[k] is None else c[k][sl]) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg", "theta", "plant", "d")}
    worst = 0.0
    refs = []
    for kw in (dict(), dict(dps=2 * hp.DPS, step="1e-16")):
        S = hp.Stage(c["model"], theta=one["theta"], sdata=one["d"], plant=one["plant"], raw=True, **kw)
        r = S.system(*[one[k] for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")])
        r.update({"m_" + k: v for k, v in S.merit(one["p"], one["x"], one["lbx"], one["ubx"]).items()})
        if c["model"].convexify:
            for mode in hc.MODES:
                cv = S.convexify(one["p"], one["x"], r["P"], mode, hc.EPS)
                r["cvx_" + mode] = cv["P"]; r["lam_" + mode] = cv["lam_min"]
        refs.append(r)
    for k in refs[0]:
        d = hp.raw_distance(refs[1][k], refs[0][k])
        worst = max(worst, d)
        assert d <= SELF, (name, k, d)
    print(name, "largest difference between the two references %.2e" % worst)


def test_whole_vector_and_term_by_term_differencing_agree():
    """the scatter arithmetic of the term-wise route against no scatter at all, on the model with every kind of term"""
    c = hc.case("every_pf2")
    a = hc.restatement("every_pf2", whole=True, raw=True).system(*[v[:2] for v in hc.args(c)])
    b = hc.restatement("every_pf2", whole=False, raw=True).system(*[v[:2] for v in hc.args(c)])
    for k in ("P", "q", "A", "l", "u", "f"):
        assert hp.raw_distance(a[k], b[k]) <= SELF, k


# ------------------------------------------------------------------------------------------------ 2. the statement against the reference
@pytest.mark.parametrize("name", hc.STAGE + hc.CONVEXIFY)
def test_statement_local_system_objective_and_violation(name):
    c = hc.case(name)
    mdl = c["model"]
    ref = hc.ref_system(name)
    got = _statement_system(c)
    S = hc.restatement(name)
    assert (S.n, S.m, S.np, S.ng) == (mdl.n, mdl.m, mdl.np, mdl.ng)
    d = hc.system_distances(mdl, got, ref)
    mr = hc.ref_merit(name)
    with hc.rows_on_statement(c):
        f = mdl.objective(c["p"], c["x"]); v, g = mdl.violation(c["x"], c["lbx"], c["ubx"])
    d.update(f=hp.distance(f, mr["f"]), l1=hp.distance(v, mr["l1"]), gmax=hp.distance(g, mr["gmax"]), f_sys=hp.distance(ref["f"], mr["f"]))
    print(name, "n", mdl.n, "whole-vector" if S.whole else "term by term", " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)
    # the pattern misses nothing: where the CSC pattern has no slot the reference is zero
    for b in range(ref["q"].shape[0]):
        _, Pm, Am = hc.dense_system(mdl, got["P"], got["q"], got["A"], got["l"], got["u"], b)
        for M, R, what in ((Pm, ref["P"][b], "P"), (Am, ref["A"][b], "A")):
            assert np.abs(R[~M]).max(initial=0.0) <= 1e-14 * np.abs(R).max(), (name, what, b)
    # the bounds of the general rows, read from the model's plain attributes, are the ones the cases hand to the kernels
    lo, hi = S.row_bounds()
    assert np.array_equal(np.broadcast_to(lo, c["lbg"].shape), c["lbg"]) and np.array_equal(np.broadcast_to(hi, c["ubg"].shape), c["ubg"])


@pytest.mark.parametrize("name", hc.STAGE)
def test_points_lie_on_both_sides_of_every_bound(name):
    """every box, path and link row with a finite bound is violated in one instance and satisfied in another; the dynamics rows are violated
    everywhere (a random iterate); l and u are finite exactly where the bounds are"""
    c = hc.case(name)
    S = hc.restatement(name)
    rows = hc.ref_merit(name)["rows"]
    nvar = S.nvar
    lo, hi = S.row_bounds()
    bounded = np.concatenate([np.isfinite(c["lbx"]).any(axis=0) | np.isfinite(c["ubx"]).any(axis=0), np.isfinite(lo) | np.isfinite(hi)])
    dyn = slice(nvar, nvar + (S.N - 1) * S.nx)
    assert (rows[:, dyn] > 0).all()
    other = bounded.copy(); other[dyn] = False
    assert (rows[:, other] > 0).any(axis=0).all(), (name, np.nonzero(~(rows[:, other] > 0).any(axis=0))[0])
    assert (rows[:, other] == 0).any(axis=0).all(), (name, np.nonzero(~(rows[:, other] == 0).any(axis=0))[0])
    assert (rows[:, ~bounded] == 0).all()
    ref = hc.ref_system(name)
    want_l = np.concatenate([np.ones_like(c["p"], bool), np.isfinite(c["lbx"]), np.isfinite(c["lbg"])], axis=1)
    want_u = np.concatenate([np.ones_like(c["p"], bool), np.isfinite(c["ubx"]), np.isfinite(c["ubg"])], axis=1)
    assert np.array_equal(np.isfinite(ref["l"]), want_l) and np.array_equal(np.isfinite(ref["u"]), want_u)


# ------------------------------------------------------------------------------------------------ 3. the line search
@pytest.mark.parametrize("name", hc.STAGE + hc.LONG)
def test_statement_line_search(name):
    c = hc.case(name)
    mdl = c["model"]
    q, dw, y = hc.step(name)
    ref = hc.ref_line_search(name)
    mu = hc.MU0.copy()
    with hc.rows_on_statement(c):
        got = mdl.line_search(c["p"], c["x"].copy(), c["lbx"], c["ubx"], q, dw, y, status=c["status"], mu=mu, alpha0=1.0, candidates=hc.CANDIDATES)
    ok = np.isin(c["status"], hp.OK)
    assert ok.any() and (~ok).any()
    # the reference alone: no instance inside the margin, so no decision is left out
    near, same = hc.decision_check(got["accepted"], ref)
    assert not near.any(), (name, ref["margin"])
    assert same, (name, got["accepted"], ref["accepted"])
    assert np.array_equal(got["alpha"], ref["alpha"]) and (ref["accepted"][~ok] == -2).all()
    rows = np.arange(len(ok))
    sel = np.where(ref["accepted"] >= 0, ref["accepted"] + 1, np.where(ref["accepted"] == -1, hc.CANDIDATES, 0))
    d = dict(mu=hp.distance(got["mu"], ref["mu"]), phi0=hp.distance(got["phi"][:, 0], ref["phis"][:, 0]), phi1=hp.distance(got["phi"][:, 1], ref["phis"][rows, sel]),
             f=hp.distance(got["f"], ref["fs"][rows, sel]), gmax=hp.distance(got["gmax"], ref["gmaxs"][rows, sel]))
    print(name, "accepted", ref["accepted"], " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)
    assert len(set(ref["accepted"][ok])) > 1 or name in hc.LONG, (name, ref["accepted"])      # the search reaches several candidates


# ------------------------------------------------------------------------------------------------ 4. convexification
@pytest.mark.parametrize("mode", hc.MODES)
@pytest.mark.parametrize("name", hc.CONVEXIFY + hc.EVERY)
def test_statement_convexify(name, mode):
    c = hc.case(name)
    mdl = c["model"]
    ref = hc.ref_convexify(name, mode)
    with hc.rows_on_statement(c):
        P0 = mdl.local_system(*hc.args(c)).P
        P1, touched, lam = mdl.convexify_system(c["p"], c["x"], P0, mode, hc.EPS)
    bar_frame, bar_inst = cc.bar({"hnorm": ref["hnorm"]})
    assert (np.abs(ref["lam_min"] - hc.EPS) > 1e-3).all()                   # the points keep every eigenvalue away from eps
    assert np.array_equal(touched, ref["touched"]) and (ref["touched"] == 0).any() and (ref["touched"] > 0).any()
    dl = np.abs(lam - ref["lam_min"]) / bar_frame
    dP = np.array([np.abs(hp.dense(mdl.Pp, mdl.Pi, P1[b], mdl.n)[0] - ref["P"][b]).max() for b in range(len(touched))]) / bar_inst
    print(name, mode, "touched", ref["touched"], "max |P - ref| / bar %.2e  max |lam_min - ref| / bar %.2e" % (dP.max(), dl.max()))
    assert (dl <= 1.0).all() and (dP <= 1.0).all()
    for b in range(len(touched)):                                           # the closed pattern has a slot for every entry of the correction
        M = hp.dense(mdl.Pp, mdl.Pi, P1[b], mdl.n)[1]
        assert np.abs(ref["P"][b][~M]).max(initial=0.0) <= 1e-14 * np.abs(ref["P"][b]).max()


# ------------------------------------------------------------------------------------------------ 5. the hand-over
@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("tail", ["rollout", "repeat"])
@pytest.mark.parametrize("name", hc.ADVANCE)
def test_statement_advance(name, tail, measured):
    c = hc.case(name)
    mdl = c["model"]
    ref = hc.ref_advance(name, tail, measured)
    with hc.rows_on_statement(c, plant=True):
        got = mdl.advance(c["x"], c["lbx"], c["ubx"], status=c["status"], s_meas=c["s_meas"] if measured else None, w=None if measured else c["w"],
                          tail=tail, p=c["p"])
    if c["plant"] is not None:
        assert (np.abs(c["plant"] - c["theta"]).max(axis=1) > 1e-3).all()                # the plant's parameters are not the model's
    d = {k: hp.distance(got[k], ref[k]) for k in ("applied", "x", "stage_cost")}
    print(name, tail, measured, " ".join("%s %.2e" % kv for kv in d.items()))
    assert d["applied"] == 0.0 and d["x"] <= TOL and d["stage_cost"] <= TOL
    f = mdl.f
    assert np.array_equal(got["lbx"][:, :f], got["x"][:, :f]) and np.array_equal(got["ubx"][:, :f], got["x"][:, :f])
    if measured:
        assert np.array_equal(got["x"][:, :mdl.nx], c["s_meas"])


# ------------------------------------------------------------------------------------------------ 6. the general path
@pytest.mark.parametrize("name", hc.GENERAL)
def test_statement_general_problem(name):
    c = hc.general_case(name)
    m = c["model"]
    ref = hc.ref_general(name)
    ls = m.local_system(*hc.args(c))
    d = hc.system_distances(m, dict(P=ls.P, q=ls.q, A=ls.A, l=ls.l, u=ls.u), ref)
    d.update(f=hp.distance(m.objective(c["p"], c["x"]), ref["f"]), gmax=hp.distance(gp.violation(m, c["p"], c["x"], c["lbg"], c["ubg"]), ref["gmax"]))
    print(name, "n", m.n, "whole-vector", " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)
    assert (ref["gmax"] > 0).any()
    for b in range(ref["q"].shape[0]):
        _, Pm, Am = hc.dense_system(m, ls.P, ls.q, ls.A, ls.l, ls.u, b)
        assert np.abs(ref["P"][b][~Pm]).max(initial=0.0) <= 1e-14 * np.abs(ref["P"][b]).max()
        assert np.abs(ref["A"][b][~Am]).max(initial=0.0) <= 1e-14 * np.abs(ref["A"][b]).max()
