"""CPU: the feedback gains along the plan (mpcqp_stage_riccati / mpcqp_stage_feedback) -- the NumPy statements models.StageOCP.riccati_gains and
feedback against a 60-digit restatement of the rule and against the algebra the rule must satisfy, the clamp, the failure and frozen rules, the
refusals, ClosedLoopMPC's argument checks, the ABI, and the recipe that motivates it on the CPU oracle."""
import os
import re

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from tests.support import riccati_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = rc.bits


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("N", rc.HORIZONS)
@pytest.mark.parametrize("name", rc.MODELS)
def test_statement_against_60_digits(name, N):
    """riccati_gains against the restatement in mpmath, on local systems at drawn iterates and on random data on the same patterns; the statement's
    own error e_np is printed and may not exceed rc.E_NP, the figure the device bar is derived from"""
    mdl = rc.model(name, N)
    B = 2
    for kind, d in (("local", rc.local_data(mdl, B)), ("random", rc.random_data(mdl, B))):
        g = mdl.riccati_gains(d["P"], d["A"])
        assert (g["failed"] == -1).all() and np.isfinite(g["K"]).all() and np.isfinite(g["V"]).all()
        for b in range(B):
            K, V, failed = rc.riccati_mp(mdl, d["P"][b], d["A"][b])
            eK, eV = rc.rel_err(g["K"][b], K), rc.rel_err(g["V"][b], V)
            print(name, N, kind, b, "e_np: K %.2e V %.2e" % (eK, eV))
            assert failed == -1 and eK <= rc.E_NP and eV <= rc.E_NP, (name, N, kind, b, eK, eV)
    # with the clamp, the regularisation and the pinned first frame
    d = rc.local_data(mdl, B)
    g = mdl.riccati_gains(d["P"], d["A"], x=d["x"], lbx=d["lbx"], ubx=d["ubx"], clamp_tol=1e-9, reg=1e-3)
    K, V, failed = rc.riccati_mp(mdl, d["P"][0], d["A"][0], x=d["x"][0], lbx=d["lbx"][0], ubx=d["ubx"][0], clamp_tol=1e-9, reg=1e-3)
    assert failed == -1 and rc.rel_err(g["K"][0], K) <= rc.E_NP and rc.rel_err(g["V"][0], V) <= rc.E_NP
    assert (g["K"][:, 0] == 0.0).all()


def test_slot_tables_agree_with_the_pattern():
    for name in rc.MODELS:
        mdl = rc.model(name, 3)
        ps, as_ = mdl._riccati_slots()
        ps2, as2 = rc.slots_from_pattern(mdl)
        assert np.array_equal(ps, ps2) and np.array_equal(as_, as2)
        assert (as_ >= 0).all() and (ps[:, np.arange(mdl.f), np.arange(mdl.f)] >= 0).all()


def test_double_integrator_gain_is_the_riccati_fixed_point():
    """constant weights, N = 60: K_1 is the 58th iterate of the discrete Riccati equation from V = Q (to rounding), and that sequence has all but
    reached its fixed point, iterated here to convergence: a horizon of 60 frames leaves 7e-7 of K_inf (the iteration contracts by about 0.88 a
    step), so the bar against the fixed point is 1e-5, the one against the test's own 58th iterate 1e-11.  The cost is sum Q e^2 + R u^2: H = 2 diag(Q, R)"""
    mdl = models.DoubleIntegrator(60)
    d = rc.local_data(mdl, 1)
    g = mdl.riccati_gains(d["P"], d["A"])
    J = mdl.dF(np.zeros((1, 2)), np.zeros((1, 1)))[0]
    A, Bm = J[:, :2], J[:, 2:]
    Q, R = 2.0 * np.diag(mdl.Qk[0]), 2.0 * np.diag(mdl.Rk[0])
    gain = lambda V: -np.linalg.solve(R + Bm.T @ V @ Bm, Bm.T @ V @ A)
    V, K58 = Q.copy(), None
    for it in range(1, 100000):
        K = gain(V)
        if it == mdl.N - 2:
            K58 = K
        Vn = Q + A.T @ V @ A + A.T @ V @ Bm @ K
        Vn = 0.5 * (Vn + Vn.T)
        done = np.abs(Vn - V).max() <= 1e-14 * np.abs(Vn).max()
        V = Vn
        if done and K58 is not None:
            break
    Kinf = gain(V)
    e58 = np.abs(g["K"][0, 1] - K58).max() / np.abs(K58).max()
    einf = np.abs(g["K"][0, 1] - Kinf).max() / np.abs(Kinf).max()
    print("iterations", it, "K_inf", Kinf, "K_1", g["K"][0, 1], "against the 58th iterate", e58, "against the fixed point", einf)
    assert e58 <= 1e-11 and einf <= 1e-5


def test_value_matrices_are_symmetric_bit_for_bit_and_last_gain_is_zero():
    for name in rc.MODELS:
        mdl = rc.model(name, 20)
        d = rc.local_data(mdl, 2)
        g = mdl.riccati_gains(d["P"], d["A"])
        assert _same(g["V"], g["V"].transpose(0, 1, 3, 2))
        if not mdl.general_cost:                       # a diagonal cost has no Q_us in the last frame
            assert (g["K"][:, -1] == 0.0).all()
        else:
            assert np.abs(g["K"][:, -1]).max() > 0.0


def _without_input(mdl, d, k, i):
    """the data of the problem in which input i of frame k cannot move: its column of B_k removed (zeroed) and its cross terms with the other
    variables of the frame removed from H_k"""
    ps, as_ = mdl._riccati_slots()
    P, A = d["P"].copy(), d["A"].copy()
    c = mdl.nx + i
    A[:, as_[k, :, c]] = 0.0
    for r in range(mdl.f):
        if r != c:
            for e in (ps[k, r, c], ps[k, c, r]):
                if e >= 0:
                    P[:, e] = 0.0
    return P, A


@pytest.mark.parametrize("name", ("quadrotor", "coupled_pendulum", "linear16x8"))
def test_clamp(name):
    mdl = rc.model(name, 20)
    B, k, i = 2, 7, mdl.nu - 1
    d = rc.local_data(mdl, B)
    X = d["x"].reshape(B, mdl.N, mdl.f)
    lbx, ubx = d["lbx"].copy(), d["ubx"].copy()
    e = k * mdl.f + mdl.nx + i
    ubx[:, e] = X[:, k, mdl.nx + i]                    # the input sits on its upper bound
    g = mdl.riccati_gains(d["P"], d["A"], x=d["x"], lbx=lbx, ubx=ubx)
    assert (g["failed"] == -1).all()
    assert (g["K"][:, k, i] == 0.0).all() and (g["K"][:, 0] == 0.0).all()      # the clamped row, and the pinned first frame
    free = mdl.riccati_gains(d["P"], d["A"], x=d["x"], lbx=d["lbx"], ubx=d["ubx"])
    assert np.abs(free["K"][:, k, i]).max() > 0.0
    # the other rows are the gains of the problem without that input's column of B_k
    P2, A2 = _without_input(mdl, d, k, i)
    ref = mdl.riccati_gains(P2, A2, x=d["x"], lbx=d["lbx"], ubx=d["ubx"])
    others = [j for j in range(mdl.nu) if j != i]
    for arr, sel in (("K", (slice(None), slice(None, k + 1), others)), ("V", (slice(None), slice(None, k + 1)))):
        if arr == "K" and not others:                  # a single input: nothing left to compare but V
            continue
        err = rc.rel_err(g[arr][sel], ref[arr][sel])
        print(name, arr, "clamped against the reduced problem", err)
        assert err <= rc.DEVICE_BAR
    assert _same(g["K"][:, k + 1:], free["K"][:, k + 1:])                    # the frames above do not know


@pytest.mark.parametrize("bad", (-1.0, np.nan))
def test_failure(bad):
    mdl = rc.model("quadrotor", 20)
    B, k = 3, 11
    d = rc.local_data(mdl, B)
    ps, _ = mdl._riccati_slots()
    P = d["P"].copy()
    P[1, ps[k, mdl.nx + 2, mdl.nx + 2]] = bad         # one uu diagonal slot of frame k, instance 1
    g = mdl.riccati_gains(P, d["A"])
    ref = mdl.riccati_gains(d["P"], d["A"])
    assert g["failed"].tolist() == [-1, k, -1]
    assert (g["K"][1, :k + 1] == 0.0).all() and (g["V"][1, :k + 1] == 0.0).all()
    assert _same(g["K"][1, k + 1:], ref["K"][1, k + 1:]) and _same(g["V"][1, k + 1:], ref["V"][1, k + 1:])
    assert _same(g["K"][[0, 2]], ref["K"][[0, 2]]) and _same(g["V"][[0, 2]], ref["V"][[0, 2]])
    K, V, failed = rc.riccati_mp(mdl, P[1], d["A"][1])
    assert failed == k


def test_frozen_and_reg():
    mdl = rc.model("cartpole", 3)
    d = rc.local_data(mdl, 4)
    ref = mdl.riccati_gains(d["P"], d["A"])
    g = mdl.riccati_gains(d["P"], d["A"], frozen=np.array([0, 1, 0, 5], np.int32))
    assert (g["K"][[1, 3]] == 0.0).all() and (g["V"][[1, 3]] == 0.0).all() and (g["failed"] == -1).all()
    assert _same(g["K"][[0, 2]], ref["K"][[0, 2]])
    # reg on the diagonal of Q_uu is the same as a heavier input weight in every frame
    ps, _ = mdl._riccati_slots()
    P = d["P"].copy()
    for k in range(mdl.N):
        P[:, ps[k, mdl.nx, mdl.nx]] += 0.25
    a, b = mdl.riccati_gains(d["P"], d["A"], reg=0.25), mdl.riccati_gains(P, d["A"])
    assert _same(a["K"], b["K"]) and _same(a["V"], b["V"]) and not _same(a["K"], ref["K"])


def test_feedback_statement():
    mdl = rc.model("quadrotor", 3)
    B, nx, nu, f = 5, mdl.nx, mdl.nu, mdl.f
    rng = np.random.default_rng(3)
    K = rng.normal(size=(B, 3, nu, nx)); s = rng.normal(size=(B, nx)); sn = rng.normal(size=(B, nx)); un = rng.normal(size=(B, nu))
    out = mdl.feedback(K, 1, s, sn, un)
    ref = un + np.einsum("bij,bj->bi", K[:, 1], s - sn)
    assert np.abs(out["u"] - ref).max() <= 1e-13 and _same(out["du"], out["u"] - un)
    lo, hi = np.full((B, nu), -0.5), np.full((B, nu), 0.5)
    x = rng.normal(size=(B, mdl.nvar)); lbx = x - 1.0; ubx = x + 1.0
    c = mdl.feedback(K, 1, s, sn, un, lo=lo, hi=hi, x=x, lbx=lbx, ubx=ubx)
    assert _same(c["u"], np.clip(out["u"], -0.5, 0.5)) and (np.abs(out["u"]) > 0.5).any()
    for key, src in (("x", x), ("lbx", lbx), ("ubx", ubx)):
        assert _same(c[key][:, nx:f], c["u"])
        keep = np.ones(mdl.nvar, bool); keep[nx:f] = False
        assert _same(c[key][:, keep], src[:, keep])
    # a zero gain is the plan's input
    assert _same(mdl.feedback(np.zeros_like(K), 2, s, sn, un)["u"], un)


def test_refusals():
    mdl = rc.model("double_integrator", 3)
    d = rc.local_data(mdl, 2)
    for kw in (dict(x=d["x"]), dict(x=d["x"], lbx=d["lbx"]), dict(lbx=d["lbx"], ubx=d["ubx"]), dict(clamp_tol=-1.0), dict(reg=-1e-3), dict(reg=np.nan)):
        with pytest.raises(ValueError):
            mdl.riccati_gains(d["P"], d["A"], **kw)
    with pytest.raises(ValueError):
        mdl.riccati_gains(d["P"][:, :-1], d["A"])
    from tests.support import convexify_cases as cc
    link = cc.case("bump_link")["model"]
    with pytest.raises(ValueError) as e:
        link.riccati_gains(np.zeros((1, len(link.Pi))), np.zeros((1, len(link.Ai))))
    assert "link cost" in str(e.value)
    K = np.zeros((2, 3, 1, 2)); z = np.zeros((2, 2)); u = np.zeros((2, 1))
    for k in (-1, 3):
        with pytest.raises(ValueError):
            mdl.feedback(K, k, z, z, u)
    with pytest.raises(ValueError):
        mdl.feedback(K, 0, z, z, u, lo=u)
    with pytest.raises(ValueError):
        mdl.feedback(K, 0, z, z, u, lbx=d["lbx"])


def test_closed_loop_argument_checks():
    """the checks of ClosedLoopMPC(feedback=...) that run before anything touches a device"""
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl = rc.model("double_integrator", 3)
    for bad in (False, 1, "yes", {"gain": 1.0}, {"reg": -1.0}, {"clamp_tol": -1e-9}):
        with pytest.raises(ValueError):
            ClosedLoopMPC(mdl, batch=1, feedback=bad)
    from tests.support import convexify_cases as cc
    with pytest.raises(ValueError) as e:
        ClosedLoopMPC(cc.case("bump_link")["model"], batch=1, feedback=True)
    assert "link cost" in str(e.value)


def test_abi(built):
    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert "int mpcqp_stage_riccati(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_args *a, void *stream);" in header
    assert "int mpcqp_stage_feedback(mpcqp_stage *s, int batch, const mpcqp_stage_feedback_args *a, void *stream);" in header
    assert "mpcqp_stage_riccati" in _lib.EXPORTS and "mpcqp_stage_feedback" in _lib.EXPORTS
    m = re.search(r"#define MPCQP_RICCATI_PIVOT (\S+)", header)
    assert float(m.group(1)) == models.StageOCP.RICCATI_PIVOT == rc.PIVOT
    from optimal_control_problem_amd import stage_eval as se
    for cname, cls in (("mpcqp_stage_riccati_args", se.RiccatiArgs), ("mpcqp_stage_feedback_args", se.FeedbackArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"\*?\b([a-z_0-9A-Z]+)\s*[,;]", body)
        assert names == [f[0] for f in cls._fields_], (names, [f[0] for f in cls._fields_])
    L = se._bind(_lib.lib())
    assert L.mpcqp_stage_riccati(None, 1, None, None) == _lib.ERR_ARG
    assert L.mpcqp_stage_feedback(None, 1, None, None) == _lib.ERR_ARG
    assert [se.riccati_groups_per_block(f) for f in (3, 8, 9, 16, 17, 24)] == [16, 16, 4, 4, 2, 2]
    hpp = open(os.path.join(ROOT, "optimal_control_problem_amd", "csrc", "stage_riccati.hpp")).read()
    assert "static_assert(G * tile * 8 <= 48 * 1024" in hpp


def test_recipe_gains_beat_open_loop_holds(built):
    """double integrator, 8 instances, N = 20 on the host SQP loop over the CPU oracle: solve, then four holds with an impulse on the first.  In
    EVERY instance the plant ends nearer the plan with the gains than with open-loop holds"""
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, frame0, w = rc.recipe()
    dev_fb, cost_fb = rc.recipe_host(mdl, frame0, w, OracleCuCaQP(rc.RECIPE_B, nthreads=4), True)
    dev_ol, cost_ol = rc.recipe_host(mdl, frame0, w, OracleCuCaQP(rc.RECIPE_B, nthreads=4), False)
    print("deviation with gains", dev_fb, "open loop", dev_ol, "ratio", dev_fb / dev_ol)
    assert (dev_fb < dev_ol).all()
    assert (dev_fb / dev_ol).max() < 0.5               # with room to spare: measured 0.391 in every instance
