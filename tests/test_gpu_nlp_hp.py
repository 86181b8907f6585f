"""GPU: the stage kernels (mpcqp_stage_eval, _merit, _linesearch, _convexify, _advance) and the general evaluator (mpcqp_nlp_eval, _merit)
against the independent high-precision restatement of the NLP (tests/support/nlp_hp.py; cases and references in tests/support/hp_cases.py).

Every other GPU test of these kernels compares with the NumPy statement in models.StageOCP, which shares its tapes and its assembly tables with
what the kernels were written against.  The references here share nothing: 60-digit differences of the model's user callbacks
(tests/test_nlp_hp_host.py measures their own error: none at float64).  Bars: 1e-12 max(1, |ref|) for P, q, A, l, u, f, the violations and the
merit values, convexify_cases.bar for everything behind the eigen-solve, equal non-finite patterns, bit for bit for what is copied or
must stay untouched.  Outputs are NaN-filled before every launch.  Each test prints its largest measured distance."""
import numpy as np
import pytest

from tests.support import convexify_cases as cc
from tests.support import hp_cases as hc
from tests.support import nlp_hp as hp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = hc.TOL


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def evaluators(built):
    """one evaluator per case for the whole module; every test leaves it with nothing set"""
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    evs = {}
    yield lambda name: evs[name] if name in evs else evs.setdefault(name, StageEvaluator(hc.case(name)["model"]))
    for ev in evs.values():
        ev.close()


class _rows:
    """the case's rows on the evaluator for the duration of a block (plant: the plant's rows as well)"""

    def __init__(self, ev, c, plant=False):
        self.ev, self.c, self.plant = ev, c, plant

    def __enter__(self):
        ev, c = self.ev, self.c
        mdl = c["model"]
        assert ev.nsd == (mdl.nsd if c["d"] is not None else 0) and ev.param_count == (mdl.ntheta if c["theta"] is not None else 0)
        assert (ev.n, ev.m, ev.np, ev.nnzP, ev.nnzA) == (mdl.n, mdl.m, mdl.np, len(mdl.Pi), len(mdl.Ai))
        assert np.array_equal(ev.Pp, mdl.Pp) and np.array_equal(ev.Pi, mdl.Pi) and np.array_equal(ev.Ap, mdl.Ap) and np.array_equal(ev.Ai, mdl.Ai)
        if c["d"] is not None:
            ev.set_stage_data(c["d"])
        if c["theta"] is not None:
            ev.set_instance_params(c["theta"])
            if self.plant:
                ev.set_instance_params(c["plant"], plant=True)
        return ev

    def __exit__(self, *exc):
        ev, c = self.ev, self.c
        if c["d"] is not None:
            ev.set_stage_data(None)
        if c["theta"] is not None:
            ev.set_instance_params(None)
            if self.plant:
                ev.set_instance_params(None, plant=True)
        return False


def _eval(ev, c):
    out = ev.alloc(c["x"].shape[0])
    for v in out.values():
        v.fill_(float("nan"))
    ev.eval(*[_dev(a) for a in hc.args(c)], out=out)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ 1. mpcqp_stage_eval
@pytest.mark.parametrize("name", hc.STAGE + hc.CONVEXIFY)
def test_eval(evaluators, name):
    c = hc.case(name)
    ref = hc.ref_system(name)
    with _rows(evaluators(name), c) as ev:
        got = {k: v.cpu().numpy() for k, v in _eval(ev, c).items()}
    d = hc.system_distances(c["model"], got, ref)
    print(name, "library" if ev.library else "zoo", "PF" if ev.per_frame_reference else "shared", "theta %d data %d" % (ev.param_count, ev.nsd),
          " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)


# ------------------------------------------------------------------------------------------------ 2. mpcqp_stage_merit
@pytest.mark.parametrize("name", hc.STAGE + hc.LONG)
def test_merit(evaluators, name):
    c = hc.case(name)
    ref = hc.ref_merit(name)
    with _rows(evaluators(name), c) as ev:
        f, g = ev.merit(_dev(c["p"]), _dev(c["x"]))
        torch.cuda.synchronize()
    d = dict(f=hp.distance(f.cpu().numpy(), ref["f"]), gmax=hp.distance(g.cpu().numpy(), ref["gmax"]))
    print(name, " ".join("%s %.2e" % kv for kv in d.items()))
    assert d["f"] <= TOL and d["gmax"] <= TOL, (name, d)


# ------------------------------------------------------------------------------------------------ 3. mpcqp_stage_linesearch
@pytest.mark.parametrize("name", hc.STAGE + hc.LONG)
def test_linesearch(evaluators, name):
    """phi, f and gmax at the alpha the kernel returned against the reference's values at that candidate; the decision against the Armijo test
    decided in 60 digits, an instance within hp_cases.MARGIN of a threshold left out of it (at most one; the CPU side asserts there is none)"""
    c = hc.case(name)
    B = c["x"].shape[0]
    q, dw, y = hc.step(name)
    ref = hc.ref_line_search(name)
    out = {k: _nan(B) for k in ("alpha", "step_max", "f", "gmax")}
    out["accepted"] = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    phi = _nan(B, 2); xs = _dev(c["x"]); mu = _dev(hc.MU0)
    with _rows(evaluators(name), c) as ev:
        ev.line_search(_dev(c["p"]), xs, _dev(c["lbx"]), _dev(c["ubx"]), _dev(q), _dev(dw), _dev(y), status=_dev(c["status"], torch.int32), mu=mu,
                       alpha0=1.0, candidates=hc.CANDIDATES, out=out, phi=phi)
        torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["phi"] = phi.cpu().numpy(); got["x"] = xs.cpu().numpy(); got["mu"] = mu.cpu().numpy()
    ok = np.isin(c["status"], hp.OK)
    assert ok.any() and (~ok).any()
    # instances without a point: nothing moves, the penalty stays
    assert (got["accepted"][~ok] == -2).all() and (got["alpha"][~ok] == 0.0).all() and _bits(got["x"][~ok], c["x"][~ok]) and _bits(got["mu"][~ok], hc.MU0[~ok])
    assert hp.distance(got["mu"][ok], ref["mu"][ok]) <= TOL
    # the values at the candidate the kernel took
    sel = np.zeros(B, np.int64)
    for b in np.nonzero(ok)[0]:
        j = np.nonzero(ref["alphas"] == got["alpha"][b])[0]
        assert len(j) == 1 and got["accepted"][b] in (j[0], -1), (name, b, got["alpha"][b], got["accepted"][b])
        sel[b] = j[0] + 1
    rows = np.arange(B)
    dx = np.where(ok[:, None], dw[:, c["model"].np:], 0.0)
    assert _bits(got["x"], c["x"] + got["alpha"][:, None] * dx)               # (alpha is a power of two: the product is exact)
    d = dict(phi0=hp.distance(got["phi"][:, 0], ref["phis"][:, 0]), phi1=hp.distance(got["phi"][:, 1], ref["phis"][rows, sel]),
             f=hp.distance(got["f"], ref["fs"][rows, sel]), gmax=hp.distance(got["gmax"], ref["gmaxs"][rows, sel]))
    near, same = hc.decision_check(got["accepted"], ref)
    print(name, "accepted", got["accepted"], "reference", ref["accepted"], "left out", int(near.sum()), " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)
    assert near.sum() <= 1 and same, (name, got["accepted"], ref["accepted"], near)


# ------------------------------------------------------------------------------------------------ 4. mpcqp_stage_convexify
@pytest.mark.parametrize("mode", hc.MODES)
@pytest.mark.parametrize("name", hc.CONVEXIFY + hc.EVERY)
def test_convexify(evaluators, name, mode):
    c = hc.case(name)
    mdl = c["model"]
    B = c["x"].shape[0]
    ref = hc.ref_convexify(name, mode)
    with _rows(evaluators(name), c) as ev:
        assert ev.has_convexify
        out = _eval(ev, c)
        P0 = out["P"].cpu().numpy()
        touched = torch.full((B,), -77, dtype=torch.int32, device="cuda"); lam = _nan(B, ev.horizon)
        ev.convexify(_dev(c["p"]), _dev(c["x"]), out["P"], mode, hc.EPS, touched=touched, lam_min=lam)
        torch.cuda.synchronize()
    P1, touched, lam = out["P"].cpu().numpy(), touched.cpu().numpy(), lam.cpu().numpy()
    bar_frame, bar_inst = cc.bar({"hnorm": ref["hnorm"]})
    dl = np.abs(lam - ref["lam_min"]) / bar_frame
    dP = np.array([np.abs(hp.dense(mdl.Pp, mdl.Pi, P1[b], mdl.n)[0] - ref["P"][b]).max() for b in range(B)]) / bar_inst
    print(name, mode, "touched", touched, "max |P - ref| / bar %.2e  max |lam_min - ref| / bar %.2e" % (dP.max(), dl.max()))
    assert np.array_equal(touched, ref["touched"])
    assert np.isfinite(P1).all() and (dl <= 1.0).all() and (dP <= 1.0).all()
    assert (ref["touched"] == 0).any()
    for b in np.nonzero(ref["touched"] == 0)[0]:
        assert _bits(P1[b], P0[b]), (name, b)                                # an instance the reference marks untouched keeps every bit of P


# ------------------------------------------------------------------------------------------------ 5. mpcqp_stage_advance
@pytest.mark.parametrize("tail", ["rollout", "repeat"])
@pytest.mark.parametrize("name", hc.ADVANCE)
def test_advance(evaluators, name, tail):
    """the plant step under the plant's parameters, the measured state taking precedence, the shift, the rollout tail under the model's
    parameters and the stage cost of frame 0"""
    c = hc.case(name)
    mdl = c["model"]
    B, N, nx, f = c["x"].shape[0], mdl.N, mdl.nx, mdl.f
    ok = np.isin(c["status"], hp.OK)
    with _rows(evaluators(name), c, plant=True) as ev:
        for measured in (False, True):
            ref = hc.ref_advance(name, tail, measured)
            o = dict(x_out=_nan(B, mdl.nvar), applied=_nan(B, f), stage_cost=_nan(B))
            lb, ub = _dev(c["lbx"]), _dev(c["ubx"])
            kw = dict(s_meas=_dev(c["s_meas"])) if measured else dict(w=_dev(c["w"]))
            if mdl.pref:
                o["p_out"] = _nan(B, mdl.np)
                kw.update(p_in=_dev(c["p"]), p_out=o["p_out"])
            else:
                kw.update(p=_dev(c["p"]))
            ev.advance(_dev(c["x"]), o["x_out"], lb, ub, status=_dev(c["status"], torch.int32), tail=tail, applied=o["applied"], stage_cost=o["stage_cost"], **kw)
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in o.items()}
            X = c["x"].reshape(B, N, f); G = got["x_out"].reshape(B, N, f); R = ref["x"].reshape(B, N, f)
            d = dict(first=hp.distance(G[:, 0, :nx], R[:, 0, :nx]), tail=hp.distance(G[:, N - 1, :nx], R[:, N - 1, :nx]),
                     stage_cost=hp.distance(got["stage_cost"], ref["stage_cost"]))
            print(name, tail, "measured" if measured else "plant step", " ".join("%s %.2e" % kv for kv in d.items()))
            assert _bits(got["applied"], X[:, 0]) and _bits(got["applied"], ref["applied"])
            assert d["first"] <= TOL and d["tail"] <= TOL and d["stage_cost"] <= TOL, (name, tail, measured, d)
            if measured:
                assert _bits(G[:, 0, :nx], c["s_meas"])
            assert _bits(G[:, 0, nx:], np.where(ok[:, None], X[:, 1, nx:], X[:, 0, nx:])) and _bits(G[:, 0, nx:], R[:, 0, nx:])
            assert _bits(G[:, 1:N - 1], X[:, 2:]) and _bits(G[:, N - 1, nx:], X[:, N - 1, nx:])
            if tail == "repeat":
                assert _bits(G[:, N - 1], X[:, N - 1])
            for bound, old in ((lb.cpu().numpy(), c["lbx"]), (ub.cpu().numpy(), c["ubx"])):
                assert _bits(bound[:, :f], G[:, 0]) and _bits(bound[:, f:], old[:, f:])
            if mdl.pref:
                P = c["p"].reshape(B, N, nx)
                assert _bits(got["p_out"], np.concatenate([P[:, 1:], P[:, -1:]], axis=1).reshape(B, -1))


# ------------------------------------------------------------------------------------------------ 6. mpcqp_nlp_eval, mpcqp_nlp_merit
@pytest.mark.parametrize("name", hc.GENERAL)
def test_general_evaluator(built, name):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    c = hc.general_case(name)
    m = c["model"]
    ref = hc.ref_general(name)
    ev = GeneralEvaluator(m)
    try:
        out = ev.alloc(c["x"].shape[0])
        for v in out.values():
            v.fill_(float("nan"))
        ev.eval(*[_dev(a) for a in hc.args(c)], out=out)
        f, g = ev.merit(_dev(c["p"]), _dev(c["x"]))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        ev.close()
    d = hc.system_distances(m, got, ref)
    d.update(f=hp.distance(f.cpu().numpy(), ref["f"]), gmax=hp.distance(g.cpu().numpy(), ref["gmax"]))
    print(name, " ".join("%s %.2e" % kv for kv in d.items()))
    for k, dist in d.items():
        assert dist <= TOL, (name, k, dist)
