"""Cases shared by tests/test_nlp_hp_host.py (CPU) and tests/test_gpu_nlp_hp.py -- TEST INFRASTRUCTURE ONLY.  The models the other suites lean on,
at the smallest shapes that still have the structure, each with its reference from tests/support/nlp_hp.py (computed once per case and left
unchanged; callers copy what they change).

Points: instance 0 is the random iterate itself and starts on its pinned first frame; instances 1 and 4 are their draws put far outside every
finite bound, one above and one below, so every violation measure has instances on both sides.  The convexify cases keep the points of tests/support/convexify_cases.py."""
import zlib

import numpy as np

from optimal_control_problem_amd import models
from tests.support import convexify_cases as cc
from tests.support import general_problems as gp
from tests.support import link_cost_cases as lkc
from tests.support import nlp_hp as hp
from tests.support import stage_data_cases as sdc

BATCH = 5                                           # not a multiple of the four waves per block
STATUS = np.array([1, 2, 7, 3, 1], np.int32)       # instance 3: the QP returned no point
SCALES = sdc.SCALES[:BATCH]                         # dw of the one oracle QP, scaled per instance
MU0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0])
CANDIDATES = 4
MODES = cc.MODES
EPS = cc.EPS
TOL = 1e-12                                         # the project's evaluator bar, relative to max(1, |ref|)
MARGIN = 1e-9                                       # an Armijo test closer than this to its threshold may tip in float64


# ------------------------------------------------------------------------------------------------ the new model: everything on one model
class Everything(models.StageOCP):
    """nx = 3, nu = 2 (f = 5 does not divide 64); two path rows with bounds that differ by frame and one infinite side; one link row; two plant
    parameters read in cdyn; three stage-data values read in hfun, lcost and lterm; a stage cost with cross terms between s, u and r that uses every
    traced operation and has a Gaussian bump on s_0 (not convex near its centre d_0); a terminal cost of its own; a non-quadratic link cost that
    couples states and inputs of both frames."""
    nx, nu, name = 3, 2, "everything"
    nh = 2
    nk = 1; k_lo = [-0.4]; k_hi = [0.6]
    ntheta = 2
    theta = np.array([0.9, 0.25])
    nsd = 3
    sdata = np.array([0.3, 1.2, 0.5])
    convexify = True

    def __init__(self, N, dt=0.05):
        k = np.arange(N, dtype=float)
        self.h_lo = np.stack([np.full(N, -np.inf), -1.0 - 0.1 * k], axis=1)
        self.h_hi = np.stack([1.5 + 0.2 * k, 1.0 + 0.1 * k], axis=1)
        super().__init__(N, dt, Q=[1.0, 1.0, 1.0], R=[0.1, 0.1])

    def cdyn(self, s, u):
        a, c = self.theta[0], self.theta[1]
        return np.stack([s[..., 1] + 0.1 * u[..., 1], (-9.81 / a) * np.sin(s[..., 0]) - c * s[..., 1] + u[..., 0] / (a * a),
                         -0.5 * s[..., 2] + s[..., 0] * u[..., 1]], axis=-1)

    def hfun(self, s, u):
        d = self.sdata
        return np.stack([(s[..., 0] - d[0]) ** 2 + 0.5 * u[..., 0] + 0.1 * s[..., 2], d[2] * s[..., 1] + np.sin(s[..., 2]) * u[..., 1]], axis=-1)

    def _bowl(self, s, u, r, w):
        v = 0.0
        for i in range(3):
            e = s[..., i] - r[..., i]
            v = v + w * e * e + 0.5 * s[..., i] * s[..., i] + 0.4 * r[..., i] * r[..., i]
        return v + 0.3 * u[..., 0] * u[..., 0] + 0.4 * u[..., 1] * u[..., 1]

    def lcost(self, s, u, r):
        d = self.sdata
        e0, e1, e2 = s[..., 0] - r[..., 0], s[..., 1] - r[..., 1], s[..., 2] - r[..., 2]
        v = self._bowl(s, u, r, 2.0) + d[1] * 2.0 * (1.0 - np.cos(e0))
        v = v + 0.04 * u[..., 0] * s[..., 1] + 0.03 * u[..., 1] * r[..., 2] + 0.02 * s[..., 0] * r[..., 1]
        v = v + np.sqrt(1.0 + e2 ** 2 + u[..., 1] ** 2) + 0.1 * np.log(1.0 + s[..., 1] ** 2 + 0.5 * u[..., 0] ** 2)
        v = v + 0.2 * np.tanh(0.5 * s[..., 2] * u[..., 0]) + 0.05 * np.tan(0.3 * np.tanh(s[..., 0] + r[..., 0])) ** 2
        v = v + 0.3 / (2.0 + e1 ** 2 + r[..., 2] ** 2) + 0.1 * np.sin(s[..., 2] + u[..., 1]) + 0.01 * s[..., 0] ** 4
        return v + 6.0 * d[2] * np.exp(-(s[..., 0] - d[0]) ** 2 / (2.0 * 0.35 * 0.35))

    def lterm(self, s, u, r):
        d = self.sdata
        e0 = s[..., 0] - r[..., 0]
        v = self._bowl(s, u, r, 5.0) + 4.0 * d[1] * e0 ** 2 + 0.1 * np.sqrt(1.0 + s[..., 0] ** 2) + 0.3 * s[..., 0] * r[..., 1]
        return v + 9.0 * d[2] * np.exp(-(s[..., 0] - d[0]) ** 2 / (2.0 * 0.5 * 0.5))

    def llink(self, s, u, sn, un):
        v = np.sqrt(1.0 + (sn[..., 0] - s[..., 0]) ** 2 + 0.5 * (sn[..., 2] * u[..., 1]) ** 2) * (1.0 + 0.1 * u[..., 0] * un[..., 0])
        return v + 0.05 * (un[..., 1] - u[..., 1]) ** 2 + 0.02 * np.sin(s[..., 1] * un[..., 1])

    def kfun(self, s, u, sn, un):
        return np.stack([un[..., 0] - u[..., 0] + 0.2 * (sn[..., 1] - s[..., 1]) * s[..., 2]], axis=-1)

    def frame_bounds(self):
        return np.array([-2.0, -np.inf, -4.0, -3.0, -np.inf]), np.array([2.0, 5.0, np.inf, 3.0, 2.5])


class EverythingTracking(Everything):
    name = "everything_tracking"; per_frame_reference = True


# ------------------------------------------------------------------------------------------------ the zoo with weights and references per frame
def _zoo(cls, N, dt, tracking):
    """the zoo class as it is (shared reference, its constant weights) or with a reference and weights per frame; still the built-in functor"""
    if not tracking:
        return cls(N, dt)
    base = cls(N, dt)
    ramp = np.linspace(1.0, 2.5, N)[:, None]

    class PerFrame(cls):
        per_frame_reference = True

        def __init__(self):
            models.StageOCP.__init__(self, N, dt, base.Q[None, :] * ramp, base.R[None, :] * ramp[::-1])
    PerFrame.__name__ = cls.__name__ + "PerFrame"
    return PerFrame()


class PendulumSmoothTracking(lkc.PendulumSmooth):
    """plant parameters without stage data on a tracking handle"""
    name = "param_pendulum_smooth_tracking"; per_frame_reference = True


def _path3():
    mdl = sdc.make(sdc.PathDataPendulum, 3)
    mdl.h_lo = np.array([[-3.0], [-np.inf], [-1.0]]); mdl.h_hi = np.array([[3.0], [2.0], [0.5]])       # bounds that differ by frame
    return mdl


_STAGE = {
    "di2": lambda: _zoo(models.DoubleIntegrator, 2, 0.05, False), "di2_pfw": lambda: _zoo(models.DoubleIntegrator, 2, 0.05, True),
    "cartpole3": lambda: _zoo(models.CartPole, 3, 0.02, False), "cartpole3_pfw": lambda: _zoo(models.CartPole, 3, 0.02, True),
    "quadrotor2": lambda: _zoo(models.Quadrotor, 2, 0.02, False), "quadrotor2_pfw": lambda: _zoo(models.Quadrotor, 2, 0.02, True),
    "data2": lambda: sdc.make(sdc.DataPendulum, 2), "data3": lambda: sdc.make(sdc.DataPendulum, 3),
    "tracking_data2": lambda: sdc.make(sdc.TrackingDataPendulum, 2), "tracking_data3": lambda: sdc.make(sdc.TrackingDataPendulum, 3),
    "theta_data2": lambda: sdc.make(sdc.ThetaDataPendulum, 2), "theta_data3": lambda: sdc.make(sdc.ThetaDataPendulum, 3),
    "path_data2": lambda: sdc.make(sdc.PathDataPendulum, 2), "path_data3": _path3,
    "link_smooth": lambda: lkc.make("smooth", 3), "link_smooth_tracking": lambda: lkc.make("smooth_tracking", 3),
    "link_nonquad": lambda: lkc.make("nonquad", 3), "link_general": lambda: lkc.make("general", 3),
    "link_general_tracking": lambda: lkc.make("general_tracking", 3), "link_everything": lambda: lkc.make("everything", 3),
    "link_pendulum": lambda: lkc.make("pendulum", 3), "link_pendulum_tracking": lambda: PendulumSmoothTracking(3, 0.05, Q=[10.0, 1.0], R=[0.1]),
    "link_quadrotor": lambda: lkc.make("quadrotor", 2),
    "every2": lambda: Everything(2), "every3": lambda: Everything(3), "every4": lambda: Everything(4),
    "every_pf2": lambda: EverythingTracking(2), "every_pf3": lambda: EverythingTracking(3), "every_pf4": lambda: EverythingTracking(4),
}
STAGE = tuple(_STAGE)                                # eval, merit, line search (and advance, convexify where they apply)
LONG = ("data70",)                                   # more frames than lanes: merit and line-search values only
CONVEXIFY = ("bump3", "bump_pf", "bump_term", "bump_link", "bump_sd", "quad_dense", "wide")
EVERY = tuple(k for k in STAGE if k.startswith("every"))
ADVANCE = ("cartpole3", "quadrotor2_pfw", "theta_data2", "theta_data3", "link_pendulum", "link_pendulum_tracking") + EVERY      # the theta cases and the everything model
GENERAL = ("pendulum", "skip_coupled")
TERM_KINDS = ("di2", "data3", "link_general", "bump_term", "every_pf3")     # one per term kind, for the self-accuracy of the reference


def _theta_rows(mdl, B, roll=0):
    sc = np.roll(np.linspace(0.7, 1.5, B), roll)
    th = np.tile(np.asarray(mdl.theta, float), (B, 1))
    first, second = {"quadrotor": (0, 4), "cartpole": (2, 1)}.get(mdl.name.split("_")[0], (0, 1))
    th[:, first] *= sc; th[:, second] *= np.roll(sc, 1)
    return th


_CASES = {}
_RESEED = {"theta_data2": 1, "link_everything": 1, "every3": 1, "every_pf3": 1}      # name -> n: the n-th redraw, where the first draw left a row on one side of its bounds in every instance


def case(name):
    """dict: model, p, x, lbx, ubx, lbg, ubg, theta, plant, d (rows or None), status, w, s_meas, and kind = stage | long | convexify"""
    if name in _CASES:
        return _CASES[name]
    if name in CONVEXIFY:
        c0 = cc.case(name)
        c = {k: c0[k] for k in ("model", "p", "x", "lbx", "ubx", "lbg", "ubg", "d")}
        c.update(name=name, kind="convexify", theta=None, plant=None)
        _CASES[name] = c
        return c
    mdl = sdc.make(sdc.DataPendulum, 70) if name == "data70" else _STAGE[name]()
    B, N, nx, f = BATCH, mdl.N, mdl.nx, mdl.f
    rng = np.random.default_rng(zlib.crc32(name.encode()) % 10000 + 10000 * _RESEED.get(name, 0))      # (a seed that does not move when a case is added)
    X = rng.normal(0.0, 0.3, size=(B, N, f))
    quad = isinstance(mdl, models.Quadrotor)
    if quad:
        X[:, :, nx:] += mdl.hover_thrust
    if name.startswith("every"):
        X[0, :, 0] = mdl.sdata[0] + 1.6 + rng.normal(0.0, 0.05, size=N)       # far from the bump: convex in every frame
        X[2:, :, 0] = mdl.sdata[0] + rng.normal(0.0, 0.1, size=(B - 2, N))      # on the bump
    frame0 = X[:, 0].copy()
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    # instances 1 and 4: every entry with a finite bound beyond it by more than 3 + 5 k in frame k (1: above the upper bound where there is one,
    # 4: below the lower one), the others scaled far out with either sign -- rows that are nearly linear are violated on one side or the other
    for b_, up in ((1, True), (4, False)):
        draw = X[b_].reshape(-1)
        wild = draw * ((3.0 if quad else 40.0) * (1.0 if up else -1.0))
        excess = 3.0 + np.abs(draw) + 5.0 * np.repeat(np.arange(N, dtype=float), f)
        hi_, lo_ = np.isfinite(ubx[b_]), np.isfinite(lbx[b_])
        above = hi_ if up else hi_ & ~lo_
        below = lo_ & ~hi_ if up else lo_
        wild[above] = ubx[b_][above] + excess[above]
        wild[below] = lbx[b_][below] - excess[below]
        X[b_] = wild.reshape(N, f)
    c = dict(name=name, kind="long" if name in LONG else "stage", model=mdl, p=rng.normal(0.0, 0.2, size=(B, mdl.np)), x=X.reshape(B, -1),
             lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, theta=None, plant=None, d=None, status=STATUS.copy(),
             w=rng.normal(0.0, 0.01, size=(B, nx)), s_meas=rng.normal(0.0, 0.3, size=(B, nx)))
    # (a zoo class on the generated path -- a link cost, a path row -- keeps its constants in the code: no parameter rows on that handle)
    generated_zoo = isinstance(mdl, (models.Quadrotor, models.CartPole)) and bool(mdl.nh or mdl.nk or mdl.general_cost or mdl.link_cost)
    if mdl.ntheta and not generated_zoo:
        c["theta"] =_theta_rows(mdl, B); c["plant"] = _theta_rows(mdl, B, roll=2)
    if mdl.nsd:
        d = np.tile(np.asarray(mdl.sdata, float), (B, N, 1))
        d[..., 0] += rng.uniform(-0.2, 0.2, size=(B, N)); d[..., 1] *= rng.uniform(0.7, 1.5, size=(B, N))
        if mdl.nsd > 2:
            d[..., 2] *= rng.uniform(0.7, 1.4, size=(B, N))
        c["d"] = d
    _CASES[name] = c
    return c


def restatement(name, **kw):
    c = case(name)
    return hp.Stage(c["model"], theta=c["theta"], sdata=c["d"], plant=c["plant"], **kw)


class rows_on_statement:
    """the case's rows on the NumPy statement for the duration of a block (plant: the plant's rows as well)"""

    def __init__(self, c, plant=False):
        self.c, self.plant = c, plant

    def __enter__(self):
        c, mdl = self.c, self.c["model"]
        if c["d"] is not None:
            mdl.set_stage_data(c["d"])
        if c["theta"] is not None:
            mdl.set_instance_params(c["theta"], c["plant"] if self.plant else None)
        return mdl

    def __exit__(self, *exc):
        c, mdl = self.c, self.c["model"]
        if c["d"] is not None:
            mdl.set_stage_data(None)
        if c["theta"] is not None:
            mdl.set_instance_params()
        return False


_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def args(c):
    return [c[k] for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")]


def ref_system(name):
    return _cached((name, "system"), lambda: restatement(name).system(*args(case(name))))


def ref_merit(name):
    c = case(name)
    return _cached((name, "merit"), lambda: restatement(name).merit(c["p"], c["x"], c["lbx"], c["ubx"]))


def step(name):
    """(q, dw, y) of the line search: q the reference's gradient (the statement's for the long case, whose system is not differenced), dw and y
    from one oracle QP of the statement's local system, dw scaled per instance"""
    def make():
        from oracle import oracle as orc
        c = case(name)
        with rows_on_statement(c) as mdl:
            ls = mdl.local_system(*args(c))
        pat = orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
        res = pat.solve(ls.P, ls.q, ls.A, ls.l, ls.u, orc.default_settings(eps_abs=1e-3, eps_rel=1e-3, max_iter=20000))
        q = np.array(ls.q) if c["kind"] == "long" else ref_system(name)["q"]
        dw = np.array(res["x"]) * SCALES[:, None]
        dw[~np.isfinite(dw)] = 0.1
        dw[[1, 4]] *= 1e-2                             # (instances 1 and 4 are far out: a small step keeps their candidates distinct and finite)
        return q, dw, np.nan_to_num(np.array(res["y"]))
    return _cached((name, "step"), make)


def ref_line_search(name):
    def make():
        c = case(name)
        q, dw, y = step(name)
        return restatement(name).line_search(c["p"], c["x"], c["lbx"], c["ubx"], q, dw, y, status=c["status"], mu=MU0, candidates=CANDIDATES)
    return _cached((name, "ls"), make)


def ref_convexify(name, mode):
    """both modes from one restatement object, which remembers the frame Hessians"""
    c = case(name)
    S = _cached((name, "stage"), lambda: restatement(name))
    return _cached((name, "cvx", mode), lambda: S.convexify(c["p"], c["x"], ref_system(name)["P"], mode, EPS))


def ref_advance(name, tail, measured):
    c = case(name)
    return _cached((name, "adv", tail, measured), lambda: restatement(name).advance(
        c["x"], c["p"], status=c["status"], s_meas=c["s_meas"] if measured else None, w=None if measured else c["w"], tail=tail))


# ------------------------------------------------------------------------------------------------ the general path
_GENERAL_FG = {"pendulum": (gp.pendulum_cost, gp.pendulum_constraints)}


def general_case(name, B=3):
    def make():
        pr = gp.problem(name)
        p, x, lbx, ubx, lbg, ubg = gp.point(pr, B, seed=17)
        x[1] *= 8.0                                    # instance 1 violates the general rows by a wide margin
        cost, cons = _GENERAL_FG[name] if name in _GENERAL_FG else (pr["cost"], pr["constraints"])
        m = pr["model"]
        return dict(name=name, model=m, p=p, x=x, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, restatement=hp.General(cost, cons, m.nvar, m.np))
    return _cached((name, "general"), make)


def ref_general(name):
    c = general_case(name)
    return _cached((name, "general_system"), lambda: c["restatement"].system(*args(c)))


# ------------------------------------------------------------------------------------------------ comparisons
def dense_system(mdl, P, q, A, l, u, b):
    """instance b of a local system in CSC values as dense arrays, with the pattern masks"""
    Pd, Pm = hp.dense(mdl.Pp, mdl.Pi, P[b], mdl.n)
    Ad, Am = hp.dense(mdl.Ap, mdl.Ai, A[b], mdl.m)
    return dict(P=Pd, q=q[b], A=Ad, l=l[b], u=u[b]), Pm, Am


def system_distances(mdl, got, ref):
    """{P, q, A, l, u: the largest distance over the batch}; got: CSC values by name"""
    out = dict.fromkeys(("P", "q", "A", "l", "u"), 0.0)
    for b in range(ref["q"].shape[0]):
        d, _, _ = dense_system(mdl, got["P"], got["q"], got["A"], got["l"], got["u"], b)
        for k in out:
            out[k] = max(out[k], hp.distance(d[k], ref[k][b]))
    return out


def decision_check(got_accepted, ref):
    """the instances whose decision may be left out (a candidate within MARGIN max(1, |phi_0|) of its Armijo threshold) and whether every other
    instance took the reference's decision"""
    near = (ref["margin"] <= MARGIN * np.maximum(1.0, np.abs(ref["phi0"]))[:, None]).any(axis=1)
    same = np.asarray(got_accepted) == ref["accepted"]
    return near, bool(same[~near].all())
