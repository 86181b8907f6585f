"""Models, inputs, the 60-digit restatement and the recipes shared by tests/test_direct_qp_host.py (CPU) and tests/test_gpu_direct_qp.py -- TEST
INFRASTRUCTURE ONLY.

`direct_mp` restates the rule of mpcqp_stage_riccati_solve from include/mpcqp.h for one instance: it reads P and A through the CSC pattern (not
through the statement's slot tables), substitutes the pins and solves the KKT system of the equality-constrained problem as ONE dense system -- no
Riccati recursion -- by LU in float64 with iterative refinement, the residual taken in mpmath at 60 digits until it is below 1e-45 of the right-hand
side.  The multipliers of the dynamics rows and of the pinned identity rows are the KKT system's own; the parameter rows and z follow the header."""
import numpy as np

from optimal_control_problem_amd import models

from tests.support import riccati_cases as rc
from tests.support.riccati_cases import rel_err  # noqa: F401
from tests.support.rollout_cases import bits  # noqa: F401

HORIZONS = rc.HORIZONS


class PathLinkIntegrator(models.StageOCP):
    """the double integrator with two path rows and one link row (a rate limit): the rows the direct solve tests but does not solve for"""
    nx, nu, name = 2, 1, "pathlink_integrator"
    nh = 2; h_lo = [-3.0, -5.0]; h_hi = [3.0, 5.0]
    nk = 1; k_lo = [-1.5]; k_hi = [1.5]

    def F(self, s, u):
        return np.stack([s[..., 0] + 0.05 * s[..., 1], s[..., 1] + 0.05 * u[..., 0]], axis=-1)

    def hfun(self, s, u):
        return np.stack([s[..., 0] + 0.5 * s[..., 1], s[..., 1] - 2.0 * u[..., 0]], axis=-1)

    def kfun(self, s, u, sn, un):
        return np.stack([un[..., 0] - u[..., 0] + 0.1 * sn[..., 1]], axis=-1)

    def frame_bounds(self):
        return np.array([-np.inf, -2.0, -1.0]), np.array([np.inf, 2.0, 1.0])


# the five size cases (f = 3, 5, 16, 17, 24) and the one with path and link rows
MODELS = ("double_integrator", "cartpole", "quadrotor", "linear13x4", "linear16x8", "pathlink_integrator")
_CACHE = {}

# The statement's own error against the restatement, relative to max(1, max |ref|) per array, the worst over every case of
# tests/test_direct_qp_host.py::test_statement_against_60_digits (which asserts that no case exceeds it).  Measured: w 1.1e-15, y 1.4e-15 (DESIGN
# 6.30); E_NP_W and E_NP_Y are those values rounded up.  The device bar is max(1e-12, 16 E_NP), the convention of DESIGN 6.29.
E_NP_W = 2e-15
E_NP_Y = 3e-15
DEVICE_BAR_W = max(1e-12, 16.0 * E_NP_W)
DEVICE_BAR_Y = max(1e-12, 16.0 * E_NP_Y)


def model(name, N):
    if name != "pathlink_integrator":
        return rc.model(name, N)
    if (name, N) not in _CACHE:
        _CACHE[(name, N)] = PathLinkIntegrator(N, 0.05, Q=[1.0, 0.5], R=[0.2])
    return _CACHE[(name, N)]


def local_qp(mdl, B, seed=0, scale=1.0):
    """the local system at a drawn iterate, first frame pinned: dict P, q, A, l, u"""
    p, x, lbx, ubx, lbg, ubg = rc.iterate(mdl, B, seed)
    if scale != 1.0 and mdl.name != "quadrotor":
        x = x * scale
        lbx[:, :mdl.f] = x[:, :mdl.f]; ubx[:, :mdl.f] = x[:, :mdl.f]
    ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
    return {k: np.array(getattr(ls, k), float) for k in ("P", "q", "A", "l", "u")}


def read_slots(mdl):
    """boolean masks (P, A) of the slots the rule reads, looked up in the CSC pattern: the frame blocks of P and the parameter columns' entries in
    frame rows; of A the dynamics blocks over frame k (not the +1 entries on s_{k+1}), the path rows and the link rows"""
    N, f, nx, npp, n = mdl.N, mdl.f, mdl.nx, mdl.np, mdl.n
    rp = np.zeros(len(mdl.Pi), bool); ra = np.zeros(len(mdl.Ai), bool)
    for j in range(n):
        for e in range(mdl.Pp[j], mdl.Pp[j + 1]):
            i = int(mdl.Pi[e])
            if j < npp:
                rp[e] = i >= npp
            else:
                rp[e] = i >= npp and (i - npp) // f == (j - npp) // f
    for j in range(npp, n):
        k = (j - npp) // f
        for e in range(mdl.Ap[j], mdl.Ap[j + 1]):
            i = int(mdl.Ai[e])
            if i >= n + mdl.ngd:
                ra[e] = True
            elif i >= n:
                ra[e] = (i - n) // nx == k
    return rp, ra


def random_qp(mdl, B, seed=0, pins="all"):
    """random data on the model's pattern (rc.random_data for the frame blocks: H_k with eigenvalues in [0.5, 2], dynamics blocks of norm 1), path and
    link rows and the parameter columns' frame entries drawn, q drawn; every slot the rule does not read is NaN.  Bounds: p rows 0, frame 0's
    states pinned at drawn values, its inputs pinned ("all"), free ("none") or alternating ("mix"); the other identity rows +-50, dynamics rows
    l = u drawn, path and link rows +-50."""
    rng = np.random.default_rng(911 * mdl.N + 7 * B + seed + mdl.f)
    d = rc.random_data(mdl, B, seed)
    P, A = d["P"], d["A"]
    rp, ra = read_slots(mdl)
    fill = rp & np.isnan(P[0])
    P[:, fill] = rng.uniform(-0.3, 0.3, size=(B, int(fill.sum())))
    fill = ra & np.isnan(A[0])
    A[:, fill] = rng.uniform(-1.0, 1.0, size=(B, int(fill.sum())))
    assert not np.isnan(P[:, rp]).any() and np.isnan(P[:, ~rp]).all() and not np.isnan(A[:, ra]).any() and np.isnan(A[:, ~ra]).all()
    n, m, npp, f, nx = mdl.n, mdl.m, mdl.np, mdl.f, mdl.nx
    q = rng.normal(0.0, 0.5, size=(B, n))
    l = np.full((B, m), -50.0); u = np.full((B, m), 50.0)
    l[:, :npp] = 0.0; u[:, :npp] = 0.0
    v = rng.normal(0.0, 0.3, size=(B, f))
    l[:, npp:npp + f] = v; u[:, npp:npp + f] = v
    for i in range(mdl.nu):
        if pins == "none" or (pins == "mix" and i % 2 == 0):
            l[:, npp + nx + i] = -50.0; u[:, npp + nx + i] = 50.0
    b = rng.normal(0.0, 0.1, size=(B, mdl.ngd))
    l[:, n:n + mdl.ngd] = b; u[:, n:n + mdl.ngd] = b
    return dict(P=P, q=q, A=A, l=l, u=u)


def dense_from_csc(cp, ri, vals, nrow, ncol):
    M = np.zeros((nrow, ncol)); S = np.zeros((nrow, ncol), bool)
    for j in range(ncol):
        for e in range(cp[j], cp[j + 1]):
            M[ri[e], j] = vals[e]; S[ri[e], j] = True
    return M, S


def eligible(mdl, l, u):
    """the eligibility rule of the header for one instance, and the pin mask of frame 0's inputs"""
    n, npp, f, nx = mdl.n, mdl.np, mdl.f, mdl.nx
    with np.errstate(all="ignore"):
        ok = bool(np.all(l[:npp] == 0.0) and np.all(u[:npp] == 0.0))
        ok = ok and bool(np.all(l[npp:npp + nx] == u[npp:npp + nx]))
        li, ui = l[npp + nx:npp + f], u[npp + nx:npp + f]
        ok = ok and not (np.isnan(li).any() or np.isnan(ui).any())
        lr, ur = l[npp + f:n], u[npp + f:n]
        ok = ok and not (np.isnan(lr).any() or np.isnan(ur).any() or np.any(lr == ur))
        ok = ok and bool(np.all(l[n:n + mdl.ngd] == u[n:n + mdl.ngd]))
        return ok, li == ui


def direct_mp(mdl, P, q, A, l, u, feas_tol=0.0, reg=0.0, digits=60):
    """the rule for one instance -> dict w [n], y [m], z [m] (float64 arrays rounded from the mpmath values), direct (1, 0 or -1; the pivot test is
    not restated: the caller gives strictly convex data), margin: the smallest distance of a tested z_i from l_i - feas_tol and u_i + feas_tol,
    relative to max(1, |bound|) (negative: violated; infinite bounds do not count); kinv_norm: the infinity norm of the inverse of the
    equality-constrained KKT matrix, which maps residuals of the KKT conditions to errors in (w, y)."""
    import mpmath as mp
    N, f, nx, nu, npp, n, m, ngd = mdl.N, mdl.f, mdl.nx, mdl.nu, mdl.np, mdl.n, mdl.m, mdl.ngd
    ok, pin = eligible(mdl, l, u)
    if not ok:
        return dict(direct=-1, w=None, y=None, z=None, margin=None, kinv_norm=None)
    nv = N * f
    # the equality rows of the frame variables: pins (identity rows), then the dynamics rows with the entry on s_{k+1} taken as 1
    pinned = list(range(nx)) + [nx + i for i in range(nu) if pin[i]]
    ne = len(pinned) + ngd
    Pnz = {}      # (row, col) -> slot over the frame variables, read through the pattern
    for j in range(npp, n):
        for e in range(mdl.Pp[j], mdl.Pp[j + 1]):
            i = int(mdl.Pi[e])
            if i >= npp and (i - npp) // f == (j - npp) // f:
                Pnz[(i - npp, j - npp)] = e
    Cnz = {}      # (equality row, col) -> value
    for t, c in enumerate(pinned):
        Cnz[(t, c)] = 1.0
    for j in range(npp, n):
        k = (j - npp) // f
        for e in range(mdl.Ap[j], mdl.Ap[j + 1]):
            i = int(mdl.Ai[e])
            if n <= i < n + ngd:
                kk = (i - n) // nx
                if kk == k:
                    Cnz[(len(pinned) + i - n, j - npp)] = float(A[e])
                elif kk == k - 1:
                    assert (i - n) % nx == (j - npp) % f
                    Cnz[(len(pinned) + i - n, j - npp)] = 1.0
    free_u = np.ones(nv, bool)
    for k in range(N):
        free_u[k * f:k * f + nx] = False
    for c in pinned:
        free_u[c] = False
    Knz = {}
    for (i, j), e in Pnz.items():      # (the callers' H_k are symmetric: which triangle the rule reads makes no difference here)
        Knz[(i, j)] = float(P[e])
    for c in np.flatnonzero(free_u):
        Knz[(c, c)] = Knz.get((c, c), 0.0) + reg
    for (t, j), v in Cnz.items():
        Knz[(nv + t, j)] = v; Knz[(j, nv + t)] = v
    dim = nv + ne
    Kd = np.zeros((dim, dim))
    for (i, j), v in Knz.items():
        Kd[i, j] = v
    rhs = np.zeros(dim)
    rhs[:nv] = -q[npp:n]
    rhs[nv:nv + len(pinned)] = [l[npp + c] for c in pinned]
    rhs[nv + len(pinned):] = l[n:n + ngd]
    Kinv = np.linalg.inv(Kd)
    with mp.workdps(digits):
        ent = [(i, j, mp.mpf(v)) for (i, j), v in Knz.items()]
        rm = [mp.mpf(float(v)) for v in rhs]
        x = [mp.mpf(0)] * dim
        scale = max(1.0, float(np.abs(rhs).max()))
        for _ in range(12):
            r = list(rm)
            for i, j, v in ent:
                r[i] -= v * x[j]
            rf = np.array([float(t) for t in r])
            if np.abs(rf).max() <= 1e-45 * scale:
                break
            dx = Kinv @ rf
            x = [x[i] + mp.mpf(float(dx[i])) for i in range(dim)]
        else:
            raise AssertionError("the refinement of the restatement did not reach 1e-45")
        wm = [mp.mpf(0)] * npp + x[:nv]
        ym = [mp.mpf(0)] * m
        for t, c in enumerate(pinned):
            ym[npp + c] = x[nv + t]
        for t in range(ngd):
            ym[n + t] = x[nv + len(pinned) + t]
        for j in range(npp):
            acc = mp.mpf(float(q[j]))
            for e in range(mdl.Pp[j], mdl.Pp[j + 1]):
                if int(mdl.Pi[e]) >= npp:
                    acc += mp.mpf(float(P[e])) * wm[int(mdl.Pi[e])]
            ym[j] = -acc
        zm = list(wm) + [mp.mpf(float(v)) for v in l[n:n + ngd]] + [mp.mpf(0)] * (m - n - ngd)
        for j in range(npp, n):
            for e in range(mdl.Ap[j], mdl.Ap[j + 1]):
                i = int(mdl.Ai[e])
                if i >= n + ngd:
                    zm[i] += mp.mpf(float(A[e])) * wm[j]
        tested = np.ones(m, bool)
        tested[:npp + nx] = False
        tested[npp + nx:npp + f] = ~pin
        tested[n:n + ngd] = False
        margin = mp.inf
        nan = False
        for i in np.flatnonzero(tested):
            for bound, sgn in ((l[i], 1), (u[i], -1)):
                if np.isnan(bound):
                    nan = True
                elif np.isfinite(bound):
                    slack = sgn * (zm[i] - mp.mpf(float(bound))) + mp.mpf(feas_tol)
                    margin = min(margin, slack / max(1.0, abs(float(bound))))
        direct = 1 if (not nan and margin >= 0) else 0
        return dict(direct=direct, w=np.array([float(v) for v in wm]), y=np.array([float(v) for v in ym]), z=np.array([float(v) for v in zm]),
                    margin=float(margin), kinv_norm=float(np.abs(Kinv).sum(axis=1).max()))


_REF = {}


REF_FEAS_TOL = 1e3      # wider than any bound of the cases: every instance is accepted, so w, y, z of every instance are compared


def reference(name, N, kind, B=3):
    """(data dict, list of direct_mp results per instance at feas_tol = REF_FEAS_TOL) for a case, computed once per process and shared"""
    key = (name, N, kind, B)
    if key not in _REF:
        mdl = model(name, N)
        d = local_qp(mdl, B, seed=1, scale=0.1) if kind == "local" else random_qp(mdl, B, seed=2, pins={"random": "all", "random_mix": "mix", "random_free": "none"}[kind])
        _REF[key] = (d, [direct_mp(mdl, *(d[k][b] for k in ("P", "q", "A", "l", "u")), feas_tol=REF_FEAS_TOL) for b in range(B)])
    return _REF[key]


def certificate(mdl, d, w, y, b):
    """(stationarity, bound violation, multiplier on a slack row) of instance b, each relative to max(1, |P|_max |w|_inf, |q|_inf); P and A are used as
    dense matrices.  The NaN (unread) slots of random data are taken as the rule takes them: an entry of P as its mirror image (P is symmetric; the
    parameter block, NaN on both sides, multiplies dp = 0), the identity and s_{k+1} entries of A as 1."""
    Pd, _ = dense_from_csc(mdl.Pp, mdl.Pi, d["P"][b], mdl.n, mdl.n)
    Pd = np.nan_to_num(np.where(np.isnan(Pd), Pd.T, Pd), nan=0.0)
    Ad, _ = dense_from_csc(mdl.Ap, mdl.Ai, np.where(np.isnan(d["A"][b]), 1.0, d["A"][b]), mdl.m, mdl.n)
    q, l, u = d["q"][b], d["l"][b], d["u"][b]
    sc = max(1.0, float(np.abs(Pd).max() * np.abs(w).max()), float(np.abs(q).max()))
    stat = np.abs(Pd @ w + q + Ad.T @ y).max() / sc
    z = Ad @ w
    viol = max(0.0, float(np.max(l - z)), float(np.max(z - u))) / sc
    slack = np.abs(y[l < u]).max() / sc if (l < u).any() else 0.0
    return stat, viol, slack


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The mask batch: double-integrator and cart-pole local systems at iterates of growing size, so that the restatement accepts the small ones and
# rejects the large ones, each with a margin of at least 1e-6 of the bound's scale (asserted on the CPU from the restatement alone).
MASK_N = 6


def mask_batch(name):
    """(model, data dict of B = 8 instances, restatement results)"""
    key = ("mask", name)
    if key not in _REF:
        mdl = model(name, MASK_N)
        scales = (0.02, 0.05, 0.1, 0.3, 2.0, 6.0, 12.0, 25.0) if name == "double_integrator" else (0.02, 0.05, 0.1, 0.3, 8.0, 15.0, 30.0, 60.0)
        parts = [local_qp(mdl, 1, seed=10 + i, scale=s) for i, s in enumerate(scales)]
        d = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        _REF[key] = (mdl, d, [direct_mp(mdl, *(d[k][b] for k in ("P", "q", "A", "l", "u"))) for b in range(d["P"].shape[0])])
    return _REF[key]


def spoiled(mdl, d, b, how):
    """a copy of instance b of d with one of these defects: -> (dict of [1, ...] arrays, expected direct)"""
    o = {k: v[b:b + 1].copy() for k, v in d.items()}
    n, npp, f, nx = mdl.n, mdl.np, mdl.f, mdl.nx
    if how == "pinned_later_state":
        o["l"][0, npp + f] = o["u"][0, npp + f] = 0.0
        return o, -1
    if how == "unpinned_first_state":
        o["u"][0, npp] = o["l"][0, npp] + 1.0
        return o, -1
    if how == "open_dynamics_row":
        o["u"][0, n] = o["l"][0, n] + 1.0
        return o, -1
    if how == "nonzero_p_row":
        o["l"][0, 0] = o["u"][0, 0] = 0.5
        return o, -1
    if how == "nan_bound":
        o["l"][0, npp + f + 1] = np.nan
        return o, -1
    pslot, _ = rc.slots_from_pattern(mdl)
    e = pslot[mdl.N - 1, f - 1, f - 1]
    if how == "indefinite":
        o["P"][0, e] = -1.0
        return o, -2
    if how == "nan_slot":
        o["P"][0, e] = np.nan
        return o, -2
    raise ValueError(how)


SPOILS = ("pinned_later_state", "unpinned_first_state", "open_dynamics_row", "nonzero_p_row", "nan_bound", "indefinite", "nan_slot")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The loop recipes, 8 instances on a horizon of 20 frames, 4 SQP iterations at alpha = 1.
# "near": the double integrator at rest within 5 cm of the origin, zero iterate -- no input of the plan comes near |u| <= 1 and no velocity near
# |v| <= 2: every QP of every iteration is accepted.  (The double integrator is linear: x + dw is the same point in every iteration, so its verdicts
# cannot change along a loop.)
# "far": the cart-pole, pole 0.05 to 0.1 rad off upright, started from a poor iterate (states drawn with deviation 8, inputs with 80).  The first
# linearisation is far from the dynamics it stands for and its step leaves the box |pos| <= 2.4, |u| <= 20: every instance is rejected and goes
# through the ADMM; from the third iteration on the iterate is near the interior optimum and every instance is accepted.
RECIPE_B, RECIPE_N, RECIPE_ITERS = 8, 20, 4


def recipe(which):
    """(model, the dict getOptimalSolution takes, the iterate to start from [B, nvar])"""
    rng = np.random.default_rng(5)
    if which == "near":
        mdl = models.DoubleIntegrator(RECIPE_N)
        frame0 = np.zeros((RECIPE_B, mdl.f))
        frame0[:, 0] = rng.uniform(-0.05, 0.05, size=RECIPE_B)
        x0 = np.zeros((RECIPE_B, mdl.nvar))
    else:
        mdl = models.CartPole(RECIPE_N)
        frame0 = np.zeros((RECIPE_B, mdl.f))
        frame0[:, 1] = rng.uniform(0.05, 0.1, size=RECIPE_B)
        x0 = rng.normal(0.0, 8.0, size=(RECIPE_B, mdl.N, mdl.f)); x0[:, :, mdl.nx:] *= 10.0
        x0[:, 0] = frame0
        x0 = x0.reshape(RECIPE_B, -1)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    return mdl, dict(p=np.zeros((RECIPE_B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg), x0
