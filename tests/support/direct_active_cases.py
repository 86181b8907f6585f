"""Cases, the restatement and the recipes shared by tests/test_direct_active_host.py (CPU) and tests/test_gpu_direct_active.py -- TEST INFRASTRUCTURE
ONLY.

`active_mp` restates the rule of mpcqp_stage_riccati_solve_active from include/mpcqp.h for one instance.  Every round is ONE dense KKT system of the
equality-constrained problem with the pins, the held input rows and the dynamics rows as equalities, P and A read through the CSC pattern (no
Riccati recursion, no slot tables): LU in float64 with iterative refinement, the residual in mpmath at 60 digits (digits=None: the residual in long
double, for the margin checks, whose 1e-6 is far above either).  The set logic around the solves is written from the header alone."""
import numpy as np

from tests.support import direct_qp_cases as dc
from tests.support import riccati_cases as rc
from tests.support.direct_qp_cases import MODELS, model, rel_err, bits, certificate  # noqa: F401

HORIZONS = (2, 3, 20)
MARGIN = 1e-6

# The statement's own error against the restatement (relative to max(1, max |ref|) per array), the worst over every accepted instance of
# tests/test_direct_active_host.py::test_statement_against_60_digits, which asserts that no case exceeds these.  Measured: w and z 3.4e-16, y 3.8e-16
# (DESIGN 6.31); E_NP_W and E_NP_Y are those values rounded up to about twice.  The device bar is max(1e-12, 16 E_NP).
E_NP_W = 7e-16
E_NP_Y = 8e-16
DEVICE_BAR_W = max(1e-12, 16.0 * E_NP_W)
DEVICE_BAR_Y = max(1e-12, 16.0 * E_NP_Y)


def _solve_held(mdl, P, q, A, l, reg, held, digits):
    """the equality-constrained problem with the frame variables of `held` ({column over the frames: value}) fixed and the dynamics rows as
    equalities -> (w [n], y [m] with the multipliers of the held identity rows and the dynamics rows, the other rows 0; kinv_norm), as mpmath
    numbers (digits) or long doubles (digits=None)"""
    N, f, nx, npp, n, m, ngd = mdl.N, mdl.f, mdl.nx, mdl.np, mdl.n, mdl.m, mdl.ngd
    nv = N * f
    cols = sorted(held)
    Knz = {}
    for j in range(npp, n):
        for e in range(mdl.Pp[j], mdl.Pp[j + 1]):
            i = int(mdl.Pi[e])
            if i >= npp and (i - npp) // f == (j - npp) // f:
                Knz[(i - npp, j - npp)] = float(P[e])
    for k in range(N):
        for c in range(nx, f):
            if k * f + c not in held:
                Knz[(k * f + c, k * f + c)] = Knz.get((k * f + c, k * f + c), 0.0) + reg
    for t, c in enumerate(cols):
        Knz[(nv + t, c)] = 1.0; Knz[(c, nv + t)] = 1.0
    for j in range(npp, n):
        k = (j - npp) // f
        for e in range(mdl.Ap[j], mdl.Ap[j + 1]):
            i = int(mdl.Ai[e])
            if n <= i < n + ngd:
                kk = (i - n) // nx
                v = float(A[e]) if kk == k else 1.0 if kk == k - 1 else None
                if v is not None:
                    r = nv + len(cols) + i - n
                    Knz[(r, j - npp)] = v; Knz[(j - npp, r)] = v
    dim = nv + len(cols) + ngd
    Kd = np.zeros((dim, dim))
    for (i, j), v in Knz.items():
        Kd[i, j] = v
    rhs = np.zeros(dim)
    rhs[:nv] = -q[npp:n]
    rhs[nv:nv + len(cols)] = [held[c] for c in cols]
    rhs[nv + len(cols):] = l[n:n + ngd]
    Kinv = np.linalg.inv(Kd)
    scale = max(1.0, float(np.abs(rhs).max()))
    if digits is None:
        ii = np.array([k[0] for k in Knz]); jj = np.array([k[1] for k in Knz]); vv = np.array(list(Knz.values()), np.longdouble)
        x = np.zeros(dim, np.longdouble)
        for _ in range(4):
            r = rhs.astype(np.longdouble)
            np.subtract.at(r, ii, vv * x[jj])
            x = x + (Kinv @ r.astype(float)).astype(np.longdouble)
        num = lambda v: np.longdouble(v)      # noqa: E731
        zero = np.longdouble(0)
    else:
        import mpmath as mp      # (active_mp has set the working precision)
        ent = [(i, j, mp.mpf(v)) for (i, j), v in Knz.items()]
        rm = [mp.mpf(float(v)) for v in rhs]
        x = [mp.mpf(0)] * dim
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
        num = lambda v: mp.mpf(float(v))      # noqa: E731
        zero = mp.mpf(0)
    w = [zero] * npp + [x[i] for i in range(nv)]
    y = [zero] * m
    for t, c in enumerate(cols):
        y[npp + c] = x[nv + t]
    for t in range(ngd):
        y[n + t] = x[nv + len(cols) + t]
    for j in range(npp):
        acc = num(q[j])
        for e in range(mdl.Pp[j], mdl.Pp[j + 1]):
            if int(mdl.Pi[e]) >= npp:
                acc += num(P[e]) * w[int(mdl.Pi[e])]
        y[j] = -acc
    z = list(w) + [num(v) for v in l[n:n + ngd]] + [zero] * (m - n - ngd)
    for j in range(npp, n):
        for e in range(mdl.Ap[j], mdl.Ap[j + 1]):
            i = int(mdl.Ai[e])
            if i >= n + ngd:
                z[i] += num(A[e]) * w[j]
    return w, y, z, float(np.abs(Kinv).sum(axis=1).max())


def active_mp(mdl, P, q, A, l, u, feas_tol=0.0, reg=0.0, rounds=4, dual_tol=0.0, guess=None, digits=60):
    if digits is None:
        return _active_mp(mdl, P, q, A, l, u, feas_tol, reg, rounds, dual_tol, guess, None)
    import mpmath as mp
    with mp.workdps(digits):
        return _active_mp(mdl, P, q, A, l, u, feas_tol, reg, rounds, dual_tol, guess, digits)


def _active_mp(mdl, P, q, A, l, u, feas_tol, reg, rounds, dual_tol, guess, digits):
    """the rule for one instance -> dict direct (1, 0, -1; the pivot test is not restated: the caller gives strictly convex data), w, y, z (float64,
    accepted instances only), act [N, nu], rounds_used, margin: the smallest distance of any primal or dual decision of any round from its threshold,
    relative to max(1, |bound|) resp. max(1, |y|_inf) (infinite bounds do not count), kinv_norm of the accepting round"""
    N, f, nx, nu, npp, n, m, ngd = mdl.N, mdl.f, mdl.nx, mdl.nu, mdl.np, mdl.n, mdl.m, mdl.ngd
    ok, pin = dc.eligible(mdl, l, u)
    if not ok:
        return dict(direct=-1, w=None, y=None, z=None, act=None, rounds_used=None, margin=None, kinv_norm=None)
    guess = np.zeros((N, nu), int) if guess is None else np.asarray(guess).reshape(N, nu)
    fixed = {c: l[npp + c] for c in range(nx)}
    fixed.update({nx + i: l[npp + nx + i] for i in range(nu) if pin[i]})
    inputs = [(k, i) for k in range(N) for i in range(nu) if not (k == 0 and pin[i])]
    row = lambda k, i: npp + k * f + nx + i      # noqa: E731
    hard = [npp + k * f + c for k in range(1, N) for c in range(nx)] + list(range(n + ngd, m))
    S = {}      # (k, i) -> -1 / +1
    margin = np.inf
    out = dict(direct=0, w=None, y=None, z=None, kinv_norm=None)

    def gap(v, thr, scale):
        nonlocal margin
        margin = min(margin, abs(float(v - thr)) / scale)

    for r in range(rounds + 1):
        held = dict(fixed)
        for (k, i), s in S.items():
            held[k * f + nx + i] = (l if s < 0 else u)[row(k, i)]
        wm, ym, zm, kn = _solve_held(mdl, P, q, A, l, reg, held, digits)
        used = r
        hopeless = False
        for j in hard:
            for bound, sgn in ((l[j], 1), (u[j], -1)):
                if np.isnan(bound):
                    hopeless = True
                elif np.isfinite(bound):
                    gap(sgn * (zm[j] - float(bound)), -feas_tol, max(1.0, abs(float(bound))))
                    hopeless = hopeless or sgn * (zm[j] - float(bound)) < -feas_tol
        viol = {}
        for (k, i) in inputs:
            if (k, i) in S:
                continue
            j = row(k, i)
            for bound, sgn in ((l[j], 1), (u[j], -1)):
                if np.isfinite(bound):
                    gap(sgn * (zm[j] - float(bound)), -feas_tol, max(1.0, abs(float(bound))))
                    if sgn * (zm[j] - float(bound)) < -feas_tol and (k, i) not in viol:
                        viol[(k, i)] = -sgn
        if hopeless:
            break
        ys = max(1.0, max(abs(float(v)) for v in ym))
        wrong = []
        for (k, i), s in S.items():
            yj = ym[row(k, i)]
            gap(s * yj, -dual_tol, ys)
            if not s * yj >= -dual_tol:
                wrong.append((k, i))
        if not viol and not wrong:
            f64 = lambda v: np.array([float(t) for t in v])      # noqa: E731
            out = dict(direct=1, w=f64(wm), y=f64(ym), z=f64(zm), kinv_norm=kn)
            break
        if r == rounds:
            break
        if r == 0:
            for (k, i) in inputs:
                s = int(np.sign(guess[k, i]))
                if s and (k, i) not in viol and np.isfinite((l if s < 0 else u)[row(k, i)]):
                    S[(k, i)] = s
        for key in wrong:
            del S[key]
        S.update(viol)
    act = np.zeros((N, nu), np.int32)
    for (k, i), s in S.items():
        act[k, i] = s
    out.update(act=act, rounds_used=used, margin=margin)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The case batch of a model and horizon: random strictly convex data on the pattern (dc.random_qp), one instance per role.  TIGHT: the box on the
# inputs the roles with active bounds use, as a fraction of the largest input of the unconstrained step; the states, path and link rows keep +-50.
TIGHT, TIGHT2 = 0.5, 0.2
ROLES = ("round0", "tight", "wrong_guess", "inf_guess", "all_held", "hopeless_state", "hopeless_path", "hopeless_link", "tight2",
         "ineligible", "failed", "frozen")
_REF = {}


def _inputs(mdl, k):
    return slice(mdl.np + k * mdl.f + mdl.nx, mdl.np + (k + 1) * mdl.f)


def case_batch(name, N, reg=0.0, seed=0):
    """(model, data dict [B, ...], guess [B, N, nu] int32, frozen [B] int32, roles: the role of every instance).  Deterministic; the hopeless and
    the wrong-guess instances are placed with the help of the NumPy statement's round 0 (where the step lies), which decides nothing about what
    the tests then expect: that comes from the restatement."""
    key = (name, N, reg, seed)
    if key in _REF:
        return _REF[key]
    mdl = model(name, N)
    roles = [r for r in ROLES if mdl.nh or r != "hopeless_path"]
    roles = [r for r in roles if mdl.nk or r != "hopeless_link"]
    B = len(roles)
    rng = np.random.default_rng(77 * N + mdl.f + seed)
    base = dc.random_qp(mdl, B, seed=3 + seed, pins="mix")
    free = dc.random_qp(mdl, B, seed=3 + seed, pins="none")
    d = {k: v.copy() for k, v in base.items()}
    guess = np.zeros((B, N, mdl.nu), np.int32)
    frozen = np.zeros(B, np.int32)
    npp, f, nx, nu, n = mdl.np, mdl.f, mdl.nx, mdl.nu, mdl.n

    def tighten(b, c=TIGHT):
        for k in range(N):
            s = _inputs(mdl, k)
            fr = d["l"][b, s] != d["u"][b, s]
            d["l"][b, s] = np.where(fr, -c, d["l"][b, s]); d["u"][b, s] = np.where(fr, c, d["u"][b, s])

    # the box of the roles with active bounds: a fraction of the largest free input of the unconstrained step, so that round 0 violates it
    w00 = mdl.direct_qp(d["P"], d["q"], d["A"], d["l"], d["u"], feas_tol=1e6, reg=reg)[0]
    box = np.zeros(B)
    for b, role in enumerate(roles):
        du0 = np.concatenate([np.where(d["l"][b, _inputs(mdl, k)] != d["u"][b, _inputs(mdl, k)], w00[b, _inputs(mdl, k)], 0.0) for k in range(N)])
        box[b] = float(np.abs(du0).max()) * (TIGHT2 if role == "tight2" else TIGHT)
        if role in ("tight", "tight2", "wrong_guess", "inf_guess", "hopeless_state", "hopeless_path", "hopeless_link", "frozen"):
            tighten(b, box[b])
        if role == "all_held":      # no pins; a linear term that pushes every input far above a low ceiling; wide state boxes
            for k2 in d:
                d[k2][b] = free[k2][b]
            for k in range(N):
                d["q"][b, _inputs(mdl, k)] = -25.0 - rng.uniform(0.0, 5.0, nu)
                d["u"][b, _inputs(mdl, k)] = 0.05
                d["l"][b, _inputs(mdl, k)] = -1e3
            for k in range(1, N):
                d["l"][b, npp + k * f:npp + k * f + nx] = -1e4; d["u"][b, npp + k * f:npp + k * f + nx] = 1e4
            d["l"][b, n + mdl.ngd:] = -1e4; d["u"][b, n + mdl.ngd:] = 1e4
    # where round 0 and the final point lie (placement only)
    w0 = mdl.direct_qp(d["P"], d["q"], d["A"], d["l"], d["u"], feas_tol=1e6, reg=reg)[0]
    wf, _, zf, drf, actf, _ = mdl.direct_qp_active(d["P"], d["q"], d["A"], d["l"], d["u"], reg=reg, rounds=8)
    for b, role in enumerate(roles):
        if role == "wrong_guess":      # an input the solution leaves strictly inside its box, named as held at its upper bound
            assert drf[b] == 1
            cand = [(k, i) for k in range(N) for i in range(nu) if actf[b, k, i] == 0 and d["l"][b, npp + k * f + nx + i] != d["u"][b, npp + k * f + nx + i]
                    and abs(wf[b, npp + k * f + nx + i]) < 0.9 * box[b]]
            if cand:
                k, i = cand[len(cand) // 2]
                guess[b, k, i] = 1
            else:                      # every free input ends held: name them all at the opposite bound
                guess[b] = -actf[b]
        if role == "inf_guess":
            k, i = N - 1, nu - 1
            d["l"][b, npp + k * f + nx + i] = -np.inf
            guess[b, k, i] = -1
        if role == "hopeless_state":      # a state of the last frame may not reach where every round puts it
            j = npp + (N - 1) * f
            d["u"][b, j] = min(w0[b, j], wf[b, j] if drf[b] == 1 else w0[b, j]) - 1.0
            d["l"][b, j] = d["u"][b, j] - 100.0
        if role == "hopeless_path":
            j = n + mdl.ngd + (N - 1) * mdl.nh
            d["l"][b, j] = 60.0; d["u"][b, j] = 70.0
        if role == "hopeless_link":
            j = n + mdl.ngd + N * mdl.nh
            d["l"][b, j] = -70.0; d["u"][b, j] = -60.0
        if role == "ineligible":
            o, _ = dc.spoiled(mdl, d, b, "pinned_later_state")
            for k2 in d:
                d[k2][b] = o[k2][0]
        if role == "failed":
            o, _ = dc.spoiled(mdl, d, b, "indefinite")
            for k2 in d:
                d[k2][b] = o[k2][0]
        if role == "frozen":
            frozen[b] = 1
    _REF[key] = (mdl, d, guess, frozen, roles)
    return _REF[key]


def restated(name, N, reg=0.0, rounds=4, digits=None, seed=0):
    """the restatement's results for every instance of the case batch (None for the frozen and the failed one: the pivot test is not restated),
    computed once per process and shared"""
    key = ("mp", name, N, reg, rounds, digits, seed)
    if key not in _REF:
        mdl, d, guess, frozen, roles = case_batch(name, N, reg, seed)
        res = []
        for b, role in enumerate(roles):
            if role in ("failed", "frozen"):
                res.append(None)
            else:
                res.append(active_mp(mdl, *(d[k][b] for k in ("P", "q", "A", "l", "u")), reg=reg, rounds=rounds, guess=guess[b], digits=digits))
        _REF[key] = res
    return _REF[key]


def tiled(name, N, B, reg=0.0):
    """the case batch repeated cyclically to B instances (device batches around the groups per block)"""
    mdl, d, guess, frozen, roles = case_batch(name, N, reg)
    idx = np.arange(B) % len(roles)
    return mdl, {k: np.ascontiguousarray(v[idx]) for k, v in d.items()}, np.ascontiguousarray(guess[idx]), np.ascontiguousarray(frozen[idx]), [roles[i] for i in idx]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The bound-riding recipe: double integrators started far enough out that |u| <= 1 saturates over the first part of the plan while the velocity
# stays inside |v| <= 2 -- direct_qp alone accepts nothing, the active set accepts everything.  The double integrator is linear and its cost
# quadratic: every SQP iteration sees the same QP solution.
RECIPE_B, RECIPE_N, RECIPE_ITERS = 8, 20, 3


def recipe():
    """(model, the dict getOptimalSolution takes, the iterate to start from [B, nvar])"""
    from optimal_control_problem_amd import models
    rng = np.random.default_rng(11)
    mdl = models.DoubleIntegrator(RECIPE_N)
    frame0 = np.zeros((RECIPE_B, mdl.f))
    frame0[:, 0] = rng.uniform(0.6, 0.9, size=RECIPE_B) * rng.choice([-1.0, 1.0], size=RECIPE_B)
    x0 = np.zeros((RECIPE_B, mdl.nvar))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    return mdl, dict(p=np.zeros((RECIPE_B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg), x0


MIXED_ROUNDS = 3


def mixed_block():
    """(model, data dict of 16 instances -- one block of the f <= 8 class --, restatement results at rounds = MIXED_ROUNDS): local systems of the
    double integrator on 20 frames at the zero iterate, started 0.01 m to 0.9 m out on either side, so that inside one block some instances are
    accepted in round 0, some in round 2 or later, and some spend their rounds"""
    key = ("mixed",)
    if key not in _REF:
        from optimal_control_problem_amd import models
        mdl = models.DoubleIntegrator(RECIPE_N)
        B = 16
        frame0 = np.zeros((B, mdl.f))
        frame0[:, 0] = np.array([0.01, 0.6, -0.9, 0.02, 0.75, -0.3, 0.9, -0.03, 0.35, 0.85, -0.8, 0.04, 0.4, -0.45, 0.5, -0.05])
        frame0[:, 1] = np.array([0.0, 0.1, -0.2, 0.0, 0.3, 0.2, -0.1, 0.0, -0.3, 0.15, 0.25, 0.0, -0.15, 0.05, 0.2, 0.0])
        lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
        ls = mdl.local_system(np.zeros((B, mdl.np)), np.zeros((B, mdl.nvar)), lbx, ubx, lbg, ubg)
        d = {k: np.array(getattr(ls, k), float) for k in ("P", "q", "A", "l", "u")}
        ref = [active_mp(mdl, *(d[k][b] for k in ("P", "q", "A", "l", "u")), rounds=MIXED_ROUNDS, digits=None) for b in range(B)]
        _REF[key] = (mdl, d, ref)
    return _REF[key]


def kkt_certificate(mdl, d, w, y, b):
    """the QP's own KKT conditions for instance b: (stationarity, bound violation, the worst wrong-signed multiplier, complementarity), each relative
    to max(1, |P|_max |w|_inf, |q|_inf).  Unread (NaN) slots are taken as dc.certificate takes them."""
    Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, d["P"][b], mdl.n, mdl.n)
    Pd = np.nan_to_num(np.where(np.isnan(Pd), Pd.T, Pd), nan=0.0)
    Ad, _ = dc.dense_from_csc(mdl.Ap, mdl.Ai, np.where(np.isnan(d["A"][b]), 1.0, d["A"][b]), mdl.m, mdl.n)
    q, l, u = d["q"][b], d["l"][b], d["u"][b]
    sc = max(1.0, float(np.abs(Pd).max() * np.abs(w).max()), float(np.abs(q).max()))
    z = Ad @ w
    stat = np.abs(Pd @ w + q + Ad.T @ y).max() / sc
    viol = max(0.0, float(np.max(l - z)), float(np.max(z - u))) / sc
    ineq = l < u
    with np.errstate(invalid="ignore"):
        up = np.where(np.isfinite(u), u - z, np.inf); lo = np.where(np.isfinite(l), z - l, np.inf)
        # y > 0 needs z at u, y < 0 needs z at l
        compl = max(float(np.max(np.where(ineq, np.maximum(y, 0.0) * np.minimum(up, 1e300), 0.0))),
                    float(np.max(np.where(ineq, np.maximum(-y, 0.0) * np.minimum(lo, 1e300), 0.0)))) / sc
    sign = 0.0      # a multiplier pushing against a bound that is not there
    sign = max(sign, float(np.max(np.where(ineq & ~np.isfinite(u), np.maximum(y, 0.0), 0.0))), float(np.max(np.where(ineq & ~np.isfinite(l), np.maximum(-y, 0.0), 0.0)))) / sc
    return stat, viol, sign, compl
