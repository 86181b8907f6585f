"""Cases, the exact minimiser and the recipes shared by tests/test_direct_ipm_host.py (CPU) and tests/test_gpu_direct_ipm.py -- TEST INFRASTRUCTURE
ONLY.

The exact minimiser of a case comes from something independent of the interior-point iteration: the CPU oracle (an ADMM) at eps 1e-9 names the
active set, then ONE dense KKT system with the pins, the active box rows and the dynamics rows as equalities is solved by
direct_active_cases._solve_held (LU in float64 with iterative refinement, the residual in mpmath at 60 digits), and the QP's KKT conditions are
checked on the 60-digit values: multiplier signs, feasibility of the inactive rows, strict complementarity."""
import numpy as np

from tests.support import direct_active_cases as da
from tests.support import direct_qp_cases as dc
from tests.support.direct_qp_cases import MODELS, model, rel_err, bits  # noqa: F401

HORIZONS = (2, 3, 20)
KEYS = ("P", "q", "A", "l", "u")
MARGIN = 1e-6
STRICT = 1e-6              # strict complementarity: the smallest active multiplier and the smallest inactive slack of a kept case
ITERS = 30
FEAS_TOL, COMP_TOL, STAT_TOL = 1e-9, 1e-6, 1e-5      # the defaults of options["direct_qp"]["interior_point"]

# The statement's rounding sensitivity e_np: the float64 statement against the same iteration in np.longdouble (direct_qp_ipm(dtype=np.longdouble)),
# relative to max(1, max |ref|) per array, the worst over every accepted instance of tests/test_direct_ipm_host.py::test_rounding_sensitivity, on
# batches whose every decision has a margin of MARGIN.  E_NP_*_MEASURED are the measured values; that test asserts that no case exceeds
# twice those (E_NP_W, E_NP_Y: headroom for another platform's rounding).  They are this large because a slack t = w - l of the size of mu is formed
# as a difference of numbers of size 1 -- it is known to eps / t of itself, about 1e-9 at the default comp_tol -- and every multiplier of an active
# row follows it (the header says so); iteration 0 acceptances agree to 4e-16.  The device bar is max(1e-12, 16 e_np) with the MEASURED e_np.
E_NP_W_MEASURED = 1.4e-9
E_NP_Y_MEASURED = 2.0e-8
E_NP_W = 2.0 * E_NP_W_MEASURED
E_NP_Y = 2.0 * E_NP_Y_MEASURED
DEVICE_BAR_W = max(1e-12, 16.0 * E_NP_W_MEASURED)
DEVICE_BAR_Y = max(1e-12, 16.0 * E_NP_Y_MEASURED)

# The distance of an accepted point to the exact minimiser at the default tolerances, relative to max(1, max |ref|): measured worst values over the
# kept cases (tests/test_direct_ipm_host.py::test_distance_to_the_exact_minimiser prints them; DESIGN 6.32 records them) and the bars a factor above.
DIST_W_MEASURED, DIST_Y_MEASURED = 2.5e-4, 3.2e-4
DIST_W_BAR, DIST_Y_BAR = 1e-3, 1e-3

ROLES = ("iter0", "state_upper", "state_lower", "input_bound", "several", "one_sided", "path_violated", "link_violated", "infeasible",
         "ineligible", "failed", "frozen")
ACTIVE_ROLES = ("state_upper", "state_lower", "input_bound", "several", "one_sided")
_REF = {}


def _state(mdl, k, c):
    return mdl.np + k * mdl.f + c


def _inputs(mdl, k):
    return slice(mdl.np + k * mdl.f + mdl.nx, mdl.np + (k + 1) * mdl.f)


def case_batch(name, N, reg=0.0, seed=0):
    """(model, data dict [B, ...], frozen [B] int32, roles).  Deterministic.  Random strictly convex data on the pattern (dc.random_qp: boxes +-50,
    which no unconstrained step comes near); the bounds of the roles are placed relative to the unconstrained step w0 of the instance (placement
    only: what the tests expect comes from the exact minimiser)."""
    key = (name, N, reg, seed)
    if key in _REF:
        return _REF[key]
    mdl = model(name, N)
    roles = [r for r in ROLES if (mdl.nh or r != "path_violated") and (mdl.nk or r != "link_violated")]
    B = len(roles)
    d = {k: v.copy() for k, v in dc.random_qp(mdl, B, seed=13 + seed, pins="mix").items()}
    frozen = np.zeros(B, np.int32)
    npp, f, nx, nu, n = mdl.np, mdl.f, mdl.nx, mdl.nu, mdl.n
    w0 = mdl.direct_qp(*(d[k] for k in KEYS), feas_tol=1e6, reg=reg)[0]
    last = N - 1

    def state_upper(b, k=last, c=0, by=0.3):
        j = _state(mdl, k, c)
        d["u"][b, j] = w0[b, j] - by * max(1.0, abs(w0[b, j]))

    for b, role in enumerate(roles):
        if role in ("state_upper", "path_violated", "link_violated", "frozen"):
            state_upper(b)
        if role == "state_lower":
            j = _state(mdl, last, nx - 1)
            d["l"][b, j] = w0[b, j] + 0.3 * max(1.0, abs(w0[b, j]))
        if role == "input_bound":      # the box of the free inputs at half the largest input of the unconstrained step
            free = np.concatenate([d["l"][b, _inputs(mdl, k)] != d["u"][b, _inputs(mdl, k)] for k in range(N)])
            u0 = np.concatenate([w0[b, _inputs(mdl, k)] for k in range(N)])
            c = 0.5 * float(np.abs(u0[free]).max())
            for k in range(N):
                s = _inputs(mdl, k)
                fr = d["l"][b, s] != d["u"][b, s]
                d["l"][b, s] = np.where(fr, -c, d["l"][b, s]); d["u"][b, s] = np.where(fr, c, d["u"][b, s])
        if role == "several":
            # A bound on the first state of every frame k >= 2, the first input of the last frame and the first free input of frame 0, each half way between the unconstrained
            # step w0 and a second trajectory wp -- the unconstrained step under a linear term that pushes these columns.  wp meets the dynamics and
            # the pins and lies strictly inside every bound so placed: the box is feasible by construction, and w0 violates every one of them.
            qp = d["q"].copy()
            cols = [_state(mdl, k, 0) for k in range(2, N)]          # (frame 1's states hang on frame 0's inputs alone, which get a bound of their own)
            cols += [npp + nx + i for i in range(nu) if d["l"][b, npp + nx + i] != d["u"][b, npp + nx + i]][:1]
            cols += [npp + last * f + nx]          # (the last frame's input moves nothing else: its bound is active for sure)
            qp[b, cols] += 3.0
            wp = mdl.direct_qp(d["P"][b:b + 1], qp[b:b + 1], d["A"][b:b + 1], d["l"][b:b + 1], d["u"][b:b + 1], feas_tol=1e6, reg=reg)[0][0]
            for j in cols:
                if abs(wp[j] - w0[b, j]) < 1e-2 * max(1.0, abs(w0[b, j])):      # a column the inputs do not move (the pattern's zeros) gets no bound
                    continue
                mid = 0.5 * (w0[b, j] + wp[j])
                if wp[j] < w0[b, j]:
                    d["u"][b, j] = mid
                else:
                    d["l"][b, j] = mid
        if role == "one_sided":
            state_upper(b)
            d["l"][b, _state(mdl, last, 0)] = -np.inf
            for k in range(1, N):
                d["l"][b, _inputs(mdl, k)] = -np.inf
        if role == "path_violated":
            j = n + mdl.ngd + last * mdl.nh
            d["l"][b, j] = 60.0; d["u"][b, j] = 70.0
        if role == "link_violated":
            j = n + mdl.ngd + N * mdl.nh
            d["l"][b, j] = -70.0; d["u"][b, j] = -60.0
        if role == "infeasible":       # inputs of at most 0.01 cannot move the last frame's first state by 10
            for k in range(N):
                s = _inputs(mdl, k)
                fr = d["l"][b, s] != d["u"][b, s]
                d["l"][b, s] = np.where(fr, -0.01, d["l"][b, s]); d["u"][b, s] = np.where(fr, 0.01, d["u"][b, s])
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
    b = roles.index("infeasible")
    wt = mdl.direct_qp_ipm(*(d[k][b:b + 1] for k in KEYS), reg=reg, iters=40)
    assert wt[3][0] == 1                 # (placement: where the last frame lies under the tiny input box)
    j = _state(mdl, last, 0)
    d["u"][b, j] = wt[0][0, j] - 10.0; d["l"][b, j] = d["u"][b, j] - 1.0
    _REF[key] = (mdl, d, frozen, roles)
    return _REF[key]


def filled(mdl, d, rows):
    """the data of instances `rows` with the unread (NaN) slots as the rule takes them: P symmetric, the identity and s_{k+1} entries of A 1"""
    out = {k: d[k][rows].copy() for k in KEYS}
    out["A"] = np.where(np.isnan(out["A"]), 1.0, out["A"])
    for i in range(len(rows)):
        Pd, _ = dc.dense_from_csc(mdl.Pp, mdl.Pi, out["P"][i], mdl.n, mdl.n)
        Pd = np.nan_to_num(np.where(np.isnan(Pd), Pd.T, Pd), nan=0.0)
        out["P"][i] = np.array([Pd[mdl.Pi[e], j] for j in range(mdl.n) for e in range(mdl.Pp[j], mdl.Pp[j + 1])])
    return out


def exact(name, N, reg=0.0):
    """per instance of the case batch None, or dict(w, y [float64, rounded from 60 digits], active: number of active box rows, strict: the smallest
    active multiplier / inactive slack, states_up, states_lo, inputs, frames: which kinds of rows are active) -- only for the ACTIVE_ROLES, and only
    where the oracle solved the QP; `strict` is NOT filtered here: the test asserts it"""
    key = ("exact", name, N, reg)
    if key in _REF:
        return _REF[key]
    import mpmath as mp
    from oracle import oracle as orc
    mdl, d, frozen, roles = case_batch(name, N, reg)
    npp, f, nx, nu, n, ngd = mdl.np, mdl.f, mdl.nx, mdl.nu, mdl.n, mdl.ngd
    rows = [b for b, r in enumerate(roles) if r in ACTIVE_ROLES]
    dd = filled(mdl, d, rows)
    if reg:      # reg sits on the free inputs' diagonal: the QP the rule solves
        pslot, _ = mdl._riccati_slots()
        for i, b in enumerate(rows):
            pin = d["l"][b, npp + nx:npp + f] == d["u"][b, npp + nx:npp + f]
            for k in range(N):
                for c in range(nx, f):
                    if not (k == 0 and pin[c - nx]):
                        dd["P"][i, pslot[k, c, c]] += reg
    st = orc.default_settings()
    st.eps_abs = st.eps_rel = 1e-9; st.max_iter = 400000
    out = orc.Pattern(mdl.n, mdl.m, mdl.Pp, mdl.Pi, mdl.Ap, mdl.Ai).solve(*(dd[k] for k in KEYS), st)
    res = [None] * len(roles)
    for i, b in enumerate(rows):
        if out["status"][i] != 1:
            continue
        l, u = d["l"][b], d["u"][b]
        held = {c: l[npp + c] for c in range(f) if l[npp + c] == u[npp + c]}
        sides = {}
        for c in range(f, N * f):
            j = npp + c
            if out["y"][i, j] > 5e-7:
                held[c] = u[j]; sides[c] = 1
            elif out["y"][i, j] < -5e-7:
                held[c] = l[j]; sides[c] = -1
        for c in range(nx, f):
            j = npp + c
            if l[j] != u[j]:
                if out["y"][i, j] > 5e-7:
                    held[c] = u[j]; sides[c] = 1
                elif out["y"][i, j] < -5e-7:
                    held[c] = l[j]; sides[c] = -1
        with mp.workdps(60):
            wm, ym, zm, kn = da._solve_held(mdl, d["P"][b], d["q"][b], d["A"][b], l, reg, held, 60)
            strict = mp.inf
            for c, s in sides.items():
                strict = min(strict, s * ym[npp + c])             # the right sign, by a margin
            for c in range(nx, N * f):
                j = npp + c
                if c in held:
                    continue
                for bound, sgn in ((l[j], 1), (u[j], -1)):
                    if np.isfinite(bound):
                        strict = min(strict, sgn * (wm[j] - mp.mpf(float(bound))))
            for j in range(n + ngd, mdl.m):                       # path and link rows: inactive
                for bound, sgn in ((l[j], 1), (u[j], -1)):
                    strict = min(strict, sgn * (zm[j] - mp.mpf(float(bound))))
            res[b] = dict(w=np.array([float(v) for v in wm]), y=np.array([float(v) for v in ym]), strict=float(strict), active=len(sides), kinv_norm=kn,
                          states_up=[c for c, s in sides.items() if c % f < nx and s > 0], states_lo=[c for c, s in sides.items() if c % f < nx and s < 0],
                          inputs=[c for c in sides if c % f >= nx], frames=sorted({c // f for c in sides}))
    _REF[key] = res
    return res


def margins(mdl, d, trace, direct, used, feas_tol=FEAS_TOL, comp_tol=COMP_TOL, stat_tol=STAT_TOL):
    """the smallest distance of any decision of the statement's run from its threshold, per instance [B]: alpha against MPCQP_IPM_ALPHA_SHORT, max
    lambda t and mu against comp_tol and stat against stat_tol (relative to the threshold), (at a candidate) every path and link row against its
    bound -+ feas_tol (relative to max(1, |bound|)), and every barriered row against its bound -+ feas_tol relative to feas_tol + |w - bound|: an
    active row sits a slack t of the size of mu inside its bound, so no margin relative to the bound can be asked of it; the slack itself is known
    to about 1e-8 of its size, and it is against that that the distance counts.  alpha itself is min(1, FRAC min ratios), a continuous function of the
    data: which entry attains the minimum is no decision.  (Iteration 0's test is direct_qp's, whose margins tests/test_direct_qp_host.py covers;
    here the first trace entry's box margins stand for the cases that start iterating.)"""
    B = direct.shape[0]
    npp, n, N, f, nx = mdl.np, mdl.n, mdl.N, mdl.f, mdl.nx
    lf = d["l"][:, npp:n].reshape(B, N, f); uf = d["u"][:, npp:n].reshape(B, N, f)
    bar = np.ones((B, N, f), bool); bar[:, 0, :nx] = False; bar[:, 0, nx:] = lf[:, 0, nx:] != uf[:, 0, nx:]
    rowh = n + mdl.ngd
    out = np.full(B, np.inf)
    with np.errstate(all="ignore"):
        for t in trace:
            o = t["open"]
            m = np.abs(t["alpha"] - mdl.IPM_ALPHA_SHORT)
            m = np.minimum(m, np.abs(t["comp"] - comp_tol) / comp_tol)
            m = np.minimum(m, np.abs(t["mu"] - comp_tol) / comp_tol)
            m = np.minimum(m, np.where(np.isnan(t["stat"]), np.inf, np.abs(t["stat"] - stat_tol) / stat_tol))
            near = t["comp"] <= 10.0 * comp_tol                   # (further out the box test decides nothing)
            gl = np.where(bar & np.isfinite(lf), np.abs(t["d"] - (lf - feas_tol)) / (feas_tol + np.abs(t["d"] - lf)), np.inf).min(axis=(1, 2))
            gu = np.where(bar & np.isfinite(uf), np.abs(t["d"] - (uf + feas_tol)) / (feas_tol + np.abs(t["d"] - uf)), np.inf).min(axis=(1, 2))
            m = np.minimum(m, np.where(near, np.minimum(gl, gu), np.inf))
            if "z" in t and d["l"].shape[1] > rowh:
                zl, zu = d["l"][:, rowh:], d["u"][:, rowh:]
                gz = np.minimum(np.abs(t["z"][:, rowh:] - (zl - feas_tol)) / np.maximum(1.0, np.abs(zl)),
                                np.abs(t["z"][:, rowh:] - (zu + feas_tol)) / np.maximum(1.0, np.abs(zu))).min(axis=1)
                m = np.minimum(m, np.where(t["cand"], gz, np.inf))
            out = np.where(o, np.minimum(out, m), out)
    return out


def tiled(name, N, B, reg=0.0):
    """the case batch repeated cyclically to B instances (device batches around the groups per block)"""
    mdl, d, frozen, roles = case_batch(name, N, reg)
    idx = np.arange(B) % len(roles)
    return mdl, {k: np.ascontiguousarray(v[idx]) for k, v in d.items()}, np.ascontiguousarray(frozen[idx]), [roles[i] for i in idx]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The state-bound recipe: double integrators 3 to 4 m out, moving towards the origin at 1.6 to 1.9 m/s.  Every plan speeds up to the limit
# |v| <= 2 under u = -+1, rides it, and brakes: a state bound and an input bound are active in every QP.  direct_qp alone violates both; the
# active set holds the input and then finds the velocity outside its box, which no held input repairs.  The model is linear and its cost quadratic:
# every SQP iteration sees the same QP solution.
RECIPE_B, RECIPE_N, RECIPE_ITERS = 8, 20, 3


def recipe():
    """(model, the dict getOptimalSolution takes, the iterate to start from [B, nvar])"""
    from optimal_control_problem_amd import models
    rng = np.random.default_rng(23)
    mdl = models.DoubleIntegrator(RECIPE_N)
    sgn = rng.choice([-1.0, 1.0], size=RECIPE_B)
    frame0 = np.zeros((RECIPE_B, mdl.f))
    frame0[:, 0] = sgn * rng.uniform(3.0, 4.0, size=RECIPE_B)
    frame0[:, 1] = -sgn * rng.uniform(1.6, 1.9, size=RECIPE_B)
    x0 = np.zeros((RECIPE_B, mdl.nvar))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    return mdl, dict(p=np.zeros((RECIPE_B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg), x0


def mixed_block():
    """(model, data dict of 16 instances -- one block of the f <= 8 class -- and frozen): local systems of the double integrator on 20 frames at
    the zero iterate, some near the origin (accepted in iteration 0), some riding the velocity limit from different distances (accepted after
    different numbers of iterations), one whose first frame already breaks the velocity limit by so much that the box cannot be met (rejected
    after `iters`), one ineligible, one frozen"""
    key = ("mixed",)
    if key not in _REF:
        from optimal_control_problem_amd import models
        mdl = models.DoubleIntegrator(RECIPE_N)
        B = 16
        frame0 = np.zeros((B, mdl.f))
        frame0[:, 0] = np.array([0.01, 3.0, -3.5, 0.02, 4.0, -0.3, 0.9, -0.03, 3.2, 0.85, -3.8, 0.04, 0.4, -2.5, 2.0, -0.05])
        frame0[:, 1] = np.array([0.0, -1.7, 1.8, 0.0, -1.9, 0.2, -0.1, 0.0, -1.6, 0.15, 1.9, 0.0, -0.15, 1.5, 2.6, 0.0])
        lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
        ls = mdl.local_system(np.zeros((B, mdl.np)), np.zeros((B, mdl.nvar)), lbx, ubx, lbg, ubg)
        d = {k: np.array(getattr(ls, k), float) for k in KEYS}
        o, _ = dc.spoiled(mdl, d, 12, "pinned_later_state")
        for k in KEYS:
            d[k][12] = o[k][0]
        frozen = np.zeros(B, np.int32); frozen[7] = 1
        _REF[key] = (mdl, d, frozen)
    return _REF[key]


def statement(name, N, reg=0.0, iters=ITERS):
    """the NumPy statement's result on the case batch at the default tolerances, computed once per process and shared (the statement treats every
    instance on its own: a tiled batch has the tiled results)"""
    key = ("st", name, N, reg, iters)
    if key not in _REF:
        mdl, d, frozen, roles = case_batch(name, N, reg)
        _REF[key] = mdl.direct_qp_ipm(*(d[k] for k in KEYS), feas_tol=FEAS_TOL, reg=reg, iters=iters, comp_tol=COMP_TOL, stat_tol=STAT_TOL, frozen=frozen)
    return _REF[key]
