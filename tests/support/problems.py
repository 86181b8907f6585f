"""Shared problem builders for the test-suite (test infrastructure)."""
import numpy as np

from optimal_control_problem_amd import models


def toy_local_system(mdl, arg, x=None):
    p = np.asarray(arg["p"], float).reshape(1, -1)
    x = np.zeros((1, mdl.nx)) if x is None else np.asarray(x, float).reshape(1, -1)
    return mdl.local_system(p, x, np.asarray(arg["lbx"], float)[None], np.asarray(arg["ubx"], float)[None],
                            np.asarray(arg["lbg"], float).reshape(1, -1), np.asarray(arg["ubg"], float).reshape(1, -1))


def oracle_solve(ls, settings=None, nthreads=1, x0=None, y0=None, rho0=None, **kw):
    """settings: an oracle Settings object, or keyword settings; x0 / y0: warm start; rho0: per-instance starting rho"""
    from oracle import oracle as orc
    pat = orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
    s = settings or orc.default_settings(**kw)
    return pat.solve(ls.P, ls.q, ls.A, ls.l, ls.u, s, nthreads=nthreads, x0=x0, y0=y0, rho0=rho0)


# Settings under which the workloads change rho often enough to reach the iteration kernel's in-place re-factorisation (the last launch
# pair of a solve in the two-kernel on-chip form): id -> (workload, N, batch, settings, the MPCQP_RESUME_ROUNDS values it is used at, whether at
# least half of the batch reaches the last pair at each of them -- otherwise only some do).  tests/test_rho_recipes.py holds the oracle's update
# counts to what tests/test_gpu_rho_resume.py relies on.
_Q_RHO = dict(adaptive_rho_interval=20, rho=10.0, adaptive_rho_tolerance=1.5, eps_abs=1e-7, eps_rel=1e-7)
RHO_RECIPES = {
    "q20": ("quadrotor", 20, 24, _Q_RHO, (0, 1), True),
    "q50": ("quadrotor", 50, 12, _Q_RHO, (0, 1), True),
    "cp30": ("cartpole", 30, 24, dict(adaptive_rho_tolerance=1.5, eps_abs=1e-6, eps_rel=1e-6), (0,), True),
    "cp100": ("cartpole", 100, 12, dict(rho=1e-3), (0,), True),
    "di60": ("double_integrator", 60, 24, dict(adaptive_rho_tolerance=1.5, eps_abs=1e-6, eps_rel=1e-6), (0, 1), False),
}


def rho_recipe(rid, batch=None):
    """-> (model, LocalSystem, meta, settings dict) of one RHO_RECIPES entry (default seeds; batch overrides the recipe's)"""
    name, N, B, settings = RHO_RECIPES[rid][:4]
    mdl, ls, meta = models.make_workload(name, batch or B, N=N)
    return mdl, ls, meta, dict(settings)


def oracle_rho_updates(ls, nthreads=8, rho0=None, x0=None, y0=None, steps=False, **settings):
    """Number of rho changes per instance, from oracle prefix runs: max_iter = k * interval + 1 for k = 1, 2, ... shows the rho in force after the
    adaptive-rho step of iteration k * interval; a change counts while the instance is still running: its full run goes beyond that iteration, or ends
    there on the iteration limit without having passed a termination check in that iteration (the update is then the last thing the run did).
    steps=True: -> (counts, changed [B, K] bool, interval) with changed[b, k - 1] = instance b changed rho at iteration k * interval."""
    start = {k: v for k, v in dict(rho0=rho0, x0=x0, y0=y0).items() if v is not None}
    from oracle import oracle as orc
    full = oracle_solve(ls, nthreads=nthreads, **start, **settings)
    s = orc.default_settings(**settings)
    interval = s.adaptive_rho_interval or 4 * s.check_termination
    prev = np.full(ls.batch, s.rho) if rho0 is None else np.where(np.asarray(rho0, float) > 0, rho0, s.rho)
    prev = np.broadcast_to(prev, (ls.batch,)).copy()
    K = int(full["iters"].max()) // interval if s.adaptive_rho and interval > 0 else 0
    changed = np.zeros((ls.batch, K), bool)
    for k in range(1, K + 1):
        r = oracle_solve(ls, nthreads=nthreads, **start, **dict(settings, max_iter=min(k * interval + 1, s.max_iter)))
        # (the loop leaves on a termination check before the rho step: statuses 1, 3, 5 of a check made in this iteration)
        left = np.isin(full["status"], (1, 3, 5)) if s.check_termination and k * interval % s.check_termination == 0 else np.zeros(ls.batch, bool)
        running = (full["iters"] > k * interval) | ((full["iters"] == k * interval) & (s.max_iter == k * interval) & ~left)
        changed[:, k - 1] = running & (r["rho"] != prev)
        prev = np.where(running, r["rho"], prev)
    assert np.array_equal(prev, full["rho"]), "prefix runs do not end at the full run's rho"
    counts = changed.sum(axis=1)
    return (counts, changed, interval) if steps else counts


def oracle_stable_mask(ls, draws=3, nthreads=8, rho0=None, x0=None, y0=None, **settings):
    """Instances whose decisions (iteration count, every rho update) do not hang on rounding: iters and rho of the oracle stay the same when
    P, A, q are multiplied entry by entry by 1 + 1e-12 * N(0, 1), `draws` times.  Only these can be asked for equal iteration counts of two
    implementations that round differently."""
    start = {k: v for k, v in dict(rho0=rho0, x0=x0, y0=y0).items() if v is not None}
    ref = oracle_solve(ls, nthreads=nthreads, **start, **settings)
    rng = np.random.default_rng(99)
    ok = np.ones(ls.batch, bool)
    for _ in range(draws):
        P, A, q = (a * (1.0 + 1e-12 * rng.standard_normal(a.shape)) for a in (ls.P, ls.A, ls.q))
        r = oracle_solve(models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, P, q, A, ls.l, ls.u), nthreads=nthreads, **start, **settings)
        # (rho "the same": to 1e-6 -- a decision that falls the other way moves it by adaptive_rho_tolerance or more, a value that moves by more than the
        # parity bar under this perturbation cannot be held to it)
        ok &= (r["iters"] == ref["iters"]) & (np.abs(r["rho"] - ref["rho"]) <= 1e-6 * np.abs(ref["rho"])) & (r["status"] == ref["status"])
    return ok


def take(ls, idx):
    """the instances idx of a batch, as a batch of their own"""
    pick = lambda a: a if a.ndim == 1 else np.ascontiguousarray(a[idx])
    return models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, pick(ls.P), pick(ls.q), pick(ls.A), pick(ls.l), pick(ls.u), ls.np)


# Iteration limits on a rho update, as (MPCQP_RESUME_ROUNDS, which update of an instance: 0 = first, 1 = second, whether the update parks the instance).  The
# launches of a solve are rounds + 1 iteration kernels <RF=0>, each of which parks an instance on its next update, and a last one <RF=1> that re-factorises in
# place: update number j (from 1) parks iff j <= rounds + 1.  Parked on the limit, the instance is picked up by a launch that has no iteration left to do (one
# at limit + 1) and ends in the kernel's tail with the state read back from the slab; in place on the limit, <RF=1> re-factorises in its last iteration.
UPDATE_LIMIT_CASES = [(0, 0, True), (1, 1, True), (0, 1, False)]


def update_limits(ls, settings, which):
    """(k * interval, k * interval + 1) for the k of the first (which = 0) or second (1) rho update of the first instance that has that many: iteration limits at
    which an update and the limit fall in the same step, and at which one iteration is left after the update"""
    counts, changed, interval = oracle_rho_updates(ls, steps=True, **settings)
    b = int(np.argmax(counts > which))
    assert counts[b] > which
    k = int(np.flatnonzero(changed[b])[which]) + 1
    return k * interval, k * interval + 1


def split_rho(batch):
    """per-instance starting rho: the first half of the batch at 0.1, the second at 10"""
    return np.r_[np.full(batch // 2, 0.1), np.full(batch - batch // 2, 10.0)]


def warm_point(ls, settings):
    """-> (x0, y0, settings with warm_start = 1): the oracle's solution of the batch with q perturbed by 5 %"""
    rng = np.random.default_rng(5)
    near = models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, ls.P, ls.q * (1.0 + 0.05 * rng.standard_normal(ls.q.shape)), ls.A, ls.l, ls.u)
    w = oracle_solve(near, nthreads=8, **settings)
    return w["x"], w["y"], dict(settings, warm_start=1)


# ---------------------------------------------------------------------------------------------- settings and exit statuses
# The MPC workloads with two instances spoilt, so that every kernel family (the on-chip ones take stage patterns only) meets certificates of
# infeasibility next to ordinary solves: id -> (workload, N, batch).  tests/test_settings_recipes.py holds the oracle's outcomes on them to what
# tests/test_gpu_settings.py relies on.
HARD_WORKLOADS = {"q20": ("quadrotor", 20, 8), "cp30": ("cartpole", 30, 6), "q50": ("quadrotor", 50, 4), "cp100": ("cartpole", 100, 4)}
DUAL_INFEASIBLE, PRIMAL_INFEASIBLE = 1, 2          # the instances hard_stage_batch alters


def hard_stage_batch(wid, dual=True, dual_q=-1.0):
    """-> (model, LocalSystem, meta) of HARD_WORKLOADS[wid] with
      * instance 2 primal infeasible: the second frame's first state boxed into [50, 60], which the pinned first frame cannot reach in one step;
      * instance 1 dual infeasible (dual=True): the last frame's last input -- which no dynamics row reads -- without curvature (its row and column of P
        zero), with q = dual_q = -1 and its only row of A (its box) unbounded: an unbounded direction of descent.
    P is materialised per instance where the workload shares it; meta["dual_rows"]: the rows of A that were unbounded.
    wid: an id of HARD_WORKLOADS, or any (workload, N, batch) with batch >= 3 (tests/support/instance_cases.py)."""
    name, N, B = HARD_WORKLOADS[wid] if isinstance(wid, str) else wid
    mdl, ls, meta = models.make_workload(name, B, N=N)
    P = np.array(np.broadcast_to(ls.P, (B, len(ls.Pi)))); q, l, u = ls.q.copy(), ls.l.copy(), ls.u.copy()
    row = mdl.np + mdl.f
    l[PRIMAL_INFEASIBLE, row], u[PRIMAL_INFEASIBLE, row] = 50.0, 60.0
    rows_of_j = np.zeros(0, int)
    if dual:
        j = ls.n - 1
        cols = np.repeat(np.arange(ls.n), np.diff(ls.Pp))
        P[DUAL_INFEASIBLE, (cols == j) | (np.asarray(ls.Pi) == j)] = 0.0
        q[DUAL_INFEASIBLE, j] = dual_q
        rows_of_j = np.asarray(ls.Ai[ls.Ap[j]:ls.Ap[j + 1]], int)
        l[DUAL_INFEASIBLE, rows_of_j] = -np.inf; u[DUAL_INFEASIBLE, rows_of_j] = np.inf
    hard = models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, P, q, ls.A, l, u, ls.np)
    return mdl, hard, dict(meta, dual_rows=rows_of_j)


# id -> settings: every numeric field of mpcqp_settings that changes what the loop does, at a value other than its default, one at a time (and the
# iteration limits that end a run off a termination check).  A check_termination = 0 entry carries a small max_iter: nothing else stops such a run.
from collections import OrderedDict      # noqa: E402
SETTINGS_MATRIX = OrderedDict([
    ("default", {}),
    ("max_iter=24", dict(max_iter=24)),
    ("max_iter=37", dict(max_iter=37)),
    ("max_iter=60", dict(max_iter=60)),
    ("check=0,max_iter=40", dict(check_termination=0, max_iter=40)),
    ("check=7,max_iter=30", dict(check_termination=7, max_iter=30)),
    ("check=1", dict(check_termination=1)),
    ("alpha=1.0", dict(alpha=1.0)),
    ("scaling=0", dict(scaling=0)),
    ("scaled_termination=1", dict(scaled_termination=1)),
    ("eps_dual_inf=1e-7", dict(eps_dual_inf=1e-7)),
    ("eps_prim_inf=1e-7,eps_dual_inf=1e-2", dict(eps_prim_inf=1e-7, eps_dual_inf=1e-2)),
    ("alpha=1.9", dict(alpha=1.9)),
    ("sigma=1e-3", dict(sigma=1e-3)),
    ("scaling=3", dict(scaling=3)),
    ("adaptive_rho=0", dict(adaptive_rho=0)),
    ("rho=1.0", dict(rho=1.0)),
    ("scaling=25", dict(scaling=25)),
])


def _ends_in_the_tail(st):
    check, limit = st.get("check_termination", 25), st.get("max_iter", 10000)
    return check == 0 or limit % check != 0


# the settings under which a run that reaches the iteration limit is judged in the code after the loop, not by a termination check inside it
TAIL_CASES = tuple(k for k, st in SETTINGS_MATRIX.items() if _ends_in_the_tail(st))
# ... and, of these, the ones under which nothing in the loop looks at the iterates' last steps before that (no check, no rho update) on the quadrotor N=20
NEVER_SAVED = ("max_iter=24", "check=0,max_iter=40")
# the settings the kept-workspace leg runs under (the kept path scales q, l, u with parked D, E, c and has its own entry into the loop)
KEPT_CASES = ("alpha=1.0", "scaling=0", "scaled_termination=1", "check=7,max_iter=30")
# ... and the reduced-form leg (the settings have to reach the inner handle)
REDUCED_CASES = ("alpha=1.0", "check=7,max_iter=30")


def kept_q(ls):
    """the q of the second, vectors-only solve of the kept-workspace leg"""
    return ls.q * (1.0 + 0.1 * np.random.default_rng(17).standard_normal(ls.q.shape))


def oracle_kept_solves(ls, q2, nthreads=8, l2=None, u2=None, **settings):
    """-> (full solve, vectors-only solve with q2 -- and the bounds l2, u2 where given, else the first solve's) of the oracle's kept workspaces
    (osqp_update_data_vec semantics)"""
    from oracle import oracle as orc
    state = orc.State(orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai), ls.batch, orc.default_settings(**settings))
    return (state.solve(ls.P, ls.q, ls.A, ls.l, ls.u, nthreads=nthreads),
            state.solve_vectors(q2, ls.l if l2 is None else l2, ls.u if u2 is None else u2, nthreads=nthreads))


def oracle_kept_stable_mask(ls, q2, draws=3, nthreads=8, l2=None, u2=None, **settings):
    """oracle_stable_mask for the pair of solves of a kept workspace: -> (mask of the full solve, mask of the vectors-only solve)"""
    if l2 is not None or u2 is not None:
        settings = dict(settings, l2=l2, u2=u2)
    ref = oracle_kept_solves(ls, q2, nthreads, **settings)
    rng = np.random.default_rng(99)
    ok = [np.ones(ls.batch, bool), np.ones(ls.batch, bool)]
    for _ in range(draws):
        P, A, q, qq = (a * (1.0 + 1e-12 * rng.standard_normal(a.shape)) for a in (ls.P, ls.A, ls.q, q2))
        got = oracle_kept_solves(models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, P, q, A, ls.l, ls.u), qq, nthreads, **settings)
        for k in (0, 1):
            ok[k] &= (got[k]["iters"] == ref[k]["iters"]) & (np.abs(got[k]["rho"] - ref[k]["rho"]) <= 1e-6 * np.abs(ref[k]["rho"])) & (got[k]["status"] == ref[k]["status"])
    return ok[0], ok[1]


BIG_BATCH = 700          # more instances than an MI355X has compute units: the eight-wave instances run one workgroup per CU and queue the rest


def big_batch_sample(rid, batch=BIG_BATCH):
    """-> (the oracle's sample of a recipe at BIG_BATCH as a batch of its own, its indices, settings): 64 instances, 32 for the slow cart-pole N=100"""
    _, ls, _, settings = rho_recipe(rid, batch)
    idx = np.arange(0, batch, 11)[:64] if rid != "cp100" else np.arange(0, batch, 22)[:32]
    return take(ls, idx), idx, settings


def random_qp(n, m, seed, density=0.3, infeasible=None):
    """Random strictly convex QP with mixed equality / inequality / one-sided / free rows, dense patterns."""
    rng = np.random.default_rng(seed)
    Mx = rng.normal(size=(n, n)) * (rng.random((n, n)) < density)
    P = Mx @ Mx.T + 0.1 * np.eye(n)
    A = rng.normal(size=(m, n)) * (rng.random((m, n)) < density)
    for i in range(m):
        if not A[i].any():
            A[i, rng.integers(n)] = 1.0
    xf = rng.normal(size=n)
    ax = A @ xf
    l = ax - rng.random(m); u = ax + rng.random(m)
    kind = rng.integers(0, 4, size=m)
    l[kind == 1] = -np.inf; u[kind == 2] = np.inf
    eq = kind == 3
    u[eq] = l[eq] = ax[eq]
    q = rng.normal(size=n)
    if infeasible == "primal":      # two contradictory rows
        A[0] = 0; A[0, 0] = 1.0; A[1] = 0; A[1, 0] = 1.0
        l[0], u[0] = 1.0, 2.0; l[1], u[1] = -2.0, -1.0
    if infeasible == "dual":        # unbounded direction: zero curvature + free along e0
        P[0, :] = 0; P[:, 0] = 0; A[:, 0] = 0; q[0] = -1.0
    hm = np.ones((n, n), bool); am = np.ones((m, n), bool)
    Pp, Pi = models._csc_from_dense_mask(hm); Ap, Ai = models._csc_from_dense_mask(am)
    return models.LocalSystem(n, m, Pp, Pi, Ap, Ai, P.T[hm.T][None].copy(), q[None].copy(), A.T[am.T][None].copy(), l[None].copy(), u[None].copy())


def fuzz_pattern_draw(c):
    """(n, m, B, density) of pattern c of the randomised sweep's slice in tests/test_gpu_fuzz.py (the generator of tools/fuzz_gpu.py); sparse_batch(n, m, B, c, density)
    is its batch"""
    rng = np.random.default_rng(1000 + c)
    n = int(rng.integers(2, 140)); m = int(rng.integers(1, 200)); B = int(rng.integers(1, 9))
    return n, m, B, float(rng.choice([0.05, 0.15, 0.4, 1.0]))


def sparse_batch(n, m, B, seed, dens):
    """Batch of B convex QPs sharing a random SPARSE pattern (symmetric P mask with full diagonal, A mask with no empty row),
    mixed equality / inequality / one-sided rows."""
    rng = np.random.default_rng(seed)
    hm = np.eye(n, dtype=bool) | (rng.random((n, n)) < dens)
    hm = hm | hm.T
    am = rng.random((m, n)) < dens
    for i in range(m):
        if not am[i].any():
            am[i, rng.integers(n)] = True
    Pp, Pi = models._csc_from_dense_mask(hm); Ap, Ai = models._csc_from_dense_mask(am)
    Ps, As, qs, ls, us = [], [], [], [], []
    for b in range(B):
        Mx = rng.normal(size=(n, n)) * hm * (rng.random((n, n)) < 0.7)
        L = np.tril(Mx); P = L @ L.T
        P = P * hm + np.diag(np.abs(P).sum(axis=1) * (1 - hm).sum(axis=1) + 0.1)      # masked + diagonally dominant => PSD
        P = 0.5 * (P + P.T)
        A = rng.normal(size=(m, n)) * am
        xf = rng.normal(size=n); ax = A @ xf
        l = ax - rng.random(m); u = ax + rng.random(m)
        kind = rng.integers(0, 4, size=m)
        l[kind == 1] = -np.inf; u[kind == 2] = np.inf
        eq = kind == 3; u[eq] = l[eq] = ax[eq]
        Ps.append(P.T[hm.T]); As.append(A.T[am.T]); qs.append(rng.normal(size=n)); ls.append(l); us.append(u)
    return models.LocalSystem(n, m, Pp, Pi, Ap, Ai, np.array(Ps), np.array(qs), np.array(As), np.array(ls), np.array(us))




def reduce_qp(ls, fixed_rows):
    """NumPy statement of the reduced form (mpcqp_create_reduced): substitute the variables of the named equality singleton rows.
    Returns (reduced LocalSystem, free variable indices, kept row indices, fixed variable indices, x_fixed [B, nfix])."""
    import scipy.sparse as sp
    from optimal_control_problem_amd import models
    n, m, B = ls.n, ls.m, ls.batch
    fixed_rows = np.asarray(fixed_rows, int)
    Apat = sp.csc_matrix((np.arange(1, len(ls.Ai) + 1), ls.Ai, ls.Ap), shape=(m, n)).tocsr()
    fvars = np.array([Apat[i].indices[0] for i in fixed_rows]); asrc = np.array([Apat[i].data[0] - 1 for i in fixed_rows])
    free = np.setdiff1d(np.arange(n), fvars); kept = np.setdiff1d(np.arange(m), fixed_rows)
    Av = np.broadcast_to(ls.A, (B, len(ls.Ai))); Pv = np.broadcast_to(ls.P, (B, len(ls.Pi)))
    xfix = ls.l[:, fixed_rows] / Av[:, asrc]
    cols = np.repeat(np.arange(n), np.diff(ls.Pp)); colsA = np.repeat(np.arange(n), np.diff(ls.Ap))
    isfree = np.zeros(n, bool); isfree[free] = True; iskept = np.zeros(m, bool); iskept[kept] = True
    pk = isfree[ls.Pi] & isfree[cols]; ak = iskept[ls.Ai] & isfree[colsA]
    newv = -np.ones(n, int); newv[free] = np.arange(len(free)); newr = -np.ones(m, int); newr[kept] = np.arange(len(kept))
    def csc(rows, cs, ncol):
        ptr = np.zeros(ncol + 1, np.int64); np.add.at(ptr, cs + 1, 1); return np.cumsum(ptr).astype(np.int32), rows.astype(np.int32)
    Ppr, Pir = csc(newv[ls.Pi[pk]], newv[cols[pk]], len(free)); Apr, Air = csc(newr[ls.Ai[ak]], newv[colsA[ak]], len(free))
    qr = ls.q[:, free].copy(); lr = ls.l[:, kept].copy(); ur = ls.u[:, kept].copy()
    for b in range(B):
        Pd, Ad = ls.dense(b)
        Pd = np.triu(Pd) + np.triu(Pd, 1).T                      # only entries with row <= col count
        qr[b] += Pd[np.ix_(free, fvars)] @ xfix[b]
        shift = Ad[np.ix_(kept, fvars)] @ xfix[b]
        lr[b] = np.where(lr[b] <= -1e30, lr[b], lr[b] - shift); ur[b] = np.where(ur[b] >= 1e30, ur[b], ur[b] - shift)
    red = models.LocalSystem(len(free), len(kept), Ppr, Pir, Apr, Air, np.ascontiguousarray(Pv[:, pk]), qr, np.ascontiguousarray(Av[:, ak]), lr, ur)
    return red, free, kept, fvars, xfix


def random_stage_ocp(seed, family="oc4"):
    """One random stage-OCP local system for the on-chip kernel families (the generator of tools/fuzz_oc.py): random state / input sizes, horizon,
    weights, nonlinear dynamics and iterate -- block tridiagonal + arrow patterns with single and twisted chains, phantom slots, hubs that share
    their block with the last frame.  family "oc8": horizons drawn so that the chain part is 21 ... 56 blocks of 16 variables.  Returns
    (ls, dims string, rng); the problem the reference would hand to CuCaQP::setSystem at that iterate (src/sqp_solver/SQPOptimizationSolver.cpp:100-120)."""
    from optimal_control_problem_amd import models
    rng = np.random.default_rng(5000 + seed)
    nx = int(rng.integers(2, 13)); nu = int(rng.integers(1, 5)); N = int(rng.integers(4, 26)); B = int(rng.integers(1, 6))
    if family == "oc8":
        N = int(rng.integers((21 * 16) // (nx + nu) + 1, (56 * 16) // (nx + nu) + 1)); B = int(rng.integers(1, 4))
    Am = np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)); Bm = 0.3 * rng.normal(size=(nx, nu)); w = rng.normal(size=nx)

    class M(models.StageOCP):
        name = "fuzz"

        def F(self, s, u):
            return s @ Am.T + u @ Bm.T + 0.05 * np.sin(s * w)

        def frame_bounds(self):
            return np.concatenate([np.full(nx, -5.0), np.full(nu, -1.0)]), np.concatenate([np.full(nx, 5.0), np.full(nu, 1.0)])
    M.nx, M.nu = nx, nu
    mdl = M(N, 0.05, rng.uniform(0.1, 10.0, nx), rng.uniform(0.01, 1.0, nu))
    x = rng.normal(0, 0.3, (B, mdl.nvar)); p = rng.normal(0, 0.2, (B, nx))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(x[:, :mdl.f].copy())
    ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
    return ls, "nx=%d nu=%d N=%d B=%d n=%d m=%d" % (nx, nu, N, B, ls.n, ls.m), rng


def selection_grid():
    """tests/golden/selection_grid.json: what the library reported per row before select_kernel existed (tools/selection_grid.py)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "selection_grid.json")) as f:
        return json.load(f)


def selection_row_id(r):
    return "%s-N%d-x%d%s%s" % (r["workload"], r["N"], r["batch"], "-reduced" if r["reduced"] else "", "".join("-%s=%s" % kv for kv in sorted(r["env"].items())))


def selection_pattern(row, inner=False, _cache={}):
    """(n, m, Pp, Pi, Ap, Ai, fixed_rows or None) of a row of tests/golden/selection_grid.json (tools/selection_grid.py): a workload's
    pattern; for a reduced row the parameter rows the reduced form eliminates, or (inner) the reduced pattern its inner handle is created on"""
    from optimal_control_problem_amd import models
    key = (row["workload"], row["N"])
    if key not in _cache:
        mdl, ls, _ = models.make_workload(row["workload"], 2, N=row["N"])
        _cache[key] = (ls, list(range(mdl.np)))
    ls, fixed = _cache[key]
    if row["reduced"] and inner:
        ls, fixed = reduce_qp(ls, fixed)[0], None
    return ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, (fixed if row["reduced"] else None)
