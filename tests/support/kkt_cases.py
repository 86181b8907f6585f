"""Patterns, hand-built instances and the recipe shared by tests/test_kkt_host.py (CPU) and tests/test_gpu_kkt.py -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

from optimal_control_problem_amd import models

INF = float("inf")
BIG = 1e30
TOL = 0.25                      # the tolerance of the hand-built instances (a power of two: tol * 1 and the values "exactly at" it are exact)


# ------------------------------------------------------------------------------------------------ hand-built instances, one per branch
# A small pattern with a parameter column: n = 3 (col0 = 1), m = 5: rows 0..2 the identity, row 3 = [0, 2, 1], row 4 = [5, 0, -1] (the entry in the
# parameter column must not reach stat).  CSC: column 0: rows 0, 4; column 1: rows 1, 3; column 2: rows 2, 3, 4.
HAND_N, HAND_M, HAND_COL0 = 3, 5, 1
HAND_AP = np.array([0, 2, 4, 7], np.int32)
HAND_AI = np.array([0, 4, 1, 3, 2, 3, 4], np.int32)
HAND_A = np.array([1.0, 5.0, 1.0, 2.0, 1.0, 1.0, -1.0])


def _inst(q=(0.0, 0.0, 0.0), l=None, u=None, y=None, A=None):
    l = np.array([0.0, -1.0, -1.0, -1.0, -1.0] if l is None else l, float)
    u = np.array([0.0, 1.0, 1.0, 1.0, 1.0] if u is None else u, float)
    return dict(q=np.array(q, float), A=HAND_A.copy() if A is None else np.array(A, float), l=l, u=u, y=np.zeros(HAND_M) if y is None else np.array(y, float))


def hand_instances():
    """[(name, instance dict, expected (stat, feas, compl, scale) or None for NaN, expected converged at TOL)]"""
    nan = float("nan")
    out = []
    # interior, no multipliers: all zero
    out.append(("interior", _inst(), (0.0, 0.0, 0.0, 0.0), True))
    # infinite and 1e30 bounds without multipliers: nothing
    out.append(("loose_bounds", _inst(l=[0.0, -INF, -BIG, -INF, -1.0], u=[0.0, INF, BIG, BIG, INF]), (0.0, 0.0, 0.0, 0.0), True))
    # an equality row (l = u = 0) with a large multiplier of either sign: complementarity 0; its A'y is balanced by q
    #   y_3 = 8: t_1 = 2 * 8 = 16, t_2 = 8; q = (0, -16, -8) -> stat 0, scale 16
    out.append(("equality_row", _inst(q=(0.0, -16.0, -8.0), l=[0.0, -1.0, -1.0, 0.0, -1.0], u=[0.0, 1.0, 1.0, 0.0, 1.0], y=[0, 0, 0, 8.0, 0]),
                (0.0, 0.0, 0.0, 16.0), True))
    # right-sign multiplier on an active upper bound (u_1 = 0, y_1 = 3 > 0): complementarity 0; stationarity balanced by q_1 = -3
    out.append(("active_upper_right_sign", _inst(q=(0.0, -3.0, 0.0), u=[0.0, 0.0, 1.0, 1.0, 1.0], y=[0, 3.0, 0, 0, 0]), (0.0, 0.0, 0.0, 3.0), True))
    # wrong-sign multiplier on that bound (y_1 = -3 pushes on the lower bound, 1 away): min(3, 1) = 1
    out.append(("active_upper_wrong_sign", _inst(q=(0.0, 3.0, 0.0), u=[0.0, 0.0, 1.0, 1.0, 1.0], y=[0, -3.0, 0, 0, 0]), (0.0, 0.0, 1.0, 3.0), False))
    # a multiplier on an infinite and on a 1e30 bound counts in full: y_2 = 0.5 against u_2 = inf, y_1 = -0.75 against l_1 = -1e30
    out.append(("multiplier_on_infinite_bound", _inst(q=(0.0, 0.75, -0.5), l=[0.0, -BIG, -1.0, -1.0, -1.0], u=[0.0, 1.0, INF, 1.0, 1.0], y=[0, -0.75, 0.5, 0, 0]),
                (0.0, 0.0, 0.75, 0.75), False))
    # infeasible: l_2 = 0.5 > 0 (row 2 below its lower bound), u_4 = -2 (row 4 above its upper bound)
    out.append(("infeasible", _inst(l=[0.0, -1.0, 0.5, -1.0, -3.0], u=[0.0, 1.0, 1.0, 1.0, -2.0]), (0.0, 2.0, 0.0, 0.0), False))
    # the parameter column takes no part: q_0 = 100, y_4 = 1 puts 5 into t_0 and -1 into t_2, balanced by q_2 = 1; y_4 > 0 sits on the active u_4 = 0: compl 0
    out.append(("parameter_column_skipped", _inst(q=(100.0, 0.0, 1.0), u=[0.0, 1.0, 1.0, 1.0, 0.0], y=[0, 0, 0, 0, 1.0]), (0.0, 0.0, 0.0, 1.0), True))
    # exactly at each tolerance: <= holds
    out.append(("stat_at_tol", _inst(q=(0.0, TOL, 0.0)), (TOL, 0.0, 0.0, TOL), True))
    out.append(("stat_at_scaled_tol", _inst(q=(0.0, -16.0 + 16.0 * TOL, -8.0), l=[0.0, -1.0, -1.0, 0.0, -1.0], u=[0.0, 1.0, 1.0, 0.0, 1.0], y=[0, 0, 0, 8.0, 0]),
                (16.0 * TOL, 0.0, 0.0, 16.0), True))
    out.append(("feas_at_tol", _inst(l=[0.0, TOL, -1.0, -1.0, -1.0]), (0.0, TOL, 0.0, 0.0), True))
    out.append(("compl_at_tol", _inst(q=(0.0, -TOL, 0.0), y=[0, TOL, 0, 0, 0]), (0.0, 0.0, TOL, TOL), True))
    # one ulp above each: not converged
    up = np.nextafter(TOL, 1.0)
    out.append(("stat_above_tol", _inst(q=(0.0, up, 0.0)), (up, 0.0, 0.0, up), False))
    out.append(("feas_above_tol", _inst(l=[0.0, up, -1.0, -1.0, -1.0]), (0.0, up, 0.0, 0.0), False))
    out.append(("compl_above_tol", _inst(q=(0.0, -up, 0.0), y=[0, up, 0, 0, 0]), (0.0, 0.0, up, up), False))
    # a NaN in each of the five arrays (in the parameter column too): everything NaN, not converged
    for name, kw in (("nan_q", dict(q=(0.0, nan, 0.0))), ("nan_q_parameter_column", dict(q=(nan, 0.0, 0.0))),
                     ("nan_A", dict(A=[1.0, 5.0, 1.0, nan, 1.0, 1.0, -1.0])), ("nan_A_parameter_column", dict(A=[1.0, nan, 1.0, 2.0, 1.0, 1.0, -1.0])),
                     ("nan_l", dict(l=[0.0, -1.0, nan, -1.0, -1.0])), ("nan_u", dict(u=[0.0, 1.0, 1.0, nan, 1.0])), ("nan_y", dict(y=[0, 0, 0, 0, nan])),
                     ("nan_y_all", dict(y=[nan] * 5))):
        out.append((name, _inst(**kw), None, False))
    return out


def stack(insts):
    """dict of batched arrays q, A, l, u, y from a list of instance dicts"""
    return {k: np.stack([i[k] for i in insts]) for k in ("q", "A", "l", "u", "y")}


# ------------------------------------------------------------------------------------------------ systems of the zoo
def zoo_model(name, N):
    return {"double_integrator": models.DoubleIntegrator, "quadrotor": models.Quadrotor, "cartpole": models.CartPole}[name](N)


def zoo_system(name, N, B, seed=0):
    """(model, LocalSystem at a random iterate with some rows outside their bounds, multipliers y [B, m] of mixed sign with zeros)"""
    mdl = zoo_model(name, N)
    rng = np.random.default_rng(100 * N + seed + len(name))
    X = rng.normal(0.0, 0.4, size=(B, mdl.N, mdl.f))
    if name == "quadrotor":
        X[:, :, mdl.nx:] += mdl.hover_thrust
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(X[:, 0].copy())
    p = rng.normal(0.0, 0.2, size=(B, mdl.np))
    ls = mdl.local_system(p, X.reshape(B, -1), lbx, ubx, lbg, ubg)
    y = rng.normal(0.0, 2.0, size=(B, mdl.m)) * (rng.random((B, mdl.m)) < 0.7)
    return mdl, ls, y


# ------------------------------------------------------------------------------------------------ the recipe
# Cart-pole N = 20 near the upright position, 8 instances whose start angles grow geometrically from 0.01 to 0.7 rad, full steps (alpha = 1) from
# x = 0.  The small angles are all but linear and meet the tolerance after a couple of QPs, the large ones need more: converged_at differs across
# the batch.  Every number is a closed form, so that the C++ program (tests/support/stagesqp_kkt_test.cpp) states the same recipe.
RECIPE_N, RECIPE_BATCH, RECIPE_MAX_ITER, RECIPE_ALPHA = 20, 8, 12, 1.0
RECIPE_TOL = 2e-3               # read off the logged history: see tests/test_kkt_host.py test_recipe_tolerance


def recipe_angles():
    a = [0.01]
    for _ in range(RECIPE_BATCH - 1):                  # (products, not powers: the C++ program forms the same doubles)
        a.append(a[-1] * 1.835)
    return np.array(a)


def recipe():
    mdl = models.CartPole(RECIPE_N, 0.02)
    B = RECIPE_BATCH
    frame0 = np.zeros((B, mdl.f))
    frame0[:, 1] = recipe_angles()
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    return mdl, dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)


def recipe_options(**extra):
    return dict({"max_iter": RECIPE_MAX_ITER, "alpha": RECIPE_ALPHA, "kkt_tol": RECIPE_TOL}, **extra)


# ------------------------------------------------------------------------------------------------ the branches on a handle's pattern
def branch_instances(Ap, Ai, n, m, col0, tol):
    """the branches of the hand-built instances on any pattern with at least two rows behind col0 (the kernel runs on a handle's pattern): a dict of
    batched arrays q, A, l, u, y and the expected verdicts at `tol` (a power of two).  Base: q = 0, A = 1 everywhere, l = -1, u = 1, y = 0.  i is an
    identity row of a non-parameter column, g the last row."""
    nan = float("nan")
    nnz = len(Ai)
    i, g, j = col0, m - 1, n - 1
    up = np.nextafter(tol, 1.0)
    edits = [
        ({}, True),                                                                              # interior
        ({"l": {i: -INF, g: -BIG}, "u": {i: INF, g: BIG}}, True),                                # loose bounds, no multipliers
        ({"l": {g: 0.0}, "u": {g: 0.0}, "y": {g: 8.0}}, None),                                   # an equality row with a multiplier (verdict: stat decides)
        ({"u": {i: 0.0}, "y": {i: 3.0}, "q": {i: -3.0}}, True),                                  # right sign on an active upper bound
        ({"u": {i: 0.0}, "y": {i: -3.0}, "q": {i: 3.0}}, False),                                 # wrong sign: min(3, 1) = 1
        ({"u": {i: INF}, "l": {g: -BIG}, "y": {i: 0.5, g: -0.75}}, False),                       # multipliers on an infinite and a 1e30 bound
        ({"l": {i: 0.5}, "u": {g: -2.0}}, False),                                                # infeasible rows
        ({"q": {j: tol}}, True), ({"q": {j: up}}, False),                                        # stat at / above the tolerance (scale < 1)
        ({"l": {i: tol}}, True), ({"l": {i: up}}, False),                                        # feas at / above
        ({"y": {i: tol}, "q": {i: -tol}}, True), ({"y": {i: up}, "q": {i: -up}}, False),         # compl at / above
        ({"q": {j: nan}}, False), ({"q": {0: nan}}, False), ({"A": {nnz - 1: nan}}, False), ({"A": {0: nan}}, False),
        ({"l": {g: nan}}, False), ({"u": {i: nan}}, False), ({"y": {g: nan}}, False), ({"y": {k: nan for k in range(m)}}, False),
    ]
    K = len(edits)
    d = dict(q=np.zeros((K, n)), A=np.ones((K, nnz)), l=-np.ones((K, m)), u=np.ones((K, m)), y=np.zeros((K, m)))
    for b, (e, _) in enumerate(edits):
        for key, items in e.items():
            for idx, v in items.items():
                d[key][b, idx] = v
    return d, [v for _, v in edits]


def rounding_bar(Ap, Ai, q, A, y, col0):
    """[B]: the rounding bar of stat and scale, 2 (k + 2) 2^-53 max_{j >= col0} (|q_j| + sum_k |A_kj y_k|), k = the longest column's entry count plus
    one (k + 1 rounded operations on terms of that total size, with a factor 2 to spare)"""
    Ap = np.asarray(Ap); Ai = np.asarray(Ai)
    tot = np.abs(np.asarray(q, float)).copy()
    for j in range(len(Ap) - 1):
        e = slice(Ap[j], Ap[j + 1])
        tot[:, j] += np.abs(A[:, e] * y[:, Ai[e]]).sum(axis=1)
    k = int(np.diff(Ap).max()) + 1
    return 2 * (k + 2) * 2.0 ** -53 * np.nanmax(tot[:, col0:], axis=1) * (1 + 2.0 ** -40)
