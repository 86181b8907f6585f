"""Dense NumPy statement of OSQP's solution polishing for one QP, in unscaled space with a plain Cholesky -- the reference the polish kernel
(optimal_control_problem_amd/csrc/kernel_polish.hpp) is tested against.  Written from the published algorithm (Stellato et al., "OSQP: an
operator splitting solver for quadratic programs", section 5.2, and the acceptance rule of OSQP's polish()); used by tests only.

    min 1/2 x'Px + q'x   s.t.  l <= Ax <= u,     (x, y, z) = an ADMM iterate with residuals (pri, dua)

1. active rows from the iterate: lower when z_i - l_i < -y_i, else upper when u_i - z_i < y_i; b_i = the bound hit
2. the regularised KKT system [P + delta I, A_a'; A_a, -delta I] in condensed form: M = P + delta I + A_a' A_a / delta
3. from (x, y_a) = 0, 1 + refine_iter times:  r_x = -(P x + q + A_a' y_a),  r_y = b_a - A_a x,  M dx = r_x + A_a' r_y / delta,
   y_a += (A_a dx - r_y) / delta,  x += dx      (iterative refinement against the unregularised matrix)
4. candidate: y = 0 off the active rows, z = clip(A x, l, u); accepted iff both residuals are smaller than the iterate's, or one is
   smaller while the other was already below 1e-10
"""
import numpy as np

LINSYS_ERROR, FAILED, NOT_PERFORMED, SUCCESS = -2, -1, 0, 1
SOLVED = 1


def dense_qp(ls, b=0):
    """(P, A, q, l, u) of instance b of a models.LocalSystem, P symmetric from its upper triangle (the entries the engine reads)"""
    pick = lambda a: a if a.ndim == 1 else a[b]
    P = np.zeros((ls.n, ls.n)); A = np.zeros((ls.m, ls.n))
    P[ls.Pi, np.repeat(np.arange(ls.n), np.diff(ls.Pp))] = pick(ls.P)
    A[ls.Ai, np.repeat(np.arange(ls.n), np.diff(ls.Ap))] = pick(ls.A)
    P = np.triu(P) + np.triu(P, 1).T
    return P, A, pick(ls.q), pick(ls.l), pick(ls.u)


def residuals(P, A, q, l, u, x, y):
    """max-norm primal and dual residual of (x, y) with z = clip(A x, l, u): what a caller recomputes on the host"""
    ax = A @ x
    z = np.minimum(np.maximum(ax, np.maximum(l, -1e30)), np.minimum(u, 1e30))
    pri = np.abs(ax - z).max() if len(ax) else 0.0
    dua = np.abs(P @ x + q + A.T @ y).max()
    return pri, dua


def polish_ref(P, A, q, l, u, x, y, z, pri, dua, delta=1e-6, refine_iter=3, status=SOLVED):
    """-> dict(status, accepted, x, y, z, pri, dua, obj, n_active): the candidate (also when it is rejected) and the decision"""
    n, m = P.shape[0], A.shape[0]
    out = dict(status=NOT_PERFORMED, accepted=False, x=None, y=None, z=None, pri=np.nan, dua=np.nan, obj=np.nan, n_active=0)
    if status != SOLVED:
        return out
    l = np.maximum(l, -1e30); u = np.minimum(u, 1e30)
    low = (z - l) < -y
    upp = ~low & ((u - z) < y)
    act = low | upp
    b = np.where(low, l, u)[act]
    Aa = A[act]
    out["n_active"] = int(act.sum())
    M = P + delta * np.eye(n) + Aa.T @ Aa / delta
    try:
        Lc = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        out["status"] = LINSYS_ERROR
        return out
    solve = lambda r: np.linalg.solve(Lc.T, np.linalg.solve(Lc, r))
    xp = np.zeros(n); ya = np.zeros(len(b))
    for _ in range(1 + refine_iter):
        rx = -(P @ xp + q + Aa.T @ ya)
        ry = b - Aa @ xp
        dx = solve(rx + Aa.T @ ry / delta)
        ya = ya + (Aa @ dx - ry) / delta
        xp = xp + dx
    yp = np.zeros(m); yp[act] = ya
    ax = A @ xp
    zp = np.minimum(np.maximum(ax, l), u)
    pri_pol = np.abs(ax - zp).max() if m else 0.0
    dua_pol = np.abs(P @ xp + q + A.T @ yp).max()
    ok = (pri_pol < pri and dua_pol < dua) or (pri_pol < pri and dua < 1e-10) or (dua_pol < dua and pri < 1e-10)
    ok = bool(ok and np.isfinite(xp).all())
    out.update(status=SUCCESS if ok else FAILED, accepted=ok, x=xp, y=yp, z=zp, pri=float(pri_pol), dua=float(dua_pol),
               obj=float(0.5 * xp @ P @ xp + q @ xp))
    return out
