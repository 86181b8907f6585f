"""First-order optimality residuals of the NLP per instance: the NumPy statement of mpcqp_stage_kkt / mpcqp_nlp_kkt (include/mpcqp.h).

The reference's loop has no convergence test (src/sqp_solver/SQPOptimizationSolver.cpp:127-216).  For one instance, with the local system
(q [n], A [m x n, CSC], l [m], u [m]) evaluated at w = [p; x], rows [p; x; g], and multipliers y [m] in the solver's sign convention
(P x + q + A'y = 0, y_i > 0 on an active upper bound), and col0 = np -- the parameter columns are skipped, their pinned rows absorb any value:

    t_j    = sum_k A_kj y_k           the entries of column j added in storage order, every product and every sum rounded
    stat   = max_{j >= col0} |q_j + t_j|                  scale = max_{j >= col0} max(|q_j|, |t_j|)
    feas   = max_i max(l_i, -u_i, 0)                      the distance of 0 from [l_i, u_i]
    compl  = max_i max( min(max(y_i, 0), max(u_i, 0)), min(max(-y_i, 0), max(-l_i, 0)) )
    converged = stat <= tol_stat max(1, scale)  and  feas <= tol_feas  and  compl <= tol_compl

A NaN anywhere in the instance's q, A, l, u, y (parameter columns included) or in a q_j + t_j makes all four NaN and converged False."""
import ctypes as C

import numpy as np

RES = ("stat", "feas", "compl", "scale")      # the columns of res


def kkt_tolerances(value):
    """options["kkt_tol"]: a number = all three tolerances; a dict {stat, feas, compl}; or the triple this function returns.  Off (returns None):
    None, False, and all three tolerances zero in any of the forms, as StageSQP::setKktTolerance(0, 0, 0) switches the check off.  True is
    refused: it is no tolerance.  Returns (tol_stat, tol_feas, tol_compl)."""
    if value is None or value is False:
        return None
    if value is True:
        raise ValueError("kkt_tol: expected a number or a dict with the keys stat, feas, compl, not True")
    if isinstance(value, dict):
        if set(value) != set(RES[:3]):
            raise ValueError("kkt_tol: expected a number or a dict with the keys stat, feas, compl (got %s)" % sorted(value))
        tol = tuple(value[k] for k in RES[:3])
    elif isinstance(value, (tuple, list)):
        if len(value) != 3:
            raise ValueError("kkt_tol: a sequence must hold the three tolerances stat, feas, compl")
        tol = tuple(value)
    else:
        tol = (value,) * 3
    if any(isinstance(t, bool) for t in tol):
        raise ValueError("kkt_tol: a tolerance is a number, not a bool")
    tol = tuple(float(t) for t in tol)
    if not all(t >= 0.0 for t in tol):
        raise ValueError("kkt_tol: the tolerances must not be negative or NaN")
    return None if tol == (0.0, 0.0, 0.0) else tol


def kkt_residuals(Ap, Ai, q, A, l, u, y, col0, tol=1e-3):
    """(res [B, 4] = stat, feas, compl, scale; converged [B] bool) for a batch of instances on one pattern.  tol: what kkt_tolerances takes."""
    Ap = np.asarray(Ap); Ai = np.asarray(Ai)
    q = np.atleast_2d(np.asarray(q, float)); A = np.atleast_2d(np.asarray(A, float))
    l = np.atleast_2d(np.asarray(l, float)); u = np.atleast_2d(np.asarray(u, float)); y = np.atleast_2d(np.asarray(y, float))
    B, n = q.shape
    tol = kkt_tolerances(tol) or (0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        t = np.zeros((B, n))
        length = np.diff(Ap)
        for r in range(int(length.max(initial=0))):       # entry r of every column that has one: storage order inside a column
            cols = np.nonzero(length > r)[0]
            e = Ap[cols] + r
            t[:, cols] = t[:, cols] + A[:, e] * y[:, Ai[e]]
        rr = q + t
        bad = np.isnan(q).any(axis=1) | np.isnan(A).any(axis=1) | np.isnan(l).any(axis=1) | np.isnan(u).any(axis=1) | np.isnan(y).any(axis=1) | \
            np.isnan(rr).any(axis=1)
        stat = np.fmax.reduce(np.abs(rr[:, col0:]), axis=1, initial=0.0)
        scale = np.fmax.reduce(np.fmax(np.abs(q[:, col0:]), np.abs(t[:, col0:])), axis=1, initial=0.0)
        feas = np.fmax.reduce(np.fmax(np.fmax(l, -u), 0.0), axis=1, initial=0.0) + 0.0
        cm = np.fmax(np.fmin(np.fmax(y, 0.0), np.fmax(u, 0.0)), np.fmin(np.fmax(-y, 0.0), np.fmax(-l, 0.0)))
        cmpl = np.fmax.reduce(cm, axis=1, initial=0.0) + 0.0
        conv = ~bad & (stat <= tol[0] * np.fmax(1.0, scale)) & (feas <= tol[1]) & (cmpl <= tol[2])
        res = np.stack([stat, feas, cmpl, scale], axis=1)
        res[bad] = np.nan
    return res, conv


class KktArgs(C.Structure):
    """mpcqp_kkt_args (include/mpcqp.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("q", "A", "l", "u", "y", "res", "converged", "frozen")] + \
               [(k, C.c_double) for k in ("tol_stat", "tol_feas", "tol_compl")]


def device_kkt(entry, ev, ls, y, tol=1e-3, out=None, frozen=None, stream=None):
    """what StageEvaluator.kkt and GeneralEvaluator.kkt share: one launch of `entry` (mpcqp_stage_kkt / mpcqp_nlp_kkt) on the evaluator's handle.
    ls: the dict eval wrote (q, A, l, u); y [B, m]; out: (res [B, 4] float64, converged [B] int32) to write into; frozen [B] int32, optional: an
    instance with a nonzero entry is neither read nor written.  Contiguous CUDA tensors.  Returns (res, converged)."""
    import torch
    from . import _lib
    from .stage_eval import _check, _check_int32
    B = y.shape[0]
    tol = kkt_tolerances(tol) or (0.0, 0.0, 0.0)
    if out is None:
        out = (torch.empty((B, 4), dtype=torch.float64, device=y.device), torch.empty(B, dtype=torch.int32, device=y.device))
    res, conv = out
    a = KktArgs()
    a.q, a.A, a.l, a.u = _check(ls["q"], (B, ev.n), "q"), _check(ls["A"], (B, ev.nnzA), "A"), _check(ls["l"], (B, ev.m), "l"), _check(ls["u"], (B, ev.m), "u")
    a.y, a.res, a.converged = _check(y, (B, ev.m), "y"), _check(res, (B, 4), "res"), _check_int32(conv, B, "converged")
    if frozen is not None:
        a.frozen = _check_int32(frozen, B, "frozen")
    a.tol_stat, a.tol_feas, a.tol_compl = tol
    _lib.check(entry(ev._h, B, C.byref(a), stream))
    return res, conv
