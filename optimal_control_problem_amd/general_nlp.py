"""General (slow) local-system evaluation for NLPs that are not stage-structured: what the reference does for ANY problem.

The reference accepts arbitrary CasADi SX expressions over the whole decision vector as cost terms and constraints
(reference src/OptimalControlProblem.cpp:444-497,574-600), assembles {x, f, g, p} (:235-240) and lets CasADi differentiate:
exact Hessian of f and Jacobian of [p; x; g] with their true sparsity (src/sqp_solver/SQPOptimizationSolver.cpp:47-77).  The fast
path of this build compiles the stage pattern (models.StageOCP, device-resident evaluation); everything else lands here:

* the cost f(p, x) and the constraints g(p, x), given as NumPy callables on 1-D arrays, are traced once into SSA tapes with the
  tracer of codegen.py (the same one that records user dynamics);
* the gradient is derived on the tape (reverse sweep), the Hessian's structure is read off a forward sweep over the gradient tape
  (identically-zero entries fold away), the Jacobian's structure off the dependency sets of g's outputs: the QP carries the exact
  sparsity, like CasADi's;
* per SQP iteration the values come from the tapes evaluated in NumPy over the whole batch at once -- gradient directly, Hessian and
  Jacobian columns by complex-step differentiation (exact to rounding for the analytic operations the tracer knows).

Cost: O(n) tape evaluations per iteration on the host.  The QPs are solved on the GPU by the generic path of the engine
(mpcqp_create takes any sparsity pattern).  The object has the interface SQPOptimizationSolver expects of a model (n, m, np,
local_system, objective), formulated exactly like the reference: w = [p; x], rows [p; x; g], shifted bounds.
"""
import numpy as np

from . import codegen
from .models import LocalSystem, _csc_from_dense_mask


def _flat(v):
    """tracer scalars / constants of whatever a traced callable returned: a vector tracer, a scalar tracer, numbers, or nested sequences of those"""
    if isinstance(v, codegen.TV):
        return list(v.items)
    if isinstance(v, codegen.TS):
        return [v]
    if isinstance(v, (list, tuple)):
        return [t for e in v for t in _flat(e)]
    return [float(a) for a in np.atleast_1d(np.asarray(v, float)).ravel()]


def _trace(fn, n_in, what):
    """tape of fn(w) over a traced vector w of n_in scalars; fn returns a vector tracer, a scalar tracer or a (nested) sequence of them"""
    tape = codegen.Tape(n_in)
    w = codegen.TV(tape, [codegen.TS(tape, k) for k in range(n_in)])
    tape.outputs = [v.idx if isinstance(v, codegen.TS) else tape.const(v) for v in _flat(fn(w))]
    if not tape.outputs and what == "cost":
        raise ValueError("the cost function returned nothing")
    return tape


def _contracted_gradient(constraints, n, ng):
    """gradient over w of the scalar lam' g(w): a tape with inputs [w (n); lam (ng)] and n outputs.  The multipliers carry no derivative
    (plain_from = n): the generated body takes them as plain values"""
    tape = codegen.Tape(n + ng)
    w = codegen.TV(tape, [codegen.TS(tape, k) for k in range(n)])
    out = [v.idx if isinstance(v, codegen.TS) else tape.const(v) for v in _flat(constraints(w))]
    if len(out) != ng:
        raise ValueError("the constraints returned %d values, then %d" % (ng, len(out)))
    acc = tape.const(0.0)
    for i, o in enumerate(out):
        acc = tape.s_add(acc, tape.s_mul(n + i, o))
    tape.outputs = [acc]
    g = codegen.gradient_tape(tape)
    g.outputs = g.outputs[:n]
    g.plain_from = n
    return g


def _depends(tape):
    """[n_out, n_in] structural dependency of every output on every input (reachability on the tape)"""
    n = tape.n_in
    dep = [None] * len(tape.nodes)
    for i, nd in enumerate(tape.nodes):
        k = nd[0]
        if k == "in":
            s = np.zeros(n, bool); s[nd[1]] = True
        elif k == "const":
            s = np.zeros(n, bool)
        elif len(nd) == 2:
            s = dep[nd[1]]
        else:
            s = dep[nd[1]] | dep[nd[2]]
        dep[i] = s
    return np.array([dep[o] for o in tape.outputs]).reshape(len(tape.outputs), n)


class GeneralNLP:
    """min f(p, x)  s.t.  lbx <= x <= ubx, lbg <= g(p, x) <= ubg, with f and g arbitrary traced NumPy callables of w = [p; x]."""

    name = "general_nlp"

    def __init__(self, nvar, npar, cost, constraints=None, exact_hessian=False):
        """exact_hessian (opt-in): the structure of the constraints' curvature joins the pattern of P, so that lagrangian_system /
        mpcqp_nlp_lagrangian can add it; without the flag the pattern, the generated text and every attribute are what they were"""
        self.nvar, self.np = int(nvar), int(npar)
        self.n = self.np + self.nvar
        self._ftape = _trace(lambda w: cost(w), self.n, "cost")
        if len(self._ftape.outputs) != 1:
            raise ValueError("the cost must be a scalar")
        self._gtape = codegen.gradient_tape(self._ftape)
        self.hm = codegen.hessian_mask(self._gtape)
        self._ctape = _trace(lambda w: constraints(w), self.n, "constraints") if constraints is not None else None
        self.ng = len(self._ctape.outputs) if self._ctape is not None else 0
        self.m = self.n + self.ng
        jm = _depends(self._ctape) if self.ng else np.zeros((0, self.n), bool)
        self.am = np.vstack([np.eye(self.n, dtype=bool), jm])
        if exact_hessian:
            # the gradient over w of the contracted scalar sum_i lam_i g_i(w), the ng multipliers being extra tape inputs without a derivative
            # (codegen._contracted_gradient does this per frame on the stage path); cm: the structure of its Hessian, valid for any multipliers,
            # plus the diagonal entry of every column that has curvature -- the slot the DOMINANT safeguard writes its shift to
            self.exact_hessian = True
            self._cgtape = _contracted_gradient(constraints, self.n, self.ng) if self.ng else None
            cm = codegen.hessian_mask(self._cgtape) if self.ng else np.zeros((self.n, self.n), bool)
            cols = cm.any(axis=0)
            cm[cols, cols] = True
            self.cm = cm
            self._ccols = np.nonzero(cols)[0]
            self.hm = self.hm | cm
        self.Pp, self.Pi = _csc_from_dense_mask(self.hm)
        self.Ap, self.Ai = _csc_from_dense_mask(self.am)
        # columns that carry any derivative at all: the others are never perturbed
        self._hcols = np.nonzero(self.hm.any(axis=0))[0]
        self._jcols = np.nonzero(jm.any(axis=0))[0]

    # -- evaluation, vectorised over the batch: inputs[k] is an array [B]
    @staticmethod
    def _inputs(w):
        return [w[:, k] for k in range(w.shape[1])]

    def objective(self, p, x):
        w = np.concatenate([np.asarray(p, float), np.asarray(x, float)], axis=1)
        (f,) = self._ftape.evaluate(self._inputs(w))
        return np.broadcast_to(np.asarray(f, float), (w.shape[0],)).copy()

    def constraints(self, p, x):
        w = np.concatenate([np.asarray(p, float), np.asarray(x, float)], axis=1)
        return self._eval_vec(self._ctape, w) if self.ng else np.zeros((w.shape[0], 0))

    @staticmethod
    def _eval_vec(tape, w):
        out = tape.evaluate(GeneralNLP._inputs(w))
        return np.stack([np.broadcast_to(np.asarray(o), (w.shape[0],)) for o in out], axis=1)

    def derivatives(self, w):
        """gradient [B, n], Hessian [B, n, n], g [B, ng], Jacobian [B, ng, n] at w [B, n] (complex-step columns)"""
        B = w.shape[0]; h = 1e-30
        grad = self._eval_vec(self._gtape, w).real.astype(float)
        H = np.zeros((B, self.n, self.n)); J = np.zeros((B, self.ng, self.n))
        wc = w.astype(complex)
        for k in self._hcols:
            wc[:, k] += 1j * h
            H[:, :, k] = self._eval_vec(self._gtape, wc).imag / h
            wc[:, k] = w[:, k]
        gv = np.zeros((B, 0))
        if self.ng:
            gv = self._eval_vec(self._ctape, w).real.astype(float)
            for k in self._jcols:
                wc[:, k] += 1j * h
                J[:, :, k] = self._eval_vec(self._ctape, wc).imag / h
                wc[:, k] = w[:, k]
        H = 0.5 * (H + H.transpose(0, 2, 1))
        return grad, H, gv, J

    # -- the exact Hessian of the Lagrangian (include/mpcqp.h, mpcqp_nlp_lagrangian; csrc/general_kernels.hpp general_curvature_kernel) -------------
    DOMINANT = 1                           # MPCQP_NLP_DOMINANT

    def _need_exact(self):
        if not getattr(self, "exact_hessian", False):
            raise ValueError("this GeneralNLP was built without exact_hessian=True: the curvature's structure is not part of its pattern")

    def constraint_curvature(self, p, x, y):
        """C [B, n, n] = sum_i y[:, n + i] d2 g_i / dw2 at w = [p; x] (complex-step columns of the contracted gradient, symmetrised as
        `derivatives` does); y [B, m] are multipliers of the rows [p; x; g]"""
        self._need_exact()
        x = np.asarray(x, float)
        B = x.shape[0]
        C = np.zeros((B, self.n, self.n))
        if not len(self._ccols):
            return C
        h = 1e-30
        w = np.concatenate([np.broadcast_to(np.asarray(p, float).reshape(-1, self.np) if self.np else np.zeros((1, 0)), (B, self.np)), x], axis=1)
        wl = np.concatenate([w, np.asarray(y, float)[:, self.n:]], axis=1).astype(complex)
        for k in self._ccols:
            wl[:, k] += 1j * h
            C[:, :, k] = self._eval_vec(self._cgtape, wl).imag / h
            wl[:, k] = w[:, k]
        return 0.5 * (C + C.transpose(0, 2, 1))

    def lagrangian_system(self, p, x, y, P, status=None, mode=0):
        """NumPy statement of mpcqp_nlp_lagrangian: (P', shift [B, n]) from P [B, nnzP] as local_system returned it at the same (p, x).
        mode 0: P' = P + C on the curvature's slots.  mode DOMINANT: with R_c = sum_{r != c} |C_rc| and d_c = max(0, R_c - C_cc), the diagonal
        slot of column c takes (P + C) + d_c -- C + diag(d) is diagonally dominant with a non-negative diagonal, hence positive semidefinite, so
        P' is at least the cost's Hessian whatever the multipliers are.  A slot whose addend is zero keeps its bits.  An instance whose status
        is not in STATUS_OK keeps every bit of P and gets shift = 0 (its y may be NaN)."""
        self._need_exact()
        if mode not in (0, self.DOMINANT):
            raise ValueError("mode must be 0 or GeneralNLP.DOMINANT")
        P = np.array(P, float)
        B = P.shape[0]
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), self.STATUS_OK)
        shift = np.zeros((B, self.n))
        if not len(self._ccols):
            return P, shift
        with np.errstate(all="ignore"):
            C = self.constraint_curvature(p, x, np.where(ok[:, None], np.asarray(y, float), 0.0))
            Cv = C.transpose(0, 2, 1)[:, self.hm.T]
            new = np.where(Cv != 0.0, P + Cv, P)
            if mode == self.DOMINANT:
                dg = np.arange(self.n)
                R = np.abs(C).sum(axis=1) - np.abs(C[:, dg, dg])
                d = np.fmax(0.0, R - C[:, dg, dg])
                d[:, ~self.cm.any(axis=0)] = 0.0
                cols = np.repeat(np.arange(self.n), np.diff(self.Pp))
                isdiag = np.asarray(self.Pi) == cols
                dv = np.zeros_like(new); dv[:, isdiag] = d[:, cols[isdiag]]
                new = np.where(dv > 0.0, new + dv, new)
                shift = np.where(ok[:, None], d, 0.0)
        return np.where(ok[:, None], new, P), shift

    # -- the per-instance merit line search (include/mpcqp.h, mpcqp_nlp_linesearch; csrc/general_kernels.hpp general_linesearch_kernel) ------
    STATUS_OK = (1, 2, 7)                  # MPCQP_SOLVED, _SOLVED_INACCURATE, _MAX_ITER_REACHED: the QP returned a point
    line_search_takes_row_bounds = True    # the SQP loops hand lbg / ubg to line_search (a stage OCP carries its row bounds itself)

    def violation(self, p, x, lbx, ubx, lbg, ubg):
        """(v [B], gmax [B]): the l1 violation measure of the line search -- general rows outside lbg / ubg, entries of x outside lbx / ubx; an
        infinite bound contributes 0 -- and the max-norm violation mpcqp_nlp_merit returns (general rows only, floor 0)"""
        with np.errstate(all="ignore"):
            x = np.asarray(x, float)
            B = x.shape[0]
            g = self.constraints(np.broadcast_to(np.asarray(p, float), (B, self.np)), x)
            lbg = np.broadcast_to(np.asarray(lbg, float).reshape(-1, self.ng) if self.ng else np.zeros((1, 0)), (B, self.ng))
            ubg = np.broadcast_to(np.asarray(ubg, float).reshape(-1, self.ng) if self.ng else np.zeros((1, 0)), (B, self.ng))
            v = (np.fmax(lbg - g, 0.0) + np.fmax(g - ubg, 0.0)).sum(axis=1)
            gmax = np.fmax.reduce(np.fmax(lbg - g, g - ubg), axis=1, initial=0.0)
            v = v + (np.fmax(lbx - x, 0.0) + np.fmax(x - ubx, 0.0)).sum(axis=1)
        return v, gmax

    def line_search(self, p, x, lbx, ubx, q, dw, y, status=None, mu=None, alpha0=1.0, candidates=4, beta=0.5, c1=1e-4, mu_min=1.0, mu_factor=1.1,
                    lbg=None, ubg=None):
        """Host statement of mpcqp_nlp_linesearch: models.StageOCP.line_search word for word, with this class's violation(p, x, lbx, ubx, lbg, ubg)
        and objective(p, x).  x [B, nvar] (float64 array) and, when given, mu [B] are updated in place.  phi(x) = f + mu_b v(x) with
        mu_b = max(mu[b], mu_min, mu_factor max_{i >= np} |y_i|); D = min(0, q[np:]' dw[np:] - mu_b v(x)); the first alpha_j = alpha0 beta^j,
        j < candidates, whose phi(x + alpha_j dx) is finite and <= phi(x) + c1 alpha_j D is taken (accepted = j).  None: alpha_{K-1} when its
        merit is finite (accepted = -1), else alpha = 0 (accepted = -2).  An instance whose status is not in STATUS_OK keeps x, gets alpha = 0,
        accepted = -2, and its mu stays.  lbg, ubg [B, ng]: required when the problem has general rows.  Returns the same dict."""
        K = int(candidates)
        if not 1 <= K <= 8:
            raise ValueError("candidates must be in 1..8")
        if not 0.0 < beta < 1.0:
            raise ValueError("beta must lie in (0, 1)")
        if not (alpha0 > 0.0 and np.isfinite(alpha0)):
            raise ValueError("alpha0 must be positive")
        if not 0.0 <= c1 < 1.0:
            raise ValueError("c1 must lie in [0, 1)")
        if not (0.0 <= mu_min < np.inf and 0.0 <= mu_factor < np.inf):
            raise ValueError("mu_min and mu_factor must be finite and not negative")
        if self.ng and (lbg is None or ubg is None):
            raise ValueError("line_search needs the constraint bounds lbg and ubg of a problem with general rows")
        B, npp = x.shape[0], self.np
        p = np.broadcast_to(np.asarray(p, float).reshape(-1, npp) if npp else np.zeros((1, 0)), (B, npp))
        lbx = np.asarray(lbx, float); ubx = np.asarray(ubx, float)
        lbg = np.zeros((B, 0)) if not self.ng else np.asarray(lbg, float)
        ubg = np.zeros((B, 0)) if not self.ng else np.asarray(ubg, float)
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), self.STATUS_OK)
        alphas = np.empty(K)
        alphas[0] = alpha0
        for j in range(1, K):
            alphas[j] = alphas[j - 1] * beta
        with np.errstate(all="ignore"):
            dx = np.where(ok[:, None], np.asarray(dw, float)[:, npp:], 0.0)
            mub = np.full(B, float(mu_min)) if mu is None else np.fmax(mu_min, np.asarray(mu, float))
            ymax = np.fmax.reduce(np.abs(np.where(ok[:, None], np.asarray(y, float)[:, npp:], 0.0)), axis=1, initial=0.0)
            mub = np.where(ok, np.fmax(mub, mu_factor * ymax), mub)
            cost = np.full((B, K + 1), np.nan); vio = np.full((B, K + 1), np.nan); gmx = np.full((B, K + 1), np.nan)
            for j in range(K + 1):
                xc = x if j == 0 else x + alphas[j - 1] * dx
                cost[:, j] = self.objective(p, xc)
                vio[:, j], gmx[:, j] = self.violation(p, xc, lbx, ubx, lbg, ubg)
            phis = cost + mub[:, None] * vio
            D = (np.asarray(q, float)[:, npp:] * dx).sum(axis=1) - mub * vio[:, 0]
            D = np.where(D < 0.0, D, 0.0)
            sel = np.zeros(B, np.int64); acc = np.full(B, -2, np.int64)
            found = ~ok
            for j in range(1, K + 1):
                take = ~found & np.isfinite(phis[:, j]) & (phis[:, j] <= phis[:, 0] + c1 * alphas[j - 1] * D)
                sel[take] = j; acc[take] = j - 1
                found = found | take
            last = ~found & np.isfinite(phis[:, K])
            sel[last] = K; acc[last] = -1
            alpha = np.where(sel > 0, alphas[np.maximum(sel, 1) - 1], 0.0)
            step = alpha[:, None] * dx
            moved = sel > 0
            x[moved] = x[moved] + step[moved]
            phis[~ok, 1:] = np.nan
        if mu is not None:
            mu[ok] = mub[ok]
        rows = np.arange(B)
        return {"x": x, "alpha": alpha, "accepted": acc, "step_max": np.where(moved, np.abs(step).max(axis=1), 0.0), "f": cost[rows, sel],
                "gmax": gmx[rows, sel], "phi": np.stack([phis[:, 0], phis[rows, sel]], axis=1), "mu": mub, "D": D, "alphas": alphas, "phis": phis}

    # -- the optimality residuals (include/mpcqp.h, mpcqp_nlp_kkt; csrc/kkt_kernels.hpp) ---------------------------------------------------
    def kkt_residuals(self, ls, y, tol=1e-3):
        """Host statement of mpcqp_nlp_kkt: (res [B, 4] = stat, feas, compl, scale; converged [B]) of the local system `ls` (what local_system
        returned at the iterate) under the multipliers y [B, m]; kkt.kkt_residuals states the measure"""
        from .kkt import kkt_residuals
        return kkt_residuals(self.Ap, self.Ai, ls.q, ls.A, ls.l, ls.u, y, self.np, tol)

    def local_system(self, p, x, lbx, ubx, lbg, ubg):
        """reference SQPOptimizationSolver.cpp:47-77,100-120: P = Hessian of f wrt w, q = gradient, A = [I; dg/dw], bounds shifted by the
        current [p; x; g]"""
        p = np.asarray(p, float); x = np.asarray(x, float)
        B = x.shape[0]
        w = np.concatenate([np.broadcast_to(p, (B, self.np)), x], axis=1)
        grad, H, gv, J = self.derivatives(w)
        Afull = np.concatenate([np.broadcast_to(np.eye(self.n), (B, self.n, self.n)), J], axis=1)
        P = H.transpose(0, 2, 1)[:, self.hm.T]          # column-major order of the masked entries
        A = Afull.transpose(0, 2, 1)[:, self.am.T]
        c = np.concatenate([w, gv], axis=1)
        lo = np.concatenate([w[:, :self.np], np.broadcast_to(lbx, (B, self.nvar)), np.broadcast_to(lbg, (B, self.ng))], axis=1) - c
        hi = np.concatenate([w[:, :self.np], np.broadcast_to(ubx, (B, self.nvar)), np.broadcast_to(ubg, (B, self.ng))], axis=1) - c
        return LocalSystem(self.n, self.m, self.Pp, self.Pi, self.Ap, self.Ai, P, grad, A, lo, hi, self.np)
