"""Model zoo + batched local-system (QP) builder in the reference's formulation.

The reference builds one CasADi function (p, x, l, u) -> (H, grad, J, l - c, u - c) with augmented
variables w = [p; x] and augmented rows c = [p; x; g(p, x)]
(reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77) and evaluates it at the current SQP iterate
with l = [p; lbx; lbg], u = [p; ubx; ubg] (SQPOptimizationSolver.cpp:100-120).  CasADi is not available
here, so every model below carries hand-derived (or complex-step) derivatives and a fixed structural
sparsity, batched over instances with NumPy.  Outputs are exactly what CuCaQP::setSystem receives
(reference src/sqp_solver/CuCaQP.cpp:271-288): P (both triangles, CSC), q, A (CSC), l, u.

Variable layout of stage problems follows OCPConfig: X is horizon x frameSize, stage-interleaved
(reference src/OCP_config/OCPConfig.cpp:29-46,102); the whole first frame is pinned through lbx/ubx
(reference src/OptimalControlProblem.cpp:93-96).
"""
import numpy as np

INF = float("inf")


class LocalSystem:
    """Batch of QPs sharing one sparsity: P [B,nnzP] (both triangles), q [B,n], A [B,nnzA], l,u [B,m]."""

    def __init__(self, n, m, Pp, Pi, Ap, Ai, P, q, A, l, u, np_=0):
        self.n, self.m, self.np = n, m, np_
        self.Pp, self.Pi, self.Ap, self.Ai = Pp, Pi, Ap, Ai
        self.P, self.q, self.A, self.l, self.u = P, q, A, l, u

    @property
    def batch(self):
        return self.q.shape[0]

    def dense(self, b=0):
        """Dense (P, A) of instance b, for small tests."""
        P = np.zeros((self.n, self.n)); A = np.zeros((self.m, self.n))
        Pv = self.P if self.P.ndim == 1 else self.P[b]
        Av = self.A if self.A.ndim == 1 else self.A[b]
        for j in range(self.n):
            for k in range(self.Pp[j], self.Pp[j + 1]):
                P[self.Pi[k], j] = Pv[k]
            for k in range(self.Ap[j], self.Ap[j + 1]):
                A[self.Ai[k], j] = Av[k]
        return P, A


def _csc_from_dense_mask(mask):
    """CSC (colptr, rowidx) of a boolean structure matrix."""
    rows, cols = mask.shape
    p = [0]; idx = []
    for j in range(cols):
        r = np.nonzero(mask[:, j])[0]
        idx.extend(r.tolist()); p.append(len(idx))
    return np.asarray(p, dtype=np.int32), np.asarray(idx, dtype=np.int32)


class DenseNLP:
    """Small NLP given by callables; structure is taken dense-by-mask.  Used for the reference's
    test/test.cpp cases (test/test.cpp:13-211).  f, grad, hess, g, jac act on w = [p; x] (1-D)."""

    def __init__(self, nx, np_, f, grad, hess, g, jac, hess_mask=None, jac_mask=None, name=""):
        self.nx, self.np, self.name = nx, np_, name
        self.n = nx + np_
        self.f, self.grad, self.hess, self.g, self.jac = f, grad, hess, g, jac
        w0 = np.zeros(self.n)
        self.ng = len(np.atleast_1d(g(w0))) if g is not None else 0
        self.m = self.n + self.ng
        hm = np.ones((self.n, self.n), bool) if hess_mask is None else hess_mask
        jm = np.ones((self.ng, self.n), bool) if jac_mask is None else jac_mask
        am = np.vstack([np.eye(self.n, dtype=bool), jm])
        self.hm, self.am = hm, am
        self.Pp, self.Pi = _csc_from_dense_mask(hm)
        self.Ap, self.Ai = _csc_from_dense_mask(am)

    def objective(self, p, x):
        return np.array([self.f(np.concatenate([p[b], x[b]])) for b in range(x.shape[0])])

    def local_system(self, p, x, lbx, ubx, lbg, ubg):
        B = x.shape[0]
        P = np.zeros((B, len(self.Pi))); A = np.zeros((B, len(self.Ai)))
        q = np.zeros((B, self.n)); l = np.zeros((B, self.m)); u = np.zeros((B, self.m))
        for b in range(B):
            w = np.concatenate([p[b], x[b]])
            H = np.atleast_2d(self.hess(w)); J = np.zeros((self.ng, self.n))
            gv = np.zeros(0)
            if self.ng:
                J = np.atleast_2d(self.jac(w)); gv = np.atleast_1d(self.g(w))
            Afull = np.vstack([np.eye(self.n), J])
            P[b] = H.T[self.hm.T]       # column-major order of masked entries
            A[b] = Afull.T[self.am.T]
            q[b] = self.grad(w)
            c = np.concatenate([w, gv])
            l[b] = np.concatenate([p[b], lbx[b], lbg[b]]) - c
            u[b] = np.concatenate([p[b], ubx[b], ubg[b]]) - c
        return LocalSystem(self.n, self.m, self.Pp, self.Pi, self.Ap, self.Ai, P, q, A, l, u, self.np)

    def kkt_residuals(self, ls, y, tol=1e-3):
        """the optimality residuals of the local system `ls` under the multipliers y (kkt.kkt_residuals states the measure)"""
        from .kkt import kkt_residuals
        return kkt_residuals(self.Ap, self.Ai, ls.q, ls.A, ls.l, ls.u, y, self.np, tol)


def reference_test_cases():
    """The 8 NLPs of the reference's test/test.cpp (cases 1-8), as (model, arg, expected-or-None).
    INF there is float infinity (test/test.cpp:11)."""
    cases = []

    def quad(c):  # f = sum (x_i - c_i)^2
        c = np.asarray(c, float)
        return (lambda w: float(np.sum((w - c) ** 2)), lambda w: 2 * (w - c), lambda w: 2 * np.eye(len(c)))

    f, gr, he = quad([0, 0])
    m = DenseNLP(2, 0, f, gr, he, lambda w: np.array([w[0] + w[1] - 1]), lambda w: np.array([[1.0, 1.0]]), np.eye(2, dtype=bool), name="case1")
    cases.append((m, dict(lbx=[-50, -100], ubx=[50, 100], lbg=[0.0], ubg=[0.0], p=[]), [0.5, 0.5]))
    f, gr, he = quad([3, -2])
    m = DenseNLP(2, 0, f, gr, he, None, None, np.eye(2, dtype=bool), name="case2")
    cases.append((m, dict(lbx=[-50, -100], ubx=[50, 100], lbg=[], ubg=[], p=[]), [3, -2]))
    f, gr, he = quad([2, 3])
    m = DenseNLP(2, 0, f, gr, he, lambda w: np.array([w[0] + w[1] - 1]), lambda w: np.array([[1.0, 1.0]]), np.eye(2, dtype=bool), name="case3")
    cases.append((m, dict(lbx=[-100, -100], ubx=[100, 100], lbg=[1.0], ubg=[INF], p=[]), [2, 3]))
    f, gr, he = quad([0, 0])
    m = DenseNLP(2, 0, f, gr, he, lambda w: np.array([w[0], w[1]]), lambda w: np.eye(2), np.eye(2, dtype=bool), np.eye(2, dtype=bool), name="case4")
    cases.append((m, dict(lbx=[-100, -100], ubx=[100, 100], lbg=[1.0, 2.0], ubg=[INF, INF], p=[]), [1, 2]))
    f, gr, he = quad([1, 2, 3])
    m = DenseNLP(3, 0, f, gr, he, lambda w: np.array([w.sum() - 5]), lambda w: np.ones((1, 3)), np.eye(3, dtype=bool), name="case5")
    cases.append((m, dict(lbx=[0, 0, 0], ubx=[INF, INF, INF], lbg=[0.0], ubg=[0.0], p=[]), [2.0 / 3, 5.0 / 3, 8.0 / 3]))
    # case 6: w = [p; x1; x2], f = (x1 - p)^2 + x2^2
    f6 = lambda w: float((w[1] - w[0]) ** 2 + w[2] ** 2)
    g6 = lambda w: np.array([-2 * (w[1] - w[0]), 2 * (w[1] - w[0]), 2 * w[2]])
    h6 = lambda w: np.array([[2.0, -2, 0], [-2, 2, 0], [0, 0, 2]])
    hm6 = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], bool)
    m = DenseNLP(2, 1, f6, g6, h6, None, None, hm6, name="case6")
    cases.append((m, dict(lbx=[-100, -100], ubx=[100, 100], lbg=[], ubg=[], p=[5.0]), [5, 0]))
    f, gr, he = quad([3, 4])
    m = DenseNLP(2, 0, f, gr, he, None, None, np.eye(2, dtype=bool), name="case7")
    cases.append((m, dict(lbx=[0, 0], ubx=[2, 3], lbg=[], ubg=[], p=[]), [2, 3]))
    # case 8: non-convex objective, no pinned answer (test/test.cpp:187-211)
    f8 = lambda w: float(w[0] ** 2 - w[1] ** 2)
    m = DenseNLP(2, 0, f8, lambda w: np.array([2 * w[0], -2 * w[1]]), lambda w: np.diag([2.0, -2.0]),
                 lambda w: np.array([w[0] ** 2 + w[1] ** 2 - 1]), lambda w: np.array([[2 * w[0], 2 * w[1]]]), np.eye(2, dtype=bool), name="case8")
    cases.append((m, dict(lbx=[-100, -100], ubx=[100, 100], lbg=[-INF], ubg=[1.0], p=[]), None))
    return cases


# --------------------------------------------------------------------------------------------- stage OCPs
class StageOCP:
    """min sum_k (s_k - p)' Q (s_k - p) + u_k' R u_k   s.t.  s_{k+1} = F(s_k, u_k),  frame bounds,
    frame_k = [s_k; u_k], N frames, p = reference state (np = nx).  Q, R diagonal (addVectorCost,
    reference src/OptimalControlProblem.cpp:574-600, sums w_i e_i^2 -- no 1/2, so the Hessian is 2Q).
    Dynamics enter as (N-1)*nx equality rows g_k = s_{k+1} - F(s_k, u_k) in [0, 0]
    (addEquationConstraint, reference src/OptimalControlProblem.cpp:448-470)."""

    nx = 0; nu = 0; name = "ocp"
    # optional per-stage path constraint lo <= h(s_k, u_k) <= hi, nh rows per frame (addInequalityConstraint, reference
    # src/OptimalControlProblem.cpp:448-470); rows are stacked behind the dynamics rows: c = [p; x; g; h].  h_lo, h_hi: [nh] for
    # every frame, or [N, nh] when they differ by frame (a terminal constraint is loose, -inf / +inf, on every frame but the last)
    nh = 0; h_lo = None; h_hi = None
    # optional link constraint between consecutive frames, k_lo <= kfun(s_k, u_k, s_{k+1}, u_{k+1}) <= k_hi, nk rows per stage
    # k = 0 .. N-2 (rate limits u_{k+1} - u_k and the like; in the reference any SX over the whole decision vector can be a
    # constraint, src/OptimalControlProblem.cpp:448-489); rows behind the path rows: c = [p; x; g; h; r]
    nk = 0; k_lo = None; k_hi = None

    def kfun(self, s, u, sn, un):
        """[..., nk] link-constraint values; must accept complex input (override together with nk, k_lo, k_hi)"""
        raise NotImplementedError

    def link_bounds(self):
        """([N-1, nk], [N-1, nk]) bounds of the link constraint per stage (the same on every stage)"""
        return (np.broadcast_to(np.asarray(self.k_lo, float), (self.N - 1, self.nk)).copy(),
                np.broadcast_to(np.asarray(self.k_hi, float), (self.N - 1, self.nk)).copy())

    def dk(self, s, u, sn, un):
        """[..., nk, 2 f] Jacobian of kfun wrt [s; u; s_next; u_next] by complex-step differentiation"""
        eps = 1e-30
        args = [s.astype(complex), u.astype(complex), sn.astype(complex), un.astype(complex)]
        out = np.empty(s.shape[:-1] + (self.nk, 2 * self.f))
        col = 0
        for a, w in enumerate((self.nx, self.nu, self.nx, self.nu)):
            for c in range(w):
                pert = [v.copy() if i == a else v for i, v in enumerate(args)]
                pert[a][..., c] += 1j * eps
                out[..., :, col] = np.asarray(self._kfun(*pert)).imag / eps
                col += 1
        return out

    def link_values(self, x):
        s, u = self.frames(x)
        return np.asarray(self._kfun(s[:, :-1], u[:, :-1], s[:, 1:], u[:, 1:])).reshape(x.shape[0], -1)

    def path_bounds(self):
        """([N, nh], [N, nh]) bounds of the path constraint per frame"""
        return (np.broadcast_to(np.asarray(self.h_lo, float), (self.N, self.nh)).copy(),
                np.broadcast_to(np.asarray(self.h_hi, float), (self.N, self.nh)).copy())

    def hfun(self, s, u):
        """[..., nh] path-constraint values; must accept complex input (override together with nh, h_lo, h_hi)"""
        raise NotImplementedError

    # optional general stage cost: lcost(s, u, r) -> [...] replaces the diagonal tracking terms, f = sum_k lcost(s_k, u_k, p),
    # lterm the same for the last frame only.  Any SX expression can be a cost term in the reference (addScalarCost,
    # src/OptimalControlProblem.cpp:491-497) and its QP uses the exact Hessian (SQPOptimizationSolver.cpp:55-60); here the
    # callables are traced (codegen.trace_cost), the gradient is derived on the tape and the Hessian is its derivative.
    lcost = None; lterm = None
    # optional Gauss-Newton frame cost, the third form: rcost(s, u, r) -> [..., nr] (an array or a list of components, like hfun),
    # f = sum_k |rcost(s_k, u_k, r)|^2 -- no 1/2 and no weight vector, the convention of the docstring above (addVectorCost with a nonlinear e): the
    # user scales the residuals -- and rterm -> [..., nrt] the same for the last frame only.  q is the exact gradient 2 J' r; P takes 2 J'J over
    # [s_k; u_k; r], positive semidefinite by construction, in place of the exact Hessian of lcost.  It excludes lcost / lterm; it may read self.sdata
    # and may not read self.theta, as lcost; general_cost stays True for such a model and gauss_newton is True; cost_mask is the structure of J'J.
    # convexify and exact_hessian are refused.  At most NR_MAX rows each.
    rcost = None; rterm = None
    NR_MAX = 32
    # opt-in trajectory tracking: one reference state per frame, p = [r_0; ...; r_{N-1}] (np = N nx), and frame k's cost terms take r_k:
    # sum_k (s_k - r_k)' Q_k (s_k - r_k) + u_k' R_k u_k, or sum_k l(s_k, u_k, r_k).  The reference needs nothing special for it: setReference
    # takes an SX of any size (src/OptimalControlProblem.cpp:570-572), computeOptimalTrajectory checks the size only (:85-90) and the user
    # subtracts slice k in the cost of step k.  Variables stay [p; frames], rows [p; frames; dynamics; path; link]; only np grows.
    per_frame_reference = False
    # optional link cost: llink(s, u, s_next, u_next) -> [...], summed over the stages k = 0 .. N-2 and added to the frame cost (diagonal weights or
    # lcost / lterm): f += sum_{k<N-1} llink(s_k, u_k, s_{k+1}, u_{k+1}) -- a move penalty (u_{k+1} - u_k)' S (u_{k+1} - u_k), a slew penalty on a state.
    # It takes no reference and no theta (a link cost that needs either stays on the facade's general path).  Any SX over two frames is a cost term
    # in the reference (addScalarCost, src/OptimalControlProblem.cpp:491-497); here the callable is traced (codegen.trace_link_cost), its gradient is
    # derived on the tape and its exact Hessian M (2 f x 2 f) couples frame k to frame k + 1 in P, as the dynamics and the link constraints do in A.
    llink = None
    # opt-in plant parameters: a model declares ntheta = k <= 8 and theta = np.array([...]) (the defaults) and reads self.theta[i] inside F or cdyn
    # (not in hfun, kfun, lcost, lterm).  The zoo classes map their attributes (mass, length, ...) onto the same vector, in the order of
    # stage_eval.model_params.  set_instance_params gives every instance of a batch its own row: a batch of different robots.
    ntheta = 0; theta = None
    NTHETA_MAX = 8
    _theta_rows = None; _plant_rows = None

    # opt-in stage data: a model declares nsd = k <= 8 and sdata = np.array([...]) (the defaults) and reads self.sdata[i] inside hfun, lcost and
    # lterm (not in F / cdyn, kfun, llink; a cost that reads it is a method, not a staticmethod).  The values are data of the world -- an obstacle's
    # centre, a corridor's width, a scheduled weight -- not variables: no column, row or entry of P or A comes with them.  set_stage_data gives
    # every frame of every instance its own row: a batch of different worlds.  In the reference the parameter SX may appear in any
    # constraint or cost (src/OptimalControlProblem.cpp:444-497).
    nsd = 0; sdata = None
    NSD_MAX = 8
    _sdata_rows = None
    # opt-in transition data: a model with nsd > 0 sets transition_data = True and F / cdyn, kfun and llink read self.sdata[i] as well --
    # a step length per frame (a non-uniform time grid), a previewed disturbance, a schedule.  The functions of the transition k -> k + 1 take row k;
    # row N-1 is read by hfun, the costs and the rollout tail of advance.  The rows stay data: no column, row, entry or derivative comes with them.
    # Without the flag the three stay refused and nothing changes.
    transition_data = False

    # opt-in convexification of the frame term: a model with lcost sets convexify = True when its cost is not convex everywhere (a
    # Gaussian bump, an inverse-distance potential, a cosine swing-up term).  The QP otherwise takes the exact, indefinite Hessian and comes back
    # NON_CVX.  The flag closes cost_mask under the fill-in of V f(Lambda) V' -- every pair of indices inside one connected component of the
    # Hessian's sparsity graph -- so that convexify_system (host) and mpcqp_stage_convexify (device) find a slot for every entry of the
    # correction, and makes the generated library export the launcher.  Without the flag nothing changes: the same mask, pattern and source.
    convexify = False
    CONVEXIFY_MODES = {"project": 1, "mirror": 2}      # MPCQP_CONVEXIFY_*

    # opt-in exact Lagrangian Hessian: a model with lcost sets exact_hessian = True and the SQP loops (options["exact_hessian"]) add the
    # curvature of the constraints, C_k = -sum_i lam_i d2F_i + sum_i mu_i d2h_i over [s_k; u_k], to the Hessian of the cost that the reference's QP
    # takes (hessian(f, w), src/sqp_solver/SQPOptimizationSolver.cpp:55-60).  The flag ORs the structure of C_k into the [s; u] block of cost_mask
    # (before the closure of convexify), so that lagrangian_system (host) and mpcqp_stage_lagrangian (device) find a slot for every entry, and makes
    # the generated library carry the functors FG, HG and export the launchers.  Without the flag nothing changes: the same mask, pattern and source.
    exact_hessian = False

    def set_stage_data(self, d=None):
        """Host statement of mpcqp_stage_set_stage_data.  d [B, N, nsd]: frame k of instance b takes row d[b, k] in hfun, lcost and lterm -- in
        path_values, dh, constraints, objective, cost_derivatives, local_system, violation, line_search and the stage_cost of advance (d[b, 0]).
        None returns to the defaults self.sdata on every frame.  A call with more instances than rows is a ValueError, a smaller batch uses the
        first rows.  With nothing set every method returns the bits it always did.  A model with transition_data: F, kfun and llink of the transition
        k -> k + 1 take row d[b, k] as well -- in constraints, dF, dk, the link cost, rollout (row k at step k), advance (row 0 for the plant step, row
        N-1 for the rollout tail) and constraint_curvature."""
        if d is not None:
            if self.nsd == 0:
                raise ValueError("this model has no stage data (nsd = 0)")
            d = np.array(d, float)
            if d.ndim != 3 or d.shape[0] < 1 or d.shape[1:] != (self.N, self.nsd):
                raise ValueError("d: expected an array [B, %d, %d], got %s" % (self.N, self.nsd, d.shape))
        self._sdata_rows = d

    def shift_stage_data(self, d_new=None):
        """Host statement of mpcqp_stage_shift_data: row (b, k) becomes row (b, k + 1), the last row d_new [B, nsd] or, without one, the old
        last row again.  The data describe the world: they shift whatever the QP's status was."""
        if self._sdata_rows is None:
            raise ValueError("no stage data are stored (set_stage_data): the defaults do not shift")
        d = self._sdata_rows
        last = d[:, -1:] if d_new is None else np.asarray(d_new, float).reshape(d.shape[0], 1, self.nsd)
        self._sdata_rows = np.concatenate([d[:, 1:], last], axis=1)

    def _stage_data(self, B):
        """[B, N, nsd]: the rows in force for a batch of B instances"""
        if self._sdata_rows is None:
            return np.broadcast_to(np.asarray(self.sdata, float), (B, self.N, self.nsd))
        if self._sdata_rows.shape[0] < B:
            raise ValueError("batch %d is larger than the stored stage data (%d instances)" % (B, self._sdata_rows.shape[0]))
        return self._sdata_rows[:B]

    def _hfun(self, s, u, rows=None):
        """hfun on frames [B, N, .] (rows: a frame subset of the data, [B, n, nsd]) with self.sdata[i] = the [B, N] values of the rows in force"""
        if self.nsd == 0:
            return self.hfun(s, u)
        saved = self.sdata
        try:
            self.sdata = np.moveaxis(self._stage_data(s.shape[0]) if rows is None else rows, -1, 0)
            return self.hfun(s, u)
        finally:
            self.sdata = saved

    def _with_rows(self, rows, fn, *args):
        """fn(*args) with self.sdata[i] = column i of `rows` ([B, n, nsd] for frames [B, n, .], [B, nsd] for one frame per instance)"""
        saved = self.sdata
        try:
            self.sdata = np.moveaxis(rows, -1, 0)
            return fn(*args)
        finally:
            self.sdata = saved

    def _F(self, s, u, rows=None):
        """F on the first frames of the transitions, s [B, n, nx] = frames 0 .. n-1 (rows: their data, [B, n, nsd]; default: the rows in force), or
        on one frame per instance, s [B, nx], with rows [B, nsd].  A model without transition_data: F as it is"""
        if not self.transition_data:
            return self.F(s, u)
        return self._with_rows(self._stage_data(s.shape[0])[:, :s.shape[1]] if rows is None else rows, self.F, s, u)

    def _kfun(self, s, u, sn, un, rows=None):
        """kfun on the pairs (k, k + 1), k = 0 .. n-1, with the rows of the first frames (a model with transition_data; else kfun as it is)"""
        if not self.transition_data:
            return self.kfun(s, u, sn, un)
        return self._with_rows(self._stage_data(s.shape[0])[:, :s.shape[1]] if rows is None else rows, self.kfun, s, u, sn, un)

    def set_instance_params(self, theta=None, plant=None):
        """Host statement of mpcqp_stage_set_instance_params.  theta [B, ntheta]: instance b's parameters, what local_system, objective,
        constraints, violation, line_search and the rollout tail of advance use; plant [B, ntheta]: what the plant step of advance uses (unset:
        the model's rows).  None returns that set to the shared values self.theta.  A call with more instances than rows is a ValueError, a
        smaller batch uses the first rows.  The methods evaluate instance by instance with that instance's values put on the object: this is
        the checker, its batches are small.  With nothing set every method returns the bits it always did."""
        rows = []
        for v, what in ((theta, "theta"), (plant, "plant")):
            if v is not None:
                if self.ntheta == 0:
                    raise ValueError("this model has no parameters (ntheta = 0)")
                v = np.array(v, float)
                if v.ndim != 2 or v.shape[1] != self.ntheta or v.shape[0] < 1:
                    raise ValueError("%s: expected an array [B, %d]" % (what, self.ntheta))
            rows.append(v)
        self._theta_rows, self._plant_rows = rows

    def _each_instance(self, rows, B, fn):
        """[fn(slice(b, b + 1)) for every instance b], each with row b of `rows` as self.theta and no per-instance set in force"""
        if rows.shape[0] < B:
            raise ValueError("batch %d is larger than the stored per-instance parameters (%d rows)" % (B, rows.shape[0]))
        saved = (np.array(self.theta, float), self._theta_rows, self._plant_rows)
        data = self._sdata_rows
        if data is not None and data.shape[0] < B:
            raise ValueError("batch %d is larger than the stored stage data (%d instances)" % (B, data.shape[0]))
        out = []
        try:
            self._theta_rows = self._plant_rows = None
            for b in range(B):
                self.theta = rows[b].copy()
                if data is not None:
                    self._sdata_rows = data[b:b + 1]      # the one-instance call sees its own stage data
                out.append(fn(slice(b, b + 1)))
        finally:
            self.theta, self._theta_rows, self._plant_rows = saved
            self._sdata_rows = data
        return out

    def __init__(self, N, dt, Q, R):
        self.N, self.dt = int(N), float(dt)
        if self.ntheta > self.NTHETA_MAX:
            raise ValueError("a model may declare at most %d parameters (ntheta = %d)" % (self.NTHETA_MAX, self.ntheta))
        if self.nsd > self.NSD_MAX:
            raise ValueError("a model may declare at most %d stage-data values (nsd = %d)" % (self.NSD_MAX, self.nsd))
        if self.nsd and np.size(self.sdata) != self.nsd:
            raise ValueError("sdata must hold the nsd = %d default values" % self.nsd)
        if self.transition_data and not self.nsd:
            raise ValueError("transition_data needs stage data (nsd > 0): it lets F / cdyn, kfun and llink read self.sdata")
        # diagonal weights, the same for every frame ([nx], [nu]) or one row per frame ([N, nx], [N, nu]: terminal costs,
        # ramps) -- addVectorCost is called per step in the reference (readme.md:121-128), so weights may differ by step
        self.Q = np.asarray(Q, float); self.R = np.asarray(R, float)
        self.varying_weights = self.Q.ndim == 2 or self.R.ndim == 2
        self.Qk = np.broadcast_to(self.Q, (int(N), self.nx)).copy(); self.Rk = np.broadcast_to(self.R, (int(N), self.nu)).copy()
        self.f = self.nx + self.nu
        self.pref = bool(self.per_frame_reference)
        self.np = self.N * self.nx if self.pref else self.nx
        self.nvar = self.N * self.f
        self.n = self.np + self.nvar
        self.ngd = (self.N - 1) * self.nx                 # dynamics rows
        self.ng = self.ngd + self.N * self.nh + (self.N - 1) * self.nk    # all general rows: dynamics, nh path rows per frame, nk link rows per stage
        self.m = self.n + self.ng
        self.gauss_newton = self.rcost is not None
        self.general_cost = self.lcost is not None or self.gauss_newton
        if self.gauss_newton:
            from . import codegen
            if self.lcost is not None or self.lterm is not None:
                raise ValueError("rcost excludes lcost / lterm: the frame cost is either a scalar with its exact Hessian or a residual with the "
                                 "Gauss-Newton one")
            if self.convexify:
                raise ValueError(codegen.GN_REFUSES_CONVEXIFY)
            if self.exact_hessian:
                raise ValueError(codegen.GN_REFUSES_EXACT)
            self._rtape = codegen.trace_residual(self.rcost, self.nx, self.nu, self.nx, self.nsd, self)
            d = codegen.residual_tapes(self._rtape)
            self._ltape, self._gtape, mask = d["L"], d["G"], d["mask"]
            self._rttape = self._lttape = self._gttape = None
            if self.rterm is not None:
                self._rttape = codegen.trace_residual(self.rterm, self.nx, self.nu, self.nx, self.nsd, self)
                d = codegen.residual_tapes(self._rttape)
                self._lttape, self._gttape, mask = d["L"], d["G"], mask | d["mask"]
            self.nr, self.nrt = self._rtape.n_out, (self._rttape or self._rtape).n_out
            self.cost_mask = mask
        elif self.rterm is not None:
            raise ValueError("a terminal residual (rterm) needs a stage residual (rcost)")
        elif self.general_cost:
            from . import codegen
            dkw = {"nsd": self.nsd, "model": self} if self.nsd else {}
            self._ltape, self._gtape = codegen.trace_cost(self.lcost, self.nx, self.nu, self.nx, **dkw)
            mask = codegen.hessian_mask(self._gtape)
            self._lttape = self._gttape = None
            if self.lterm is not None:
                self._lttape, self._gttape = codegen.trace_cost(self.lterm, self.nx, self.nu, self.nx, **dkw)
                mask = mask | codegen.hessian_mask(self._gttape)
            self.cost_mask = mask | np.eye(mask.shape[0], dtype=bool)
            if self.exact_hessian:
                self._trace_curvature(codegen)
            if self.convexify:
                self.cost_mask = codegen.closed_mask(self.cost_mask)
        elif self.exact_hessian:
            raise ValueError("exact_hessian needs a stage cost (lcost): the pattern of diagonal weights has no off-diagonal slots for the curvature")
        self.link_cost = self.llink is not None
        if self.link_cost:
            from . import codegen
            tkw = {"nsd": self.nsd, "model": self} if self.transition_data else {}
            self._lktape, self._lkgtape = codegen.trace_link_cost(self.llink, self.nx, self.nu, **tkw)
            self.lmask = codegen.hessian_mask(self._lkgtape)      # exact structure of M over [s; u; s_next; u_next]: no diagonal forced in
        self._build_pattern()
        if self.general_cost:
            self._build_cost_pattern()

    # -- structure -------------------------------------------------------------------------------
    def _build_pattern(self):
        nx, nu, f, N, npp, n = self.nx, self.nu, self.f, self.N, self.np, self.n
        # P (both triangles): diag everywhere, p_i <-> s_k[i] couplings
        Pp = [0]; Pi = []
        self._P_pp = np.zeros(npp, np.int64); self._P_ps = np.zeros((N, nx), np.int64)  # value slots
        self._P_sp = np.zeros((N, nx), np.int64); self._P_ss = np.zeros((N, nx), np.int64); self._P_uu = np.zeros((N, nu), np.int64)
        self._P_la, self._P_lb = [], []
        for i in range(npp):                       # column p_i (per-frame references: column p_k[i'], i = k nx + i', rows p_k[i'], s_k[i'])
            self._P_pp[i] = len(Pi); Pi.append(i)
            for k in ([i // nx] if self.pref else range(N)):
                self._P_sp[k, i % nx] = len(Pi); Pi.append(npp + k * f + i % nx)   # row s_k[i], col p_i
            Pp.append(len(Pi))
        for k in range(N):
            for c in range(f):                     # column s_k[c], u_k[c - nx]: the p row of a state, then the frame rows (the diagonal and the link cost's)
                if c < nx:
                    self._P_ps[k, c] = len(Pi); Pi.append(k * nx + c if self.pref else c)
                own = self._frame_column_rows(Pi, k, c, lambda r: r == c)
                if c < nx: self._P_ss[k, c] = own[c]
                else: self._P_uu[k, c - nx] = own[c]
                Pp.append(len(Pi))
        self.Pp = np.asarray(Pp, np.int32); self.Pi = np.asarray(Pi, np.int32)
        self._P_la = np.asarray(self._P_la, np.int64).reshape(-1, 4); self._P_lb = np.asarray(self._P_lb, np.int64).reshape(-1, 4)
        # A = [I_n; dg/dw]; dg_k/dframe_k dense nx x f, dg_k/ds_{k+1} = I
        Ap = [0]; Ai = []
        self._A_id = np.zeros(n, np.int64)
        self._A_next = np.zeros((N, nx), np.int64)          # slot of +1 in row g_{k-1}[i], col s_k[i] (k>=1)
        self._A_blk = np.zeros((N - 1, nx, f), np.int64)    # slot of -dF[r, c] for stage k
        nh = self.nh; nk = self.nk
        self._A_h = np.zeros((N, nh, f), np.int64)          # slot of +dh[r, c] for frame k
        self._A_k0 = np.zeros((max(N - 1, 0), nk, f), np.int64)   # slot of d r_k / d frame_k [r, c]
        self._A_k1 = np.zeros((max(N - 1, 0), nk, f), np.int64)   # slot of d r_k / d frame_{k+1} [r, c]
        krow0 = n + (N - 1) * nx + N * nh
        for j in range(npp):
            self._A_id[j] = len(Ai); Ai.append(j); Ap.append(len(Ai))
        for k in range(N):
            for c in range(f):
                j = npp + k * f + c
                self._A_id[j] = len(Ai); Ai.append(j)
                if k >= 1 and c < nx:
                    self._A_next[k, c] = len(Ai); Ai.append(n + (k - 1) * nx + c)
                if k < N - 1:
                    for r in range(nx):
                        self._A_blk[k, r, c] = len(Ai); Ai.append(n + k * nx + r)
                for r in range(nh):
                    self._A_h[k, r, c] = len(Ai); Ai.append(n + (N - 1) * nx + k * nh + r)
                if k >= 1:
                    for r in range(nk):
                        self._A_k1[k - 1, r, c] = len(Ai); Ai.append(krow0 + (k - 1) * nk + r)
                if k < N - 1:
                    for r in range(nk):
                        self._A_k0[k, r, c] = len(Ai); Ai.append(krow0 + k * nk + r)
                Ap.append(len(Ai))
        self.Ap = np.asarray(Ap, np.int32); self.Ai = np.asarray(Ai, np.int32)

    def _frame_column_rows(self, Pi, k, c, base):
        """append to Pi the rows of column frame_k[c] that lie in the frames (behind its p rows), ascending: with a link cost the rows frame_{k-1}[r]
        with lmask[r][f + c] (k >= 1); the rows frame_k[r] with base(r), lmask[r][c] (k < N-1) or lmask[f + r][f + c] (k >= 1); the rows
        frame_{k+1}[r] with lmask[f + r][c] (k < N-1).  Returns {r: slot} of the frame_k rows.  The link entries go to the slot tables
        _P_la (what pair k-1 adds, this column in its second frame) and _P_lb (pair k, first frame): rows (slot, pair, row of M, column of M)."""
        f, N, npp = self.f, self.N, self.np
        lm = self.lmask if self.link_cost else None
        own = {}
        if lm is not None and k >= 1:
            for r in range(f):
                if lm[r, f + c]: self._P_la.append((len(Pi), k - 1, r, f + c)); Pi.append(npp + (k - 1) * f + r)
        for r in range(f):
            a = lm is not None and k >= 1 and lm[f + r, f + c]
            b = lm is not None and k < N - 1 and lm[r, c]
            if base(r) or a or b:
                own[r] = len(Pi)
                if a: self._P_la.append((len(Pi), k - 1, f + r, f + c))
                if b: self._P_lb.append((len(Pi), k, r, c))
                Pi.append(npp + k * f + r)
        if lm is not None and k < N - 1:
            for r in range(f):
                if lm[f + r, c]: self._P_lb.append((len(Pi), k, f + r, c)); Pi.append(npp + (k + 1) * f + r)
        return own

    def _build_cost_pattern(self):
        """P structure of a general stage cost (csrc/stage_models.hpp sm_build_cost_pattern): both triangles, rows ascending;
        _P_src: per entry of the frame cost the Hessian element it takes and its slot: (frame k or -1 = summed over the frames, local row,
        local column, slot).  Without a link cost the slots are 0 .. nnz(P)-1 in order; with one, the entries only it has lie between them."""
        nx, f, N, npp = self.nx, self.f, self.N, self.np
        mk = self.cost_mask
        Pp = [0]; Pi = []; src = []
        self._P_la, self._P_lb = [], []

        def frame_rows(k, c):      # the frame rows of column frame_k[c]: entry `slot` takes element (k, r, c) of the frame Hessian where the cost's mask has it
            for r, slot in self._frame_column_rows(Pi, k, c, lambda r: mk[r, c]).items():
                if mk[r, c]: src.append((k, r, c, slot))

        def finish():
            self.Pp = np.asarray(Pp, np.int32); self.Pi = np.asarray(Pi, np.int32)
            self._P_src = np.asarray(src, np.int64)
            self._P_la = np.asarray(self._P_la, np.int64).reshape(-1, 4); self._P_lb = np.asarray(self._P_lb, np.int64).reshape(-1, 4)
        if self.pref:
            # per-frame references: nothing sums over the frames, every entry is one element of frame k's Hessian over [s; u; r_k]
            for k in range(N):
                for i in range(nx):
                    for r in range(nx):
                        if mk[f + r, f + i]: src.append((k, f + r, f + i, len(Pi))); Pi.append(k * nx + r)
                    for r in range(f):
                        if mk[r, f + i]: src.append((k, r, f + i, len(Pi))); Pi.append(npp + k * f + r)
                    Pp.append(len(Pi))
            for k in range(N):
                for c in range(f):
                    for i in range(nx):
                        if mk[f + i, c]: src.append((k, f + i, c, len(Pi))); Pi.append(k * nx + i)
                    frame_rows(k, c)
                    Pp.append(len(Pi))
            finish()
            return
        for i in range(npp):
            for r in range(npp):
                if mk[f + r, f + i]: src.append((-1, f + r, f + i, len(Pi))); Pi.append(r)
            for k in range(N):
                for r in range(f):
                    if mk[r, f + i]: src.append((k, r, f + i, len(Pi))); Pi.append(npp + k * f + r)
            Pp.append(len(Pi))
        for k in range(N):
            for c in range(f):
                for i in range(npp):
                    if mk[f + i, c]: src.append((k, f + i, c, len(Pi))); Pi.append(i)
                frame_rows(k, c)
                Pp.append(len(Pi))
        finish()

    def _cost_inputs(self, p, x):
        s, u = self.frames(x)
        r = p.reshape(s.shape) if self.pref else np.broadcast_to(p[:, None, :], s.shape)
        ins = [s[..., i] for i in range(self.nx)] + [u[..., i] for i in range(self.nu)] + [r[..., i] for i in range(self.nx)]
        if self.nsd:       # the frames' stage data behind [s; u; r]: inputs of the tapes without a derivative
            d = self._stage_data(x.shape[0])
            ins += [d[..., i] for i in range(self.nsd)]
        return ins

    def _cost_eval(self, tape, ttape, inputs):
        """outputs of tape on every frame [B, N], the last frame taken from ttape when there is a terminal cost"""
        shape = np.shape(inputs[0]); dt = np.result_type(*inputs)
        out = [np.broadcast_to(np.asarray(v), shape).astype(dt) for v in tape.evaluate(inputs)]
        if ttape is not None:
            for o, v in zip(out, ttape.evaluate(inputs)):
                o[:, -1] = np.broadcast_to(np.asarray(v), shape)[:, -1]
        return out

    @staticmethod
    def _residual_jacobian(tape, inputs, nl):
        """(r [B, n, nr], J [B, n, nr, nl]) of a residual tape on the frames of `inputs`: values directly, columns by complex-step differentiation"""
        shape = np.shape(inputs[0]); eps = 1e-30
        ev = lambda ins: np.stack([np.broadcast_to(np.asarray(o), shape) for o in tape.evaluate(ins)], axis=-1)
        r = ev(inputs).astype(float)
        J = np.zeros(shape + (len(tape.outputs), nl))
        for c in range(nl):
            ins = [np.asarray(v).astype(complex) for v in inputs]
            ins[c] = ins[c] + 1j * eps
            J[..., c] = ev(ins).imag / eps
        return r, J

    def cost_derivatives(self, p, x):
        """(grad [B, N, nl], hess [B, N, nl, nl]) of the stage cost on every frame over [s; u; r]: gradient tape evaluated
        directly, Hessian columns by complex-step differentiation of the gradient tape (exact to rounding).  A Gauss-Newton cost (rcost):
        (2 J' r, 2 J'J), J the residual's Jacobian by complex-step differentiation of the residual tape"""
        inputs = self._cost_inputs(p, x)
        nl = len(inputs) - self.nsd; B, N = inputs[0].shape
        if self.gauss_newton:
            grad = np.zeros((B, N, nl)); hess = np.zeros((B, N, nl, nl))
            for tape, sl in ((self._rtape, slice(0, N if self._rttape is None else N - 1)), (self._rttape, slice(N - 1, N))):
                if tape is None:
                    continue
                r, J = self._residual_jacobian(tape, [v[:, sl] for v in inputs], nl)
                grad[:, sl] = 2.0 * np.einsum("bkic,bki->bkc", J, r)
                hess[:, sl] = 2.0 * np.einsum("bkia,bkic->bkac", J, J)
            return grad, hess
        grad = np.stack(self._cost_eval(self._gtape, self._gttape, inputs), axis=-1)
        hess = np.zeros((B, N, nl, nl)); eps = 1e-30
        for c in range(nl):
            ins = [v.astype(complex) for v in inputs]
            ins[c] = ins[c] + 1j * eps
            hess[..., :, c] = np.stack(self._cost_eval(self._gtape, self._gttape, ins), axis=-1).imag / eps
        return grad, hess

    def convexify_system(self, p, x, P, mode="project", eps=1e-6):
        """Host statement of mpcqp_stage_convexify.  P [B, nnzP] as local_system wrote it at (p, x) -> (P_new, touched [B] int, lam_min [B, N]).
        Every frame's Hessian H_k over [s_k; u_k; r] (cost_derivatives; the terminal cost's on the last frame) with lam_min(H_k) < eps is
        replaced by V f(Lambda) V', f(lam) = max(lam, eps) (project) or max(|lam|, eps) (mirror): the correction D_k = f(H_k) - H_k = V (f(Lambda) -
        Lambda) V' (np.linalg.eigh on the full block) is added to the frame's slots (_P_src), and the summed entries of a shared reference's p-p
        block take the sum of D_k over the touched frames, k ascending.  An untouched frame writes nothing; q, A, l, u do not change."""
        if not (self.general_cost and self.convexify):
            raise ValueError("convexify needs a model with a stage cost (lcost) and convexify = True")
        if mode not in self.CONVEXIFY_MODES:
            raise ValueError("mode must be 'project' or 'mirror'")
        eps = float(eps)
        if not (eps > 0.0 and np.isfinite(eps)):
            raise ValueError("eps must be positive and finite")
        p = np.asarray(p, float); x = np.asarray(x, float)
        _, hess = self.cost_derivatives(p, x)
        B, N, nl = hess.shape[:3]
        P_new = np.array(P, float)
        touched = np.zeros(B, np.int64); lam_min = np.zeros((B, N))
        src = self._P_src
        per_frame = [src[src[:, 0] == k] for k in range(N)]
        summed = src[src[:, 0] < 0]
        for b in range(B):
            acc = np.zeros((nl, nl)); any_touched = False
            for k in range(N):
                lam, V = np.linalg.eigh(hess[b, k])
                lam_min[b, k] = lam[0]
                if not lam[0] < eps:
                    continue
                a = np.abs(lam) if mode == "mirror" else lam
                D = (V * (np.maximum(a, eps) - lam)) @ V.T
                D = 0.5 * (D + D.T)                          # (both triangles the same bits)
                touched[b] += 1; any_touched = True
                e = per_frame[k]
                P_new[b, e[:, 3]] += D[e[:, 1], e[:, 2]]
                acc += D
            if any_touched and len(summed):
                P_new[b, summed[:, 3]] += acc[summed[:, 1], summed[:, 2]]
        return P_new, touched, lam_min

    # -- the exact Lagrangian Hessian (include/mpcqp.h, mpcqp_stage_lagrangian; csrc/stage_kernels.hpp stage_lagrangian_kernel) ----------
    def _trace_curvature(self, codegen):
        """the gradient tapes of lam' F and mu' hfun over [s; u] (codegen.trace_curvature, what the generated library compiles) and the structure of
        their Hessians, which joins the [s; u] block of cost_mask"""
        tkw = {"nsd": self.nsd, "model": self} if self.transition_data else {}
        if self.nk and not codegen.link_is_linear(codegen._trace_link(self.kfun, self.nx, self.nu, self.nk, **tkw)):
            raise ValueError("exact_hessian does not cover a nonlinear link constraint (kfun): its curvature couples two frames; a linear kfun "
                             "(rate limits) is fine")
        # (the zoo classes on the generated path keep their constants in the code: no parameter inputs, as in stage_eval.StageEvaluator)
        self._curv_ntheta = 0 if isinstance(self, (Quadrotor, CartPole)) else int(self.ntheta)
        t = codegen.trace_curvature(self.F, self.nx, self.nu, self.hfun if self.nh else None, self.nh, self._curv_ntheta, self.nsd, self,
                                    **({"transition_data": True} if self.transition_data else {}))
        self._fgtape, self._hgtape, self.curvature_mask = t["FG"], t["HG"], t["mask"]
        self.cost_mask[:self.f, :self.f] |= self.curvature_mask

    @staticmethod
    def _tape_hessian(gtape, inputs, f):
        """[..., f, f]: the derivative of the gradient tape's f outputs over its first f inputs, column by column by complex-step differentiation
        (exact to rounding), like cost_derivatives"""
        shape = np.shape(inputs[0]); eps = 1e-30
        out = np.zeros(shape + (f, f))
        for c in range(f):
            ins = [np.asarray(v).astype(complex) for v in inputs]
            ins[c] = ins[c] + 1j * eps
            out[..., :, c] = np.stack([np.broadcast_to(np.asarray(o), shape) for o in gtape.evaluate(ins)], axis=-1).imag / eps
        return out

    def constraint_curvature(self, x, y):
        """C [B, N, f, f]: the curvature of the constraints at x under the multipliers y [B, m] (rows [p; x; dynamics; path; link], what mpcqp_get
        returns), C_k = -sum_i y_dyn[k, i] d2F_i(s_k, u_k) (k < N-1) + sum_i y_path[k, i] d2h_i(s_k, u_k), formed as -CF + CH.  F takes the
        instance's parameter row, hfun the frame's stage-data row.  The rows p and x are linear; a link constraint must be (trace refuses another)."""
        if not (self.general_cost and self.exact_hessian):
            raise ValueError("the constraint curvature needs a model with a stage cost (lcost) and exact_hessian = True")
        x = np.asarray(x, float); y = np.asarray(y, float)
        B = x.shape[0]; N, nx, nh, f, n = self.N, self.nx, self.nh, self.f, self.n
        s, u = self.frames(x)
        frame = [s[..., i] for i in range(nx)] + [u[..., i] for i in range(self.nu)]
        lam = np.zeros((B, N, nx))
        lam[:, :N - 1] = y[:, n:n + self.ngd].reshape(B, N - 1, nx)
        par = []
        if self._curv_ntheta:
            rows = self._theta_rows
            if rows is not None and rows.shape[0] < B:
                raise ValueError("batch %d is larger than the stored per-instance parameters (%d rows)" % (B, rows.shape[0]))
            rows = np.broadcast_to(np.asarray(self.theta, float), (B, self._curv_ntheta)) if rows is None else rows[:B]
            par = [np.broadcast_to(rows[:, i:i + 1], (B, N)) for i in range(self._curv_ntheta)]
        tdata = [self._stage_data(B)[..., i] for i in range(self.nsd)] if self.transition_data else []      # (frame k under row k)
        C = -self._tape_hessian(self._fgtape, frame + par + [lam[..., i] for i in range(nx)] + tdata, f)
        C[:, N - 1] = 0.0                                       # the last frame has no dynamics row
        if nh:
            mu = y[:, n + self.ngd:n + self.ngd + N * nh].reshape(B, N, nh)
            d = self._stage_data(B) if self.nsd else None
            data = [d[..., i] for i in range(self.nsd)] if self.nsd else []
            C = C + self._tape_hessian(self._hgtape, frame + [mu[..., i] for i in range(nh)] + data, f)
        return C

    def lagrangian_system(self, p, x, y, P, status=None, mode=None, eps=1e-6):
        """Host statement of mpcqp_stage_lagrangian.  P [B, nnzP] as local_system wrote it at (p, x) -> (P_new, touched [B] int, lam_min [B, N]).
        Every frame's curvature C_k (constraint_curvature) is added to the frame's slots of the [s; u] block (_P_src; the entries of curvature_mask).
        With mode ("project" / "mirror"; a model that also sets convexify = True) the rule of convexify_system then runs on H_k^L = H_k + C_k, C_k
        zero-padded over r: a frame with lam_min(H_k^L) < eps takes the correction V (f(Lambda) - Lambda) V' on top, a shared reference's p-p block the
        sum over the touched frames, k ascending; an untouched frame keeps the bits mode = None gives.  An instance whose status is not in STATUS_OK
        keeps every bit of P, counts no touched frame and has lam_min = NaN.  Without mode, touched is zero and lam_min NaN.  q, A, l, u do not change."""
        if not (self.general_cost and self.exact_hessian):
            raise ValueError("the Lagrangian Hessian needs a model with a stage cost (lcost) and exact_hessian = True")
        if mode is not None:
            if not self.convexify:
                raise ValueError("a mode needs a model that also sets convexify = True")
            if mode not in self.CONVEXIFY_MODES:
                raise ValueError("mode must be None, 'project' or 'mirror'")
            eps = float(eps)
            if not (eps > 0.0 and np.isfinite(eps)):
                raise ValueError("eps must be positive and finite")
        p = np.asarray(p, float); x = np.asarray(x, float)
        C = self.constraint_curvature(x, y)
        B, N, f = C.shape[:3]
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), self.STATUS_OK)
        P_new = np.array(P, float)
        touched = np.zeros(B, np.int64); lam_min = np.full((B, N), np.nan)
        src = self._P_src
        e = src[(src[:, 0] >= 0) & (src[:, 1] < f) & (src[:, 2] < f)]
        e = e[self.curvature_mask[e[:, 1], e[:, 2]]]
        for b in np.nonzero(ok)[0]:
            P_new[b, e[:, 3]] += C[b, e[:, 0], e[:, 1], e[:, 2]]
        if mode is None:
            return P_new, touched, lam_min
        _, hess = self.cost_derivatives(p, x)
        nl = hess.shape[2]
        per_frame = [src[src[:, 0] == k] for k in range(N)]
        summed = src[src[:, 0] < 0]
        for b in np.nonzero(ok)[0]:
            acc = np.zeros((nl, nl)); any_touched = False
            for k in range(N):
                HL = hess[b, k].copy()
                HL[:f, :f] += C[b, k]
                lam, V = np.linalg.eigh(HL)
                lam_min[b, k] = lam[0]
                if not lam[0] < eps:
                    continue
                a = np.abs(lam) if mode == "mirror" else lam
                D = (V * (np.maximum(a, eps) - lam)) @ V.T
                D = 0.5 * (D + D.T)                          # (both triangles the same bits)
                touched[b] += 1; any_touched = True
                ek = per_frame[k]
                P_new[b, ek[:, 3]] += D[ek[:, 1], ek[:, 2]]
                acc += D
            if any_touched and len(summed):
                P_new[b, summed[:, 3]] += acc[summed[:, 1], summed[:, 2]]
        return P_new, touched, lam_min

    # -- dynamics (override) ---------------------------------------------------------------------
    def cdyn(self, s, u):
        """continuous dynamics ds/dt, arrays [..., nx], [..., nu]; must accept complex input"""
        raise NotImplementedError

    def F(self, s, u):
        """discrete map, RK4 over dt"""
        h = self.dt
        k1 = self.cdyn(s, u); k2 = self.cdyn(s + 0.5 * h * k1, u)
        k3 = self.cdyn(s + 0.5 * h * k2, u); k4 = self.cdyn(s + h * k3, u)
        return s + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)

    def dF(self, s, u):
        """[..., nx, f] Jacobian of F wrt [s; u] by complex-step differentiation (exact to rounding); a model with transition_data: s, u are the
        frames 0 .. n-1 [B, n, .], each under its own row"""
        eps = 1e-30
        out = np.empty(s.shape[:-1] + (self.nx, self.f))
        sc = s.astype(complex); uc = u.astype(complex)
        for c in range(self.f):
            if c < self.nx:
                sp = sc.copy(); sp[..., c] += 1j * eps
                out[..., :, c] = self._F(sp, uc).imag / eps
            else:
                up = uc.copy(); up[..., c - self.nx] += 1j * eps
                out[..., :, c] = self._F(sc, up).imag / eps
        return out

    # -- evaluation ------------------------------------------------------------------------------
    def frames(self, x):
        X = x.reshape(x.shape[0], self.N, self.f)
        return X[:, :, :self.nx], X[:, :, self.nx:]

    def objective(self, p, x):
        if self._theta_rows is not None:       # (the parameters enter F only; evaluated per instance like every other method, for one rule)
            return np.concatenate(self._each_instance(self._theta_rows, x.shape[0], lambda i: self.objective(p[i], x[i])))
        if self.link_cost:
            return self._frame_objective(p, x) + self.link_cost_values(x).sum(axis=1)
        return self._frame_objective(p, x)

    def _frame_objective(self, p, x):
        """the sum of the frame terms (everything but the link cost)"""
        if self.general_cost:
            return self._cost_eval(self._ltape, self._lttape, self._cost_inputs(p, x))[0].sum(axis=1)
        s, u = self.frames(x)
        e = s - (p.reshape(s.shape) if self.pref else p[:, None, :])
        if self.varying_weights:
            return np.einsum("bki,ki->b", e * e, self.Qk) + np.einsum("bki,ki->b", u * u, self.Rk)
        return np.einsum("bki,i->b", e * e, self.Q) + np.einsum("bki,i->b", u * u, self.R)

    def _link_cost_inputs(self, x):
        s, u = self.frames(x)
        ins = ([s[:, :-1, i] for i in range(self.nx)] + [u[:, :-1, i] for i in range(self.nu)]
               + [s[:, 1:, i] for i in range(self.nx)] + [u[:, 1:, i] for i in range(self.nu)])
        if self.transition_data:       # the rows of the pairs' first frames behind the two frames: inputs of the tapes without a derivative
            d = self._stage_data(x.shape[0])[:, :-1]
            ins += [d[..., i] for i in range(self.nsd)]
        return ins

    def link_cost_values(self, x):
        """[B, N-1]: llink(s_k, u_k, s_{k+1}, u_{k+1}) on every stage"""
        ins = self._link_cost_inputs(x)
        return np.broadcast_to(np.asarray(self._lktape.evaluate(ins)[0]), ins[0].shape)

    def link_cost_derivatives(self, x):
        """(grad [B, N-1, 2 f], hess [B, N-1, 2 f, 2 f]) of the link cost on every stage over [s_k; u_k; s_{k+1}; u_{k+1}]: gradient tape evaluated
        directly, Hessian columns by complex-step differentiation of the gradient tape (exact to rounding), like cost_derivatives"""
        ins = self._link_cost_inputs(x)
        n2 = 2 * self.f; shape = ins[0].shape
        ev = lambda v: np.stack([np.broadcast_to(np.asarray(o), shape) for o in self._lkgtape.evaluate(v)], axis=-1)
        grad = ev(ins).astype(float)
        hess = np.zeros(shape + (n2, n2)); eps = 1e-30
        for c in range(n2):
            pert = [v.astype(complex) for v in ins]
            pert[c] = pert[c] + 1j * eps
            hess[..., :, c] = ev(pert).imag / eps
        return grad, hess

    def dh(self, s, u):
        """[..., nh, f] Jacobian of hfun wrt [s; u] by complex-step differentiation (a model with stage data: s, u are all frames [B, N, .])"""
        eps = 1e-30
        out = np.empty(s.shape[:-1] + (self.nh, self.f))
        sc = s.astype(complex); uc = u.astype(complex)
        for c in range(self.f):
            if c < self.nx:
                sp = sc.copy(); sp[..., c] += 1j * eps
                out[..., :, c] = np.asarray(self._hfun(sp, uc)).imag / eps
            else:
                up = uc.copy(); up[..., c - self.nx] += 1j * eps
                out[..., :, c] = np.asarray(self._hfun(sc, up)).imag / eps
        return out

    def constraints(self, x):
        """dynamics defects only (the equality rows)"""
        if self._theta_rows is not None:
            return np.concatenate(self._each_instance(self._theta_rows, x.shape[0], lambda i: self.constraints(x[i])))
        s, u = self.frames(x)
        return (s[:, 1:, :] - self._F(s[:, :-1, :], u[:, :-1, :])).reshape(x.shape[0], -1)

    def path_values(self, x):
        s, u = self.frames(x)
        return np.asarray(self._hfun(s, u)).reshape(x.shape[0], -1)

    def local_system(self, p, x, lbx, ubx, lbg, ubg):
        if self._theta_rows is not None:
            one = self._each_instance(self._theta_rows, x.shape[0], lambda i: self.local_system(p[i], x[i], lbx[i], ubx[i], lbg[i], ubg[i]))
            cat = lambda k: np.concatenate([getattr(o, k) for o in one])
            return LocalSystem(self.n, self.m, self.Pp, self.Pi, self.Ap, self.Ai, cat("P"), cat("q"), cat("A"), cat("l"), cat("u"), self.np)
        B = x.shape[0]; N, nx, nu, f, npp, n = self.N, self.nx, self.nu, self.f, self.np, self.n
        s, u = self.frames(x)
        e = s - (p.reshape(s.shape) if self.pref else p[:, None, :])
        q = np.zeros((B, n))
        if self.general_cost:
            grad, hess = self.cost_derivatives(p, x)
            src = self._P_src; summed = src[:, 0] < 0
            P = np.zeros((B, len(self.Pi)))
            P[:, src[summed, 3]] = hess[:, :, src[summed, 1], src[summed, 2]].sum(axis=1)
            P[:, src[~summed, 3]] = hess[:, src[~summed, 0], src[~summed, 1], src[~summed, 2]]
            q[:, :npp] = grad[:, :, f:].reshape(B, -1) if self.pref else grad[:, :, f:].sum(axis=1)
            q[:, npp:] = grad[:, :, :f].reshape(B, -1)
        else:
            # Hessian values are constant
            Pv = np.zeros(len(self.Pi))
            Pv[self._P_pp] = 2.0 * self.Qk.ravel() if self.pref else 2.0 * self.Qk.sum(axis=0) if self.varying_weights else 2.0 * N * self.Q
            Pv[self._P_sp] = -2.0 * self.Qk; Pv[self._P_ps] = -2.0 * self.Qk
            Pv[self._P_ss] = 2.0 * self.Qk; Pv[self._P_uu] = 2.0 * self.Rk
            P = np.broadcast_to(Pv, (B, len(Pv))).copy()
            if self.pref:
                q[:, :npp] = (-2.0 * e * self.Qk).reshape(B, -1)
            else:
                q[:, :npp] = -2.0 * (np.einsum("bki,ki->bi", e, self.Qk) if self.varying_weights else np.einsum("bki,i->bi", e, self.Q))
            qf = q[:, npp:].reshape(B, N, f)
            qf[:, :, :nx] = 2.0 * e * self.Qk; qf[:, :, nx:] = 2.0 * u * self.Rk
        if self.link_cost:
            # the link cost, in the order the device sums it: the frame term stands; then what pair k-1 adds (this frame its second), then pair k
            gl, Ml = self.link_cost_derivatives(x)               # [B, N-1, 2 f], [B, N-1, 2 f, 2 f]
            la, lb = self._P_la, self._P_lb
            P[:, la[:, 0]] += Ml[:, la[:, 1], la[:, 2], la[:, 3]]
            P[:, lb[:, 0]] += Ml[:, lb[:, 1], lb[:, 2], lb[:, 3]]
            qf = q[:, npp:].reshape(B, N, f)
            qf[:, 1:] += gl[..., f:]
            qf[:, :-1] += gl[..., :f]
        J = self.dF(s[:, :-1, :], u[:, :-1, :])                 # [B, N-1, nx, f]
        A = np.zeros((B, len(self.Ai)))
        A[:, self._A_id] = 1.0
        A[:, self._A_next[1:].ravel()] = 1.0
        A[:, self._A_blk.ravel()] = -J.reshape(B, -1)
        g = (s[:, 1:, :] - self._F(s[:, :-1, :], u[:, :-1, :])).reshape(B, -1)
        if self.nh:
            A[:, self._A_h.ravel()] = self.dh(s, u).reshape(B, -1)
            g = np.concatenate([g, np.asarray(self._hfun(s, u)).reshape(B, -1)], axis=1)
        if self.nk:
            Jk = self.dk(s[:, :-1], u[:, :-1], s[:, 1:], u[:, 1:])          # [B, N-1, nk, 2 f]
            A[:, self._A_k0.ravel()] = Jk[..., :f].reshape(B, -1)
            A[:, self._A_k1.ravel()] = Jk[..., f:].reshape(B, -1)
            g = np.concatenate([g, self.link_values(x)], axis=1)
        c = np.concatenate([p, x, g], axis=1)
        l = np.concatenate([p, lbx, lbg], axis=1) - c
        uu = np.concatenate([p, ubx, ubg], axis=1) - c
        return LocalSystem(n, self.m, self.Pp, self.Pi, self.Ap, self.Ai, P, q, A, l, uu, npp)

    # -- bounds as computeOptimalTrajectory stacks them (OptimalControlProblem.cpp:93-99) ----------
    def frame_bounds(self):
        """per-frame (lower, upper) of length f; override"""
        return np.full(self.f, -INF), np.full(self.f, INF)

    def stacked_bounds(self, frame0):
        B = frame0.shape[0]
        lo, hi = self.frame_bounds()
        lbx = np.tile(lo, (B, self.N)); ubx = np.tile(hi, (B, self.N))
        lbx[:, :self.f] = frame0; ubx[:, :self.f] = frame0
        lbg = np.zeros((B, self.ng)); ubg = np.zeros((B, self.ng))
        if self.nh:
            lo, hi = self.path_bounds()
            lbg[:, self.ngd:self.ngd + self.N * self.nh] = lo.ravel(); ubg[:, self.ngd:self.ngd + self.N * self.nh] = hi.ravel()
        if self.nk:
            lo, hi = self.link_bounds()
            lbg[:, self.ngd + self.N * self.nh:] = lo.ravel(); ubg[:, self.ngd + self.N * self.nh:] = hi.ravel()
        return lbx, ubx, lbg, ubg

    # -- soft constraint rows of the stacked QP (include/mpcqp.h, mpcqp_set_soft_rows) ----------
    SOFT_HARD = 1e30      # the l1 weight of a hard row: the library's infinity

    def soft_rows(self, state=None, input=None, path=None, link=None):
        """(w1, w2) over the m = n + ng rows of the stacked QP, where local_system puts them: the box rows of the states / inputs of frames 1 .. N-1, the
        nh path rows of every frame, the nk link rows of every stage.  Each argument is a pair (w1, w2) of l1 / quadratic weights, scalars or one value per
        component (nx, nu, nh, nk); None = hard.  The parameter rows, the pinned first frame and the dynamics rows are always hard.  The weights belong to
        horizon positions: a receding horizon does not shift them."""
        N, nx, nu, f, npp = self.N, self.nx, self.nu, self.f, self.np
        w1 = np.full(self.m, self.SOFT_HARD); w2 = np.zeros(self.m)

        def put(arg, rows, width, name):
            if arg is None or width == 0:
                return
            a1, a2 = (np.broadcast_to(np.asarray(a, dtype=np.float64), (width,)) for a in arg)
            if (a1 < 0).any() or (a2 < 0).any():
                raise ValueError("soft_rows: %s weights must be >= 0" % name)
            w1[rows] = a1; w2[rows] = a2            # (rows: [count, width])

        k = np.arange(1, N)[:, None]
        put(state, npp + k * f + np.arange(nx)[None, :], nx, "state")
        put(input, npp + k * f + nx + np.arange(nu)[None, :], nu, "input")
        put(path, self.n + self.ngd + np.arange(N)[:, None] * self.nh + np.arange(self.nh)[None, :], self.nh, "path")
        put(link, self.n + self.ngd + N * self.nh + np.arange(N - 1)[:, None] * self.nk + np.arange(self.nk)[None, :], self.nk, "link")
        return w1, w2

    # -- the hand-over between two MPC ticks (include/mpcqp.h, mpcqp_stage_advance; csrc/stage_kernels.hpp stage_advance_kernel) ----------
    STATUS_OK = (1, 2, 7)      # solved, solved_inaccurate, max_iter_reached: the QP returned a point (what mpcqp_stage_step takes too)

    def _shift_blocks(self, v, base, width, count, ok):
        """block k of `count` blocks of `width` entries from `base` becomes block k + 1, the last one zero; all zero where not ok"""
        out = np.zeros((v.shape[0], width * count))
        keep = width * (count - 1)
        out[:, :keep] = v[:, base + width:base + width + keep]
        out[~ok] = 0.0
        return out

    def advance(self, x, lbx, ubx, status=None, s_meas=None, w=None, tail="rollout", p=None, r_new=None, dw=None, y=None):
        """Host statement of mpcqp_stage_advance, out of place: x, lbx, ubx [B, nvar] -> dict with the shifted trajectory `x`, the re-pinned
        `lbx`, `ubx`, `applied` = frame 0 of x, and -- when their inputs are given -- `p` (per-frame references [B, N nx], last block r_new or
        repeated), `dw` [B, n], `y` [B, m] (every row block shifted by its own stage width, zero last block, all zero where the QP failed) and
        `stage_cost` (the k = 0 term of `objective`; p is the shared reference [B, nx] or the per-frame block).  The plant is s_meas when
        given, else F(s_0, u_0) (+ w); the input u_1 where status is in STATUS_OK (or status is None), else u_0 is held."""
        if tail not in ("repeat", "rollout"):
            raise ValueError("tail must be 'repeat' or 'rollout'")
        if s_meas is not None and w is not None:
            raise ValueError("give w or s_meas, not both")
        if self._theta_rows is not None or self._plant_rows is not None:
            # the rollout tail and everything else by the model rows; the plant step F(s_0, u_0) by the plant rows (unset: the model's)
            B = x.shape[0]
            mrows = self._theta_rows if self._theta_rows is not None else np.broadcast_to(np.array(self.theta, float), (B, self.ntheta))
            prows = self._plant_rows if self._plant_rows is not None else mrows
            sl = lambda v, i, dt=float: None if v is None else np.asarray(v, dt).reshape(B, -1)[i]
            call = lambda i: self.advance(sl(x, i), sl(lbx, i), sl(ubx, i), None if status is None else np.asarray(status).reshape(B)[i], sl(s_meas, i), sl(w, i),
                                          tail, sl(p, i), sl(r_new, i), sl(dw, i), sl(y, i))
            one = self._each_instance(mrows, B, call)
            out = {k: np.concatenate([o[k] for o in one]) for k in one[0]}
            if s_meas is None:
                plant = np.concatenate([o["x"][:, :self.nx] for o in self._each_instance(prows, B, call)])
                for k in ("x", "lbx", "ubx"):
                    out[k][:, :self.nx] = plant
            return out
        B, N, nx, f, npp, n = x.shape[0], self.N, self.nx, self.f, self.np, self.n
        X = np.asarray(x, float).reshape(B, N, f)
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), self.STATUS_OK)
        if s_meas is not None:
            sp = np.array(s_meas, float).reshape(B, nx)
        else:
            sp = np.asarray(self._F(X[:, 0, :nx], X[:, 0, nx:], self._stage_data(B)[:, 0] if self.transition_data else None), float)
            if w is not None:
                sp = sp + np.asarray(w, float).reshape(B, nx)
        up = np.where(ok[:, None], X[:, 1, nx:], X[:, 0, nx:])
        Xo = np.empty_like(X)
        Xo[:, 0, :nx] = sp; Xo[:, 0, nx:] = up
        Xo[:, 1:N - 1] = X[:, 2:]
        Xo[:, N - 1] = X[:, N - 1]
        if tail == "rollout":
            Xo[:, N - 1, :nx] = self._F(X[:, N - 1, :nx], X[:, N - 1, nx:], self._stage_data(B)[:, N - 1] if self.transition_data else None)
        out = {"x": Xo.reshape(B, -1), "lbx": np.array(lbx, float), "ubx": np.array(ubx, float), "applied": X[:, 0].copy()}
        out["lbx"][:, :f] = Xo[:, 0]; out["ubx"][:, :f] = Xo[:, 0]
        if self.pref and p is not None:
            P = np.asarray(p, float).reshape(B, N, nx)
            out["p"] = np.concatenate([P[:, 1:], (P[:, -1:] if r_new is None else np.asarray(r_new, float).reshape(B, 1, nx))], axis=1).reshape(B, -1)
        par = (lambda v: self._shift_blocks(v, 0, nx, N, ok)) if self.pref else (lambda v: np.where(ok[:, None], v[:, :nx], 0.0))
        if dw is not None:
            dw = np.asarray(dw, float)
            out["dw"] = np.concatenate([par(dw), self._shift_blocks(dw, npp, f, N, ok)], axis=1)
        if y is not None:
            y = np.asarray(y, float)
            out["y"] = np.concatenate([par(y), self._shift_blocks(y, npp, f, N, ok), self._shift_blocks(y, n, nx, N - 1, ok),
                                       self._shift_blocks(y, n + self.ngd, self.nh, N, ok),
                                       self._shift_blocks(y, n + self.ngd + N * self.nh, self.nk, N - 1, ok)], axis=1)
        if p is not None:
            r0 = np.asarray(p, float).reshape(B, -1)[:, :nx]
            s0, u0 = X[:, 0, :nx], X[:, 0, nx:]
            if self.general_cost:
                ins = [s0[:, i] for i in range(nx)] + [u0[:, i] for i in range(self.nu)] + [r0[:, i] for i in range(nx)]
                if self.nsd:       # the k = 0 term takes d_0, the row before any shift
                    d0 = self._stage_data(B)[:, 0]
                    ins += [d0[:, i] for i in range(self.nsd)]
                out["stage_cost"] = np.broadcast_to(np.asarray(self._ltape.evaluate(ins)[0], float), (B,)).copy()
            else:
                c = np.zeros(B)
                for i in range(nx):
                    e = s0[:, i] - r0[:, i]; c = c + e * e * self.Qk[0, i]
                for i in range(self.nu):
                    c = c + u0[:, i] * u0[:, i] * self.Rk[0, i]
                out["stage_cost"] = c
        return out

    # -- the dynamically feasible start (include/mpcqp.h, mpcqp_stage_rollout; csrc/stage_kernels.hpp stage_rollout_kernel) ----------
    ROLLOUT_INPUTS = ("iterate", "hold")

    def rollout(self, x, lbx=None, ubx=None, inputs="iterate", frozen=None):
        """Host statement of mpcqp_stage_rollout: x [B, nvar] -> dict with `x` (the first frame and the inputs clipped to lbx / ubx, the states
        s_{k+1} = F(s_k, u_k)), `diverged` [B] (the first step k at which s_k, u_k or F(s_k, u_k) is not finite -- every later state holds s_k --
        or -1) and `box_viol` [B] (max over all entries of max(lbx - x, x - ubx, 0)).  inputs: "iterate" keeps x's own inputs, "hold" repeats
        u_0; the states of x's frames k >= 1 are not read.  clip is (v < lo ? lo : v), then (v > hi ? hi : v): a NaN passes through.  frozen [B]:
        an instance with a nonzero entry keeps its row of x and reports -1 and 0 (the device leaves its entries as they were).  The map uses
        the per-instance model rows of set_instance_params where they are set."""
        if inputs not in self.ROLLOUT_INPUTS:
            raise ValueError("inputs must be 'iterate' or 'hold'")
        if (lbx is None) != (ubx is None):
            raise ValueError("give both lbx and ubx or neither")
        x = np.asarray(x, float)
        B, N, nx, f = x.shape[0], self.N, self.nx, self.f
        if self._theta_rows is not None:
            sl = lambda v, i: None if v is None else np.asarray(v, float).reshape(B, -1)[i]
            one = self._each_instance(self._theta_rows, B, lambda i: self.rollout(x[i], sl(lbx, i), sl(ubx, i), inputs,
                                                                                  None if frozen is None else np.asarray(frozen).reshape(B)[i]))
            return {k: np.concatenate([o[k] for o in one]) for k in one[0]}
        X = x.reshape(B, N, f)
        box = lbx is not None
        if box:
            Lo = np.asarray(lbx, float).reshape(B, N, f); Hi = np.asarray(ubx, float).reshape(B, N, f)

        def clip(v, k, cols):
            if not box:
                return v
            lo, hi = Lo[:, k, cols], Hi[:, k, cols]
            v = np.where(v < lo, lo, v)
            return np.where(v > hi, hi, v)

        fr, st, un = slice(0, f), slice(0, nx), slice(nx, f)
        out = np.empty_like(X)
        out[:, 0] = clip(X[:, 0], 0, fr)
        s, u0 = out[:, 0, :nx].copy(), out[:, 0, nx:].copy()
        div = np.full(B, -1, np.int64)
        D = self._stage_data(B) if self.transition_data else None      # step k takes row k
        with np.errstate(all="ignore"):
            for k in range(N - 1):
                u = out[:, k, nx:]
                sn = np.asarray(self._F(s, u, D[:, k] if D is not None else None), float)
                bad = (div < 0) & ~(np.isfinite(s).all(axis=1) & np.isfinite(u).all(axis=1) & np.isfinite(sn).all(axis=1))
                div = np.where(bad, k, div)
                s = np.where((div < 0)[:, None], sn, s)
                out[:, k + 1, :nx] = s
                out[:, k + 1, nx:] = clip(u0 if inputs == "hold" else X[:, k + 1, nx:], k + 1, un)
            viol = np.zeros(B)
            if box:
                viol = np.fmax.reduce(np.fmax(Lo - out, out - Hi).reshape(B, -1), axis=1, initial=0.0)
        out = out.reshape(B, -1)
        if frozen is not None:
            fz = np.asarray(frozen).reshape(B) != 0
            out = np.where(fz[:, None], x, out); div = np.where(fz, -1, div); viol = np.where(fz, 0.0, viol)
        return {"x": out, "diverged": div.astype(np.int32), "box_viol": viol}

    # -- the feedback gains along the plan (include/mpcqp.h, mpcqp_stage_riccati / mpcqp_stage_feedback; csrc/stage_riccati.hpp) ----------
    RICCATI_PIVOT = 1e-12      # MPCQP_RICCATI_PIVOT

    def _riccati_slots(self):
        """(pslot [N, f, f], aslot [N - 1, nx, f]): the slot of P that holds H_k[r][c] and the slot of A that holds -[A_k B_k][r][c]; -1 where the
        pattern has no such entry (the tables the handle builds on the device)"""
        if getattr(self, "_ric_slots", None) is None:
            N, f, npp = self.N, self.f, self.np
            pslot = np.full((N, f, f), -1, np.int64)
            for k in range(N):
                for c in range(f):
                    col = npp + k * f + c
                    for e in range(self.Pp[col], self.Pp[col + 1]):
                        r = int(self.Pi[e]) - npp - k * f
                        if 0 <= r < f:
                            pslot[k, r, c] = e
            self._ric_slots = (pslot, self._A_blk.copy())
        return self._ric_slots

    def riccati_gains(self, P, A, x=None, lbx=None, ubx=None, clamp_tol=0.0, reg=0.0, frozen=None):
        """Host statement of mpcqp_stage_riccati (include/mpcqp.h has the rule in full): the time-varying LQR gains of the equality-constrained
        tangent problem of a local system, P [B, nnzP] and A [B, nnzA] on this model's pattern.  x, lbx, ubx [B, nvar] (all three or none): an
        input within clamp_tol of a bound is clamped -- its row of K_k is 0 and it does not enter V_k.  reg >= 0 is added to the diagonal of
        Q_uu (free inputs).  Returns dict K [B, N, nu, nx], V [B, N, nx, nx], failed [B] (the frame whose pivot failed, -1: none; K and V are
        zero at and below it).  frozen [B]: an instance with a nonzero entry reports zeros and -1 (the device leaves its entries as they were).
        Sums run in ascending index order from 0, as in the header."""
        if self.link_cost:
            raise ValueError("riccati_gains: this model has a link cost: its P couples neighbouring frames, and a sweep over the frame blocks alone "
                             "would drop those terms")
        if len({x is None, lbx is None, ubx is None}) != 1:
            raise ValueError("the clamp needs x, lbx and ubx: give all three or none")
        if not (clamp_tol >= 0.0) or not (reg >= 0.0):
            raise ValueError("clamp_tol and reg must not be negative")
        P = np.asarray(P, float); A = np.asarray(A, float)
        B, N, nx, nu, f = P.shape[0], self.N, self.nx, self.nu, self.f
        if P.shape != (B, len(self.Pi)) or A.shape != (B, len(self.Ai)):
            raise ValueError("P, A: expected shapes [B, %d] and [B, %d] (dimension mismatch)" % (len(self.Pi), len(self.Ai)))
        pslot, aslot = self._riccati_slots()
        Pz = np.concatenate([P, np.zeros((B, 1))], axis=1)      # slot -1 reads the appended zero
        clamp = x is not None
        if clamp:
            X, LB, UB = [np.asarray(v, float).reshape(B, N, f)[:, :, nx:] for v in (x, lbx, ubx)]
        K = np.zeros((B, N, nu, nx)); Vout = np.zeros((B, N, nx, nx)); failed = np.full(B, -1, np.int64)
        alive = np.ones(B, bool) if frozen is None else np.asarray(frozen).reshape(B) == 0
        V = np.zeros((B, nx, nx))
        iu, ju = np.triu_indices(f)
        ix, jx = np.triu_indices(nx)
        dg = np.arange(nu)

        def mirrored(M, i, j):
            out = np.empty_like(M)
            out[:, i, j] = M[:, i, j]; out[:, j, i] = M[:, i, j]
            return out

        with np.errstate(all="ignore"):
            for k in range(N - 1, -1, -1):
                Q = Pz[:, pslot[k]]
                if k < N - 1:
                    AB = -A[:, aslot[k]]
                    T = np.zeros((B, nx, f))
                    for j in range(nx):
                        T = T + V[:, :, j, None] * AB[:, j, None, :]
                    acc = np.zeros((B, f, f))
                    for j in range(nx):
                        acc = acc + AB[:, j, :, None] * T[:, j, None, :]
                    Q = mirrored(Q + acc, iu, ju)
                Qss = Q[:, :nx, :nx]
                M = Q[:, nx:, :].copy()      # the input rows [Q_us Q_uu]: they become [Y U]
                if clamp:
                    cm = (X[:, k] - LB[:, k] <= clamp_tol) | (UB[:, k] - X[:, k] <= clamp_tol)
                    M[:, :, :nx] = np.where(cm[:, :, None], 0.0, M[:, :, :nx])
                    M[:, :, nx:] = np.where(cm[:, :, None] | cm[:, None, :], np.eye(nu), M[:, :, nx:])
                else:
                    cm = np.zeros((B, nu), bool)
                M[:, dg, nx + dg] = M[:, dg, nx + dg] + np.where(cm, 0.0, reg)
                dmax = np.ones(B)
                for i in range(nu):
                    v = np.abs(M[:, i, nx + i])
                    dmax = np.where(v > dmax, v, dmax)
                thr = self.RICCATI_PIVOT * dmax
                bad = np.zeros(B, bool)
                ud = np.zeros((B, nu))
                for jj in range(nu):
                    acc = np.zeros(B)
                    for t in range(jj):
                        acc = acc + M[:, t, nx + jj] * M[:, t, nx + jj]
                    d = M[:, jj, nx + jj] - acc
                    bad |= ~(d > thr)
                    ud[:, jj] = np.sqrt(d)
                    s = np.zeros((B, f))
                    for t in range(jj):
                        s = s + M[:, t, nx + jj, None] * M[:, t, :]
                    new = (M[:, jj, :] - s) / ud[:, jj, None]
                    cols = list(range(nx)) + list(range(nx + jj + 1, f))
                    M[:, jj, cols] = new[:, cols]
                Y = M[:, :, :nx]
                Z = np.zeros((B, nu, nx))
                for i in range(nu - 1, -1, -1):
                    s = np.zeros((B, nx))
                    for t in range(i + 1, nu):
                        s = s + M[:, i, nx + t, None] * Z[:, t, :]
                    Z[:, i, :] = (Y[:, i, :] - s) / ud[:, i, None]
                acc = np.zeros((B, nx, nx))
                for i in range(nu):
                    acc = acc + Y[:, i, :, None] * Y[:, i, None, :]
                Vn = mirrored(Qss - acc, ix, jx)
                failed = np.where(alive & (failed < 0) & bad, k, failed)
                ok = alive & (failed < 0)
                K[ok, k] = -Z[ok]; Vout[ok, k] = Vn[ok]
                V = np.where(ok[:, None, None], Vn, 0.0)
        return {"K": K, "V": Vout, "failed": failed.astype(np.int32)}

    # -- the direct solve of the stage QP (include/mpcqp.h, mpcqp_stage_riccati_solve; csrc/stage_riccati.hpp stage_direct_kernel) ----------
    def _direct_slots(self):
        """(hslot [N, nh, f], k0slot, k1slot [N - 1, nk, f], pcols): the slots of A that hold the path and link rows' entries per frame and, per
        parameter column, its entries of P below the parameter rows as (slots, rows - np) -- the tables the handle builds on the device"""
        if getattr(self, "_dir_slots", None) is None:
            npp, n = self.np, self.n
            pcols = []
            for j in range(npp):
                e = np.arange(self.Pp[j], self.Pp[j + 1])
                rows = self.Pi[e].astype(np.int64)
                keep = (rows >= npp) & (rows < n)
                pcols.append((e[keep], rows[keep] - npp))
            self._dir_slots = (self._A_h.copy(), self._A_k0.copy(), self._A_k1.copy(), pcols)
        return self._dir_slots

    def direct_qp(self, P, q, A, l, u, feas_tol=0.0, reg=0.0, frozen=None):
        """Host statement of mpcqp_stage_riccati_solve (include/mpcqp.h has the rule in full): the local QP solved as its equality-constrained
        tangent problem by one Riccati recursion with affine terms, then tested against every inequality row.  P [B, nnzP], q [B, n], A [B, nnzA],
        l, u [B, m] on this model's pattern.  Returns (w [B, n], y [B, m], z [B, m], direct [B] int32): direct 1 = accepted, the result is the QP's
        solution with its multipliers; 0 = some inequality is violated by more than feas_tol; -1 = not eligible (read from l, u); -2 = a pivot failed.
        Rows of w, y, z of an instance that is not accepted are NaN (the device leaves them as they were); a frozen instance reports direct 0 here
        (the device does not write it).  Sums run in ascending index order from 0, as in the header."""
        if self.link_cost:
            raise ValueError("direct_qp: this model has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame blocks "
                             "alone would drop those terms")
        if not (feas_tol >= 0.0) or not (reg >= 0.0):
            raise ValueError("feas_tol and reg must not be negative")
        P = np.asarray(P, float); A = np.asarray(A, float); q = np.asarray(q, float); l = np.asarray(l, float); u = np.asarray(u, float)
        B, N, nx, nu, f, npp, n, m, nh, nk = P.shape[0], self.N, self.nx, self.nu, self.f, self.np, self.n, self.m, self.nh, self.nk
        if P.shape != (B, len(self.Pi)) or A.shape != (B, len(self.Ai)) or q.shape != (B, n) or l.shape != (B, m) or u.shape != (B, m):
            raise ValueError("P, q, A, l, u: expected shapes [B, %d], [B, %d], [B, %d], [B, %d], [B, %d] (dimension mismatch)"
                             % (len(self.Pi), n, len(self.Ai), m, m))
        pslot, aslot = self._riccati_slots()
        hslot, k0slot, k1slot, pcols = self._direct_slots()
        alive = np.ones(B, bool) if frozen is None else np.asarray(frozen).reshape(B) == 0
        Pz = np.concatenate([P, np.zeros((B, 1))], axis=1)      # slot -1 reads the appended zero
        lf = l[:, npp:n].reshape(B, N, f); uf = u[:, npp:n].reshape(B, N, f)
        ld = l[:, n:n + self.ngd].reshape(B, N - 1, nx); ud = u[:, n:n + self.ngd].reshape(B, N - 1, nx)
        qf = q[:, npp:n].reshape(B, N, f)
        with np.errstate(all="ignore"):
            el = ((l[:, :npp] == 0.0) & (u[:, :npp] == 0.0)).all(axis=1)
            el &= (lf[:, 0, :nx] == uf[:, 0, :nx]).all(axis=1)
            el &= (~np.isnan(lf[:, 0, nx:]) & ~np.isnan(uf[:, 0, nx:])).all(axis=1)
            el &= (~np.isnan(lf[:, 1:]) & ~np.isnan(uf[:, 1:]) & ~(lf[:, 1:] == uf[:, 1:])).all(axis=(1, 2))
            el &= (ld == ud).all(axis=(1, 2))
            pin = lf[:, 0, nx:] == uf[:, 0, nx:]                 # [B, nu]
            pval = lf[:, 0, nx:]
            iu, ju = np.triu_indices(f)
            ix, jx = np.triu_indices(nx)
            dg = np.arange(nu)

            def mirrored(M, i, j):
                out = np.empty_like(M)
                out[:, i, j] = M[:, i, j]; out[:, j, i] = M[:, i, j]
                return out

            H = [Pz[:, pslot[k]] for k in range(N)]
            ABs = [-A[:, aslot[k]] for k in range(N - 1)]
            Kk = np.zeros((B, N, nu, nx)); kap = np.zeros((B, N, nu))
            V = np.zeros((B, nx, nx)); v = np.zeros((B, nx))
            bad = np.zeros(B, bool)
            for k in range(N - 1, -1, -1):
                Q = H[k]
                g = qf[:, k].copy()
                if k < N - 1:
                    AB = ABs[k]
                    T = np.zeros((B, nx, f))
                    for j in range(nx):
                        T = T + V[:, :, j, None] * AB[:, j, None, :]
                    acc = np.zeros((B, f, f))
                    for j in range(nx):
                        acc = acc + AB[:, j, :, None] * T[:, j, None, :]
                    Q = mirrored(Q + acc, iu, ju)
                    h = np.zeros((B, nx))
                    for i in range(nx):
                        h = h + V[:, :, i] * ld[:, k, i, None]
                    h = h + v
                    acc = np.zeros((B, f))
                    for j in range(nx):
                        acc = acc + AB[:, j, :] * h[:, j, None]
                    g = g + acc
                Qss = Q[:, :nx, :nx]
                M = Q[:, nx:, :].copy()      # the input rows [Q_us Q_uu]: they become [Y U]
                gu = g[:, nx:].copy()
                if k == 0:
                    acc = np.zeros((B, nu))
                    for p_ in range(nu):     # Q_uu[p][i] l_p over the pinned inputs p
                        acc = acc + np.where(pin[:, p_, None], M[:, p_, nx:] * pval[:, p_, None], 0.0)
                    gu = np.where(pin, -pval, np.where(pin.any(axis=1)[:, None], gu + acc, gu))
                    M[:, :, :nx] = np.where(pin[:, :, None], 0.0, M[:, :, :nx])
                    M[:, :, nx:] = np.where(pin[:, :, None] | pin[:, None, :], np.eye(nu), M[:, :, nx:])
                    cm = pin
                else:
                    cm = np.zeros((B, nu), bool)
                M[:, dg, nx + dg] = M[:, dg, nx + dg] + np.where(cm, 0.0, reg)
                dmax = np.ones(B)
                for i in range(nu):
                    vv = np.abs(M[:, i, nx + i])
                    dmax = np.where(vv > dmax, vv, dmax)
                thr = self.RICCATI_PIVOT * dmax
                ud_ = np.zeros((B, nu)); y0 = np.zeros((B, nu))
                for jj in range(nu):
                    acc = np.zeros(B)
                    for t in range(jj):
                        acc = acc + M[:, t, nx + jj] * M[:, t, nx + jj]
                    d = M[:, jj, nx + jj] - acc
                    bad |= ~(d > thr)
                    ud_[:, jj] = np.sqrt(d)
                    s = np.zeros((B, f)); s0 = np.zeros(B)
                    for t in range(jj):
                        s = s + M[:, t, nx + jj, None] * M[:, t, :]
                        s0 = s0 + M[:, t, nx + jj] * y0[:, t]
                    new = (M[:, jj, :] - s) / ud_[:, jj, None]
                    cols = list(range(nx)) + list(range(nx + jj + 1, f))
                    M[:, jj, cols] = new[:, cols]
                    y0[:, jj] = (gu[:, jj] - s0) / ud_[:, jj]
                Y = M[:, :, :nx]
                Z = np.zeros((B, nu, nx)); z0 = np.zeros((B, nu))
                for i in range(nu - 1, -1, -1):
                    s = np.zeros((B, nx)); s0 = np.zeros(B)
                    for t in range(i + 1, nu):
                        s = s + M[:, i, nx + t, None] * Z[:, t, :]
                        s0 = s0 + M[:, i, nx + t] * z0[:, t]
                    Z[:, i, :] = (Y[:, i, :] - s) / ud_[:, i, None]
                    z0[:, i] = (y0[:, i] - s0) / ud_[:, i]
                Kk[:, k] = -Z; kap[:, k] = -z0
                if k > 0:
                    acc = np.zeros((B, nx, nx)); acc0 = np.zeros((B, nx))
                    for i in range(nu):
                        acc = acc + Y[:, i, :, None] * Y[:, i, None, :]
                        acc0 = acc0 + Y[:, i, :] * y0[:, i, None]
                    V = mirrored(Qss - acc, ix, jx)
                    v = g[:, :nx] - acc0
            # forwards
            d = np.zeros((B, N, f))
            ds = lf[:, 0, :nx].copy()
            for k in range(N):
                acc = np.zeros((B, nu))
                for j in range(nx):
                    acc = acc + Kk[:, k, :, j] * ds[:, j, None]
                du = acc + kap[:, k]
                if k == 0:
                    du = np.where(pin, pval, du)
                d[:, k, :nx] = ds; d[:, k, nx:] = du
                if k < N - 1:
                    acc = np.zeros((B, nx))
                    for c in range(f):
                        acc = acc + ABs[k][:, :, c] * d[:, k, c, None]
                    ds = acc + ld[:, k]
            # the adjoint recursion
            w = np.zeros((B, n)); y = np.zeros((B, m)); z = np.zeros((B, m))
            w[:, npp:] = d.reshape(B, -1)
            lam = np.zeros((B, nx))
            for k in range(N - 1, -1, -1):
                e = np.zeros((B, f))
                for r in range(f):
                    e = e + H[k][:, r, :] * d[:, k, r, None]
                e = e + qf[:, k]
                t = np.zeros((B, f))
                if k < N - 1:
                    for r in range(nx):
                        t = t + ABs[k][:, r, :] * lam[:, r, None]
                val = t - e
                if k >= 1:
                    lam = val[:, :nx]
                    y[:, n + (k - 1) * nx:n + k * nx] = lam
                else:
                    y[:, npp:npp + nx] = val[:, :nx]
                    y[:, npp + nx:npp + f] = np.where(pin, val[:, nx:], 0.0)
            for j in range(npp):
                slots, rows = pcols[j]
                acc = np.zeros(B)
                for e_, r_ in zip(slots, rows):
                    acc = acc + P[:, e_] * w[:, npp + r_]
                y[:, j] = -(acc + q[:, j])
            # z and the test
            z[:, :n] = w
            z[:, n:n + self.ngd] = l[:, n:n + self.ngd]

            def row(slots, dk, acc):
                for c in range(f):
                    if slots[c] >= 0:
                        acc = acc + A[:, slots[c]] * dk[:, c]
                return acc
            rowh = n + self.ngd; rowk = rowh + N * nh
            for k in range(N):
                for r in range(nh):
                    z[:, rowh + k * nh + r] = row(hslot[k, r], d[:, k], np.zeros(B))
                if k < N - 1:
                    for r in range(nk):
                        z[:, rowk + k * nk + r] = row(k1slot[k, r], d[:, k + 1], row(k0slot[k, r], d[:, k], np.zeros(B)))
            inside = (l - feas_tol <= z) & (z <= u + feas_tol)
            tested = np.ones((B, m), bool)
            tested[:, :npp + nx] = False
            tested[:, npp + nx:npp + f] = ~pin
            tested[:, n:n + self.ngd] = False
            acc_ok = (inside | ~tested).all(axis=1)
        direct = np.where(~el, -1, np.where(bad, -2, np.where(acc_ok, 1, 0)))
        direct = np.where(alive, direct, 0).astype(np.int32)
        out = direct != 1
        w[out] = np.nan; y[out] = np.nan; z[out] = np.nan
        return w, y, z, direct

    # -- the direct solve with held input bounds (include/mpcqp.h, mpcqp_stage_riccati_solve_active; csrc/stage_riccati_active.hpp) -------------
    def _direct_active_round(self, P, q, A, l, u, reg, hold, cval, hadd=None, qadd=None):
        """one round of the rule: the three passes of direct_qp with the inputs of hold [B, N, nu] (the pins of frame 0 included) fixed at
        cval [B, N, nu].  Returns (d [B, N, f], y [B, m], z [B, m], bad [B]).  With no input held beyond the pins the operations are direct_qp's.
        hadd, qadd [B, N, f] (direct_qp_ipm's barrier terms): added to the diagonal of H_k and to q_k for the backward pass alone; the adjoint pass
        keeps the QP's own H_k and q_k."""
        B, N, nx, nu, f, npp, n, m, nh, nk = P.shape[0], self.N, self.nx, self.nu, self.f, self.np, self.n, self.m, self.nh, self.nk
        pslot, aslot = self._riccati_slots()
        hslot, k0slot, k1slot, pcols = self._direct_slots()
        Pz = np.concatenate([P, np.zeros((B, 1), P.dtype)], axis=1)
        lf = l[:, npp:n].reshape(B, N, f)
        ld = l[:, n:n + self.ngd].reshape(B, N - 1, nx)
        qf = q[:, npp:n].reshape(B, N, f)
        iu, ju = np.triu_indices(f)
        ix, jx = np.triu_indices(nx)
        dg = np.arange(nu)

        def mirrored(M, i, j):
            out = np.empty_like(M)
            out[:, i, j] = M[:, i, j]; out[:, j, i] = M[:, i, j]
            return out

        H = [Pz[:, pslot[k]] for k in range(N)]
        ABs = [-A[:, aslot[k]] for k in range(N - 1)]
        Kk = np.zeros((B, N, nu, nx), P.dtype); kap = np.zeros((B, N, nu), P.dtype)
        V = np.zeros((B, nx, nx), P.dtype); v = np.zeros((B, nx), P.dtype)
        bad = np.zeros(B, bool)
        for k in range(N - 1, -1, -1):
            Q = H[k]
            g = qf[:, k].copy()
            if hadd is not None:
                Q = Q.copy()
                Q[:, np.arange(f), np.arange(f)] = Q[:, np.arange(f), np.arange(f)] + hadd[:, k]
                g = g + qadd[:, k]
            if k < N - 1:
                AB = ABs[k]
                T = np.zeros((B, nx, f), P.dtype)
                for j in range(nx):
                    T = T + V[:, :, j, None] * AB[:, j, None, :]
                acc = np.zeros((B, f, f), P.dtype)
                for j in range(nx):
                    acc = acc + AB[:, j, :, None] * T[:, j, None, :]
                Q = mirrored(Q + acc, iu, ju)
                h = np.zeros((B, nx), P.dtype)
                for i in range(nx):
                    h = h + V[:, :, i] * ld[:, k, i, None]
                h = h + v
                acc = np.zeros((B, f), P.dtype)
                for j in range(nx):
                    acc = acc + AB[:, j, :] * h[:, j, None]
                g = g + acc
            Qss = Q[:, :nx, :nx]
            M = Q[:, nx:, :].copy()
            cm = hold[:, k]; cv = cval[:, k]
            anyc = cm.any(axis=1)[:, None]
            acc = np.zeros((B, f), P.dtype)
            for p_ in range(nu):         # Q[p][c] c_p over the held inputs p, every column c
                acc = acc + np.where(cm[:, p_, None], M[:, p_, :] * cv[:, p_, None], 0.0)
            gu = np.where(cm, -cv, np.where(anyc, g[:, nx:] + acc[:, nx:], g[:, nx:]))
            gs = np.where(anyc, g[:, :nx] + acc[:, :nx], g[:, :nx]) if k > 0 else g[:, :nx]
            M[:, :, :nx] = np.where(cm[:, :, None], 0.0, M[:, :, :nx])
            M[:, :, nx:] = np.where(cm[:, :, None] | cm[:, None, :], np.eye(nu), M[:, :, nx:])
            M[:, dg, nx + dg] = M[:, dg, nx + dg] + np.where(cm, 0.0, reg)
            dmax = np.ones(B)
            for i in range(nu):
                vv = np.abs(M[:, i, nx + i])
                dmax = np.where(vv > dmax, vv, dmax)
            thr = self.RICCATI_PIVOT * dmax
            ud_ = np.zeros((B, nu), P.dtype); y0 = np.zeros((B, nu), P.dtype)
            for jj in range(nu):
                acc = np.zeros(B, P.dtype)
                for t in range(jj):
                    acc = acc + M[:, t, nx + jj] * M[:, t, nx + jj]
                d = M[:, jj, nx + jj] - acc
                bad |= ~(d > thr)
                ud_[:, jj] = np.sqrt(d)
                s = np.zeros((B, f), P.dtype); s0 = np.zeros(B, P.dtype)
                for t in range(jj):
                    s = s + M[:, t, nx + jj, None] * M[:, t, :]
                    s0 = s0 + M[:, t, nx + jj] * y0[:, t]
                new = (M[:, jj, :] - s) / ud_[:, jj, None]
                cols = list(range(nx)) + list(range(nx + jj + 1, f))
                M[:, jj, cols] = new[:, cols]
                y0[:, jj] = (gu[:, jj] - s0) / ud_[:, jj]
            Y = M[:, :, :nx]
            Z = np.zeros((B, nu, nx), P.dtype); z0 = np.zeros((B, nu), P.dtype)
            for i in range(nu - 1, -1, -1):
                s = np.zeros((B, nx), P.dtype); s0 = np.zeros(B, P.dtype)
                for t in range(i + 1, nu):
                    s = s + M[:, i, nx + t, None] * Z[:, t, :]
                    s0 = s0 + M[:, i, nx + t] * z0[:, t]
                Z[:, i, :] = (Y[:, i, :] - s) / ud_[:, i, None]
                z0[:, i] = (y0[:, i] - s0) / ud_[:, i]
            Kk[:, k] = -Z; kap[:, k] = -z0
            if k > 0:
                acc = np.zeros((B, nx, nx), P.dtype); acc0 = np.zeros((B, nx), P.dtype)
                for i in range(nu):
                    acc = acc + Y[:, i, :, None] * Y[:, i, None, :]
                    acc0 = acc0 + Y[:, i, :] * y0[:, i, None]
                V = mirrored(Qss - acc, ix, jx)
                v = gs - acc0
        d = np.zeros((B, N, f), P.dtype)
        ds = lf[:, 0, :nx].copy()
        for k in range(N):
            acc = np.zeros((B, nu), P.dtype)
            for j in range(nx):
                acc = acc + Kk[:, k, :, j] * ds[:, j, None]
            du = np.where(hold[:, k], cval[:, k], acc + kap[:, k])
            d[:, k, :nx] = ds; d[:, k, nx:] = du
            if k < N - 1:
                acc = np.zeros((B, nx), P.dtype)
                for c in range(f):
                    acc = acc + ABs[k][:, :, c] * d[:, k, c, None]
                ds = acc + ld[:, k]
        w = np.zeros((B, n), P.dtype); y = np.zeros((B, m), P.dtype); z = np.zeros((B, m), P.dtype)
        w[:, npp:] = d.reshape(B, -1)
        lam = np.zeros((B, nx), P.dtype)
        for k in range(N - 1, -1, -1):
            e = np.zeros((B, f), P.dtype)
            for r in range(f):
                e = e + H[k][:, r, :] * d[:, k, r, None]
            e = e + qf[:, k]
            t = np.zeros((B, f), P.dtype)
            if k < N - 1:
                for r in range(nx):
                    t = t + ABs[k][:, r, :] * lam[:, r, None]
            val = t - e
            o = npp + k * f
            if k >= 1:
                lam = val[:, :nx]
                y[:, n + (k - 1) * nx:n + k * nx] = lam
            else:
                y[:, o:o + nx] = val[:, :nx]
            y[:, o + nx:o + f] = np.where(hold[:, k], val[:, nx:], 0.0)
        for j in range(npp):
            slots, rows = pcols[j]
            acc = np.zeros(B, P.dtype)
            for e_, r_ in zip(slots, rows):
                acc = acc + P[:, e_] * w[:, npp + r_]
            y[:, j] = -(acc + q[:, j])
        z[:, :n] = w
        z[:, n:n + self.ngd] = l[:, n:n + self.ngd]

        def row(slots, dk, acc):
            for c in range(f):
                if slots[c] >= 0:
                    acc = acc + A[:, slots[c]] * dk[:, c]
            return acc
        rowh = n + self.ngd; rowk = rowh + N * nh
        for k in range(N):
            for r in range(nh):
                z[:, rowh + k * nh + r] = row(hslot[k, r], d[:, k], np.zeros(B, P.dtype))
            if k < N - 1:
                for r in range(nk):
                    z[:, rowk + k * nk + r] = row(k1slot[k, r], d[:, k + 1], row(k0slot[k, r], d[:, k], np.zeros(B, P.dtype)))
        return d, w, y, z, bad

    def direct_qp_active(self, P, q, A, l, u, feas_tol=0.0, reg=0.0, rounds=4, dual_tol=0.0, act=None, frozen=None):
        """Host statement of mpcqp_stage_riccati_solve_active (include/mpcqp.h has the rule in full): direct_qp, then up to `rounds` primal-dual
        active-set rounds over the input box rows, every round one Riccati solve with the held inputs fixed at their bounds.  act [B, N, nu]
        (optional): the guess, -1 held at the lower bound, +1 at the upper bound, 0 free.  Returns (w [B, n], y [B, m], z [B, m], direct [B] int32,
        act [B, N, nu] int32, rounds_used [B] int32).  direct as direct_qp; rows of w, y, z of an instance that is not accepted are NaN.  act and
        rounds_used of an ineligible, failed or frozen instance are what came in (zeros without a guess) and -1: the device does not write them."""
        if self.link_cost:
            raise ValueError("direct_qp_active: this model has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame "
                             "blocks alone would drop those terms")
        if not (feas_tol >= 0.0) or not (reg >= 0.0) or not (dual_tol >= 0.0):
            raise ValueError("feas_tol, reg and dual_tol must not be negative")
        if int(rounds) != rounds or not 1 <= rounds <= 8:
            raise ValueError("rounds: expected 1 .. 8")
        P = np.asarray(P, float); A = np.asarray(A, float); q = np.asarray(q, float); l = np.asarray(l, float); u = np.asarray(u, float)
        B, N, nx, nu, f, npp, n, m, nh, nk = P.shape[0], self.N, self.nx, self.nu, self.f, self.np, self.n, self.m, self.nh, self.nk
        if P.shape != (B, len(self.Pi)) or A.shape != (B, len(self.Ai)) or q.shape != (B, n) or l.shape != (B, m) or u.shape != (B, m):
            raise ValueError("P, q, A, l, u: expected shapes [B, %d], [B, %d], [B, %d], [B, %d], [B, %d] (dimension mismatch)"
                             % (len(self.Pi), n, len(self.Ai), m, m))
        guess = np.zeros((B, N, nu), np.int32) if act is None else np.array(act, np.int32).reshape(B, N, nu)
        alive = np.ones(B, bool) if frozen is None else np.asarray(frozen).reshape(B) == 0
        lf = l[:, npp:n].reshape(B, N, f); uf = u[:, npp:n].reshape(B, N, f)
        ld = l[:, n:n + self.ngd].reshape(B, N - 1, nx); ud = u[:, n:n + self.ngd].reshape(B, N - 1, nx)
        with np.errstate(all="ignore"):
            el = ((l[:, :npp] == 0.0) & (u[:, :npp] == 0.0)).all(axis=1)
            el &= (lf[:, 0, :nx] == uf[:, 0, :nx]).all(axis=1)
            el &= (~np.isnan(lf[:, 0, nx:]) & ~np.isnan(uf[:, 0, nx:])).all(axis=1)
            el &= (~np.isnan(lf[:, 1:]) & ~np.isnan(uf[:, 1:]) & ~(lf[:, 1:] == uf[:, 1:])).all(axis=(1, 2))
            el &= (ld == ud).all(axis=(1, 2))
            pin = np.zeros((B, N, nu), bool)
            pin[:, 0] = lf[:, 0, nx:] == uf[:, 0, nx:]
            lu, uu = lf[:, :, nx:], uf[:, :, nx:]                  # the inputs' bounds [B, N, nu]
            # the rows no set over the inputs repairs: the states of the frames k >= 1, the path rows, the link rows
            hard = np.zeros((B, m), bool)
            for k in range(1, N):
                hard[:, npp + k * f:npp + k * f + nx] = True
            hard[:, n + self.ngd:] = True
            lo = np.zeros((B, N, nu), bool); hi = np.zeros((B, N, nu), bool)          # the set S
            w = np.full((B, n), np.nan); y = np.full((B, m), np.nan); z = np.full((B, m), np.nan)
            direct = np.zeros(B, np.int32)
            used = np.full(B, -1, np.int32)
            open_ = alive & el
            for r in range(rounds + 1):
                if not open_.any():
                    break
                hold = pin | lo | hi
                cval = np.where(hi, uu, lu)
                d, wr, yr, zr, bad = self._direct_active_round(P, q, A, l, u, reg, hold, cval)
                if r == 0:
                    direct[open_ & bad] = -2
                    open_ = open_ & ~bad
                else:
                    used[open_ & bad] = r
                    open_ = open_ & ~bad
                inside = (l - feas_tol <= zr) & (zr <= u + feas_tol)
                hopeless = ~(inside | ~hard).all(axis=1)
                du = d[:, :, nx:]
                free = ~hold
                vlo = free & (du < lu - feas_tol)
                vhi = free & ~vlo & (du > uu + feas_tol)
                primal = ((lu - feas_tol <= du) & (du <= uu + feas_tol) | ~free).all(axis=(1, 2))
                yu = np.stack([yr[:, npp + k * f + nx:npp + (k + 1) * f] for k in range(N)], axis=1)
                rel = (hi & ~(yu >= -dual_tol)) | (lo & ~(yu <= dual_tol))
                dual = ~rel.any(axis=(1, 2))
                used[open_ & hopeless] = r
                open_ = open_ & ~hopeless
                take = open_ & primal & dual
                w[take] = wr[take]; y[take] = yr[take]; z[take] = zr[take]
                direct[take] = 1; used[take] = r
                open_ = open_ & ~take
                if r == rounds:
                    used[open_] = r
                    break
                # the next round's set, for the instances still open
                up = open_[:, None, None]
                if r == 0:
                    can_lo = ~pin & np.isfinite(lu) & (guess < 0)
                    can_hi = ~pin & np.isfinite(uu) & (guess > 0)
                    nlo = vlo | (can_lo & ~vhi); nhi = vhi | (can_hi & ~vlo)
                else:
                    nlo = (lo | vlo) & ~rel; nhi = (hi | vhi) & ~rel
                lo = np.where(up, nlo, lo); hi = np.where(up, nhi, hi)
        done = alive & el & (direct != -2)
        act_out = np.where(done[:, None, None] & ~pin, hi.astype(np.int32) - lo.astype(np.int32), guess).astype(np.int32)
        direct = np.where(alive, np.where(~el, -1, direct), 0).astype(np.int32)
        return w, y, z, direct, act_out, used

    # -- the interior-point direct solve (include/mpcqp.h, mpcqp_stage_riccati_solve_ipm; csrc/stage_riccati_ipm.hpp) ----------------------------
    IPM_MAX_ITERS = 50         # MPCQP_IPM_MAX_ITERS
    IPM_T0 = 0.1               # MPCQP_IPM_T0
    IPM_MU0 = 1.0              # MPCQP_IPM_MU0
    IPM_FRAC = 0.995           # MPCQP_IPM_FRAC
    IPM_SIGMA = 0.1            # MPCQP_IPM_SIGMA
    IPM_SIGMA_SHORT = 0.5      # MPCQP_IPM_SIGMA_SHORT
    IPM_ALPHA_SHORT = 0.5      # MPCQP_IPM_ALPHA_SHORT
    IPM_TARGET = 0.5           # MPCQP_IPM_TARGET

    def _direct_ipm_adjoint(self, P, q, A, w, yid):
        """the adjoint pass at the point w [B, n] with yid [B, N, f] on the identity rows: val_k = [A_k B_k]' lam_k - (H_k d_k + q_k) - yid_k, the
        state columns of a frame k >= 1 give lam_{k-1}.  Returns val [B, N, f] (frame 0 and the state columns: multipliers; the input columns of
        the frames k >= 1 and the free inputs of frame 0: what is left of the stationarity condition)."""
        B, N, nx, f, npp, n = P.shape[0], self.N, self.nx, self.f, self.np, self.n
        pslot, aslot = self._riccati_slots()
        Pz = np.concatenate([P, np.zeros((B, 1), P.dtype)], axis=1)
        qf = q[:, npp:n].reshape(B, N, f)
        d = w[:, npp:n].reshape(B, N, f)
        out = np.zeros((B, N, f), P.dtype)
        lam = np.zeros((B, nx), P.dtype)
        for k in range(N - 1, -1, -1):
            Hk = Pz[:, pslot[k]]
            e = np.zeros((B, f), P.dtype)
            for r in range(f):
                e = e + Hk[:, r, :] * d[:, k, r, None]
            e = e + qf[:, k]
            t = np.zeros((B, f), P.dtype)
            if k < N - 1:
                ABk = -A[:, aslot[k]]
                for r in range(nx):
                    t = t + ABk[:, r, :] * lam[:, r, None]
            val = (t - e) - yid[:, k]
            out[:, k] = val
            lam = val[:, :nx]
        return out

    def direct_qp_ipm(self, P, q, A, l, u, feas_tol=1e-9, reg=0.0, iters=30, comp_tol=1e-6, stat_tol=1e-5, frozen=None, trace=None, dtype=float):
        """Host statement of mpcqp_stage_riccati_solve_ipm (include/mpcqp.h has the rule in full): direct_qp as iteration 0, then up to `iters`
        iterations of a primal-dual interior-point method on the box rows of the free variables (states and inputs), every iteration one backward
        and one forward pass of the direct solve on H_k + diag(lambda / t) and a shifted q_k.  Returns (w [B, n], y [B, m], z [B, m], direct [B]
        int32, iters_used [B] int32, res [B, 3]): direct as direct_qp; an accepted point meets the QP's KKT conditions within (feas_tol, comp_tol,
        stat_tol); res = (primal violation of the barriered rows, max lambda t, stationarity left on the free input columns; NaN where the exit
        point was not a candidate).  Rows of w, y, z of an instance that is not accepted are NaN; iters_used and res of an ineligible, failed or
        frozen instance are -1 and NaN (the device does not write them).  trace (a list, optional) receives one dict of the decision margins per
        iteration (tests); dtype=np.longdouble carries the same iteration out in extended precision (the rounding sensitivity of the statement)."""
        if self.link_cost:
            raise ValueError("direct_qp_ipm: this model has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame "
                             "blocks alone would drop those terms")
        if not (feas_tol >= 0.0) or not (reg >= 0.0) or not (comp_tol >= 0.0) or not (stat_tol >= 0.0):
            raise ValueError("feas_tol, reg, comp_tol and stat_tol must not be negative")
        if isinstance(iters, bool) or int(iters) != iters or not 1 <= iters <= self.IPM_MAX_ITERS:
            raise ValueError("iters: expected 1 .. %d" % self.IPM_MAX_ITERS)
        P = np.asarray(P, dtype); A = np.asarray(A, dtype); q = np.asarray(q, dtype); l = np.asarray(l, dtype); u = np.asarray(u, dtype)
        B, N, nx, nu, f, npp, n, m = P.shape[0], self.N, self.nx, self.nu, self.f, self.np, self.n, self.m
        if P.shape != (B, len(self.Pi)) or A.shape != (B, len(self.Ai)) or q.shape != (B, n) or l.shape != (B, m) or u.shape != (B, m):
            raise ValueError("P, q, A, l, u: expected shapes [B, %d], [B, %d], [B, %d], [B, %d], [B, %d] (dimension mismatch)"
                             % (len(self.Pi), n, len(self.Ai), m, m))
        alive = np.ones(B, bool) if frozen is None else np.asarray(frozen).reshape(B) == 0
        lf = l[:, npp:n].reshape(B, N, f); uf = u[:, npp:n].reshape(B, N, f)
        ld = l[:, n:n + self.ngd].reshape(B, N - 1, nx); ud = u[:, n:n + self.ngd].reshape(B, N - 1, nx)
        W = 16 if f <= 16 else 32                              # the lane group of the size class: the order of the sums across the columns
        lanes = np.arange(W)

        def across(v, op):                                     # [B, f] -> [B]: the butterfly of the group (v + v[lane ^ o], o = W / 2 .. 1)
            t = np.zeros((B, W), P.dtype) if op is np.add else np.full((B, W), -np.inf if op is np.fmax else np.inf, P.dtype)
            t[:, :f] = v
            o = W // 2
            while o >= 1:
                t = op(t, t[:, lanes ^ o]); o //= 2
            return t[:, 0]

        with np.errstate(all="ignore"):
            el = ((l[:, :npp] == 0.0) & (u[:, :npp] == 0.0)).all(axis=1)
            el &= (lf[:, 0, :nx] == uf[:, 0, :nx]).all(axis=1)
            el &= (~np.isnan(lf[:, 0, nx:]) & ~np.isnan(uf[:, 0, nx:])).all(axis=1)
            el &= (~np.isnan(lf[:, 1:]) & ~np.isnan(uf[:, 1:]) & ~(lf[:, 1:] == uf[:, 1:])).all(axis=(1, 2))
            el &= (ld == ud).all(axis=(1, 2))
            pin = np.zeros((B, N, nu), bool)
            pin[:, 0] = lf[:, 0, nx:] == uf[:, 0, nx:]
            cval = lf[:, :, nx:]
            bar = np.ones((B, N, f), bool)                     # the barriered columns: every identity row of a free variable
            bar[:, 0, :nx] = False; bar[:, 0, nx:] = ~pin[:, 0]
            mL = bar & (lf > -np.inf); mU = bar & (uf < np.inf)
            lz = np.where(mL, lf, 0.0); uz = np.where(mU, uf, 0.0)
            cnt = (mL.sum(axis=(1, 2)) + mU.sum(axis=(1, 2))).astype(P.dtype)
            rowh = n + self.ngd

            def box_ok(d):
                return ((lf - feas_tol <= d) & (d <= uf + feas_tol) | ~bar).all(axis=(1, 2))

            def rows_ok(z):
                return ((l[:, rowh:] - feas_tol <= z[:, rowh:]) & (z[:, rowh:] <= u[:, rowh:] + feas_tol)).all(axis=1)

            def viol(d):                                       # per column the frames in ascending order, then across the columns
                v = np.zeros((B, f), P.dtype)
                for k in range(N):
                    a = np.where(mL[:, k], lz[:, k] - d[:, k], 0.0); b_ = np.where(mU[:, k], d[:, k] - uz[:, k], 0.0)
                    v = np.where(a > v, a, v); v = np.where(b_ > v, b_, v)
                return across(v, np.fmax)

            def mu_comp(tL, tU, lL, lU):
                s = np.zeros((B, f), P.dtype); c = np.zeros((B, f), P.dtype)
                for k in range(N):
                    a = np.where(mL[:, k], lL[:, k] * tL[:, k], 0.0); b_ = np.where(mU[:, k], lU[:, k] * tU[:, k], 0.0)
                    s = s + a; s = s + b_
                    c = np.where(a > c, a, c); c = np.where(b_ > c, b_, c)
                return across(s, np.add) / cnt, across(c, np.fmax)

            w = np.full((B, n), np.nan, P.dtype); y = np.full((B, m), np.nan, P.dtype); z = np.full((B, m), np.nan, P.dtype)
            direct = np.zeros(B, np.int32)
            used = np.full(B, -1, np.int32)
            res = np.full((B, 3), np.nan, P.dtype)
            # ---- iteration 0: direct_qp
            d, wr, yr, zr, bad = self._direct_active_round(P, q, A, l, u, reg, pin, cval)
            open_ = alive & el
            direct[open_ & bad] = -2
            open_ = open_ & ~bad
            bok, rok = box_ok(d), rows_ok(zr)
            stat0 = self._direct_ipm_adjoint(P, q, A, wr, np.zeros((B, N, f), P.dtype))
            stat0 = across(np.max(np.where(bar & (np.arange(f) >= nx), np.abs(stat0 - reg * d), 0.0), axis=1), np.fmax)
            pv = viol(d)
            res[open_, 0] = pv[open_]; res[open_, 1] = 0.0
            used[open_] = 0
            take = open_ & bok & rok
            w[take] = wr[take]; y[take] = yr[take]; z[take] = zr[take]; direct[take] = 1; res[take, 2] = stat0[take]
            res[open_ & bok & ~rok, 2] = stat0[open_ & bok & ~rok]
            open_ = open_ & ~bok
            # ---- the start
            sl = d - lz; su = uz - d
            tL = np.where(mL, np.where(sl > self.IPM_T0, sl, self.IPM_T0), 1.0); tU = np.where(mU, np.where(su > self.IPM_T0, su, self.IPM_T0), 1.0)
            lL = np.where(mL, self.IPM_MU0 / tL, 0.0); lU = np.where(mU, self.IPM_MU0 / tU, 0.0)
            mu, _ = mu_comp(tL, tU, lL, lU)
            alpha = np.ones(B, P.dtype)
            recentre = np.zeros(B, bool)                       # the last iterate was a candidate whose stationarity was too large
            for it in range(1, int(iters) + 1):
                if not open_.any():
                    break
                sigma = np.where(recentre, 1.0, np.where(alpha >= self.IPM_ALPHA_SHORT, self.IPM_SIGMA, self.IPM_SIGMA_SHORT))
                sm = sigma * mu
                sm = np.where(sm > self.IPM_TARGET * comp_tol, sm, self.IPM_TARGET * comp_tol)[:, None, None]
                rL = lL / tL; rU = lU / tU
                hadd = np.where(mL, rL, 0.0) + np.where(mU, rU, 0.0)
                qadd = np.where(mL, -((sm / tL + lL) + rL * lz), 0.0) + np.where(mU, (sm / tU + lU) - rU * uz, 0.0)
                dn, _, _, _, bad = self._direct_active_round(P, q, A, l, u, reg, pin, cval, hadd=hadd, qadd=qadd)
                dw = dn - d
                dtL = dw + ((d - lz) - tL); dtU = ((uz - d) - tU) - dw
                dlL = (sm / tL - lL) - rL * dtL; dlU = (sm / tU - lU) - rU * dtU
                amin = np.full((B, f), np.inf, P.dtype)
                for k in range(N):
                    for msk, v, dv in ((mL, tL, dtL), (mL, lL, dlL), (mU, tU, dtU), (mU, lU, dlU)):
                        r_ = np.where(msk[:, k] & (dv[:, k] < 0.0), -v[:, k] / dv[:, k], np.inf)
                        amin = np.where(r_ < amin, r_, amin)
                amin = across(amin, np.fmin) * self.IPM_FRAC
                alpha_n = np.where(amin < 1.0, amin, 1.0)
                lost = open_ & (bad | ~((alpha_n > 0.0) & (alpha_n <= 1.0)))
                used[lost] = it
                open_ = open_ & ~lost
                up = open_[:, None, None]
                a3 = alpha_n[:, None, None]
                d = np.where(up, d + a3 * dw, d)
                tL = np.where(up & mL, tL + a3 * dtL, tL); tU = np.where(up & mU, tU + a3 * dtU, tU)
                lL = np.where(up & mL, lL + a3 * dlL, lL); lU = np.where(up & mU, lU + a3 * dlU, lU)
                alpha = np.where(open_, alpha_n, alpha)
                mun, comp = mu_comp(tL, tU, lL, lU)
                mu = np.where(open_, mun, mu)
                pv = viol(d)
                res[open_, 0] = pv[open_]; res[open_, 1] = comp[open_]; res[open_, 2] = np.nan
                used[open_] = it
                cand = open_ & box_ok(d) & (comp <= comp_tol) & (mu <= comp_tol)
                recentre = cand
                if trace is not None:
                    trace.append(dict(it=it, open=open_.copy(), alpha=alpha_n.copy(), mu=mu.copy(), comp=comp.copy(), pv=pv.copy(), cand=cand.copy(),
                                      d=d.copy(), stat=np.full(B, np.nan)))
                if cand.any():
                    wc = np.zeros((B, n), P.dtype); wc[:, npp:] = d.reshape(B, -1)
                    yid = lU - lL
                    val = self._direct_ipm_adjoint(P, q, A, wc, yid)
                    stat = across(np.max(np.where(bar & (np.arange(f) >= nx), np.abs(val - reg * d), 0.0), axis=1), np.fmax)
                    if trace is not None:
                        trace[-1]["stat"] = np.where(cand, stat, np.nan)
                    yc = np.zeros((B, m), P.dtype); zc = np.zeros((B, m), P.dtype)
                    yc[:, npp:n] = np.where(bar, yid, val).reshape(B, -1)
                    for k in range(1, N):
                        yc[:, n + (k - 1) * nx:n + k * nx] = val[:, k, :nx]
                    hslot, k0slot, k1slot, pcols = self._direct_slots()
                    for j in range(npp):
                        slots, rws = pcols[j]
                        acc = np.zeros(B, P.dtype)
                        for e_, r_ in zip(slots, rws):
                            acc = acc + P[:, e_] * wc[:, npp + r_]
                        yc[:, j] = -(acc + q[:, j])
                    zc[:, :n] = wc
                    zc[:, n:rowh] = l[:, n:rowh]

                    def row(slots, dk, acc):
                        for c in range(f):
                            if slots[c] >= 0:
                                acc = acc + A[:, slots[c]] * dk[:, c]
                        return acc
                    rowk = rowh + N * self.nh
                    for k in range(N):
                        for r in range(self.nh):
                            zc[:, rowh + k * self.nh + r] = row(hslot[k, r], d[:, k], np.zeros(B, P.dtype))
                        if k < N - 1:
                            for r in range(self.nk):
                                zc[:, rowk + k * self.nk + r] = row(k1slot[k, r], d[:, k + 1], row(k0slot[k, r], d[:, k], np.zeros(B, P.dtype)))
                    res[cand, 2] = stat[cand]
                    rok = rows_ok(zc)
                    if trace is not None:
                        trace[-1]["z"] = zc.copy()
                    open_ = open_ & ~(cand & ~rok)
                    take = cand & rok & (stat <= stat_tol)
                    w[take] = wc[take]; y[take] = yc[take]; z[take] = zc[take]; direct[take] = 1
                    open_ = open_ & ~take
        direct = np.where(alive, np.where(~el, -1, direct), 0).astype(np.int32)
        gone = ~alive | (direct < 0)
        used[gone] = -1; res[gone] = np.nan
        return w, y, z, direct, used, res

    def feedback(self, K, k, s, s_nom, u_nom, lo=None, hi=None, x=None, lbx=None, ubx=None):
        """Host statement of mpcqp_stage_feedback: u = clip(u_nom + K[:, k] (s - s_nom)) with the sum over the state entries in ascending order,
        every product and sum rounded; clip is the two selects of `rollout` against lo / hi [B, nu] (both or neither).  Returns dict u, du = u - u_nom
        [B, nu], and -- for each of x, lbx, ubx [B, nvar] that is given -- a copy with u written into the input entries of the first frame."""
        if (lo is None) != (hi is None):
            raise ValueError("give both lo and hi or neither")
        if (lbx is None) != (ubx is None):
            raise ValueError("give both lbx and ubx or neither")
        k = int(k)
        if not 0 <= k < self.N:
            raise ValueError("k must be a frame of the horizon, 0 .. N - 1")
        K = np.asarray(K, float).reshape(-1, self.N, self.nu, self.nx)
        B, nx, nu = K.shape[0], self.nx, self.nu
        s = np.asarray(s, float).reshape(B, nx); s_nom = np.asarray(s_nom, float).reshape(B, nx); u_nom = np.asarray(u_nom, float).reshape(B, nu)
        acc = np.zeros((B, nu))
        for j in range(nx):
            acc = acc + K[:, k, :, j] * (s[:, j] - s_nom[:, j])[:, None]
        u = u_nom + acc
        if lo is not None:
            lo = np.asarray(lo, float).reshape(B, nu); hi = np.asarray(hi, float).reshape(B, nu)
            u = np.where(u < lo, lo, u)
            u = np.where(u > hi, hi, u)
        out = {"u": u, "du": u - u_nom}
        for name, v in (("x", x), ("lbx", lbx), ("ubx", ubx)):
            if v is not None:
                c = np.array(v, float).reshape(B, self.nvar)
                c[:, nx:nx + nu] = u
                out[name] = c
        return out

    # -- the per-instance merit line search (include/mpcqp.h, mpcqp_stage_linesearch; csrc/stage_kernels.hpp stage_linesearch_kernel) ----------
    LINE_SEARCH_DEFAULTS = {"candidates": 4, "beta": 0.5, "c1": 1e-4, "mu_min": 1.0, "mu_factor": 1.1}

    def violation(self, x, lbx, ubx):
        """(v [B], gmax [B]): the l1 violation measure of the line search -- dynamics defects, path and link rows outside their bounds, entries of
        x outside lbx / ubx; an infinite bound contributes 0 -- and the max-norm violation mpcqp_stage_merit returns (no box terms in that one)"""
        if self._theta_rows is not None:
            one = self._each_instance(self._theta_rows, np.shape(x)[0], lambda i: self.violation(np.asarray(x, float)[i], np.asarray(lbx, float)[i], np.asarray(ubx, float)[i]))
            return np.concatenate([o[0] for o in one]), np.concatenate([o[1] for o in one])
        with np.errstate(all="ignore"):
            x = np.asarray(x, float)
            d = np.abs(self.constraints(x))
            v = d.sum(axis=1)
            g = np.fmax.reduce(d, axis=1, initial=0.0)
            rows = []
            if self.nh:
                lo, hi = self.path_bounds()
                rows.append((self.path_values(x), lo.ravel(), hi.ravel()))
            if self.nk:
                lo, hi = self.link_bounds()
                rows.append((self.link_values(x), lo.ravel(), hi.ravel()))
            for h, lo, hi in rows:
                v = v + (np.fmax(lo - h, 0.0) + np.fmax(h - hi, 0.0)).sum(axis=1)
                g = np.fmax(g, np.fmax.reduce(np.fmax(lo - h, h - hi), axis=1, initial=0.0))
            v = v + (np.fmax(lbx - x, 0.0) + np.fmax(x - ubx, 0.0)).sum(axis=1)
        return v, g

    def line_search(self, p, x, lbx, ubx, q, dw, y, status=None, mu=None, alpha0=1.0, candidates=4, beta=0.5, c1=1e-4, mu_min=1.0, mu_factor=1.1):
        """Host statement of mpcqp_stage_linesearch: an l1-merit backtracking search per instance.  x [B, nvar] (float64 array) and, when given,
        mu [B] are updated in place.  phi(x) = objective(p, x) + mu_b v(x) with mu_b = max(mu[b], mu_min, mu_factor max_{i >= np} |y_i|);
        D = min(0, q[np:]' dw[np:] - mu_b v(x)); the first alpha_j = alpha0 beta^j, j < candidates, whose phi(x + alpha_j dx) is finite and
        <= phi(x) + c1 alpha_j D is taken (accepted = j).  None: alpha_{K-1} when its merit is finite (accepted = -1), else alpha = 0
        (accepted = -2).  An instance whose status is not in STATUS_OK keeps x, gets alpha = 0, accepted = -2, and its mu stays.
        Returns a dict: x, alpha, accepted, step_max = max|alpha dx|, f and gmax at the new x, phi [B, 2] = phi(x_old), phi(x_new), mu = mu_b,
        and for the tests D [B], alphas [K], phis [B, K + 1] (base point first; NaN where not evaluated)."""
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
        B, npp = x.shape[0], self.np
        p = np.asarray(p, float); lbx = np.asarray(lbx, float); ubx = np.asarray(ubx, float)
        if self._theta_rows is not None:
            # x[i] and mu[i] are views: the in-place updates of the per-instance calls land in the caller's arrays
            st = None if status is None else np.asarray(status)
            one = self._each_instance(self._theta_rows, B, lambda i: self.line_search(
                p[i], x[i], lbx[i], ubx[i], np.asarray(q, float)[i], np.asarray(dw, float)[i], np.asarray(y, float)[i], None if st is None else st[i],
                None if mu is None else mu[i], alpha0, candidates, beta, c1, mu_min, mu_factor))
            out = {k: np.concatenate([o[k] for o in one]) for k in one[0] if k not in ("x", "alphas")}
            out["x"] = x; out["alphas"] = one[0]["alphas"]
            return out
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
                vio[:, j], gmx[:, j] = self.violation(xc, lbx, ubx)
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

    # -- the optimality residuals (include/mpcqp.h, mpcqp_stage_kkt; csrc/kkt_kernels.hpp) -------------------------------------------------
    def kkt_residuals(self, ls, y, tol=1e-3):
        """Host statement of mpcqp_stage_kkt: (res [B, 4] = stat, feas, compl, scale; converged [B]) of the local system `ls` (what local_system
        returned at the iterate: its q, A, l, u) under the multipliers y [B, m]; kkt.kkt_residuals states the measure"""
        from .kkt import kkt_residuals
        return kkt_residuals(self.Ap, self.Ai, ls.q, ls.A, ls.l, ls.u, y, self.np, tol)


class DoubleIntegrator(StageOCP):
    """nx=2, nu=1 LQ-MPC (BASELINE.json configs[1]):
    A_d = [[1, dt], [0, 1]], B_d = [dt^2/2, dt], Q = diag(10, 1), R = 0.1, |u| <= 1, |v| <= 2."""
    nx = 2; nu = 1; name = "double_integrator"

    def __init__(self, N=20, dt=0.05):
        super().__init__(N, dt, [10.0, 1.0], [0.1])

    def F(self, s, u):
        h = self.dt
        pos = s[..., 0] + h * s[..., 1] + 0.5 * h * h * u[..., 0]
        vel = s[..., 1] + h * u[..., 0]
        return np.stack([pos, vel], axis=-1)

    def frame_bounds(self):
        return np.array([-INF, -2.0, -1.0]), np.array([INF, 2.0, 1.0])


class Quadrotor(StageOCP):
    """12-state quadrotor (pos, Euler roll/pitch/yaw, world velocity, body rates; 4 rotor thrusts),
    BASELINE.json configs[2] and the north-star N=20 size:
    Q = diag(10*1_3, 1*1_3, 1*1_3, 0.1*1_3), R = 0.1 I_4, 0 <= u_i <= 2 m g / 4, dt = 0.02."""
    nx = 12; nu = 4; name = "quadrotor"
    mass = 1.0; grav = 9.81; arm = 0.2; kappa = 0.05
    inertia = np.array([0.01, 0.01, 0.02])
    ntheta = 7

    @property
    def theta(self):
        """{mass, grav, arm, kappa, Jx, Jy, Jz}: the attributes as one vector (stage_eval.model_params)"""
        return np.array([self.mass, self.grav, self.arm, self.kappa] + [float(v) for v in self.inertia])

    @theta.setter
    def theta(self, v):
        self.mass, self.grav, self.arm, self.kappa = v[0], v[1], v[2], v[3]
        self.inertia = np.array(v[4:7], float)

    def __init__(self, N=20, dt=0.02):
        super().__init__(N, dt, [10.0] * 3 + [1.0] * 3 + [1.0] * 3 + [0.1] * 3, [0.1] * 4)

    @property
    def hover_thrust(self):
        return self.mass * self.grav / 4.0

    def cdyn(self, s, u):
        phi, th, psi = s[..., 3], s[..., 4], s[..., 5]
        v = s[..., 6:9]; w = s[..., 9:12]
        cph, sph, cth, sth, cps, sps = np.cos(phi), np.sin(phi), np.cos(th), np.sin(th), np.cos(psi), np.sin(psi)
        tth = sth / cth
        T = u[..., 0] + u[..., 1] + u[..., 2] + u[..., 3]
        a = T / self.mass
        # third column of R = Rz(psi) Ry(th) Rx(phi)
        ax = a * (cps * sth * cph + sps * sph)
        ay = a * (sps * sth * cph - cps * sph)
        az = a * (cth * cph) - self.grav
        p_, q_, r_ = w[..., 0], w[..., 1], w[..., 2]
        dphi = p_ + sph * tth * q_ + cph * tth * r_
        dth = cph * q_ - sph * r_
        dpsi = (sph * q_ + cph * r_) / cth
        Jx, Jy, Jz = self.inertia
        tx = self.arm * (u[..., 3] - u[..., 1]); ty = self.arm * (u[..., 2] - u[..., 0])
        tz = self.kappa * (u[..., 0] - u[..., 1] + u[..., 2] - u[..., 3])
        dp = (tx - (Jz - Jy) * q_ * r_) / Jx
        dq = (ty - (Jx - Jz) * p_ * r_) / Jy
        dr = (tz - (Jy - Jx) * p_ * q_) / Jz
        return np.stack([v[..., 0], v[..., 1], v[..., 2], dphi, dth, dpsi, ax, ay, az, dp, dq, dr], axis=-1)

    def frame_bounds(self):
        lo = np.full(self.f, -INF); hi = np.full(self.f, INF)
        lo[self.nx:] = 0.0; hi[self.nx:] = 2.0 * self.mass * self.grav / 4.0
        return lo, hi


class CartPole(StageOCP):
    """Cart-pole swing-up (BASELINE.json configs[3]): s = [x, theta, xdot,
    thetadot] with theta = 0 upright, |u| <= 20 N, track +-2.4 m, dt = 0.02; Gauss-Newton Hessian = 2Q."""
    nx = 4; nu = 1; name = "cartpole"
    mc = 1.0; mp = 0.1; length = 0.5; grav = 9.81
    ntheta = 4

    @property
    def theta(self):
        """{mc, mp, length, grav}: the attributes as one vector (stage_eval.model_params)"""
        return np.array([self.mc, self.mp, self.length, self.grav])

    @theta.setter
    def theta(self, v):
        self.mc, self.mp, self.length, self.grav = v[0], v[1], v[2], v[3]

    def __init__(self, N=100, dt=0.02):
        super().__init__(N, dt, [1.0, 10.0, 0.1, 0.1], [0.01])

    def cdyn(self, s, u):
        th, xd, thd = s[..., 1], s[..., 2], s[..., 3]
        F_ = u[..., 0]
        sn, cs = np.sin(th), np.cos(th)
        tot = self.mc + self.mp
        tmp = (F_ + self.mp * self.length * thd * thd * sn) / tot
        thdd = (self.grav * sn - cs * tmp) / (self.length * (4.0 / 3.0 - self.mp * cs * cs / tot))
        xdd = tmp - self.mp * self.length * thdd * cs / tot
        return np.stack([xd, thd, xdd, thdd], axis=-1)

    def frame_bounds(self):
        return np.array([-2.4, -INF, -INF, -INF, -20.0]), np.array([2.4, INF, INF, INF, 20.0])


class GridCartPole(StageOCP):
    """The cart-pole on a non-uniform time grid h_k = h0 g^k (transition_data): fine steps near now, coarse steps far out.  The frame's
    stage data d = [h_k] is the step of the transition k -> k + 1: in the model's own RK4, in the rate limit |u_{k+1} - u_k| / h_k <= rate (kfun)
    and in the move penalty move (u_{k+1} - u_k)^2 / h_k (llink).  The diagonal weights of frame k are scaled by h_k / h0, so that the sum
    approximates the same integral on every grid.  growth = 1 is the uniform grid; grid_rows gives the rows set_stage_data takes."""
    nx = 4; nu = 1; name = "grid_cartpole"
    mc = 1.0; mp = 0.1; length = 0.5; grav = 9.81
    nsd = 1; sdata = np.array([0.02]); transition_data = True
    nk = 1; rate = 400.0; k_lo = [-400.0]; k_hi = [400.0]
    move = 1e-5

    def __init__(self, N=20, h0=0.02, growth=1.0):
        self.h0, self.growth = float(h0), float(growth)
        self.steps = self.h0 * self.growth ** np.arange(int(N))
        self.sdata = np.array([self.h0])
        w = (self.steps / self.h0)[:, None]
        super().__init__(N, h0, w * np.array([1.0, 10.0, 0.1, 0.1]), w * np.array([0.01]))

    def grid_rows(self, batch):
        """[batch, N, 1]: frame k's step length h_k, the same grid for every instance"""
        return np.tile(self.steps[None, :, None], (int(batch), 1, 1))

    def _rate(self, th, xd, thd, force):
        sn, cs = np.sin(th), np.cos(th)
        tot = self.mc + self.mp
        tmp = (force + self.mp * self.length * thd * thd * sn) / tot
        thdd = (self.grav * sn - cs * tmp) / (self.length * (4.0 / 3.0 - self.mp * cs * cs / tot))
        return xd, thd, tmp - self.mp * self.length * thdd * cs / tot, thdd

    def F(self, s, u):
        """RK4 over the frame's own step h = self.sdata[0], component by component (h has the shape of a component)"""
        h = self.sdata[0]
        y = [s[..., i] for i in range(4)]
        force = u[..., 0]
        k1 = self._rate(y[1], y[2], y[3], force)
        k2 = self._rate(*[y[i] + 0.5 * h * k1[i] for i in (1, 2, 3)], force)
        k3 = self._rate(*[y[i] + 0.5 * h * k2[i] for i in (1, 2, 3)], force)
        k4 = self._rate(*[y[i] + h * k3[i] for i in (1, 2, 3)], force)
        return np.stack([y[i] + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(4)], axis=-1)

    def kfun(self, s, u, sn, un):
        return np.stack([(un[..., 0] - u[..., 0]) / self.sdata[0]], axis=-1)

    def llink(self, s, u, sn, un):
        d = un[..., 0] - u[..., 0]
        return self.move * d * d / self.sdata[0]

    def frame_bounds(self):
        return np.array([-2.4, -INF, -INF, -INF, -20.0]), np.array([2.4, INF, INF, INF, 20.0])


# --------------------------------------------------------------------------------------------- workloads
def make_workload(name, batch, seed=None, N=None):
    """Seeded synthetic QP batches of SURVEY.md section 8(d).  Returns (model, LocalSystem, meta)."""
    if name == "double_integrator":
        mdl = DoubleIntegrator(N or 20, 0.05); rng = np.random.default_rng(1234 if seed is None else seed)
        x0 = rng.uniform([-3.0, -1.5], [3.0, 1.5], size=(batch, 2))
        frame0 = np.concatenate([x0, np.zeros((batch, 1))], axis=1)
        p = np.zeros((batch, 2))
        xit = np.zeros((batch, mdl.nvar))                      # the reference starts SQP at x = 0
    elif name == "quadrotor":
        mdl = Quadrotor(N or 20, 0.02); rng = np.random.default_rng(2024 if seed is None else seed)
        x0 = np.zeros((batch, 12))
        x0[:, 0:3] = rng.normal(0.0, 0.5, size=(batch, 3)); x0[:, 3:6] = rng.normal(0.0, 0.1, size=(batch, 3))
        hov = mdl.hover_thrust
        frame0 = np.concatenate([x0, np.full((batch, 4), hov)], axis=1)
        p = np.zeros((batch, 12))
        # per-instance perturbed-hover iterate: every instance has its own Jacobian blocks
        X = np.zeros((batch, mdl.N, mdl.f))
        X[:, :, :12] = x0[:, None, :] + rng.normal(0.0, 0.05, size=(batch, mdl.N, 12))
        X[:, :, 12:] = hov + rng.normal(0.0, 0.3, size=(batch, mdl.N, 4))
        X[:, 0, :] = frame0
        xit = X.reshape(batch, -1)
    elif name == "cartpole":
        mdl = CartPole(N or 100, 0.02); rng = np.random.default_rng(7 if seed is None else seed)
        x0 = np.zeros((batch, 4)); x0[:, 1] = np.pi + rng.normal(0.0, 0.05, size=batch)
        frame0 = np.concatenate([x0, np.zeros((batch, 1))], axis=1)
        p = np.zeros((batch, 4))
        X = np.zeros((batch, mdl.N, mdl.f))
        X[:, :, :4] = x0[:, None, :] * np.linspace(1.0, 0.0, mdl.N)[None, :, None] + rng.normal(0.0, 0.02, size=(batch, mdl.N, 4))
        X[:, :, 4:] = rng.normal(0.0, 1.0, size=(batch, mdl.N, 1))
        X[:, 0, :] = frame0
        xit = X.reshape(batch, -1)
    else:
        raise ValueError("unknown workload %r" % name)
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    ls = mdl.local_system(p, xit, lbx, ubx, lbg, ubg)
    meta = dict(frame0=frame0, p=p, x_iterate=xit, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    return mdl, ls, meta
