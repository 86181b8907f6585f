"""The independent high-precision restatement of the NLP -- TEST INFRASTRUCTURE ONLY.

What every kernel and the NumPy statement (models.StageOCP) compute, written out once more from the documents (INTEGRATION)
with nothing shared: this module imports nothing of the package, evaluates no tape and reads no pattern.  It receives a model object and calls
its user callbacks only -- F (or cdyn through the inherited RK4 F), hfun, kfun, lcost, lterm, llink, or the diagonal weights Qk / Rk -- one frame
of one instance at a time, on object arrays of the scalar `HP` below, in mpmath arithmetic of DPS digits.  Derivatives are central first and
second differences with the step STEP in that arithmetic: truncation ~ STEP^2 = 1e-30 and rounding ~ 10^-DPS / STEP^2 = 1e-30 relative, both far
below double rounding, so the float64 arrays returned here are the correctly rounded answer for every purpose of a test at 1e-12
(tests/test_nlp_hp_host.py measures it on the unrounded values, `raw=True`: DPS 120 and STEP 1e-16 move none by more than 1.7e-27 max(1, |ref|)).

    w = [p; x],  p = r (np = nx) or [r_0; ...; r_{N-1}] (per_frame_reference),  x = [s_0; u_0; ...; s_{N-1}; u_{N-1}]
    f(w) = sum_k frame_k(s_k, u_k, r_k) + sum_{k < N-1} llink(s_k, u_k, s_{k+1}, u_{k+1})
           frame_k = lcost (lterm on the last frame where the model has one) or sum_i Qk[k, i] (s_i - r_i)^2 + sum_i Rk[k, i] u_i^2
    g(w) = [s_{k+1} - F(s_k, u_k), k < N-1;  hfun(s_k, u_k), k < N;  kfun(s_k, u_k, s_{k+1}, u_{k+1}), k < N-1]
    P = d2f/dw2,  q = df/dw,  A = [I; dg/dw],  l = [p; lbx; lbg] - [w; g],  u = [p; ubx; ubg] - [w; g]

Stage data and parameters reach the callbacks the documented way: the callbacks read self.sdata[i] and self.theta[i]; the row of the frame or
instance in force is put on a copy.copy of the model.  Differencing is over the whole of w where n <= WHOLE_MAX and term by term (every frame,
link and row block over its own arguments, scattered to w by the index arithmetic of `Stage._frame_idx`) above it; `Stage.whole` says which."""
import copy
import functools

import numpy as np
from mpmath import mp, mpf

DPS = 60
STEP = "1e-15"
WHOLE_MAX = 20          # n up to which f and g are differenced over the whole of w
OK = (1, 2, 7)          # QP statuses that returned a point (include/mpcqp.h)


# ------------------------------------------------------------------------------------------------ the scalar
def _raw(o):
    """the mpf of a scalar operand, or None for anything that is not one"""
    if isinstance(o, HP):
        return o.v
    if isinstance(o, np.ndarray):
        return _raw(o[()]) if o.ndim == 0 else None
    if isinstance(o, (bool, int, np.integer)):
        return mpf(int(o))
    if isinstance(o, (float, np.floating)):
        return mpf(float(o))          # exact: every double is an mpf
    if isinstance(o, mpf):
        return o
    return None


def _binary(op, swap=False):
    def method(self, other):
        b = _raw(other)
        if b is None:
            return NotImplemented      # (an array of more than one element: its own operator takes over, element by element)
        return HP(op(b, self.v) if swap else op(self.v, b))
    return method


def _power(a, b):
    return a ** int(b) if b == int(b) else mp.power(a, b)


class HP:
    """a real number in mpmath's working precision that NumPy object arrays and the models' callbacks can compute with"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v if isinstance(v, mpf) else _raw(v)

    __add__ = _binary(lambda a, b: a + b); __radd__ = _binary(lambda a, b: a + b, True)
    __sub__ = _binary(lambda a, b: a - b); __rsub__ = _binary(lambda a, b: a - b, True)
    __mul__ = _binary(lambda a, b: a * b); __rmul__ = _binary(lambda a, b: a * b, True)
    __truediv__ = _binary(lambda a, b: a / b); __rtruediv__ = _binary(lambda a, b: a / b, True)
    __pow__ = _binary(_power); __rpow__ = _binary(_power, True)

    def __neg__(self): return HP(-self.v)
    def __pos__(self): return self
    def __abs__(self): return HP(abs(self.v))
    def __float__(self): return float(self.v)
    def __lt__(self, o): return self.v < _raw(o)
    def __le__(self, o): return self.v <= _raw(o)
    def __gt__(self, o): return self.v > _raw(o)
    def __ge__(self, o): return self.v >= _raw(o)
    def __repr__(self): return "HP(%s)" % mp.nstr(self.v, 20)

    def sin(self): return HP(mp.sin(self.v))
    def cos(self): return HP(mp.cos(self.v))
    def tan(self): return HP(mp.tan(self.v))
    def exp(self): return HP(mp.exp(self.v))
    def log(self): return HP(mp.log(self.v))
    def sqrt(self): return HP(mp.sqrt(self.v))
    def tanh(self): return HP(mp.tanh(self.v))

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        """np.sin(x), np.float64 * x, array * x: the same ufunc on 0-d object arrays, whose loops call the operators and methods above"""
        if method != "__call__" or kwargs:
            return NotImplemented
        boxed = []
        for a in inputs:
            if isinstance(a, HP):
                box = np.empty((), object); box[()] = a
                a = box
            boxed.append(a)
        return ufunc(*boxed)


def _vec(z):
    """a 1-D object array of HP from mpf values"""
    out = np.empty(len(z), object)
    for i, v in enumerate(z):
        out[i] = HP(v)
    return out


def _scalar(o):
    v = _raw(o)
    if v is None:
        raise TypeError("a callback returned %r where a scalar was expected" % (o,))
    return v


def _list(o):
    """the mpf values of what a vector callback returned (an object array, a list of scalars)"""
    a = np.asarray(o, object).reshape(-1) if not isinstance(o, (list, tuple)) else o
    return [_scalar(v) for v in a]


def _mpfs(a):
    return [mpf(float(v)) for v in np.asarray(a, float).reshape(-1)]


def _hp(fn):
    """run a public entry in the working precision of its object and leave mpmath's global precision as it was"""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with mp.workdps(self.dps):
            return fn(self, *a, **k)
    return wrapped


# ------------------------------------------------------------------------------------------------ differencing
def grad_hess(fun, z, h):
    """(f, gradient, Hessian) of the scalar fun at z (lists of mpf) by central differences: 1 + 2 n + n (n - 1) evaluations.
    H_ij = [f(+i +j) + f(-i -j) - f(+i) - f(-i) - f(+j) - f(-j) + 2 f] / (2 h^2), error O(h^2) like the diagonal's."""
    n = len(z)
    f0 = fun(z)
    fp, fm = [], []
    for i in range(n):
        zp = list(z); zp[i] = z[i] + h; fp.append(fun(zp))
        zp[i] = z[i] - h; fm.append(fun(zp))
    g = [(fp[i] - fm[i]) / (2 * h) for i in range(n)]
    H = [[mpf(0)] * n for _ in range(n)]
    for i in range(n):
        H[i][i] = (fp[i] - 2 * f0 + fm[i]) / (h * h)
        for j in range(i + 1, n):
            zp = list(z); zp[i] = z[i] + h; zp[j] = z[j] + h; fpp = fun(zp)
            zp[i] = z[i] - h; zp[j] = z[j] - h; fmm = fun(zp)
            H[i][j] = H[j][i] = (fpp + fmm - fp[i] - fm[i] - fp[j] - fm[j] + 2 * f0) / (2 * h * h)
    return f0, g, H


def jacobian(fun, z, h):
    """(values, Jacobian rows) of the vector fun at z by central differences"""
    v0 = fun(z)
    J = [[mpf(0)] * len(z) for _ in v0]
    for i in range(len(z)):
        zp = list(z); zp[i] = z[i] + h; vp = fun(zp)
        zp[i] = z[i] - h; vm = fun(zp)
        for r in range(len(v0)):
            J[r][i] = (vp[r] - vm[r]) / (2 * h)
    return v0, J


def _f64(a, raw=False):
    """nested lists of mpf as a float64 array (raw: as an object array of the mpf values themselves, for the reference's own accuracy test)"""
    if raw:
        out = np.empty((len(a), len(a[0])) if a and isinstance(a[0], list) else (len(a),), object)
        out[...] = a
        return out
    return np.array([[float(v) for v in row] for row in a], float) if a and isinstance(a[0], list) else np.array([float(v) for v in a], float)


def _shifted(bound, c, raw=False):
    """bound - c in the working precision; an infinite bound stays infinite"""
    num = (lambda v: v) if raw else float
    return np.array([b if np.isinf(b) else num(mpf(float(b)) - v) for b, v in zip(np.asarray(bound, float), c)], object if raw else float)


# ------------------------------------------------------------------------------------------------ stage problems
class Stage:
    """the restatement of one stage model.  theta [B, ntheta], plant [B, ntheta] and sdata [B, N, nsd] are the rows in force (None: the model's
    shared values).  Every method takes batched float64 arrays and works instance by instance."""

    def __init__(self, mdl, theta=None, sdata=None, plant=None, dps=DPS, step=STEP, whole=None, raw=False):
        self.mdl, self.dps, self.step = mdl, int(dps), step
        self.raw = bool(raw)       # system, merit and convexify return object arrays of mpf, not float64: what the reference holds before rounding
        self.N, self.nx, self.nu = int(mdl.N), int(mdl.nx), int(mdl.nu)
        self.nh, self.nk = int(mdl.nh), int(mdl.nk)
        self.pf = bool(mdl.per_frame_reference)
        N, nx = self.N, self.nx
        self.f = nx + self.nu
        self.np = N * nx if self.pf else nx
        self.nvar = N * self.f
        self.n = self.np + self.nvar
        self.ng = (N - 1) * nx + N * self.nh + (N - 1) * self.nk
        self.m = self.n + self.ng
        self.whole = (self.n <= WHOLE_MAX) if whole is None else bool(whole)
        self.theta = None if theta is None else np.asarray(theta, float)
        self.plant = self.theta if plant is None else np.asarray(plant, float)
        self.sdata = None if sdata is None else np.asarray(sdata, float)
        self.general = getattr(mdl, "lcost", None) is not None
        self.has_lterm = self.general and getattr(mdl, "lterm", None) is not None
        self.has_link = getattr(mdl, "llink", None) is not None
        self._hess = {}        # frame Hessians by instance, frame and point: `system` (term by term) and `convexify` difference each one once

    def _num(self, v):
        return v if self.raw else float(v)

    # -- the model of one instance, the callbacks on one frame --------------------------------------
    def _model(self, b, plant=False):
        m = copy.copy(self.mdl)
        rows = self.plant if plant else self.theta
        if rows is not None:
            m.theta = rows[b].copy()
        return m

    def _data(self, m, b, k):
        if self.sdata is not None:
            m.sdata = self.sdata[b, k].copy()

    def _frame(self, m, b, k, z, terminal=None):
        """the frame term of frame k at z = [s; u; r] (mpf)"""
        nx, f = self.nx, self.f
        s, u, r = _vec(z[:nx]), _vec(z[nx:f]), _vec(z[f:])
        self._data(m, b, k)
        if self.general:
            last = (k == self.N - 1) if terminal is None else terminal
            return _scalar((m.lterm if last and self.has_lterm else m.lcost)(s, u, r))
        v = mpf(0)
        for i in range(nx):
            e = z[i] - z[f + i]
            v += mpf(float(m.Qk[k, i])) * e * e
        for i in range(self.nu):
            v += mpf(float(m.Rk[k, i])) * z[nx + i] * z[nx + i]
        return v

    def _frame_hess(self, m, b, k, z, h):
        """(value, gradient, Hessian) of the frame term of frame k at z, remembered"""
        key = (b, k, tuple(z))
        if key not in self._hess:
            self._hess[key] = grad_hess(lambda v: self._frame(m, b, k, v), z, h)
        return self._hess[key]

    def _link(self, m, z):
        nx, f = self.nx, self.f
        return _scalar(m.llink(_vec(z[:nx]), _vec(z[nx:f]), _vec(z[f:f + nx]), _vec(z[f + nx:])))

    def _dyn(self, m, z):
        """s_next - F(s, u) at z = [s; u; s_next]"""
        nx, f = self.nx, self.f
        Fv = _list(m.F(_vec(z[:nx]), _vec(z[nx:f])))
        return [z[f + i] - Fv[i] for i in range(nx)]

    def _path(self, m, b, k, z):
        self._data(m, b, k)
        return _list(m.hfun(_vec(z[:self.nx]), _vec(z[self.nx:])))

    def _klink(self, m, z):
        nx, f = self.nx, self.f
        return _list(m.kfun(_vec(z[:nx]), _vec(z[nx:f]), _vec(z[f:f + nx]), _vec(z[f + nx:])))

    # -- where everything lies in w: the restatement's own index arithmetic ------------------------------
    def _x_idx(self, k):
        return [self.np + k * self.f + c for c in range(self.f)]

    def _r_idx(self, k):
        return [(k * self.nx if self.pf else 0) + i for i in range(self.nx)]

    def _frame_idx(self, k):
        return self._x_idx(k) + self._r_idx(k)

    def _pair_idx(self, k):
        return self._x_idx(k) + self._x_idx(k + 1)

    # -- f and g of the whole vector ---------------------------------------------------------------
    def _cost_terms(self, m, b):
        """[(function of its own arguments, their indices in w, the frame or None for a link term)]"""
        terms = [(lambda z, k=k: self._frame(m, b, k, z), self._frame_idx(k), k) for k in range(self.N)]
        if self.has_link:
            terms += [(lambda z: self._link(m, z), self._pair_idx(k), None) for k in range(self.N - 1)]
        return terms

    def _row_terms(self, m, b):
        """[(vector function of its own arguments, their indices in w)] in row order: dynamics, path, link"""
        N, nx = self.N, self.nx
        terms = [(lambda z: self._dyn(m, z), self._x_idx(k) + self._x_idx(k + 1)[:nx]) for k in range(N - 1)]
        if self.nh:
            terms += [(lambda z, k=k: self._path(m, b, k, z), self._x_idx(k)) for k in range(N)]
        if self.nk:
            terms += [(lambda z: self._klink(m, z), self._pair_idx(k)) for k in range(N - 1)]
        return terms

    def _f(self, m, b, w):
        return sum((fn([w[i] for i in idx]) for fn, idx, _ in self._cost_terms(m, b)), mpf(0))

    def _g(self, m, b, w):
        out = []
        for fn, idx in self._row_terms(m, b):
            out += fn([w[i] for i in idx])
        return out

    def _w(self, p, x, b):
        return _mpfs(p[b]) + _mpfs(x[b])

    # -- the local system ---------------------------------------------------------------------------
    @_hp
    def system(self, p, x, lbx, ubx, lbg, ubg):
        """dict of float64 arrays: P [B, n, n], q [B, n], A [B, m, n], l, u [B, m], f [B], g [B, ng]"""
        B = np.shape(x)[0]
        n, m_ = self.n, self.m
        h = mpf(self.step)
        raw, num = self.raw, self._num
        dt = object if raw else float
        out = dict(P=np.zeros((B, n, n), dt), q=np.zeros((B, n), dt), A=np.zeros((B, m_, n), dt), l=np.zeros((B, m_), dt), u=np.zeros((B, m_), dt),
                   f=np.zeros(B, dt), g=np.zeros((B, self.ng), dt))
        for b in range(B):
            mdl = self._model(b)
            w = self._w(p, x, b)
            if self.whole:
                f0, gr, H = grad_hess(lambda z: self._f(mdl, b, z), w, h)
                gv, J = jacobian(lambda z: self._g(mdl, b, z), w, h)
                out["P"][b] = _f64(H, raw); out["q"][b] = _f64(gr, raw)
                if self.ng:
                    out["A"][b, n:] = _f64(J, raw)
            else:
                f0 = mpf(0)
                q = [mpf(0)] * n
                Pm = [[mpf(0)] * n for _ in range(n)]
                for fn, idx, k in self._cost_terms(mdl, b):
                    z = [w[i] for i in idx]
                    ft, gr, H = grad_hess(fn, z, h) if k is None else self._frame_hess(mdl, b, k, z, h)
                    f0 += ft
                    for a, i in enumerate(idx):
                        q[i] += gr[a]
                        for c, j in enumerate(idx):
                            Pm[i][j] += H[a][c]
                out["P"][b] = _f64(Pm, raw); out["q"][b] = _f64(q, raw)
                gv = []
                row = n
                for fn, idx in self._row_terms(mdl, b):
                    v, J = jacobian(fn, [w[i] for i in idx], h)
                    gv += v
                    for r in range(len(v)):
                        for a, i in enumerate(idx):
                            out["A"][b, row + r, i] = num(J[r][a])
                    row += len(v)
            out["A"][b, :n] = np.eye(n)
            c = w + gv
            lo = np.concatenate([np.asarray(p[b], float), np.asarray(lbx[b], float), np.asarray(lbg[b], float)])
            hi = np.concatenate([np.asarray(p[b], float), np.asarray(ubx[b], float), np.asarray(ubg[b], float)])
            out["l"][b] = _shifted(lo, c, raw); out["u"][b] = _shifted(hi, c, raw)
            out["f"][b] = num(f0); out["g"][b] = _f64(gv, raw) if gv else np.zeros(0)
        return out

    # -- bounds of the general rows, from the model's plain attributes --------------------------------
    def row_bounds(self):
        """(lbg, ubg) [ng]: zero on the dynamics rows, h_lo / h_hi per frame (one row for every frame or one per frame), k_lo / k_hi per stage"""
        N, nx = self.N, self.nx
        lo, hi = [np.zeros((N - 1) * nx)], [np.zeros((N - 1) * nx)]
        if self.nh:
            lo.append(np.broadcast_to(np.asarray(self.mdl.h_lo, float), (N, self.nh)).ravel())
            hi.append(np.broadcast_to(np.asarray(self.mdl.h_hi, float), (N, self.nh)).ravel())
        if self.nk:
            lo.append(np.broadcast_to(np.asarray(self.mdl.k_lo, float), (N - 1, self.nk)).ravel())
            hi.append(np.broadcast_to(np.asarray(self.mdl.k_hi, float), (N - 1, self.nk)).ravel())
        return np.concatenate(lo), np.concatenate(hi)

    def _merit(self, mdl, b, w, lbx, ubx):
        """(f, l1, gmax, per-row violations [nvar + ng]) in mpf: rows outside their bounds; an infinite bound contributes nothing; no box rows in gmax"""
        f0 = self._f(mdl, b, w)
        gv = self._g(mdl, b, w)
        lo, hi = self.row_bounds()
        rows = []
        gmax = mpf(0)
        for v, a, c in zip(gv, lo, hi):
            below = mpf(0) if np.isinf(a) else max(mpf(float(a)) - v, mpf(0))
            above = mpf(0) if np.isinf(c) else max(v - mpf(float(c)), mpf(0))
            rows.append(below + above)
            gmax = max(gmax, below, above)
        box = []
        for v, a, c in zip(w[self.np:], np.asarray(lbx, float), np.asarray(ubx, float)):
            below = mpf(0) if np.isinf(a) else max(mpf(float(a)) - v, mpf(0))
            above = mpf(0) if np.isinf(c) else max(v - mpf(float(c)), mpf(0))
            box.append(below + above)
        return f0, sum(rows, mpf(0)) + sum(box, mpf(0)), gmax, box + rows

    @_hp
    def merit(self, p, x, lbx, ubx, mu=None):
        """dict of float64: f, l1, gmax [B], rows [B, nvar + ng] (the violation of every box and general row), phi = f + mu l1 when mu [B] is given"""
        B = np.shape(x)[0]
        raw, num = self.raw, self._num
        dt = object if raw else float
        out = dict(f=np.zeros(B, dt), l1=np.zeros(B, dt), gmax=np.zeros(B, dt), rows=np.zeros((B, self.nvar + self.ng), dt))
        if mu is not None:
            out["phi"] = np.zeros(B, dt)
        for b in range(B):
            f0, l1, gmax, rows = self._merit(self._model(b), b, self._w(p, x, b), lbx[b], ubx[b])
            out["f"][b], out["l1"][b], out["gmax"][b] = num(f0), num(l1), num(gmax)
            out["rows"][b] = _f64(rows, raw)
            if mu is not None:
                out["phi"][b] = num(f0 + mpf(float(mu[b])) * l1)
        return out

    @_hp
    def line_search(self, p, x, lbx, ubx, q, dw, y, status=None, mu=None, alpha0=1.0, candidates=4, beta=0.5, c1=1e-4, mu_min=1.0, mu_factor=1.1):
        """the l1-merit backtracking search of mpcqp_stage_linesearch, every candidate evaluated and the Armijo test decided in the working
        precision.  mu_b = max(mu[b], mu_min, mu_factor max_{i >= np} |y_i|), phi = f + mu_b l1, D = min(0, q[np:]' dx - mu_b l1(x)); the first
        alpha_j = alpha0 beta^j with phi_j finite and phi_j <= phi_0 + c1 alpha_j D is taken (accepted = j); none: the last candidate when its
        merit is finite (-1); an instance whose status is not in OK keeps x (-2, alpha 0, its mu stays).  The candidates x + alpha_j dx are formed
        in float64, as the caller's x is.  Returns float64 arrays: accepted, alpha, mu [B], phis, fs, gmaxs [B, K + 1] (base point first) and
        margin [B, K] = |phi_j - (phi_0 + c1 alpha_j D)|."""
        B, K, npp = np.shape(x)[0], int(candidates), self.np
        alphas = np.empty(K); alphas[0] = alpha0
        for j in range(1, K):
            alphas[j] = alphas[j - 1] * beta
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), OK)
        out = dict(accepted=np.full(B, -2, np.int64), alpha=np.zeros(B), mu=np.zeros(B), alphas=alphas, phis=np.full((B, K + 1), np.nan),
                   fs=np.full((B, K + 1), np.nan), gmaxs=np.full((B, K + 1), np.nan), margin=np.full((B, K), np.nan), phi0=np.zeros(B))
        for b in range(B):
            mub = float(mu_min) if mu is None else max(float(mu_min), float(mu[b]))
            mdl = self._model(b)
            f0, v0, g0, _ = self._merit(mdl, b, self._w(p, x, b), lbx[b], ubx[b])
            if ok[b]:
                mub = max(mub, float(mu_factor) * float(np.abs(np.asarray(y[b], float)[npp:]).max(initial=0.0)))
            out["mu"][b] = mub
            phi0 = f0 + mpf(mub) * v0
            out["phis"][b, 0], out["fs"][b, 0], out["gmaxs"][b, 0], out["phi0"][b] = float(phi0), float(f0), float(g0), float(phi0)
            if not ok[b]:
                continue
            dx = np.asarray(dw[b], float)[npp:]
            D = sum((mpf(float(a)) * mpf(float(c)) for a, c in zip(np.asarray(q[b], float)[npp:], dx)), mpf(0)) - mpf(mub) * v0
            D = min(D, mpf(0))
            taken = None
            for j in range(K):
                xc = np.asarray(x[b], float) + alphas[j] * dx
                fj, vj, gj, _ = self._merit(mdl, b, _mpfs(p[b]) + _mpfs(xc), lbx[b], ubx[b])
                phij = fj + mpf(mub) * vj
                thr = phi0 + mpf(float(c1)) * mpf(float(alphas[j])) * D
                out["phis"][b, j + 1], out["fs"][b, j + 1], out["gmaxs"][b, j + 1] = float(phij), float(fj), float(gj)
                out["margin"][b, j] = float(abs(phij - thr))
                if taken is None and np.isfinite(float(phij)) and phij <= thr:
                    taken = j
            if taken is not None:
                out["accepted"][b], out["alpha"][b] = taken, alphas[taken]
            elif np.isfinite(out["phis"][b, K]):
                out["accepted"][b], out["alpha"][b] = -1, alphas[K - 1]
        return out

    # -- convexification --------------------------------------------------------------------------------
    @_hp
    def convexify(self, p, x, P, mode="project", eps=1e-6):
        """P [B, n, n] (dense, as `system` returned it) -> dict P [B, n, n], touched [B], lam_min [B, N], hnorm [B, N].  H_k: the frame term's
        Hessian over [s_k; u_k; r_k]; a frame with lam_min(H_k) < eps adds D_k = sum_{lam_j < eps} (f(lam_j) - lam_j) v_j v_j', f = max(lam, eps)
        (project) or max(|lam|, eps) (mirror), at its indices of w -- a shared reference's p-p block so takes the sum over the touched frames."""
        B, N = np.shape(x)[0], self.N
        h = mpf(self.step)
        e = mpf(float(eps))
        num = self._num
        dt = object if self.raw else float
        out = dict(P=np.array(P, dt), touched=np.zeros(B, np.int64), lam_min=np.zeros((B, N), dt), hnorm=np.zeros((B, N)))
        for b in range(B):
            mdl = self._model(b)
            w = self._w(p, x, b)
            add = {}
            for k in range(N):
                idx = self._frame_idx(k)
                _, _, H = self._frame_hess(mdl, b, k, [w[i] for i in idx], h)
                nl = len(idx)
                E, Q = mp.eigsy(mp.matrix(H))
                lam = [E[j] for j in range(nl)]
                out["lam_min"][b, k] = num(min(lam))
                out["hnorm"][b, k] = float(mp.sqrt(sum((H[i][j] ** 2 for i in range(nl) for j in range(nl)), mpf(0))))
                if not min(lam) < e:
                    continue
                out["touched"][b] += 1
                for j in range(nl):
                    if lam[j] < e:
                        t = max(abs(lam[j]) if mode == "mirror" else lam[j], e) - lam[j]
                        for r in range(nl):
                            for c in range(nl):
                                add[(idx[r], idx[c])] = add.get((idx[r], idx[c]), mpf(0)) + t * Q[r, j] * Q[c, j]
            for (i, j), v in add.items():
                out["P"][b, i, j] = num(_raw(out["P"][b, i, j]) + v)
        return out

    # -- the hand-over between two ticks ----------------------------------------------------------------
    @_hp
    def advance(self, x, p, status=None, s_meas=None, w=None, tail="rollout"):
        """dict of float64: applied [B, f] = frame 0; x [B, nvar]: frame 0 = [the measured state when given, else the plant step F(s_0, u_0) under
        the plant's parameters (+ w); u_1 where the QP returned a point, else u_0], frames 1 .. N-2 = the old frames 2 .. N-1, the last frame the
        old last one with (tail = rollout) its state F(s_{N-1}, u_{N-1}) under the model's parameters; stage_cost = the frame term of frame 0
        (never the terminal one) at the reference of frame 0 and the data row of frame 0."""
        B, N, nx, f = np.shape(x)[0], self.N, self.nx, self.f
        ok = np.ones(B, bool) if status is None else np.isin(np.asarray(status), OK)
        X = np.asarray(x, float).reshape(B, N, f)
        out = dict(applied=X[:, 0].copy(), x=np.zeros((B, N, f)), stage_cost=np.zeros(B))
        for b in range(B):
            z0 = _mpfs(X[b, 0])
            if s_meas is not None:
                out["x"][b, 0, :nx] = np.asarray(s_meas, float)[b]
            else:
                nxt = _list(self._model(b, plant=True).F(_vec(z0[:nx]), _vec(z0[nx:])))
                if w is not None:
                    nxt = [v + mpf(float(d)) for v, d in zip(nxt, np.asarray(w, float)[b])]
                out["x"][b, 0, :nx] = _f64(nxt)
            out["x"][b, 0, nx:] = X[b, 1, nx:] if ok[b] else X[b, 0, nx:]
            out["x"][b, 1:N - 1] = X[b, 2:]
            out["x"][b, N - 1] = X[b, N - 1]
            mdl = self._model(b)
            if tail == "rollout":
                zl = _mpfs(X[b, N - 1])
                out["x"][b, N - 1, :nx] = _f64(_list(mdl.F(_vec(zl[:nx]), _vec(zl[nx:]))))
            r0 = _mpfs(np.asarray(p, float)[b, :nx])
            out["stage_cost"][b] = float(self._frame(mdl, b, 0, z0 + r0, terminal=False))
        out["x"] = out["x"].reshape(B, -1)
        return out


# ------------------------------------------------------------------------------------------------ general problems
class General:
    """the restatement of a general (non-stage) problem from its plain callables f(w) and g(w) (g None: no general rows), w = [p; x]; always
    differenced over the whole of w"""

    def __init__(self, cost, constraints, nvar, npar, dps=DPS, step=STEP):
        self.cost, self.cons, self.nvar, self.np = cost, constraints, int(nvar), int(npar)
        self.n = self.nvar + self.np
        self.dps, self.step = int(dps), step

    def _f(self, z):
        return _scalar(self.cost(_vec(z)))

    def _g(self, z):
        return _list(self.cons(_vec(z))) if self.cons is not None else []

    @_hp
    def system(self, p, x, lbx, ubx, lbg, ubg):
        """as Stage.system, plus gmax [B] = the largest violation of lbg <= g <= ubg (0 when there is none)"""
        B, n = np.shape(x)[0], self.n
        h = mpf(self.step)
        out = None
        for b in range(B):
            w = _mpfs(p[b]) + _mpfs(x[b])
            f0, gr, H = grad_hess(self._f, w, h)
            gv, J = jacobian(self._g, w, h)
            if out is None:
                ng = len(gv)
                out = dict(P=np.zeros((B, n, n)), q=np.zeros((B, n)), A=np.zeros((B, n + ng, n)), l=np.zeros((B, n + ng)), u=np.zeros((B, n + ng)),
                           f=np.zeros(B), gmax=np.zeros(B))
            out["P"][b] = _f64(H); out["q"][b] = _f64(gr); out["A"][b, :n] = np.eye(n)
            if gv:
                out["A"][b, n:] = _f64(J)
            c = w + gv
            lo = np.concatenate([np.asarray(p[b], float), np.asarray(lbx[b], float), np.asarray(lbg[b], float)])
            hi = np.concatenate([np.asarray(p[b], float), np.asarray(ubx[b], float), np.asarray(ubg[b], float)])
            out["l"][b] = _shifted(lo, c); out["u"][b] = _shifted(hi, c)
            out["f"][b] = float(f0)
            gmax = mpf(0)
            for v, a, c_ in zip(gv, np.asarray(lbg[b], float), np.asarray(ubg[b], float)):
                if not np.isinf(a): gmax = max(gmax, mpf(float(a)) - v)
                if not np.isinf(c_): gmax = max(gmax, v - mpf(float(c_)))
            out["gmax"][b] = float(gmax)
        return out


# ------------------------------------------------------------------------------------------------ helpers of the tests
def dense(Pp, Pi, vals, rows):
    """(dense matrix [rows, n], bool mask of the pattern) of one instance's CSC values"""
    n = len(Pp) - 1
    D = np.zeros((rows, n)); M = np.zeros((rows, n), bool)
    for j in range(n):
        sl = slice(Pp[j], Pp[j + 1])
        D[Pi[sl], j] = vals[sl]; M[Pi[sl], j] = True
    return D, M


def raw_distance(got, ref):
    """`distance` for the object arrays of a raw restatement, in mpmath's arithmetic"""
    with mp.workdps(4 * DPS):
        worst = mpf(0)
        for a, b in zip(np.asarray(got, object).ravel(), np.asarray(ref, object).ravel()):
            if not (np.isfinite(float(a)) and np.isfinite(float(b))):
                if not float(a) == float(b):
                    return np.inf
                continue
            worst = max(worst, abs(_raw(a) - _raw(b)) / max(mpf(1), abs(_raw(b))))
        return float(worst)


def distance(got, ref):
    """the largest |got - ref| / max(1, |ref|) over the finite entries of ref; inf where the non-finite patterns differ"""
    got = np.asarray(got, float); ref = np.asarray(ref, float)
    fin = np.isfinite(ref)
    if got.shape != ref.shape or not np.array_equal(got[~fin], ref[~fin]) or not np.isfinite(got[fin]).all():
        return np.inf
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max(initial=0.0))
