"""GeneralEvaluator: getLocalSystem on the GPU for a general (non-stage) NLP (include/mpcqp.h, mpcqp_nlp_*).

general_nlp.GeneralNLP evaluates the local system of ANY problem on the host -- the gradient tape once, then one complex-step pass per
Hessian and Jacobian column (reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77,100-120 does the same with CasADi's compiled
function).  Here the same tapes are emitted as one scalar-generic functor (codegen.emit_general), compiled for gfx950 and run by the
kernels of csrc/general_kernels.hpp: forward-mode duals over the reverse-derived gradient for the Hessian, over the constraints for the
Jacobian.

Compression by colouring.  A pass per column would cost O(n) evaluations per instance.  The columns of a structure matrix are
partitioned into colours such that no two columns of a colour share a structurally non-zero row (greedy, in column order, on the full
symmetric pattern for the Hessian; columns without an entry get no colour).  A pass seeds the dual part 1.0 on every input of its
colour; the dual part of output row r is then exactly the entry (r, c) of the ONE column c of that colour that has row r: direct
recovery.  slot[pass][r] names the CSC value slot of that entry (-1: none) in the order GeneralNLP.Pp / Pi / Ap / Ai define."""
import ctypes as C
from ctypes import byref as _byref      # (GeneralEvaluator.lagrangian has an argument named C, the workspace of the C entry)

import numpy as np

from . import _lib


def colour_columns(mask):
    """greedy distance-1 colouring of the columns of a boolean structure matrix [rows, cols]: (colour [cols] with -1 for a column without
    entries, number of colours).  No two columns of one colour share a row."""
    mask = np.asarray(mask, bool)
    rows, cols = mask.shape
    colour = np.full(cols, -1, np.int32)
    used = []                                   # used[c]: rows taken by the columns of colour c
    for j in range(cols):
        col = mask[:, j]
        if not col.any():
            continue
        for c, taken in enumerate(used):
            if not (taken & col).any():
                taken |= col; colour[j] = c
                break
        else:
            used.append(col.copy()); colour[j] = len(used) - 1
    return colour, len(used)


def slot_table(mask, colour, ncolours, colptr, first=0):
    """slot[pass, r]: CSC value slot of entry (r, c), c the column of colour `pass` with row r, else -1.  colptr: the CSC column
    pointers; `first`: entries of the column that precede this block's rows (the identity entry of A)"""
    mask = np.asarray(mask, bool)
    rows, cols = mask.shape
    slot = np.full((max(ncolours, 0), rows), -1, np.int32)
    for j in range(cols):
        if colour[j] < 0:
            continue
        r = np.nonzero(mask[:, j])[0]
        slot[colour[j], r] = int(colptr[j]) + first + np.arange(len(r))
    return slot


def compress(model):
    """colours and slot tables of a general_nlp.GeneralNLP.  hp >= 1 (pass 0 also writes the gradient, whether or not the Hessian has an
    entry); jp = 0 without general rows, else >= 1 (pass 0 also writes their bounds)"""
    n, ng = model.n, model.ng
    hcol, nh = colour_columns(model.hm)
    hp = max(nh, 1)
    hslot = np.full((hp, n), -1, np.int32); hslot[:nh] = slot_table(model.hm, hcol, nh, model.Pp)
    jm = model.am[n:]
    jcol, nj = colour_columns(jm) if ng else (np.full(n, -1, np.int32), 0)
    jp = max(nj, 1) if ng else 0
    jslot = np.full((jp, ng), -1, np.int32)
    if ng:
        jslot[:nj] = slot_table(jm, jcol, nj, model.Ap, first=1)
    c = dict(hcol=hcol, jcol=jcol, hp=hp, jp=jp, hslot=hslot, jslot=jslot, hcolours=nh, jcolours=nj)
    if getattr(model, "exact_hessian", False):
        c.update(compress_curvature(model))
    return c


def compress_curvature(model):
    """the tables of mpcqp_nlp_lagrangian for a model built with exact_hessian=True: ccol / cp colour the columns of the curvature's structure cm
    (cp = 0: no curvature, the call is a no-op); cslot[pass, r] is the slot of entry (r, c) in P's widened CSC, c the column of colour `pass`
    with row r in cm, else -1.  For the apply kernel's walk over a column: ccols, the columns with curvature; cptr / clist, their curvature
    slots in ascending order; cdiag, the slot of each one's diagonal entry"""
    n = model.n
    ccol, cp = colour_columns(model.cm)
    rank = np.cumsum(model.hm, axis=0) - 1                 # position of row r among the entries of its column of P
    cslot = np.full((cp, n), -1, np.int32)
    ccols = np.nonzero(ccol >= 0)[0].astype(np.int32)
    cptr = [0]; clist = []; cdiag = []
    for j in ccols:
        r = np.nonzero(model.cm[:, j])[0]
        slots = int(model.Pp[j]) + rank[r, j]
        cslot[ccol[j], r] = slots
        clist += [int(v) for v in slots]; cptr.append(len(clist))
        cdiag.append(int(model.Pp[j]) + int(rank[j, j]))
    return dict(ccol=ccol, cp=cp, cslot=cslot, ccols=ccols, cptr=np.array(cptr, np.int32), clist=np.array(clist, np.int32),
                cdiag=np.array(cdiag, np.int32))


class LineSearchArgs(C.Structure):
    """mpcqp_nlp_linesearch_args (include/mpcqp.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg", "q", "dw", "y", "status", "mu", "alpha_out", "accepted", "step_max",
                                          "f_out", "gmax_out", "phi")] + \
               [(k, C.c_double) for k in ("alpha0", "beta", "c1", "mu_min", "mu_factor")] + [("candidates", C.c_int)]


class LagrangianArgs(C.Structure):
    """mpcqp_nlp_lagrangian_args (include/mpcqp.h)"""
    _fields_ = [(k, C.c_void_p) for k in ("p", "x", "y", "status", "P", "C")] + [("mode", C.c_int), ("shift", C.c_void_p)]


def _bind(L):
    if getattr(L, "_nlp_bound", False):
        return L
    vp = C.c_void_p
    L.mpcqp_nlp_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.mpcqp_nlp_destroy.argtypes = [vp]
    L.mpcqp_nlp_destroy.restype = None
    L.mpcqp_nlp_dims.argtypes = [vp, vp]
    L.mpcqp_nlp_pattern.argtypes = [vp, vp, vp, vp, vp]
    L.mpcqp_nlp_eval.argtypes = [vp, C.c_int] + [vp] * 11 + [vp]
    L.mpcqp_nlp_merit.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.mpcqp_nlp_step.argtypes = [vp, C.c_int, C.c_double, vp, vp, vp, vp, vp]
    L.mpcqp_nlp_has_linesearch.argtypes = [vp]
    L.mpcqp_nlp_linesearch.argtypes = [vp, C.c_int, C.POINTER(LineSearchArgs), vp]
    L.mpcqp_nlp_has_exact_hessian.argtypes = [vp]
    L.mpcqp_nlp_lagrangian.argtypes = [vp, C.c_int, C.POINTER(LagrangianArgs), vp]
    L.mpcqp_nlp_kkt.argtypes = [vp, C.c_int, vp, vp]
    L._nlp_bound = True
    return L


def _check(t, shape, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError("%s: expected a contiguous float64 CUDA tensor" % name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s (dimension mismatch)" % (name, tuple(shape), tuple(t.shape)))
    return t.data_ptr() or None                 # (an array without elements -- np = 0, ng = 0 -- has no address)


def _check_int32(t, B, name):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (B,)):
        raise ValueError("%s: expected a contiguous int32 CUDA tensor of shape (%d,)" % (name, B))
    return t.data_ptr()


class GeneralEvaluator:
    """the surface of stage_eval.StageEvaluator the device SQP loop uses, for a general_nlp.GeneralNLP.  library: the generated
    gfx950 library (codegen.build_general_device_library; codegen.TapeTooLarge when the problem is refused).  line_search=False builds the
    library without the line-search kernel (has_line_search is then False); ignored when `library` is given.  A model built with
    exact_hessian=True gives a library with the curvature kernels (has_exact_hessian, lagrangian)"""

    def __init__(self, model, device=-1, cap=None, library=None, line_search=True):
        from . import codegen
        self.model = model
        self.library = library if library is not None else codegen.build_general_device_library(model, cap=cap, line_search=line_search)
        L = _bind(_lib.lib())
        self._h = C.c_void_p()
        _lib.check(L.mpcqp_nlp_create(self.library.encode(), int(device), C.byref(self._h)))
        dims = np.zeros(8, np.int32)
        _lib.check(L.mpcqp_nlp_dims(self._h, dims.ctypes.data))
        self.nvar, self.np, self.ng, self.n, self.m, self.nnzP, self.nnzA, self.passes = [int(v) for v in dims]
        self.Pp = np.zeros(self.n + 1, np.int32); self.Pi = np.zeros(self.nnzP, np.int32)
        self.Ap = np.zeros(self.n + 1, np.int32); self.Ai = np.zeros(self.nnzA, np.int32)
        _lib.check(L.mpcqp_nlp_pattern(self._h, self.Pp.ctypes.data, self.Pi.ctypes.data, self.Ap.ctypes.data, self.Ai.ctypes.data))
        self._bounds = None
        self.has_line_search = bool(L.mpcqp_nlp_has_linesearch(self._h))      # the library exports mpcqp_general_linesearch
        self.has_exact_hessian = bool(L.mpcqp_nlp_has_exact_hessian(self._h))  # ... and mpcqp_general_lagrangian (a model with exact_hessian=True)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().mpcqp_nlp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, batch, device="cuda"):
        """output buffers of one evaluation: dict P, q, A, l, u"""
        import torch
        mk = lambda w: torch.empty((batch, w), dtype=torch.float64, device=device)
        return dict(P=mk(self.nnzP), q=mk(self.n), A=mk(self.nnzA), l=mk(self.m), u=mk(self.m))

    def eval(self, p, x, lbx, ubx, lbg, ubg, out=None, stream=None):
        B = x.shape[0]
        if out is None:
            out = self.alloc(B, x.device)
        args = [_check(p, (B, self.np), "p"), _check(x, (B, self.nvar), "x"), _check(lbx, (B, self.nvar), "lbx"),
                _check(ubx, (B, self.nvar), "ubx"), _check(lbg, (B, self.ng), "lbg"), _check(ubg, (B, self.ng), "ubg"),
                _check(out["P"], (B, self.nnzP), "P"), _check(out["q"], (B, self.n), "q"), _check(out["A"], (B, self.nnzA), "A"),
                _check(out["l"], (B, self.m), "l"), _check(out["u"], (B, self.m), "u")]
        _lib.check(_lib.lib().mpcqp_nlp_eval(self._h, B, *args, stream))
        self._bounds = (lbg, ubg)
        return out

    def merit(self, p, x, stream=None, lbg=None, ubg=None):
        """objective f [B] and the max-norm violation of lbg <= g <= ubg [B]; the bounds are those of the last eval unless given"""
        import torch
        B = x.shape[0]
        if lbg is None or ubg is None:
            if self._bounds is None:
                raise ValueError("merit needs the constraint bounds: give lbg and ubg, or call eval first")
            lbg, ubg = self._bounds
        f = torch.empty(B, dtype=torch.float64, device=x.device); g = torch.empty(B, dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().mpcqp_nlp_merit(self._h, B, _check(p, (B, self.np), "p"), _check(x, (B, self.nvar), "x"),
                                              _check(lbg, (B, self.ng), "lbg"), _check(ubg, (B, self.ng), "ubg"), f.data_ptr(), g.data_ptr(), stream))
        return f, g

    def step(self, alpha, dw, x, stream=None, status=None):
        """x += alpha * dw[:, np:] in place; returns max|alpha dx| per instance.  status (int32 CUDA tensor [B], optional):
        instances whose QP did not return a point keep their x"""
        import torch
        B = x.shape[0]
        sm = torch.empty(B, dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().mpcqp_nlp_step(self._h, B, float(alpha), _check(dw, (B, self.n), "dw"), _check(x, (B, self.nvar), "x"),
                                             sm.data_ptr(), None if status is None else status.data_ptr(), stream))
        return sm

    def line_search(self, p, x, lbx, ubx, q, dw, y, status=None, mu=None, alpha0=1.0, candidates=4, beta=0.5, c1=1e-4, mu_min=1.0, mu_factor=1.1,
                    out=None, phi=None, stream=None, lbg=None, ubg=None):
        """a per-instance step length by an l1-merit backtracking search, then x += alpha_b dx in place, in one kernel (mpcqp_nlp_linesearch;
        general_nlp.GeneralNLP.line_search is its host statement).  Replaces a step + merit pair: returns a dict of device tensors alpha, accepted
        (int32), step_max, f, gmax [B] (`out`: such a dict to write into) and phi [B, 2] when a tensor is given for it.  mu [B], when given, is the
        persistent penalty, updated in place.  The bounds of the general rows are those of the last eval unless given.  Arrays are contiguous
        float64 CUDA tensors (status, accepted: int32)."""
        import torch
        B = x.shape[0]
        if lbg is None or ubg is None:
            if self._bounds is None:
                raise ValueError("line_search needs the constraint bounds: give lbg and ubg, or call eval first")
            lbg, ubg = self._bounds
        a = LineSearchArgs()
        for name, t, w_ in (("p", p, self.np), ("x", x, self.nvar), ("lbx", lbx, self.nvar), ("ubx", ubx, self.nvar), ("lbg", lbg, self.ng),
                            ("ubg", ubg, self.ng), ("q", q, self.n), ("dw", dw, self.n), ("y", y, self.m)):
            setattr(a, name, _check(t, (B, w_), name))
        if out is None:
            out = {k: torch.empty(B, dtype=torch.float64, device=x.device) for k in ("alpha", "step_max", "f", "gmax")}
            out["accepted"] = torch.empty(B, dtype=torch.int32, device=x.device)
        for name, key in (("alpha_out", "alpha"), ("step_max", "step_max"), ("f_out", "f"), ("gmax_out", "gmax")):
            setattr(a, name, _check(out[key], (B,), key))
        for name, t in (("status", status), ("accepted", out["accepted"])):
            if t is not None:
                setattr(a, name, _check_int32(t, B, name))
        if mu is not None:
            a.mu = _check(mu, (B,), "mu")
        if phi is not None:
            a.phi = _check(phi, (B, 2), "phi")
            out["phi"] = phi
        a.alpha0, a.beta, a.c1, a.mu_min, a.mu_factor, a.candidates = float(alpha0), float(beta), float(c1), float(mu_min), float(mu_factor), int(candidates)
        _lib.check(_lib.lib().mpcqp_nlp_linesearch(self._h, B, C.byref(a), stream))
        return out

    MODES = {0: 0, 1: 1, "dominant": 1}    # mode 0; MPCQP_NLP_DOMINANT by its value or by the name the SQP option uses

    def lagrangian(self, p, x, y, P, status=None, mode=0, C=None, shift=None, stream=None):
        """P += C(w, y), the curvature of the constraints under the multipliers y [B, m], in place on the P of the last eval at the same (p, x)
        (mpcqp_nlp_lagrangian; general_nlp.GeneralNLP.lagrangian_system is its host statement).  mode 0 adds C; "dominant" (MPCQP_NLP_DOMINANT)
        adds the diagonal shift that keeps P at least the cost's Hessian, and needs the workspace C [B, nnzP].  shift [B, n], when given, receives
        the shift of the columns with curvature of the instances that are read (zero it beforehand).  status (int32 [B]): instances whose QP
        returned no point are neither read nor written.  Arrays are contiguous float64 CUDA tensors.  Returns P."""
        B = x.shape[0]
        if mode not in self.MODES:
            raise ValueError("mode must be 0 or 'dominant' (MPCQP_NLP_DOMINANT)")
        a = LagrangianArgs()
        for name, t, w_ in (("p", p, self.np), ("x", x, self.nvar), ("y", y, self.m), ("P", P, self.nnzP)):
            setattr(a, name, _check(t, (B, w_), name))
        if C is not None:
            a.C = _check(C, (B, self.nnzP), "C")
        if shift is not None:
            a.shift = _check(shift, (B, self.n), "shift")
        if status is not None:
            a.status = _check_int32(status, B, "status")
        a.mode = self.MODES[mode]
        _lib.check(_lib.lib().mpcqp_nlp_lagrangian(self._h, B, _byref(a), stream))
        return P

    def kkt(self, ls, y, tol=1e-3, out=None, frozen=None, stream=None):
        """the optimality residuals of every instance in one kernel (mpcqp_nlp_kkt; general_nlp.GeneralNLP.kkt_residuals is its host statement):
        ls the dict eval just wrote at the iterate, y [B, m] the multipliers of the last QP.  tol: a number or {stat, feas, compl}.  Returns
        (res [B, 4] = stat, feas, compl, scale; converged [B] int32), device tensors (`out`: such a pair to write into); frozen (int32 [B],
        optional): an instance with a nonzero entry is neither read nor written."""
        from .kkt import device_kkt
        return device_kkt(_lib.lib().mpcqp_nlp_kkt, self, ls, y, tol, out, frozen, stream)
