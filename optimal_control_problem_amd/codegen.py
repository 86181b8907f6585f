"""codegen: user-defined dynamics -> straight-line tape -> scalar-generic C++ functor -> gfx950 library.

The reference turns the CasADi local-system function into C source, compiles it with gcc and dlopens the result when
solver_settings.gen_code / load_lib are set (reference src/OptimalControlProblem.cpp:263-287,602-640).  CasADi is not
available here; the equivalent for this engine is:

1. trace(F, nx, nu): call the user's NumPy discrete map s_next = F(s, u) once on tracer objects; every arithmetic
   operation / NumPy ufunc lands on a tape in SSA form (common subexpressions merged, constants folded);
2. emit_functor(tape): the tape as a `template <class T> F(...)` functor in the form csrc/stage_models.hpp uses, so
   the evaluation kernels (csrc/stage_kernels.hpp) instantiate it with double (merit) and with one-direction dual
   numbers (Jacobian columns) exactly like the built-in zoo;
3. build_device_library(...): hipcc --offload-arch=gfx950 -shared, loaded by mpcqp_stage_create_user;
   build_host_library(...): the same functor compiled by g++ for CPU-side checks (tests, no GPU needed).

Supported inside F: + - * / ** (integer powers), unary -, np.sin cos tan exp log sqrt tanh square negative, indexing
s[..., i] / s[..., a:b], np.stack / np.concatenate along the last axis, Python and NumPy scalars as constants.
Data-dependent branches cannot be traced (the same restriction CasADi SX has)."""
import hashlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")

_UNARY = {"neg": "-", "sin": "sm_sin", "cos": "sm_cos", "tan": "sm_tan", "exp": "sm_exp", "log": "sm_log", "sqrt": "sm_sqrt", "tanh": "sm_tanh"}
_BINARY = {"add": "+", "sub": "-", "mul": "*", "div": "/"}
_NP_UNARY = {"neg": np.negative, "sin": np.sin, "cos": np.cos, "tan": np.tan, "exp": np.exp, "log": np.log, "sqrt": np.sqrt, "tanh": np.tanh}


class Tape:
    """SSA tape: nodes[i] = ("in", k) | ("const", value) | (unary, a) | (binary, a, b); outputs = node ids."""

    def __init__(self, n_in):
        self.n_in = n_in
        self.nodes = [("in", k) for k in range(n_in)]
        self._memo = {}
        self.outputs = []

    def const(self, v):
        return self._add(("const", float(v)))

    def _add(self, node):
        key = node if node[0] != "const" else ("const", np.float64(node[1]).tobytes())
        if key in self._memo:
            return self._memo[key]
        self.nodes.append(node)
        self._memo[key] = len(self.nodes) - 1
        return len(self.nodes) - 1

    def is_const(self, i):
        return self.nodes[i][0] == "const"

    def unary(self, op, a):
        if self.is_const(a):
            return self.const(_NP_UNARY[op](self.nodes[a][1]))
        return self._add((op, a))

    def binary(self, op, a, b):
        if self.is_const(a) and self.is_const(b):
            x, y = self.nodes[a][1], self.nodes[b][1]
            return self.const({"add": x + y, "sub": x - y, "mul": x * y, "div": x / y}[op])
        return self._add((op, a, b))

    # -- reference evaluation (NumPy, any dtype incl. complex): the checker for the generated code
    def evaluate(self, inputs):
        vals = [None] * len(self.nodes)
        for i, nd in enumerate(self.nodes):
            k = nd[0]
            if k == "in":
                vals[i] = inputs[nd[1]]
            elif k == "const":
                vals[i] = nd[1]
            elif k in _UNARY:
                vals[i] = _NP_UNARY[k](vals[nd[1]])
            else:
                a, b = vals[nd[1]], vals[nd[2]]
                vals[i] = a + b if k == "add" else a - b if k == "sub" else a * b if k == "mul" else a / b
        return [vals[o] for o in self.outputs]

    def live_nodes(self):
        """ids reachable from the outputs, in order"""
        need = set(); stack = list(self.outputs)
        while stack:
            i = stack.pop()
            if i in need:
                continue
            need.add(i)
            nd = self.nodes[i]
            if nd[0] in _UNARY:
                stack.append(nd[1])
            elif nd[0] in _BINARY:
                stack += [nd[1], nd[2]]
        return sorted(need)

    # -- simplifying constructors used by the symbolic differentiation (x + 0, x * 1, x * 0 ... fold away, so that a
    #    structurally zero derivative is the constant 0 and the Hessian's sparsity can be read off the tape)
    def _cv(self, i):
        return self.nodes[i][1] if self.is_const(i) else None

    def s_add(self, a, b):
        if self._cv(a) == 0.0: return b
        if self._cv(b) == 0.0: return a
        return self.binary("add", a, b)

    def s_sub(self, a, b):
        if self._cv(b) == 0.0: return a
        if self._cv(a) == 0.0: return self.s_neg(b)
        return self.binary("sub", a, b)

    def s_mul(self, a, b):
        for x, y in ((a, b), (b, a)):
            if self._cv(x) == 0.0: return self.const(0.0)
            if self._cv(x) == 1.0: return y
            if self._cv(x) == -1.0: return self.s_neg(y)
        return self.binary("mul", a, b)

    def s_div(self, a, b):
        if self._cv(a) == 0.0: return self.const(0.0)
        if self._cv(b) == 1.0: return a
        return self.binary("div", a, b)

    def s_neg(self, a):
        if self.nodes[a][0] == "neg": return self.nodes[a][1]
        return self.unary("neg", a)

    def partials(self, i):
        """[(argument, d node_i / d argument)] of node i as node ids (new nodes are appended)"""
        nd = self.nodes[i]; k = nd[0]
        one = self.const(1.0)
        if k in ("in", "const"): return []
        if k == "add": return [(nd[1], one), (nd[2], one)]
        if k == "sub": return [(nd[1], one), (nd[2], self.const(-1.0))]
        if k == "mul": return [(nd[1], nd[2]), (nd[2], nd[1])]
        if k == "div": return [(nd[1], self.s_div(one, nd[2])), (nd[2], self.s_neg(self.s_div(i, nd[2])))]
        a = nd[1]
        if k == "neg": return [(a, self.const(-1.0))]
        if k == "sin": return [(a, self.unary("cos", a))]
        if k == "cos": return [(a, self.s_neg(self.unary("sin", a)))]
        if k == "tan": return [(a, self.s_add(one, self.s_mul(i, i)))]
        if k == "exp": return [(a, i)]
        if k == "log": return [(a, self.s_div(one, a))]
        if k == "sqrt": return [(a, self.s_div(self.const(0.5), i))]
        if k == "tanh": return [(a, self.s_sub(one, self.s_mul(i, i)))]
        raise ValueError("no derivative rule for %s" % k)

    def clone(self):
        t = Tape(self.n_in)
        t.nodes = list(self.nodes); t._memo = dict(self._memo); t.outputs = list(self.outputs)
        for a in ("nx", "nu", "nr"):
            if hasattr(self, a): setattr(t, a, getattr(self, a))
        return t


def gradient_tape(tape):
    """reverse-mode sweep over the SSA tape of a scalar function: a new tape whose outputs are d out / d input_k, k < n_in"""
    g = tape.clone()
    (out,) = tape.outputs
    zero = g.const(0.0)
    bar = {out: g.const(1.0)}
    for i in sorted(tape.live_nodes(), reverse=True):
        if i not in bar or g.nodes[i][0] in ("in", "const"):
            continue
        for a, d in g.partials(i):
            bar[a] = g.s_add(bar.get(a, zero), g.s_mul(bar[i], d))
    g.outputs = [bar.get(k, zero) for k in range(tape.n_in)]
    return g


def tangent_outputs(tape, k):
    """forward-mode sweep in direction input k (symbolic): node ids of d outputs / d input_k, appended to a scratch clone"""
    t = tape.clone()
    zero, one = t.const(0.0), t.const(1.0)
    dot = {}
    for i in tape.live_nodes():
        nd = t.nodes[i]
        if nd[0] == "in":
            dot[i] = one if nd[1] == k else zero
        elif nd[0] == "const":
            dot[i] = zero
        else:
            acc = zero
            for a, d in t.partials(i):
                acc = t.s_add(acc, t.s_mul(dot[a], d))
            dot[i] = acc
    return t, [dot[o] for o in tape.outputs]


def hessian_mask(gtape):
    """structural sparsity [n, n] of the Hessian whose gradient tape is gtape (entries that are not identically zero); n = the gradient's length:
    all inputs, or the leading [s; u; r] block of a cost that also reads stage data (those carry no derivative)"""
    n = len(gtape.outputs)
    mask = np.zeros((n, n), bool)
    for k in range(n):
        t, d = tangent_outputs(gtape, k)
        for r in range(n):
            mask[r, k] = not (t.is_const(d[r]) and t.nodes[d[r]][1] == 0.0)
    return mask | mask.T


def closed_mask(mask):
    """the component closure of a symmetric structure: every pair of indices inside one connected component of the graph of mask | eye.  V f(Lambda) V'
    of a matrix with that structure fills in inside the components and nowhere else, so this is the pattern a convexified Hessian needs
    (models.StageOCP.convexify)"""
    m = np.asarray(mask, bool)
    m = m | m.T | np.eye(m.shape[0], dtype=bool)
    while True:
        r = (m.astype(np.int64) @ m.astype(np.int64)) > 0
        if np.array_equal(r, m):
            return m
        m = r


class TS:
    """scalar tracer"""
    __array_priority__ = 1000

    def __init__(self, tape, idx):
        self.tape, self.idx = tape, idx

    @staticmethod
    def _lift(tape, v):
        if isinstance(v, TS):
            return v
        if isinstance(v, (int, float, np.integer, np.floating)):
            return TS(tape, tape.const(v))
        if isinstance(v, np.ndarray) and v.ndim == 0:
            return TS(tape, tape.const(float(v)))
        raise TypeError("cannot trace a value of type %s" % type(v).__name__)

    def _bin(self, op, other, swap=False):
        if isinstance(other, TV):
            return other._bin(op, self, swap=not swap)
        o = TS._lift(self.tape, other)
        a, b = (o, self) if swap else (self, o)
        return TS(self.tape, self.tape.binary(op, a.idx, b.idx))

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("div", o)
    def __rtruediv__(self, o): return self._bin("div", o, True)
    def __neg__(self): return TS(self.tape, self.tape.unary("neg", self.idx))
    def __pos__(self): return self

    def __pow__(self, e):
        if isinstance(e, (int, np.integer)) or (isinstance(e, float) and e == int(e)):
            e = int(e)
            if e == 0:
                return TS(self.tape, self.tape.const(1.0))
            r = None; base = self; k = abs(e)
            while k:
                if k & 1:
                    r = base if r is None else r * base
                k >>= 1
                if k:
                    base = base * base
            return r if e > 0 else 1.0 / r
        if e == 0.5:
            return TS(self.tape, self.tape.unary("sqrt", self.idx))
        raise TypeError("only integer powers and ** 0.5 can be traced")

    def __bool__(self):
        raise TypeError("data-dependent branches cannot be traced (the dynamics must be straight-line code)")

    def _cmp(self, o):
        return self.__bool__()

    __lt__ = __le__ = __gt__ = __ge__ = _cmp

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        return _ufunc(self.tape, ufunc, method, inputs, kw)

    def __array_function__(self, func, types, args, kwargs):
        return _array_function(self.tape, func, args, kwargs)


class TV:
    """vector tracer standing for an array [..., k] (leading axes are the batch the device kernel supplies)"""
    __array_priority__ = 1000

    def __init__(self, tape, items):
        self.tape, self.items = tape, list(items)

    @property
    def shape(self):
        return (len(self.items),)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, key):
        if isinstance(key, tuple):
            key = [k for k in key if k is not Ellipsis]
            if len(key) != 1:
                raise IndexError("index the last axis only: s[..., i] or s[..., a:b]")
            key = key[0]
        if isinstance(key, slice):
            return TV(self.tape, self.items[key])
        if isinstance(key, (int, np.integer)):
            return self.items[int(key)]
        if isinstance(key, (list, np.ndarray)):
            return TV(self.tape, [self.items[int(i)] for i in key])
        raise IndexError("unsupported index %r" % (key,))

    def __iter__(self):
        return iter(self.items)

    def _bin(self, op, other, swap=False):
        if isinstance(other, TV):
            if len(other) != len(self):
                raise ValueError("shape mismatch %d vs %d" % (len(self), len(other)))
            others = other.items
        elif isinstance(other, np.ndarray) and other.ndim >= 1:
            if other.shape[-1] != len(self) or other.size != len(self):
                raise ValueError("constant array must have the vector's length")
            others = [float(v) for v in other.ravel()]
        else:
            others = [other] * len(self)
        out = []
        for a, b in zip(self.items, others):
            out.append(a._bin(op, b, swap))
        return TV(self.tape, out)

    def __add__(self, o): return self._bin("add", o)
    def __radd__(self, o): return self._bin("add", o, True)
    def __sub__(self, o): return self._bin("sub", o)
    def __rsub__(self, o): return self._bin("sub", o, True)
    def __mul__(self, o): return self._bin("mul", o)
    def __rmul__(self, o): return self._bin("mul", o, True)
    def __truediv__(self, o): return self._bin("div", o)
    def __rtruediv__(self, o): return self._bin("div", o, True)
    def __neg__(self): return TV(self.tape, [-a for a in self.items])
    def __pow__(self, e): return TV(self.tape, [a ** e for a in self.items])

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        return _ufunc(self.tape, ufunc, method, inputs, kw)

    def __array_function__(self, func, types, args, kwargs):
        return _array_function(self.tape, func, args, kwargs)


_UFUNC_BIN = {np.add: "add", np.subtract: "sub", np.multiply: "mul", np.true_divide: "div"}
_UFUNC_UN = {np.negative: "neg", np.sin: "sin", np.cos: "cos", np.tan: "tan", np.exp: "exp", np.log: "log", np.sqrt: "sqrt", np.tanh: "tanh"}


def _ufunc(tape, ufunc, method, inputs, kw):
    if method != "__call__" or kw.get("out") is not None:
        return NotImplemented
    if ufunc in _UFUNC_BIN:
        a, b = inputs
        op = _UFUNC_BIN[ufunc]
        if isinstance(a, (TS, TV)):
            return a._bin(op, b)
        return b._bin(op, a, True)
    if ufunc in _UFUNC_UN:
        (a,) = inputs
        op = _UFUNC_UN[ufunc]
        if isinstance(a, TV):
            return TV(tape, [TS(tape, tape.unary(op, x.idx)) for x in a.items])
        return TS(tape, tape.unary(op, a.idx))
    if ufunc is np.square:
        (a,) = inputs
        return a * a
    if ufunc is np.power:
        a, e = inputs
        return a ** e
    if ufunc is np.positive:
        return inputs[0]
    raise TypeError("NumPy function %s cannot be traced" % ufunc.__name__)


def _array_function(tape, func, args, kwargs):
    if func in (np.stack, np.concatenate):
        seq = args[0]
        axis = kwargs.get("axis", args[1] if len(args) > 1 else 0)
        if axis not in (-1,) and not (axis == 0 and all(isinstance(v, (TS, TV, int, float)) for v in seq)):
            raise TypeError("stack / concatenate along the last axis only")
        items = []
        for v in seq:
            if isinstance(v, TV):
                if func is np.stack:
                    raise TypeError("np.stack of vectors is not traceable; use np.concatenate")
                items += v.items
            else:
                items.append(TS._lift(tape, v))
        return TV(tape, items)
    raise TypeError("NumPy function %s cannot be traced" % func.__name__)


NTHETA_MAX = 8        # MPCQP_STAGE_NPAR: the width of a parameter row
NSD_MAX = 8           # MPCQP_STAGE_MAXSD (SM_MAXSD): the most stage-data values a frame may take


class _ThetaGuard:
    """stands in for model.theta while a function other than F is traced: parameters are data of the dynamics only"""

    def __init__(self, what):
        self._what = what

    def _refuse(self, *a, **k):
        raise ValueError("%s reads self.theta: model parameters are supported in F / cdyn only (not in hfun, kfun, lcost, lterm, llink)" % self._what)

    __getitem__ = __iter__ = __len__ = __array__ = __add__ = __radd__ = __mul__ = __rmul__ = __sub__ = __rsub__ = __truediv__ = __rtruediv__ = __neg__ = _refuse


class _SdataGuard:
    """stands in for model.sdata while F, kfun or llink is traced: stage data are data of the path constraint and the frame costs only"""

    def __init__(self, what):
        self._what = what

    def _refuse(self, *a, **k):
        raise ValueError("%s reads self.sdata: stage data are supported in hfun, lcost and lterm only (not in F / cdyn, kfun, llink)" % self._what)

    __getitem__ = __iter__ = __len__ = __array__ = __add__ = __radd__ = __mul__ = __rmul__ = __sub__ = __rsub__ = __truediv__ = __rtruediv__ = __neg__ = _refuse


class _bound_theta:
    """model.theta (or model.<attr>) = value for the duration of a trace (a model without parameters, or no model: nothing happens)"""

    def __init__(self, model, value, attr="theta"):
        self.model, self.value, self.attr = model, value, attr

    def __enter__(self):
        if self.model is not None:
            self.saved = getattr(self.model, self.attr)
            setattr(self.model, self.attr, self.value)

    def __exit__(self, *exc):
        if self.model is not None:
            setattr(self.model, self.attr, self.saved)
        return False


def _trace_fn(fn, nx, nu, n_out, what, ntheta=0, model=None, nsd=0):
    """ntheta > 0: that many extra tape inputs behind [s; u], bound to model.theta while fn runs (the plant parameters: par[i] in the emitted code).
    nsd > 0 (hfun; F of a model with transition_data): that many extra inputs behind [s; u] (behind the parameters, where both are given), bound to
    model.sdata (the frame's stage data: d[i] in the emitted code)"""
    tape = Tape(nx + nu + ntheta + nsd)
    s = TV(tape, [TS(tape, i) for i in range(nx)])
    u = TV(tape, [TS(tape, nx + i) for i in range(nu)])
    if nsd and ntheta:      # (F of a model with transition_data: the parameter row, then the frame's data row)
        with _bound_theta(model, TV(tape, [TS(tape, nx + nu + i) for i in range(ntheta)])), \
                _bound_theta(model, TV(tape, [TS(tape, nx + nu + ntheta + i) for i in range(nsd)]), "sdata"):
            out = fn(s, u)
        tape.in_names = [("s", nx), ("u", nu), ("par", ntheta), ("d", nsd)]
        tape.plain_from = nx + nu
    elif nsd:
        with _bound_theta(model, TV(tape, [TS(tape, nx + nu + i) for i in range(nsd)]), "sdata"):
            out = fn(s, u)
        tape.in_names = [("s", nx), ("u", nu), ("d", nsd)]
        tape.plain_from = nx + nu
    elif ntheta:
        with _bound_theta(model, TV(tape, [TS(tape, nx + nu + i) for i in range(ntheta)])):
            out = fn(s, u)
        tape.in_names = [("s", nx), ("u", nu), ("par", ntheta)]
    else:
        out = fn(s, u)
    if isinstance(out, TS):
        out = TV(tape, [out])
    if isinstance(out, (list, tuple)):
        out = TV(tape, [TS._lift(tape, v) for v in out])
    if not isinstance(out, TV) or len(out) != n_out:
        raise ValueError("%s, %d components" % (what, n_out))
    tape.outputs = [TS._lift(tape, v).idx for v in out.items]
    tape.nx, tape.nu = nx, nu
    return tape


def trace_cost(lfun, nx, nu, nr, nsd=0, model=None):
    """stage cost l(s, u, r) -> scalar on tracers; returns (value tape, gradient tape) over inputs [s; u; r].  nsd > 0: that many extra inputs
    behind r, bound to model.sdata while lfun runs (the frame's stage data); the gradient keeps the [s; u; r] block only"""
    nl = nx + nu + nr
    tape = Tape(nl + nsd)
    mk = lambda a, b: TV(tape, [TS(tape, i) for i in range(a, b)])
    with _bound_theta(model if nsd else None, mk(nl, nl + nsd), "sdata"):
        out = lfun(mk(0, nx), mk(nx, nx + nu), mk(nx + nu, nl))
    if isinstance(out, TV) and len(out) == 1:
        out = out.items[0]
    if isinstance(out, (int, float, np.integer, np.floating)):
        out = TS._lift(tape, out)
    if not isinstance(out, TS):
        raise ValueError("the stage cost must return one scalar")
    tape.outputs = [out.idx]
    tape.nx, tape.nu, tape.nr = nx, nu, nr
    g = gradient_tape(tape)
    if nsd:
        g.outputs = g.outputs[:nl]
        tape.in_names = g.in_names = [("s", nx), ("u", nu), ("r", nr), ("d", nsd)]
        tape.plain_from = g.plain_from = nl
    return tape, g


NR_MAX = 32           # the most residual rows of a Gauss-Newton frame cost (models.StageOCP.rcost / rterm): a stated limit, like NTHETA_MAX


def trace_residual(rfun, nx, nu, nr_ref, nsd=0, model=None):
    """residual r(s, u, r) -> [..., n_out] on tracers (a list of components is accepted): the residual tape over the inputs [s; u; r](; d), d the
    nsd stage-data values bound to model.sdata while rfun runs, as in trace_cost.  At most NR_MAX rows"""
    nl = nx + nu + nr_ref
    tape = Tape(nl + nsd)
    mk = lambda a, b: TV(tape, [TS(tape, i) for i in range(a, b)])
    with _bound_theta(model if nsd else None, mk(nl, nl + nsd), "sdata"):
        out = rfun(mk(0, nx), mk(nx, nx + nu), mk(nx + nu, nl))
    if isinstance(out, TS):
        out = TV(tape, [out])
    if isinstance(out, (list, tuple)):
        out = TV(tape, [TS._lift(tape, v) for v in out])
    if not isinstance(out, TV) or len(out) < 1:
        raise ValueError("the residual must return its components [..., nr] (an array or a list)")
    if len(out) > NR_MAX:
        raise ValueError("at most %d residual rows are supported (nr = %d)" % (NR_MAX, len(out)))
    tape.outputs = [TS._lift(tape, v).idx for v in out.items]
    tape.n_out = len(tape.outputs)
    tape.nx, tape.nu, tape.nr = nx, nu, nr_ref
    if nsd:
        tape.in_names = [("s", nx), ("u", nu), ("r", nr_ref), ("d", nsd)]
        tape.plain_from = nl
    return tape


def _append_inputs(tape, k):
    """the same tape with k more inputs behind its own (the node ids of everything else move up by k)"""
    t = Tape(tape.n_in + k)
    m = {i: i for i in range(tape.n_in)}
    for i in range(tape.n_in, len(tape.nodes)):
        nd = tape.nodes[i]
        m[i] = t.const(nd[1]) if nd[0] == "const" else t._add((nd[0],) + tuple(m[a] for a in nd[1:]))
    t.outputs = [m[o] for o in tape.outputs]
    for a in ("nx", "nu", "nr"):
        if hasattr(tape, a): setattr(t, a, getattr(tape, a))
    return t


def residual_tapes(rtape):
    """What a Gauss-Newton frame cost f = sum_i r_i^2 needs next to its residual tape (trace_residual): dict with
    L: the value tape sum_i r_i^2, i ascending from 0.0 (the order of Python's sum over the components);
    G: its gradient tape over [s; u; r] (gradient_tape: 2 J' r);
    RT: the transposed-Jacobian tape -- inputs [s; u; r](; d) and then n_out plain weights w, outputs J' w over [s; u; r]: gradient_tape of w' r with
        w as inputs that carry no derivative;
    mask: the structure of J'J | eye from the structural Jacobian (tangent_outputs): entry (a, b) is set when some row depends on both inputs."""
    nl = rtape.nx + rtape.nu + rtape.nr
    nsd = rtape.n_in - nl
    n_out = len(rtape.outputs)
    names = getattr(rtape, "in_names", None)
    L = rtape.clone()
    acc = L.const(0.0)
    for o in rtape.outputs:
        acc = L.binary("add", acc, L.binary("mul", o, o))
    L.outputs = [acc]
    G = gradient_tape(L)
    G.outputs = G.outputs[:nl]
    W = _append_inputs(rtape, n_out)
    acc = W.const(0.0)
    for i, o in enumerate(W.outputs):
        acc = W.s_add(acc, W.s_mul(nl + nsd + i, o))
    W.outputs = [acc]
    RT = gradient_tape(W)
    RT.outputs = RT.outputs[:nl]
    RT.in_names = [("s", rtape.nx), ("u", rtape.nu), ("r", rtape.nr)] + ([("d", nsd)] if nsd else []) + [("w", n_out)]
    RT.plain_from = nl
    if names:
        L.in_names = G.in_names = names
        L.plain_from = G.plain_from = nl
    J = np.zeros((n_out, nl), bool)
    for k in range(nl):
        t, d = tangent_outputs(rtape, k)
        J[:, k] = [not (t.is_const(v) and t.nodes[v][1] == 0.0) for v in d]
    Ji = J.astype(np.int64)
    return dict(L=L, G=G, RT=RT, mask=((Ji.T @ Ji) > 0) | np.eye(nl, dtype=bool))


GN_REFUSES_CONVEXIFY = ("convexify does not combine with a Gauss-Newton cost (rcost): 2 J'J is positive semidefinite by construction, there is nothing "
                        "to convexify")
GN_REFUSES_EXACT = ("exact_hessian does not combine with a Gauss-Newton cost (rcost): adding the constraints' curvature to a matrix that drops the "
                    "cost's own is not covered")


def _trace_link(kfun, nx, nu, nk, nsd=0, model=None):
    """kfun(s, u, s_next, u_next) -> [..., nk] on tracers over the inputs [s; u; s_next; u_next].  nsd > 0 (a model with transition_data): that many
    extra inputs behind them, bound to model.sdata while kfun runs (the data row of the pair's first frame), without a derivative"""
    tape = Tape(2 * (nx + nu) + nsd)
    mk = lambda a, b: TV(tape, [TS(tape, i) for i in range(a, b)])
    f = nx + nu
    with _bound_theta(model if nsd else None, mk(2 * f, 2 * f + nsd), "sdata"):
        out = kfun(mk(0, nx), mk(nx, f), mk(f, f + nx), mk(f + nx, 2 * f))
    if isinstance(out, TS):
        out = TV(tape, [out])
    if isinstance(out, (list, tuple)):
        out = TV(tape, [TS._lift(tape, v) for v in out])
    if not isinstance(out, TV) or len(out) != nk:
        raise ValueError("kfun must return the link-constraint values, %d components" % nk)
    tape.outputs = [TS._lift(tape, v).idx for v in out.items]
    tape.nx, tape.nu = nx, nu
    tape.in_names = [("s", nx), ("u", nu), ("sn", nx), ("un", nu)]
    if nsd:
        tape.in_names.append(("d", nsd))
        tape.plain_from = 2 * f
    return tape


def trace_link_cost(llink, nx, nu, nsd=0, model=None):
    """link cost llink(s, u, s_next, u_next) -> scalar on tracers; returns (value tape, gradient tape) over the inputs [s; u; s_next; u_next].
    nsd > 0 (a model with transition_data): that many extra inputs behind them, bound to model.sdata while llink runs (the data row of the pair's
    first frame); the gradient keeps the [s; u; s_next; u_next] block only"""
    tape = Tape(2 * (nx + nu) + nsd)
    mk = lambda a, b: TV(tape, [TS(tape, i) for i in range(a, b)])
    f = nx + nu
    with _bound_theta(model if nsd else None, mk(2 * f, 2 * f + nsd), "sdata"):
        out = llink(mk(0, nx), mk(nx, f), mk(f, f + nx), mk(f + nx, 2 * f))
    if isinstance(out, TV) and len(out) == 1:
        out = out.items[0]
    if isinstance(out, (int, float, np.integer, np.floating)):
        out = TS._lift(tape, out)
    if not isinstance(out, TS):
        raise ValueError("the link cost must return one scalar")
    tape.outputs = [out.idx]
    tape.nx, tape.nu = nx, nu
    tape.in_names = [("s", nx), ("u", nu), ("sn", nx), ("un", nu)]
    g = gradient_tape(tape)
    if nsd:
        g.outputs = g.outputs[:2 * f]
        tape.in_names.append(("d", nsd))
        tape.plain_from = g.plain_from = 2 * f
    g.in_names = tape.in_names
    return tape, g


def _contracted_gradient(fn, nx, nu, n_out, mult, what, model=None, ntheta=0, nsd=0):
    """gradient over [s; u] of the scalar mult' fn(s, u), the multipliers `mult` (n_out of them) being extra tape inputs without a derivative, like
    theta and sdata: inputs [s; u; par (ntheta)?; mult; d (nsd)?] -> outputs [f]"""
    f = nx + nu
    tape = Tape(f + ntheta + n_out + nsd)
    mk = lambda a, b: TV(tape, [TS(tape, i) for i in range(a, b)])
    m0 = f + ntheta
    d0 = m0 + n_out
    with _bound_theta(model if ntheta else None, mk(f, f + ntheta)), _bound_theta(model if nsd else None, mk(d0, d0 + nsd), "sdata"):
        out = fn(mk(0, nx), mk(nx, f))
    if isinstance(out, TS):
        out = TV(tape, [out])
    if isinstance(out, (list, tuple)):
        out = TV(tape, [TS._lift(tape, v) for v in out])
    if not isinstance(out, TV) or len(out) != n_out:
        raise ValueError("%s, %d components" % (what, n_out))
    acc = TS(tape, tape.const(0.0))
    for i, v in enumerate(out.items):
        acc = TS(tape, tape.s_add(acc.idx, tape.s_mul(m0 + i, TS._lift(tape, v).idx)))
    tape.outputs = [acc.idx]
    tape.nx, tape.nu = nx, nu
    g = gradient_tape(tape)
    g.outputs = g.outputs[:f]
    g.in_names = [("s", nx), ("u", nu)] + ([("par", ntheta)] if ntheta else []) + [(mult, n_out)] + ([("d", nsd)] if nsd else [])
    g.plain_from = f
    return g


def trace_curvature(F, nx, nu, hfun=None, nh=0, ntheta=0, nsd=0, model=None, transition_data=False):
    """The constraint curvature of the exact Lagrangian Hessian (models.StageOCP.exact_hessian): the gradient tapes over [s; u] of the
    contracted scalars lam' F(s, u) (inputs [s; u; par; lam]) and mu' hfun(s, u) (inputs [s; u; mu; d]) and the structure of their Hessians, valid
    for any multipliers.  transition_data: F reads the frame's stage data too (inputs [s; u; par; lam; d]).
    Returns dict(FG, HG (None without a path constraint), mask [f, f])."""
    guarded = model if ntheta else None
    unread = model if nsd else None
    if transition_data and nsd:
        FG = _contracted_gradient(F, nx, nu, nx, "lam", "F must return the next state", model, ntheta, nsd)
    else:
        with _bound_theta(unread, _SdataGuard("F"), "sdata"):
            FG = _contracted_gradient(F, nx, nu, nx, "lam", "F must return the next state", model, ntheta)
    mask = hessian_mask(FG)
    HG = None
    if hfun is not None and nh:
        with _bound_theta(guarded, _ThetaGuard("hfun")):
            HG = _contracted_gradient(hfun, nx, nu, nh, "mu", "hfun must return the path-constraint values", model, 0, nsd)
        mask = mask | hessian_mask(HG)
    return dict(FG=FG, HG=HG, mask=mask)


def link_is_linear(link):
    """no output of the link-constraint tape has a second derivative (a rate limit and the like)"""
    nv = 2 * (link.nx + link.nu)      # (stage data behind the two frames carry no derivative)
    for o in link.outputs:
        t = link.clone()
        t.outputs = [o]
        g = gradient_tape(t)
        g.outputs = g.outputs[:nv]
        if hessian_mask(g).any():
            return False
    return True


def trace(F, nx, nu, hfun=None, nh=0, h_lo=None, h_hi=None, lcost=None, lterm=None, kfun=None, nk=0, k_lo=None, k_hi=None, per_frame_reference=False,
          ntheta=0, theta0=None, model=None, llink=None, nsd=0, sdata0=None, convexify=False, exact_hessian=False, rcost=None, rterm=None,
          transition_data=False):
    """Run F (and the optional per-stage path constraint hfun) once on tracers.  F(s, u) -> s_next with s [..., nx],
    u [..., nu] (the contract of models.StageOCP.F); hfun(s, u) -> [..., nh] with bounds h_lo <= hfun <= h_hi.
    lcost(s, u, r) -> scalar: a general stage cost summed over the frames (r = the reference parameter, size nx), replacing
    the diagonal tracking weights; lterm: the same for the last frame only (terminal cost).  Their gradients are derived
    on the tape (reverse mode); the kernels differentiate those once more with dual numbers for the exact Hessian.
    per_frame_reference: the library is emitted for trajectory tracking (models.StageOCP.per_frame_reference: frame k's cost takes its own
    reference r_k, mpcqp_stage_create_tracking loads it); the traced functions are the same.
    ntheta = k (<= 8), theta0 = the k default values: the model (`model`, or the object F is bound to) reads its plant parameters as
    self.theta[i] inside F / cdyn; while F is traced, self.theta holds k extra tape inputs, emitted as par[i] -- data of the functor, not constants
    of its code, so that mpcqp_stage_set_instance_params can give every instance its own.  Any other traced function that touches self.theta
    raises a ValueError.
    llink(s, u, s_next, u_next) -> scalar: a link cost, summed over the stages k = 0 .. N-2 on top of the frame cost (a move penalty
    (u_{k+1} - u_k)' S (u_{k+1} - u_k) and the like).  It takes no reference and no theta.  tape.link_cost holds its value tape, its gradient
    tape and the exact structure of its Hessian over [s; u; s_next; u_next] (no diagonal is forced into it).
    nsd = k (<= 8), sdata0 = the k default values: the model reads its stage data as self.sdata[i] inside hfun, lcost and lterm (a cost that does
    is a method of the model); while those are traced, self.sdata holds k extra tape inputs, emitted as d[i] -- data of the launch
    (mpcqp_stage_set_stage_data gives every frame of every instance its own row), without a derivative: the gradient and the Hessian's structure
    are over [s; u; r] as before.  F / cdyn, kfun and llink take none: reading self.sdata there raises a ValueError (unless transition_data, below).
    convexify (models.StageOCP.convexify; needs lcost): the cost's mask becomes its component closure (closed_mask) and the library exports
    mpcqp_user_convexify, the launcher of mpcqp_stage_convexify.  Without it the library is the text it always was.
    exact_hessian (models.StageOCP.exact_hessian; needs lcost, whose pattern has the off-diagonal slots): the functors FG and HG, the gradients over
    [s; u] of lam' F and mu' hfun (trace_curvature); the structure of their Hessians joins the [s; u] block of the cost's mask before the closure of
    convexify, and the library exports the launchers of mpcqp_stage_lagrangian.  A nonlinear kfun is refused: its curvature couples two frames.
    Without it the library is the text it always was.
    rcost(s, u, r) -> [..., nr] (and rterm -> [..., nrt] for the last frame; models.StageOCP.rcost): a Gauss-Newton frame cost
    f = sum_k |rcost(s_k, u_k, r)|^2 in place of lcost / lterm.  tape.cost holds the value and gradient tapes derived from the residual tape
    (residual_tapes) and the structure of J'J as the mask; tape.residual the residual tapes and their transposed-Jacobian tapes, which the functor
    carries as R, RT (RTm, RTT: the terminal frame's).  The rules of lcost on theta and sdata hold; convexify and exact_hessian are refused.
    Without it the library is the text it always was.
    transition_data (models.StageOCP.transition_data; needs nsd): F / cdyn, kfun and llink read self.sdata[i] as well -- the row of the
    transition's first frame, k for the step k -> k + 1 -- instead of being refused: F is traced with nsd inputs behind [s; u; theta], kfun and llink
    with nsd inputs behind their two frames, the gradient tapes keep their outputs over the variables.  The functor declares tdata = 1 and every
    transition function it has takes d.  Without it the library is the text it always was."""
    ntheta = int(ntheta)
    nsd = int(nsd)
    tdata = bool(transition_data)
    if tdata and not nsd:
        raise ValueError("transition_data needs stage data (nsd > 0): it lets F / cdyn, kfun and llink read self.sdata")
    if rcost is not None and (lcost is not None or lterm is not None):
        raise ValueError("rcost excludes lcost / lterm: the frame cost is either a scalar with its exact Hessian or a residual with the Gauss-Newton one")
    if rterm is not None and rcost is None:
        raise ValueError("a terminal residual (rterm) needs a stage residual (rcost)")
    if rcost is not None and convexify:
        raise ValueError(GN_REFUSES_CONVEXIFY)
    if rcost is not None and exact_hessian:
        raise ValueError(GN_REFUSES_EXACT)
    if nsd > NSD_MAX:
        raise ValueError("at most %d stage-data values are supported (nsd = %d)" % (NSD_MAX, nsd))
    if ntheta > NTHETA_MAX:
        raise ValueError("at most %d model parameters are supported (ntheta = %d)" % (NTHETA_MAX, ntheta))
    if model is None:
        model = getattr(F, "__self__", None)
    guarded = model if ntheta else None       # whose theta the other traces may not read (without parameters in the trace, theta is numbers like any other)
    if ntheta:
        if model is None:
            raise ValueError("ntheta needs the model whose theta F reads (model=, or F as a bound method)")
        theta0 = np.asarray(model.theta if theta0 is None else theta0, float).ravel()
        if theta0.size != ntheta:
            raise ValueError("theta0 must hold ntheta = %d values" % ntheta)
    if nsd:
        if model is None:
            raise ValueError("nsd needs the model whose sdata hfun / lcost / lterm read (model=, or F as a bound method)")
        sdata0 = np.asarray(model.sdata if sdata0 is None else sdata0, float).ravel()
        if sdata0.size != nsd:
            raise ValueError("sdata0 must hold nsd = %d values" % nsd)
    unread = model if nsd and not tdata else None           # whose sdata F, kfun and llink may not read
    tnsd = nsd if tdata else 0                # the data inputs of the transition functions
    if tdata:
        tape = _trace_fn(F, nx, nu, nx, "F must return the next state", ntheta, model, nsd=nsd)
        tape.tdata = True
    else:
        with _bound_theta(unread, _SdataGuard("F"), "sdata"):
            tape = _trace_fn(F, nx, nu, nx, "F must return the next state", ntheta, model)
    if nsd:
        tape.nsd = nsd
        tape.sdata0 = [float(v) for v in sdata0]
    tape.ntheta = ntheta
    tape.theta0 = [float(v) for v in theta0] if ntheta else []
    tape.pref = bool(per_frame_reference)
    tape.nh = int(nh) if hfun is not None else 0
    tape.path = None
    if tape.nh:
        with _bound_theta(guarded, _ThetaGuard("hfun")):
            tape.path = _trace_fn(hfun, nx, nu, tape.nh, "hfun must return the path-constraint values", model=model, nsd=nsd)
        tape.h_lo = [float(v) for v in np.broadcast_to(np.asarray(h_lo, float), (tape.nh,))]
        tape.h_hi = [float(v) for v in np.broadcast_to(np.asarray(h_hi, float), (tape.nh,))]
    # link constraint k_lo <= kfun(s_k, u_k, s_{k+1}, u_{k+1}) <= k_hi between consecutive frames (rate limits and the like)
    tape.nk = int(nk) if kfun is not None else 0
    tape.link = None
    if tape.nk:
        with _bound_theta(guarded, _ThetaGuard("kfun")), _bound_theta(unread, _SdataGuard("kfun"), "sdata"):
            tape.link = _trace_link(kfun, nx, nu, tape.nk, tnsd, model)
        tape.k_lo = [float(v) for v in np.broadcast_to(np.asarray(k_lo, float), (tape.nk,))]
        tape.k_hi = [float(v) for v in np.broadcast_to(np.asarray(k_hi, float), (tape.nk,))]
    tape.cost = None
    if lcost is not None:
        with _bound_theta(guarded, _ThetaGuard("lcost")):
            L, G = trace_cost(lcost, nx, nu, nx, nsd, model)
        mask = hessian_mask(G)
        LT = GT = None
        if lterm is not None:
            with _bound_theta(guarded, _ThetaGuard("lterm")):
                LT, GT = trace_cost(lterm, nx, nu, nx, nsd, model)
            mask = mask | hessian_mask(GT)
        mask = mask | np.eye(mask.shape[0], dtype=bool)      # keep the diagonal in the pattern
        if exact_hessian:
            if tape.nk and not link_is_linear(tape.link):
                raise ValueError("exact_hessian does not cover a nonlinear link constraint (kfun): its curvature couples two frames; a linear kfun "
                                 "(rate limits) is fine")
            tape.exact = trace_curvature(F, nx, nu, hfun if tape.nh else None, tape.nh, ntheta, nsd, model, **({"transition_data": True} if tdata else {}))
            mask[:nx + nu, :nx + nu] |= tape.exact["mask"]
        if convexify:
            mask = closed_mask(mask)
            tape.convexify = True
        tape.cost = dict(L=L, G=G, LT=LT, GT=GT, mask=mask)
    elif rcost is not None:
        with _bound_theta(guarded, _ThetaGuard("rcost")):
            R = trace_residual(rcost, nx, nu, nx, nsd, model)
        d = residual_tapes(R)
        mask = d["mask"]
        Rm = dm = None
        if rterm is not None:
            with _bound_theta(guarded, _ThetaGuard("rterm")):
                Rm = trace_residual(rterm, nx, nu, nx, nsd, model)
            dm = residual_tapes(Rm)
            mask = mask | dm["mask"]
        tape.cost = dict(L=d["L"], G=d["G"], LT=dm["L"] if dm else None, GT=dm["G"] if dm else None, mask=mask)
        tape.residual = dict(R=R, RT=d["RT"], Rm=Rm, RTT=dm["RT"] if dm else None, nr=R.n_out, nrt=Rm.n_out if Rm is not None else R.n_out)
    elif lterm is not None:
        raise ValueError("a terminal cost needs a stage cost")
    elif convexify:
        raise ValueError("convexify needs a stage cost (lcost): diagonal weights have nothing to convexify")
    elif exact_hessian:
        raise ValueError("exact_hessian needs a stage cost (lcost): the pattern of diagonal weights has no off-diagonal slots for the curvature")
    tape.link_cost = None
    if llink is not None:
        with _bound_theta(guarded, _ThetaGuard("llink")), _bound_theta(unread, _SdataGuard("llink"), "sdata"):
            LK, LKG = trace_link_cost(llink, nx, nu, tnsd, model)
        tape.link_cost = dict(L=LK, G=LKG, mask=hessian_mask(LKG))
    return tape


# ------------------------------------------------------------------------------------------------- emission
def _lit(v):
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError("non-finite constant in the traced dynamics")
    return repr(float(v)) if "e" in repr(float(v)) or "." in repr(float(v)) else repr(float(v)) + ".0"


def _emit_body(tape, streaming=False):
    if streaming:
        return _emit_streaming_body(tape)
    nx = tape.nx
    live = tape.live_nodes()
    ref = {}
    lines = []
    # nodes that depend on parameters and constants only are plain doubles next to T = Dual (a parameter carries no derivative): they mix with T
    # through the double-Dual operators, as literals do
    par_from = tape.nx + tape.nu if getattr(tape, "ntheta", 0) else tape.n_in
    par_from = getattr(tape, "plain_from", par_from)      # (stage data, d[i]: plain doubles as well)
    plain = set()
    for i in live:
        nd = tape.nodes[i]
        if nd[0] == "const" or (nd[0] == "in" and nd[1] >= par_from) or (nd[0] not in ("in", "const") and all(a in plain for a in nd[1:])):
            plain.add(i)
    for i in live:
        nd = tape.nodes[i]
        if nd[0] == "in":
            nu = getattr(tape, "nu", tape.n_in - nx)
            if getattr(tape, "in_names", None):
                k = nd[1]
                for nm, cnt in tape.in_names:
                    if k < cnt:
                        ref[i] = "%s[%d]" % (nm, k); break
                    k -= cnt
            else:
                ref[i] = "s[%d]" % nd[1] if nd[1] < nx else "u[%d]" % (nd[1] - nx) if nd[1] < nx + nu else "r[%d]" % (nd[1] - nx - nu)
        elif nd[0] == "const":
            ref[i] = _lit(nd[1])
        elif nd[0] in _UNARY:
            f = _UNARY[nd[0]]
            expr = "-%s" % ref[nd[1]] if nd[0] == "neg" else "%s(%s)" % (f, ref[nd[1]])
            lines.append("    const %s w%d = %s;" % ("double" if i in plain else "T", i, expr)); ref[i] = "w%d" % i
        else:
            lines.append("    const %s w%d = %s %s %s;" % ("double" if i in plain else "T", i, ref[nd[1]], _BINARY[nd[0]], ref[nd[2]])); ref[i] = "w%d" % i
    for r, o in enumerate(tape.outputs):
        lines.append("    out[%d] = %s;" % (r, "T{} + %s" % ref[o] if o in plain else ref[o]))
    return "\n".join(lines)


def _emit_streaming_body(tape):
    """the general evaluator's form of a body: an input is formed by the accessor `in(k)` where it is first used, an output goes to the
    sink `out(r, value)` as soon as it is produced -- no array of the problem's length lives in the function.  A tape with plain_from (the
    contracted gradient of general_nlp: inputs from there on are multipliers) takes those from a second accessor `mul(i)` as plain doubles, and
    whatever depends on them and on constants alone stays a double next to T = Dual, as par and d do in the stage bodies"""
    outs_of = {}
    for r, o in enumerate(tape.outputs):
        outs_of.setdefault(o, []).append(r)
    ref = {}
    lines = []
    plain_from = getattr(tape, "plain_from", tape.n_in)
    plain = set()

    def use(i):
        if i not in ref:
            nd = tape.nodes[i]
            if nd[0] == "in" and nd[1] >= plain_from:
                lines.append("    const double m%d = mul(%d);" % (nd[1] - plain_from, nd[1] - plain_from)); ref[i] = "m%d" % (nd[1] - plain_from)
                plain.add(i)
            elif nd[0] == "in":
                lines.append("    const T x%d = in(%d);" % (nd[1], nd[1])); ref[i] = "x%d" % nd[1]
            else:
                ref[i] = _lit(nd[1])
        return ref[i]

    for i in tape.live_nodes():
        nd = tape.nodes[i]
        if nd[0] in ("in", "const"):
            continue
        args = [use(a) for a in nd[1:]]
        if nd[0] in _UNARY:
            expr = "-%s" % args[0] if nd[0] == "neg" else "%s(%s)" % (_UNARY[nd[0]], args[0])
        else:
            expr = "%s %s %s" % (args[0], _BINARY[nd[0]], args[1])
        if plain_from < tape.n_in and all(a in plain or tape.is_const(a) for a in nd[1:]):
            plain.add(i)
        lines.append("    const %s w%d = %s;" % ("double" if i in plain else "T", i, expr)); ref[i] = "w%d" % i
        for r in outs_of.get(i, ()):
            lines.append("    out(%d, %sw%d);" % (r, "T{} + " if i in plain else "", i))
    for r, o in enumerate(tape.outputs):
        nd = tape.nodes[o]
        if nd[0] == "const":
            lines.append("    out(%d, T{} + %s);" % (r, _lit(nd[1])))
        elif nd[0] == "in":
            lines.append("    out(%d, %s%s);" % (r, "T{} + " if nd[1] >= plain_from else "", use(o)))
    return "\n".join(lines)


def _blit(v):
    return "INFINITY" if v == float("inf") else "-INFINITY" if v == float("-inf") else _lit(v)


def emit_functor(tape, name="SmUser"):
    """C++ source of the functor (same shape as the zoo's functors in csrc/stage_models.hpp)"""
    nh = getattr(tape, "nh", 0)
    nk = getattr(tape, "nk", 0)
    cost = getattr(tape, "cost", None)
    hbody = _emit_body(tape.path) if nh else ""
    kbody = _emit_body(tape.link) if nk else ""
    nth = getattr(tape, "ntheta", 0)
    nsd = getattr(tape, "nsd", 0)
    dsig = "const double *d, " if nsd else ""      # (nsd > 0: H, L, LG, LT, LTG take the frame's stage-data row d behind their inputs)
    tsig = "const double *d, " if getattr(tape, "tdata", False) else ""      # (transition_data: so do F, K, LK, LKG and FG, the row of the first frame)
    # (ntheta > 0: the plant parameters are par[i] in F's body -- data of the launch, sd.par or the instance's row)
    fmt = ("struct %s {\n  static constexpr int nx = %d, nu = %d, nh = %d, nk = %d, has_cost = %d, has_term = %d;\n"
           + ("  static constexpr int ntheta = %d;\n" % nth if nth else "")
           + ("  static constexpr int nsd = %d;\n  static constexpr double sdata0[%d] = {%s};\n" % (nsd, nsd, ", ".join(_lit(v) for v in tape.sdata0)) if nsd else "")
           + ("  static constexpr int tdata = 1;\n" if tsig else "") +
           "  template <class T> SM_HD static void F(const double *" + ("par" if nth else "") + ", double, const T *s, const T *u, " + tsig + "T *out) {\n%s\n  }\n"
           "  template <class T> SM_HD static void H(const T *s, const T *u, " + dsig + "T *out) {\n%s\n  }\n"
           "  template <class T> SM_HD static void K(const T *s, const T *u, const T *sn, const T *un, " + tsig + "T *out) {\n%s\n  }\n")
    src = fmt % (name, tape.nx, tape.nu, nh, nk, 1 if cost else 0, 1 if cost and cost["LT"] is not None else 0, _emit_body(tape), hbody, kbody)
    if cost:
        # L: out[0] = l(s, u, r); LG: out[nx + nu + nx] = dl / d[s; u; r]; LT, LTG: the terminal frame's
        for fn, tp in (("L", cost["L"]), ("LG", cost["G"]), ("LT", cost["LT"] or cost["L"]), ("LTG", cost["GT"] or cost["G"])):
            src += "  template <class T> SM_HD static void %s(const T *s, const T *u, const T *r, %sT *out) {\n%s\n  }\n" % (fn, dsig, _emit_body(tp))
    res = getattr(tape, "residual", None)
    if res:
        # R: out[nr] = the residual; RT: out[nx + nu + nx] = J' w over [s; u; r], the weights w plain doubles like d; RTm, RTT: the terminal frame's
        # (nrt rows).  L, LG above are sum r_i^2 and its gradient: the Hessian 2 J'J is formed from R and RT (sm_residual_column)
        src += "  static constexpr int has_residual = 1, nr = %d, nrt = %d;\n" % (res["nr"], res["nrt"])
        for fn, tp, wsig in (("R", res["R"], ""), ("RT", res["RT"], "const double *w, "), ("RTm", res["Rm"] or res["R"], ""),
                             ("RTT", res["RTT"] or res["RT"], "const double *w, ")):
            src += "  template <class T> SM_HD static void %s(const T *s, const T *u, const T *r, %s%sT *out) {\n%s\n  }\n" % (fn, dsig, wsig, _emit_body(tp))
    if getattr(tape, "pref", False):
        src += "  static constexpr bool pref = true;\n"
    link_cost = getattr(tape, "link_cost", None)
    if link_cost:
        # LK: out[0] = llink(s, u, sn, un); LKG: out[2 f] = its gradient over [s; u; sn; un]; lmask: the structure of its Hessian, row-major (2 f)^2
        src += "  static constexpr int has_link_cost = 1;\n"
        for fn, tp in (("LK", link_cost["L"]), ("LKG", link_cost["G"])):
            src += "  template <class T> SM_HD static void %s(const T *s, const T *u, const T *sn, const T *un, %sT *out) {\n%s\n  }\n" % (fn, tsig, _emit_body(tp))
        lm = link_cost["mask"]
        src += "  static constexpr unsigned char lmask[%d] = {%s};\n" % (lm.size, ", ".join(str(int(v)) for v in lm.ravel()))
    exact = getattr(tape, "exact", None)
    if exact:
        # FG: out[f] = d(lam' F)/d[s; u]; HG: out[f] = d(mu' H)/d[s; u] -- the multipliers are plain doubles like par and d (mpcqp_stage_lagrangian)
        src += "  static constexpr int has_exact = 1;\n"
        src += ("  template <class T> SM_HD static void FG(const double *" + ("par" if nth else "") + ", double, const T *s, const T *u, const double *lam, " + tsig + "T *out) {\n%s\n  }\n"
                % _emit_body(exact["FG"]))
        if exact["HG"] is not None:
            src += "  template <class T> SM_HD static void HG(const T *s, const T *u, const double *mu, %sT *out) {\n%s\n  }\n" % (dsig, _emit_body(exact["HG"]))
    src += "};\n"
    lo = ", ".join(_blit(v) for v in tape.h_lo) if nh else "0.0"
    hi = ", ".join(_blit(v) for v in tape.h_hi) if nh else "0.0"
    src += "static const double %s_h_lo[] = {%s};\nstatic const double %s_h_hi[] = {%s};\n" % (name, lo, name, hi)
    klo = ", ".join(_blit(v) for v in tape.k_lo) if nk else "0.0"
    khi = ", ".join(_blit(v) for v in tape.k_hi) if nk else "0.0"
    src += "static const double %s_k_lo[] = {%s};\nstatic const double %s_k_hi[] = {%s};\n" % (name, klo, name, khi)
    mk = ", ".join(str(int(v)) for v in cost["mask"].ravel()) if cost else "0"
    src += "static const unsigned char %s_cost_mask[] = {%s};\n" % (name, mk)
    if nth:
        src += "static const double %s_theta0[] = {%s};\n" % (name, ", ".join(_lit(v) for v in tape.theta0))
    if nsd:
        src += "static const double %s_sdata0[] = {%s};\n" % (name, ", ".join(_lit(v) for v in tape.sdata0))
    if exact:
        src += "static const unsigned char %s_curv_mask[] = {%s};\n" % (name, ", ".join(str(int(v)) for v in exact["mask"].ravel()))
    return src


# The launchers, one per operation: (the handle's constants, batch, the argument block, ..., the rows, the stream).  stage_with_rows (stage_kernels.hpp)
# picks the kernel instance that takes the rows from the functor's members, so the text is the same for every kind of data a model declares.
# pf: the launchers' PF template argument, written after SmUser; pref: the export mpcqp_user_pref of a tracking library
_DEVICE_TMPL = '''// generated by optimal_control_problem_amd/codegen.py -- do not edit
#include "stage_kernels.hpp"

%(functor)s
extern "C" {
int mpcqp_user_abi() { return STAGE_ABI_VERSION; }
void mpcqp_user_dims(int *nx, int *nu) { *nx = SmUser::nx; *nu = SmUser::nu; }
%(pref)sint mpcqp_user_nh() { return SmUser::nh; }
void mpcqp_user_path_bounds(double *lo, double *hi) { for (int i = 0; i < SmUser::nh; i++) { lo[i] = SmUser_h_lo[i]; hi[i] = SmUser_h_hi[i]; } }
int mpcqp_user_nk() { return SmUser::nk; }
void mpcqp_user_link_bounds(double *lo, double *hi) { for (int i = 0; i < SmUser::nk; i++) { lo[i] = SmUser_k_lo[i]; hi[i] = SmUser_k_hi[i]; } }
// general stage cost: 1 and the Hessian's structure over [s; u; r] (row-major (f + nx)^2 bytes), or 0 for diagonal tracking weights
int mpcqp_user_cost(unsigned char *mask) {
  if (!SmUser::has_cost) return 0;
  const int nl = 2 * SmUser::nx + SmUser::nu;
  for (int i = 0; i < nl * nl; i++) mask[i] = SmUser_cost_mask[i];
  return 1;
}
int mpcqp_user_eval(const StageDev *sd, int batch, const StageEvalArgs *a, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_eval<SmUser%(pf)s>(*sd, batch, *a, (hipStream_t)stream, pp...); });
}
int mpcqp_user_merit(const StageDev *sd, int batch, const StageMeritArgs *a, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_merit<SmUser%(pf)s>(*sd, batch, *a, (hipStream_t)stream, pp...); });
}
// the hand-over between two MPC ticks (mpcqp_stage_advance)
int mpcqp_user_advance(const StageDev *sd, int batch, const mpcqp_stage_advance_args *a, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_advance<SmUser%(pf)s>(*sd, batch, *a, (hipStream_t)stream, pp...); });
}
// the per-instance merit line search (mpcqp_stage_linesearch)
int mpcqp_user_linesearch(const StageDev *sd, int batch, const mpcqp_stage_linesearch_args *a, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_linesearch<SmUser%(pf)s>(*sd, batch, *a, (hipStream_t)stream, pp...); });
}
%(params)s%(link_cost)s%(sdata)s%(tdata)s%(convexify)s%(exact)s%(residual)s}
'''

# the launcher of mpcqp_stage_rollout (one kernel instance for both kinds of reference: F reads none), a block of its own that library_source puts
# behind the translation unit of device_source: the text of device_source stays, byte for byte, what it was before this entry.  A library without
# the export -- every one generated before this entry, and library_source(tape, rollout=False) for the tests of that case -- answers MPCQP_ERR_LIMIT there
_DEVICE_ROLLOUT_TMPL = '''
// the dynamically feasible start (mpcqp_stage_rollout)
extern "C" int mpcqp_user_rollout(const StageDev *sd, int batch, const mpcqp_stage_rollout_args *a, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_rollout<SmUser>(*sd, batch, *a, (hipStream_t)stream, pp...); });
}
'''

# a model with exact_hessian = True only: 1 and the structure of the constraint curvature over [s; u] (row-major f^2 bytes), and the launcher of
# mpcqp_stage_lagrangian (slots: the handle's table of the curvature's slots; w: the convexification tables and scratch, used when a->mode != 0).
# A library without the exports takes no constraint curvature
_DEVICE_EXACT_TMPL = '''int mpcqp_user_exact_hessian(unsigned char *mask) {
  constexpr int f = SmUser::nx + SmUser::nu;
  for (int i = 0; i < f * f; i++) mask[i] = SmUser_curv_mask[i];
  return 1;
}
int mpcqp_user_lagrangian(const StageDev *sd, int batch, const mpcqp_stage_lagrangian_args *a, const int *slots, const StageCvxBuf *w, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, true>(*r, [&](auto... pp) { return stage_launch_lagrangian<SmUser, %(cvx)s%(pf)s>(*sd, batch, *a, slots, w, (hipStream_t)stream, pp...); });
}
'''

# a model with convexify = True only: the launcher of mpcqp_stage_convexify (w: the handle's slot tables and scratch; lcost and lterm read no
# parameters, so no instance takes them).  A library without the export takes no convexification
_DEVICE_CONVEXIFY_TMPL = '''int mpcqp_user_convexify(const StageDev *sd, int batch, const mpcqp_stage_convexify_args *a, const StageCvxBuf *w, const StageRows *r, void *stream) {
  return (int)stage_with_rows<SmUser, false>(*r, [&](auto... pp) { return stage_launch_convexify<SmUser%(pf)s>(*sd, batch, *a, *w, (hipStream_t)stream, pp...); });
}
'''

# a model with a Gauss-Newton frame cost (rcost) only: the number of residual rows.  A library without the export has a scalar cost or diagonal weights
_DEVICE_RESIDUAL_TMPL = '''int mpcqp_user_residual_cost() { return SmUser::nr; }
'''

# the host build of such a model: value by L / LT, every column of the gradient and of 2 J'J by the helper a device thread calls (sm_residual_column)
_HOST_RESIDUAL_TMPL = '''template <class M> static void host_cost_gn(const double *s, const double *u, const double *r, const double *d, int term, double *val, double *grad, double *hess) {
  constexpr int nx = M::nx, nu = M::nu, nl = 2 * nx + nu;
  double v[1];
  if (term) M::template LT<double>(s, u, r, %(d)sv); else M::template L<double>(s, u, r, %(d)sv);
  val[0] = v[0];
  for (int c = 0; c < nl; c++) {
    Dual sd[nx], ud[nu], rd[nx], gd[nl];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    for (int i = 0; i < nx; i++) rd[i] = {r[i], nx + nu + i == c ? 1.0 : 0.0};
    sm_residual_column<M, %(sd)s>(term != 0, sd, ud, rd, d, gd);
    for (int i = 0; i < nl; i++) hess[i * nl + c] = gd[i].d;
    grad[c] = gd[c].v;
  }
}
'''

# a model with a link cost (llink) only: 1 and the structure of its Hessian over [s; u; s_next; u_next] (row-major (2 f)^2 bytes).  A library
# without the export -- every one generated before this entry -- has no link cost
_DEVICE_LINK_COST_TMPL = '''int mpcqp_user_link_cost(unsigned char *mask) {
  constexpr int n2 = 2 * (SmUser::nx + SmUser::nu);
  for (int i = 0; i < n2 * n2; i++) mask[i] = SmUser::lmask[i];
  return 1;
}
'''

# a model with parameters (ntheta > 0) only: their count and their defaults (they become sd.par of the handle)
_DEVICE_PARAMS_TMPL = '''int mpcqp_user_ntheta() { return SmUser::ntheta; }
void mpcqp_user_theta0(double *par) { for (int i = 0; i < SmUser::ntheta; i++) par[i] = SmUser_theta0[i]; }
'''

# a model with stage data (nsd > 0) only: their count and their defaults.  Every kernel instance of such a library carries a StageData
_DEVICE_SDATA_TMPL = '''int mpcqp_user_nsd() { return SmUser::nsd; }
void mpcqp_user_sdata0(double *d) { for (int i = 0; i < SmUser::nsd; i++) d[i] = SmUser_sdata0[i]; }
'''

# a model with transition_data = True only: its F, K, LK, LKG and FG take the data row of the transition's first frame.  A library without the export --
# every one generated before this entry -- reads stage data in hfun and the frame costs only
_DEVICE_TDATA_TMPL = '''int mpcqp_user_transition_data() { return SmUser::tdata; }
'''

_HOST_TMPL = '''// generated by optimal_control_problem_amd/codegen.py -- host build of the same functor, for checks without a GPU
#include <cmath>
#include "stage_models.hpp"

%(functor)s
%(residual)s// val [1], grad [nl], hess [nl * nl] row-major over [s; u; r], nl = 2 nx + nu; term != 0: the terminal frame's cost
template <class M> static void host_cost(const double *s, const double *u, const double *r, int term, double *val, double *grad, double *hess) {
  if constexpr (M::has_cost != 0) {
    constexpr int nx = M::nx, nu = M::nu, nl = 2 * nx + nu;
    double v[1];
    if (term) M::template LT<double>(s, u, r, %(hd)sv); else M::template L<double>(s, u, r, %(hd)sv);
    val[0] = v[0];
    for (int c = 0; c < nl; c++) {
      Dual sd[nx], ud[nu], rd[nx], gd[nl];
      for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
      for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
      for (int i = 0; i < nx; i++) rd[i] = {r[i], nx + nu + i == c ? 1.0 : 0.0};
      if (term) M::template LTG<Dual>(sd, ud, rd, %(hd)sgd); else M::template LG<Dual>(sd, ud, rd, %(hd)sgd);
      for (int i = 0; i < nl; i++) { hess[i * nl + c] = gd[i].d; grad[i] = gd[i].v; }
    }
  }
}
extern "C" {
void user_host_dims(int *nx, int *nu) { *nx = SmUser::nx; *nu = SmUser::nu; }
// out [nx], jac [nx * (nx + nu)] row-major: forward-mode duals, one direction per pass (what a device thread does)
void user_host_eval(const double *s, const double *u, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], od[nx];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    SmUser::F<Dual>(%(theta0)s, 0.0, sd, ud, %(td)sod);
    for (int r = 0; r < nx; r++) { jac[r * f + c] = od[r].d; out[r] = od[r].v; }
  }
}
// the same with the parameter vector given (theta [ntheta]; a functor without parameters ignores it)
int user_host_ntheta() { return %(ntheta)d; }
void user_host_eval_theta(const double *theta, const double *s, const double *u, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], od[nx];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    SmUser::F<Dual>(theta, 0.0, sd, ud, %(td)sod);
    for (int r = 0; r < nx; r++) { jac[r * f + c] = od[r].d; out[r] = od[r].v; }
  }
}
int user_host_nh() { return SmUser::nh; }
int user_host_nk() { return SmUser::nk; }
// out [nk], jac [nk * 2 (nx + nu)] row-major over [s; u; s_next; u_next]
void user_host_link(const double *s, const double *u, const double *sn, const double *un, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu, nk = SmUser::nk;
  if constexpr (nk > 0) {
    for (int c = 0; c < 2 * f; c++) {
      Dual sd[nx], ud[nu], snd[nx], und[nu], od[nk];
      for (int i = 0; i < nx; i++) { sd[i] = {s[i], i == c ? 1.0 : 0.0}; snd[i] = {sn[i], f + i == c ? 1.0 : 0.0}; }
      for (int i = 0; i < nu; i++) { ud[i] = {u[i], nx + i == c ? 1.0 : 0.0}; und[i] = {un[i], f + nx + i == c ? 1.0 : 0.0}; }
      SmUser::K<Dual>(sd, ud, snd, und, %(td)sod);
      for (int r = 0; r < nk; r++) { jac[r * 2 * f + c] = od[r].d; out[r] = od[r].v; }
    }
  }
}
%(link_cost)sint user_host_has_cost() { return SmUser::has_cost; }
void user_host_cost(const double *s, const double *u, const double *r, int term, double *val, double *grad, double *hess) {
  %(cost_call)s;
}
// out [nh], jac [nh * (nx + nu)] row-major
void user_host_path(const double *s, const double *u, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu, nh = SmUser::nh;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], od[nh > 0 ? nh : 1];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    SmUser::H<Dual>(sd, ud, %(hd)sod);
    for (int r = 0; r < nh; r++) { jac[r * f + c] = od[r].d; out[r] = od[r].v; }
  }
}
%(sdata)s%(tdata)s%(exact)s}
'''

# a functor with exact_hessian only: C [f * f] row-major = -sum_i lam_i d2F_i + sum_i mu_i d2h_i over [s; u], column c by one pass of FG (dyn != 0) and
# HG on duals seeded on c, formed as -FG.d + HG.d (what a device thread does); theta [ntheta] and d [nsd] may be null = the defaults
_HOST_EXACT_TMPL = '''void user_host_curvature(const double *theta, const double *s, const double *u, const double *lam, const double *mu, const double *d, int dyn, double *C) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  (void)theta; (void)mu; (void)d;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], gf[f], gh[f];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    for (int r = 0; r < f; r++) { gf[r] = {0.0, 0.0}; gh[r] = {0.0, 0.0}; }
    if (dyn) SmUser::FG<Dual>(%(th)s, 0.0, sd, ud, lam, %(fd)sgf);
%(hg)s    for (int r = 0; r < f; r++) {
      double v = 0.0;
      if (dyn) v = -gf[r].d;
      if (SmUser::nh > 0) v += gh[r].d;
      C[r * f + c] = v;
    }
  }
}
'''

# a functor with stage data only: the path constraint and the cost with a data row d [nsd] given (the exports above use the defaults)
_HOST_SDATA_TMPL = '''int user_host_nsd() { return SmUser::nsd; }
void user_host_sdata0(double *d) { for (int i = 0; i < SmUser::nsd; i++) d[i] = SmUser_sdata0[i]; }
void user_host_path_d(const double *s, const double *u, const double *d, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu, nh = SmUser::nh;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], od[nh > 0 ? nh : 1];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    SmUser::H<Dual>(sd, ud, d, od);
    for (int r = 0; r < nh; r++) { jac[r * f + c] = od[r].d; out[r] = od[r].v; }
  }
}
}
template <class M> static void host_cost_d(const double *s, const double *u, const double *r, const double *d, int term, double *val, double *grad, double *hess) {
  if constexpr (M::has_cost != 0) {
    constexpr int nx = M::nx, nu = M::nu, nl = 2 * nx + nu;
    double v[1];
    if (term) M::template LT<double>(s, u, r, d, v); else M::template L<double>(s, u, r, d, v);
    val[0] = v[0];
    for (int c = 0; c < nl; c++) {
      Dual sd[nx], ud[nu], rd[nx], gd[nl];
      for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
      for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
      for (int i = 0; i < nx; i++) rd[i] = {r[i], nx + nu + i == c ? 1.0 : 0.0};
      if (term) M::template LTG<Dual>(sd, ud, rd, d, gd); else M::template LG<Dual>(sd, ud, rd, d, gd);
      for (int i = 0; i < nl; i++) { hess[i * nl + c] = gd[i].d; grad[i] = gd[i].v; }
    }
  }
}
extern "C" {
void user_host_cost_d(const double *s, const double *u, const double *r, const double *d, int term, double *val, double *grad, double *hess) {
  %(cost_d)s<SmUser>(s, u, r, d, term, val, grad, hess);
}
'''


# val [1], grad [2 f], hess [(2 f)^2] row-major over [s; u; s_next; u_next]: the gradient on duals, one direction per pass (what a device thread does)
_HOST_LINK_COST_TMPL = '''void user_host_link_cost(const double *s, const double *u, const double *sn, const double *un, double *val, double *grad, double *hess) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  SmUser::LK<double>(s, u, sn, un, %(td)sval);
  for (int c = 0; c < 2 * f; c++) {
    Dual sd[nx], ud[nu], snd[nx], und[nu], gd[2 * f];
    for (int i = 0; i < nx; i++) { sd[i] = {s[i], i == c ? 1.0 : 0.0}; snd[i] = {sn[i], f + i == c ? 1.0 : 0.0}; }
    for (int i = 0; i < nu; i++) { ud[i] = {u[i], nx + i == c ? 1.0 : 0.0}; und[i] = {un[i], f + nx + i == c ? 1.0 : 0.0}; }
    SmUser::LKG<Dual>(sd, ud, snd, und, %(td)sgd);
    for (int i = 0; i < 2 * f; i++) { hess[i * 2 * f + c] = gd[i].d; grad[i] = gd[i].v; }
  }
}
'''

# a functor with transition_data only: the dynamics with their Jacobian, the link rows and the link cost with a data row d [nsd] given (the exports
# above use the defaults); theta [ntheta] may be null = the defaults.  user_host_curvature takes its row already
_HOST_TDATA_TMPL = '''int user_host_transition_data() { return SmUser::tdata; }
void user_host_eval_d(const double *theta, const double *s, const double *u, const double *d, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  for (int c = 0; c < f; c++) {
    Dual sd[nx], ud[nu], od[nx];
    for (int i = 0; i < nx; i++) sd[i] = {s[i], i == c ? 1.0 : 0.0};
    for (int i = 0; i < nu; i++) ud[i] = {u[i], nx + i == c ? 1.0 : 0.0};
    SmUser::F<Dual>(%(th)s, 0.0, sd, ud, d, od);
    for (int r = 0; r < nx; r++) { jac[r * f + c] = od[r].d; out[r] = od[r].v; }
  }
}
void user_host_link_d(const double *s, const double *u, const double *sn, const double *un, const double *d, double *out, double *jac) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu, nk = SmUser::nk;
  if constexpr (nk > 0) {
    for (int c = 0; c < 2 * f; c++) {
      Dual sd[nx], ud[nu], snd[nx], und[nu], od[nk];
      for (int i = 0; i < nx; i++) { sd[i] = {s[i], i == c ? 1.0 : 0.0}; snd[i] = {sn[i], f + i == c ? 1.0 : 0.0}; }
      for (int i = 0; i < nu; i++) { ud[i] = {u[i], nx + i == c ? 1.0 : 0.0}; und[i] = {un[i], f + nx + i == c ? 1.0 : 0.0}; }
      SmUser::K<Dual>(sd, ud, snd, und, d, od);
      for (int r = 0; r < nk; r++) { jac[r * 2 * f + c] = od[r].d; out[r] = od[r].v; }
    }
  }
}
%(link_cost)s'''

_HOST_TDATA_LINK_COST_TMPL = '''void user_host_link_cost_d(const double *s, const double *u, const double *sn, const double *un, const double *d, double *val, double *grad, double *hess) {
  constexpr int nx = SmUser::nx, nu = SmUser::nu, f = nx + nu;
  SmUser::LK<double>(s, u, sn, un, d, val);
  for (int c = 0; c < 2 * f; c++) {
    Dual sd[nx], ud[nu], snd[nx], und[nu], gd[2 * f];
    for (int i = 0; i < nx; i++) { sd[i] = {s[i], i == c ? 1.0 : 0.0}; snd[i] = {sn[i], f + i == c ? 1.0 : 0.0}; }
    for (int i = 0; i < nu; i++) { ud[i] = {u[i], nx + i == c ? 1.0 : 0.0}; und[i] = {un[i], f + nx + i == c ? 1.0 : 0.0}; }
    SmUser::LKG<Dual>(sd, ud, snd, und, d, gd);
    for (int i = 0; i < 2 * f; i++) { hess[i * 2 * f + c] = gd[i].d; grad[i] = gd[i].v; }
  }
}
'''


def _private_dir(d):
    """d exists, belongs to this user and nobody else may write to it (a library found there is dlopen'ed)"""
    st = os.stat(d)
    return st.st_uid == os.getuid() and not (st.st_mode & 0o022)


def cache_dir():
    """MPCQP_CACHE_DIR, else <package>/_gen, else a per-user 0700 directory under the system temp dir (read-only installs).
    Libraries in it are loaded without a rebuild, so a directory another user could have prepared is never used."""
    import tempfile
    for d in (os.environ.get("MPCQP_CACHE_DIR"), os.path.join(_HERE, "_gen"),
              os.path.join(tempfile.gettempdir(), "mpcqp_gen_%d" % os.getuid())):
        if not d:
            continue
        try:
            os.makedirs(d, mode=0o700, exist_ok=True)
            if os.access(d, os.W_OK) and _private_dir(d):
                return d
        except OSError:
            pass
    raise RuntimeError("no private writable directory for generated dynamics libraries (set MPCQP_CACHE_DIR)")


def _build(src_text, suffix, cmd_prefix):
    # the key covers everything the library is compiled from: the generated source, every header it includes and the command
    deps = "".join(open(os.path.join(CSRC, f)).read() for f in ("stage_kernels.hpp", "stage_convexify.hpp", "general_kernels.hpp", "general_linesearch.hpp", "general_lagrangian.hpp", "stage_models.hpp", "common.hpp"))
    deps += open(os.path.join(_HERE, "..", "include", "mpcqp.h")).read()
    key = hashlib.sha256((src_text + deps + " ".join(cmd_prefix)).encode()).hexdigest()[:20]
    base = os.path.join(cache_dir(), "user_%s_%s" % (suffix, key))
    so, src = base + ".so", base + (".hip" if suffix == "dev" else ".cpp")
    if not os.path.exists(so):
        with open(src, "w") as fh:
            fh.write(src_text)
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(cmd_prefix + ["-I", CSRC, "-shared", "-fPIC", "-o", tmp, src])
        os.replace(tmp, so)
    return so


def device_source(tape):
    """the translation unit of a stage library but for the launcher library_source appends.  Traced with per_frame_reference: SmUser::pref, the PF = true kernel instances only, and the
    export mpcqp_user_pref() by which mpcqp_stage_create_tracking / _create_user tell the two kinds apart; else the text it always was"""
    pf = getattr(tape, "pref", False)
    convexify = bool(getattr(tape, "convexify", False))
    sub = {"pf": ", SmUser::pref" if pf else "", "pref": "int mpcqp_user_pref() { return SmUser::pref ? 1 : 0; }\n" if pf else "",
           "cvx": "true" if convexify else "false"}
    return _DEVICE_TMPL % dict(sub, functor=emit_functor(tape), params=_DEVICE_PARAMS_TMPL if getattr(tape, "ntheta", 0) else "",
                               link_cost=_DEVICE_LINK_COST_TMPL if getattr(tape, "link_cost", None) else "",
                               sdata=_DEVICE_SDATA_TMPL if getattr(tape, "nsd", 0) else "",
                               tdata=_DEVICE_TDATA_TMPL if getattr(tape, "tdata", False) else "", convexify=_DEVICE_CONVEXIFY_TMPL % sub if convexify else "",
                               exact=_DEVICE_EXACT_TMPL % sub if getattr(tape, "exact", None) else "",
                               residual=_DEVICE_RESIDUAL_TMPL if getattr(tape, "residual", None) else "")


def library_source(tape, rollout=True):
    """what build_device_library compiles: device_source(tape) and, behind it, the launcher mpcqp_user_rollout.  rollout=False (tests only) leaves
    the launcher and its kernel out: the text of a library generated before mpcqp_stage_rollout"""
    return device_source(tape) + (_DEVICE_ROLLOUT_TMPL if rollout else "")


def build_device_library(tape, rollout=True):
    """gfx950 shared library for mpcqp_stage_create_user / _create_tracking (hipcc cross-compiles without a GPU); cached by content.
    rollout=False (tests only): without the launcher of mpcqp_stage_rollout, which then answers MPCQP_ERR_LIMIT."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return _build(library_source(tape, rollout=rollout), "dev", [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950"])


def host_source(tape):
    """the translation unit of the host build (a functor with stage data: the exports without a data row use the defaults)"""
    nth, nsd = getattr(tape, "ntheta", 0), getattr(tape, "nsd", 0)
    res = bool(getattr(tape, "residual", None))      # (a Gauss-Newton cost: user_host_cost and user_host_cost_d go through host_cost_gn)
    tdata = bool(getattr(tape, "tdata", False))      # (transition_data: the forms without a row hand the defaults to F, K, LK, LKG; the _d forms take one)
    td = {"td": "SmUser_sdata0, " if tdata else ""}
    link_cost = bool(getattr(tape, "link_cost", None))
    return _HOST_TMPL % {"functor": emit_functor(tape), "ntheta": nth, "theta0": "SmUser_theta0" if nth else "nullptr", "td": td["td"],
                         "link_cost": _HOST_LINK_COST_TMPL % td if link_cost else "",
                         "tdata": _HOST_TDATA_TMPL % {"th": "theta ? theta : SmUser_theta0" if nth else "nullptr",
                                                      "link_cost": _HOST_TDATA_LINK_COST_TMPL if link_cost else ""} if tdata else "",
                         "hd": "SmUser_sdata0, " if nsd else "", "exact": _host_exact(tape, nth, nsd),
                         "sdata": _HOST_SDATA_TMPL % {"cost_d": "host_cost_gn" if res else "host_cost_d"} if nsd else "",
                         "residual": _HOST_RESIDUAL_TMPL % {"d": "d, " if nsd else "", "sd": "true" if nsd else "false"} if res else "",
                         "cost_call": ("host_cost_gn<SmUser>(s, u, r, %s, term, val, grad, hess)" % ("SmUser_sdata0" if nsd else "nullptr")) if res
                                      else "host_cost<SmUser>(s, u, r, term, val, grad, hess)"}


def _host_exact(tape, nth, nsd):
    exact = getattr(tape, "exact", None)
    if not exact:
        return ""
    hg = ""
    if exact["HG"] is not None:
        hg = "    SmUser::HG<Dual>(sd, ud, mu, %sgh);\n" % ("d ? d : SmUser_sdata0, " if nsd else "")
    return _HOST_EXACT_TMPL % {"th": "theta ? theta : SmUser_theta0" if nth else "nullptr", "hg": hg,
                               "fd": "d ? d : SmUser_sdata0, " if getattr(tape, "tdata", False) else ""}


def build_host_library(tape):
    return _build(host_source(tape), "host", ["g++", "-O2", "-std=c++17", "-ffp-contract=off"])


# ------------------------------------------------------------------------------------------------- general (non-stage) NLPs
# The local system of general_nlp.GeneralNLP on the device (reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77,100-120): one functor
# with the bodies F (cost), G (gradient) and C (constraints) over w = [p; x], instantiated into csrc/general_kernels.hpp.

# Largest accepted tape (operations of F, G and C together).  hipcc -O3 for gfx950 was timed on tapes of growing size (DESIGN 6.9 has the
# table): generation plus compilation of a tape of this size stays under two minutes, and the time grows faster than linearly beyond it.
GENERAL_TAPE_CAP = 6000


class TapeTooLarge(ValueError):
    """the general device evaluator refuses this problem; str(e) is the reason the facade keeps"""


def general_tape_size(model):
    """operations (neither inputs nor constants) of the bodies the general evaluator compiles"""
    count = lambda t: sum(1 for i in t.live_nodes() if t.nodes[i][0] not in ("in", "const")) if t is not None else 0
    # (a model built with exact_hessian=True also compiles the contracted gradient of its constraints, CG)
    return count(model._ftape) + count(model._gtape) + count(model._ctape) + count(getattr(model, "_cgtape", None))


def _ints(v, empty="-1"):
    v = [int(a) for a in np.asarray(v).ravel()]
    return ", ".join(str(a) for a in v) if v else empty


def emit_general(model, name="GnUser", cap=None):
    """C++ source of the functor of a general_nlp.GeneralNLP and its tables: dimensions, the CSC index arrays, the colour of every input for
    the Hessian and for the Jacobian, and the two slot tables (general_eval.compress)"""
    from .general_eval import compress
    cap = GENERAL_TAPE_CAP if cap is None else int(cap)
    size = general_tape_size(model)
    if size > cap:
        raise TapeTooLarge("the traced cost, gradient and constraints have %d operations, more than the %d the device evaluator compiles "
                           "in reasonable time" % (size, cap))
    c = compress(model)
    body = lambda t: _emit_body(t, streaming=True) if t is not None else ""
    fn = "  template <class T, class In, class Out> SM_HD static void %s(const In &in, const Out &out) {\n%s\n  }\n"
    src = ("struct %s {\n  static constexpr int n = %d, np = %d, nvar = %d, ng = %d, nnzP = %d, nnzA = %d, hp = %d, jp = %d;\n"
           % (name, model.n, model.np, model.nvar, model.ng, len(model.Pi), len(model.Ai), c["hp"], c["jp"]))
    # colour of every input (-1: the variable carries no derivative): the seed of pass `pass` is colour == pass
    src += "  GN_TABLE int hcol[%d] = {%s};\n  GN_TABLE int jcol[%d] = {%s};\n" % (model.n, _ints(c["hcol"]), model.n, _ints(c["jcol"]))
    src += fn % ("F", body(model._ftape)) + fn % ("G", body(model._gtape)) + fn % ("C", body(model._ctape if model.ng else None))
    if getattr(model, "exact_hessian", False):
        # CG: out(r) = d(sum_i mul(i) g_i)/dw_r, the multipliers plain doubles (mpcqp_nlp_lagrangian); ccol, cslot: colours and slots of the
        # curvature's structure in P's CSC; ccols, cptr, clist, cdiag: the walk of general_lagrangian.hpp over the columns with curvature
        tab = lambda nm, v: "  GN_TABLE int %s[%d] = {%s};\n" % (nm, max(np.asarray(v).size, 1), _ints(v))
        src += "  static constexpr int cp = %d, ncc = %d;\n" % (c["cp"], len(c["ccols"]))
        src += "".join(tab(nm, c[nm]) for nm in ("ccol", "cslot", "ccols", "cptr", "clist", "cdiag"))
        src += ("  template <class T, class In, class Mul, class Out> SM_HD static void CG(const In &in, const Mul &mul, const Out &out) {\n%s\n  }\n"
                % body(model._cgtape if c["cp"] else None))
    src += "};\n"
    for nm, v in (("Pp", model.Pp), ("Pi", model.Pi), ("Ap", model.Ap), ("Ai", model.Ai), ("hslot", c["hslot"]), ("jslot", c["jslot"])):
        src += "static const int %s_%s[] = {%s};\n" % (name, nm, _ints(v))
    src += "static const int %s_sizes[] = {%d, %d, %d, %d, %d, %d};\n" % (name, model.n + 1, len(model.Pi), model.n + 1, len(model.Ai),
                                                                       c["hp"] * model.n, c["jp"] * model.ng)
    return src


_GENERAL_COMMON = '''
static void gn_copy(int *dst, const int *src, int cnt) { if (dst) for (int i = 0; i < cnt; i++) dst[i] = src[i]; }
extern "C" {
// {nvar, np, ng, n, m, nnz(P), nnz(A), passes, Hessian passes}
void %(pre)s_dims(int *d) {
  d[0] = GnUser::nvar; d[1] = GnUser::np; d[2] = GnUser::ng; d[3] = GnUser::n; d[4] = GnUser::n + GnUser::ng; d[5] = GnUser::nnzP; d[6] = GnUser::nnzA;
  d[7] = GnUser::hp + GnUser::jp; d[8] = GnUser::hp;
}
// host arrays (NULL: skipped): Pp, Ap [n + 1], Pi [nnzP], Ai [nnzA], hcol, jcol [n], hslot [hp * n], jslot [jp * ng]
void %(pre)s_tables(int *Pp, int *Pi, int *Ap, int *Ai, int *hcol, int *jcol, int *hslot, int *jslot) {
  gn_copy(Pp, GnUser_Pp, GnUser_sizes[0]); gn_copy(Pi, GnUser_Pi, GnUser_sizes[1]); gn_copy(Ap, GnUser_Ap, GnUser_sizes[2]); gn_copy(Ai, GnUser_Ai, GnUser_sizes[3]);
  gn_copy(hslot, GnUser_hslot, GnUser_sizes[4]); gn_copy(jslot, GnUser_jslot, GnUser_sizes[5]);
  if (hcol) for (int i = 0; i < GnUser::n; i++) hcol[i] = GnUser::hcol[i];
  if (jcol) for (int i = 0; i < GnUser::n; i++) jcol[i] = GnUser::jcol[i];
}
}
'''

_GENERAL_DEVICE_TMPL = '''// generated by optimal_control_problem_amd/codegen.py (emit_general) -- do not edit
#include "general_kernels.hpp"
#define GN_TABLE static constexpr

namespace {      // (internal linkage: several generated libraries live in one process, each with its own GnUser)
%(functor)s}
''' + _GENERAL_COMMON % {"pre": "mpcqp_general"} + '''
extern "C" {
int mpcqp_general_abi() { return GENERAL_ABI_VERSION; }
int mpcqp_general_eval(const GnDev *gd, int batch, const double *p, const double *x, const double *lbx, const double *ubx,
                       const double *lbg, const double *ubg, double *P, double *q, double *A, double *l, double *u, void *stream) {
  return (int)general_launch_eval<GnUser>(*gd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, (hipStream_t)stream);
}
int mpcqp_general_merit(int batch, const double *p, const double *x, const double *lbg, const double *ubg, double *f, double *gmax, void *stream) {
  return (int)general_launch_merit<GnUser>(batch, p, x, lbg, ubg, f, gmax, (hipStream_t)stream);
}
%(linesearch)s%(lagrangian)s}
'''

# the optional export behind mpcqp_nlp_linesearch (found by dlsym: GnDev and GENERAL_ABI_VERSION are unchanged)
_GENERAL_DEVICE_LINESEARCH = '''// the per-instance merit line search (mpcqp_nlp_linesearch)
int mpcqp_general_linesearch(int batch, const mpcqp_nlp_linesearch_args *a, void *stream) {
  return (int)general_launch_linesearch<GnUser>(batch, *a, (hipStream_t)stream);
}
'''

# the optional export behind mpcqp_nlp_lagrangian, only in the library of a model built with exact_hessian=True
_GENERAL_DEVICE_LAGRANGIAN = '''// the exact Hessian of the Lagrangian (mpcqp_nlp_lagrangian)
int mpcqp_general_lagrangian(int batch, const mpcqp_nlp_lagrangian_args *a, void *stream) {
  return (int)general_launch_lagrangian<GnUser>(batch, *a, (hipStream_t)stream);
}
'''

# the same on the host, appended to the host build of a model built with exact_hessian=True
_GENERAL_HOST_LAGRANGIAN = '''
#include "general_lagrangian.hpp"
// GnSeededIn on the host, over p and x as the argument block carries them
struct HSeededPX { const double *p, *x; const int *col; int pass;
  Dual operator()(int k) const { return Dual{k < GnUser::np ? p[k] : x[k - GnUser::np], col[k] == pass ? 1.0 : 0.0}; } };
extern "C" {
// mpcqp_nlp_lagrangian for ONE instance on host arrays: the kernels' threads become a loop over the passes and one over the columns, with the same
// functor text, the same tables and the walk of csrc/general_lagrangian.hpp
void general_host_lagrangian(const mpcqp_nlp_lagrangian_args *a) {
  if (a->status && !gn_ls_status_ok(a->status[0])) return;
  if (GnUser::cp == 0) return;
  for (int pass = 0; pass < GnUser::cp; pass++)
    GnUser::CG<Dual>(HSeededPX{a->p, a->x, GnUser::ccol, pass}, GnMulIn{a->y + GnUser::n},
                     GnCurvOut{a->C ? a->C : a->P, GnUser::cslot + pass * GnUser::n, a->C == nullptr});
  if (a->C)
    for (int ci = 0; ci < GnUser::ncc; ci++) gn_lag_apply_column<GnUser>(ci, a->C, a->P, a->mode == MPCQP_NLP_DOMINANT, a->shift);
}
}
'''

_GENERAL_HOST_TMPL = '''// generated by optimal_control_problem_amd/codegen.py (emit_general) -- host build of the same functor, for checks without a GPU
#include <cmath>
#include "stage_models.hpp"
#include "general_linesearch.hpp"
#define GN_TABLE static constexpr

namespace {      // (internal linkage: several generated libraries live in one process, each with its own GnUser)
%(functor)s}
''' + _GENERAL_COMMON % {"pre": "general_host"} + '''
// the accessors and sinks of csrc/general_kernels.hpp, on the host, driven by a loop over the passes with the same tables
struct HSeededIn { const double *w; const int *col; int pass; Dual operator()(int k) const { return Dual{w[k], col[k] == pass ? 1.0 : 0.0}; } };
struct HValueIn { const double *w; double operator()(int k) const { return w[k]; } };
struct HHessOut { double *P, *q; const int *slot; bool first;
  void operator()(int r, Dual v) const { if (slot[r] >= 0) P[slot[r]] = v.d; if (first) q[r] = v.v; } };
struct HJacOut { double *A, *l, *u; const double *lbg, *ubg; const int *slot; bool first;
  void operator()(int r, Dual v) const { if (slot[r] >= 0) A[slot[r]] = v.d; if (first) { l[r] = lbg[r] - v.v; u[r] = ubg[r] - v.v; } } };
struct HCostOut { double *f; void operator()(int, double v) const { *f = v; } };
struct HViolationOut { const double *lbg, *ubg; double *gmax;
  void operator()(int r, double v) const { *gmax = std::fmax(*gmax, std::fmax(lbg[r] - v, v - ubg[r])); } };
extern "C" {
// one instance: w [n] = [p; x], lbx, ubx [nvar], lbg, ubg [ng] -> P [nnzP], q [n], A [nnzA], l, u [m]
void general_host_eval(const double *w, const double *lbx, const double *ubx, const double *lbg, const double *ubg,
                       double *P, double *q, double *A, double *l, double *u) {
  constexpr int n = GnUser::n, np = GnUser::np, ng = GnUser::ng;
  for (int pass = 0; pass < GnUser::hp; pass++)
    GnUser::G<Dual>(HSeededIn{w, GnUser::hcol, pass}, HHessOut{P, q, GnUser_hslot + pass * n, pass == 0});
  for (int pass = 0; pass < GnUser::jp; pass++)
    GnUser::C<Dual>(HSeededIn{w, GnUser::jcol, pass}, HJacOut{A, l + n, u + n, lbg, ubg, GnUser_jslot + pass * ng, pass == 0});
  for (int j = 0; j < n; j++) {
    A[GnUser_Ap[j]] = 1.0;
    l[j] = (j < np ? w[j] : lbx[j - np]) - w[j]; u[j] = (j < np ? w[j] : ubx[j - np]) - w[j];
  }
}
void general_host_merit(const double *w, const double *lbg, const double *ubg, double *f, double *gmax) {
  GnUser::F<double>(HValueIn{w}, HCostOut{f});
  *gmax = 0.0;
  if (GnUser::ng > 0) GnUser::C<double>(HValueIn{w}, HViolationOut{lbg, ubg, gmax});
}
}
// the line search's accessor and sink (GnCandidateIn, GnMeritOut) on the host
struct HCandidateIn { const double *p, *x, *d; double alpha; bool base;      // d: dx on a candidate, x on the base point, which never touches dx
  double operator()(int k) const {
    if (k < GnUser::np) return p[k];
    const double xv = x[k - GnUser::np], c = gn_ls_point(xv, alpha, d[k - GnUser::np]);
    return base ? xv : c;
  } };
struct HMeritOut { const double *lbg, *ubg; double *v, *gmax;
  void operator()(int r, double g) const { *gmax = std::fmax(*gmax, std::fmax(lbg[r] - g, g - ubg[r])); *v += gn_ls_outside(lbg[r], g, ubg[r]); } };
extern "C" {
// mpcqp_nlp_linesearch for ONE instance on host arrays: the kernel's lanes become a loop over the candidates, the rule is the same text
// (csrc/general_linesearch.hpp).  phis [candidates + 1] (optional): the merits, base point first, NaN where not evaluated; D_out (optional): the slope
void general_host_linesearch(const mpcqp_nlp_linesearch_args *a, double *phis, double *D_out) {
  constexpr int n = GnUser::n, np = GnUser::np, nvar = GnUser::nvar, ng = GnUser::ng, NC = MPCQP_LINESEARCH_MAX_CANDIDATES + 1;
  bool ok = true;
  if (a->status) ok = gn_ls_status_ok(a->status[0]);
  const int K = ok ? a->candidates : 0;
  const double *dx = a->dw + np;                      // (not read for an instance that is not ok)
  double cost[NC], vio[NC], gmx[NC], phi[NC];
  for (int j = 0; j <= K; j++) {
    cost[j] = 0.0; vio[j] = 0.0; gmx[j] = 0.0;
    const HCandidateIn in{a->p, a->x, j == 0 ? a->x : dx, j == 0 ? 0.0 : gn_ls_alpha(a->alpha0, a->beta, j - 1), j == 0};
    GnUser::F<double>(in, HCostOut{&cost[j]});
    if (ng > 0) GnUser::C<double>(in, HMeritOut{a->lbg, a->ubg, &vio[j], &gmx[j]});
    for (int i = 0; i < nvar; i++) vio[j] += gn_ls_outside(a->lbx[i], in(np + i), a->ubx[i]);
  }
  double qd = 0.0, ymax = 0.0;
  if (ok) {
    for (int i = 0; i < nvar; i++) qd += a->q[np + i] * dx[i];
    for (int i = np; i < n + ng; i++) ymax = std::fmax(ymax, std::fabs(a->y[i]));
  }
  const double mu = gn_ls_penalty(a->mu != nullptr, a->mu ? a->mu[0] : 0.0, a->mu_min, a->mu_factor, ok, ymax);
  for (int j = 0; j <= K; j++) phi[j] = gn_ls_merit(cost[j], mu, vio[j]);
  const double D = gn_ls_slope(qd, mu, vio[0]);
  int acc;
  const int sel = gn_ls_decide(K, a->candidates, a->alpha0, a->beta, a->c1, D, [&](int j) { return j <= K ? phi[j] : 0.0; }, &acc);
  const double alpha_sel = sel > 0 ? gn_ls_alpha(a->alpha0, a->beta, sel - 1) : 0.0;
  double mx = 0.0;
  if (sel > 0)
    for (int i = 0; i < nvar; i++) { a->x[i] = gn_ls_point(a->x[i], alpha_sel, dx[i]); mx = std::fmax(mx, std::fabs(alpha_sel * dx[i])); }
  if (a->mu && ok) a->mu[0] = mu;
  if (a->alpha_out) a->alpha_out[0] = alpha_sel;
  if (a->accepted) a->accepted[0] = acc;
  if (a->step_max) a->step_max[0] = mx;
  if (a->f_out) a->f_out[0] = cost[sel];
  if (a->gmax_out) a->gmax_out[0] = gmx[sel];
  if (a->phi) { a->phi[0] = phi[0]; a->phi[1] = phi[sel]; }
  if (phis) for (int j = 0; j <= a->candidates; j++) phis[j] = j <= K ? phi[j] : std::nan("");
  if (D_out) *D_out = D;
}
}
'''


def general_device_source(model, cap=None, line_search=True):
    """the translation unit of a general library; line_search=False leaves the export mpcqp_general_linesearch (and its kernel) out: the text of a
    library generated before mpcqp_nlp_linesearch.  A model built with exact_hessian=True adds the export mpcqp_general_lagrangian and its kernels"""
    return _GENERAL_DEVICE_TMPL % {"functor": emit_general(model, cap=cap), "linesearch": _GENERAL_DEVICE_LINESEARCH if line_search else "",
                                   "lagrangian": _GENERAL_DEVICE_LAGRANGIAN if getattr(model, "exact_hessian", False) else ""}


def build_general_device_library(model, cap=None, line_search=True):
    """gfx950 shared library for mpcqp_nlp_create (hipcc cross-compiles without a GPU); cached by content.  TapeTooLarge beyond the cap.
    line_search=False: without the line-search kernel (mpcqp_nlp_linesearch then answers MPCQP_ERR_LIMIT)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return _build(general_device_source(model, cap=cap, line_search=line_search), "dev", [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950"])


def general_host_source(model, cap=None):
    return _GENERAL_HOST_TMPL % {"functor": emit_general(model, cap=cap)} + (_GENERAL_HOST_LAGRANGIAN if getattr(model, "exact_hessian", False) else "")


def build_general_host_library(model, cap=None):
    return _build(general_host_source(model, cap=cap), "host", ["g++", "-O2", "-std=c++17", "-ffp-contract=off"])
