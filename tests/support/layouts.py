"""Caller-side memory layouts for the C ABI (include/mpcqp.h): logical [B, width] float64 arrays -> a backing buffer plus (pointer, stride in doubles).

The header promises that value arrays are instance-major with an arbitrary stride (0 shares one array across the batch), that host arrays are copied and device
arrays borrowed.  BatchQP can only hand over whole, dense allocations (stride = width or 0, the allocation's own base); the layouts here are what it cannot
produce:

  dense      stride = width, base on a 512-byte boundary of the allocation (behind the guard band): the control
  padded1/7  stride = width + 1 / + 7: every other row starts on an 8-byte but not 16-byte boundary
  offset1/3  base = the dense base + 1 / + 3 doubles, stride = width
  shared     stride 0, one row (refused when the rows differ)
  record     [P | q | A | l | u] of instance b side by side in one row of ONE buffer, one double of padding behind each field and an odd record
             length: the five strides are equal, the five pointers point into the record, the fields start at mixed alignments

Every double of a backing that is not a logical element -- pads, the doubles in front of an offset base, GUARD doubles before the first and behind the last
row -- holds a quiet NaN with a payload (POISON), so that a stray read becomes a wrong number, not a fault, and a stray write is seen: the backing keeps a
bit copy of itself, unchanged() compares pads and guards with it.  Host backings are NumPy arrays, device backings torch CUDA tensors made from them.

No GPU is needed to lay arrays out in host memory (tests/test_layouts.py)."""
import ctypes as C

import numpy as np

GUARD = 64
POISON = np.uint64(0x7FF8DEADBEEF0BAD)          # a quiet NaN
POISON32 = np.int32(0x7FF8DEAD)
MEM_HOST, MEM_DEVICE = 0, 1
SINGLE = ("dense", "padded1", "padded7", "offset1", "offset3")       # the layouts of one array on its own
_SHAPE = {"dense": (0, 0), "padded1": (0, 1), "padded7": (0, 7), "offset1": (1, 0), "offset3": (3, 0)}      # layout -> (doubles in front of the base, pad behind a row)
FIELDS = ("P", "q", "A", "l", "u")

assert np.isnan(np.array([POISON]).view(np.float64)[0])


class View:
    """what the C ABI takes for one array: pointer and stride (in doubles); .backing keeps the memory alive"""
    def __init__(self, backing, name, ptr, stride, width, rows):
        self.backing, self.name, self.ptr, self.stride, self.width, self.rows = backing, name, ptr, stride, width, rows

    def with_stride(self, stride):
        return View(self.backing, self.name, self.ptr, stride, self.width, self.rows)


class Backing:
    """one allocation holding one or more logical arrays; fields: name -> (first double, stride, width, rows)"""
    def __init__(self, host, fields, mem):
        self.mem, self.fields = mem, dict(fields)
        self.where = {}
        for k, (first, stride, width, rows) in self.fields.items():
            self.where[k] = np.zeros(len(host), dtype=bool)
            for b in range(rows):
                self.where[k][first + b * stride:first + b * stride + width] = True
        self.logical = np.logical_or.reduce(list(self.where.values()))
        self.bits = host.view(np.uint64).copy()
        if mem == MEM_DEVICE:
            import torch
            self.buf = torch.from_numpy(host).cuda()
            assert self.buf.data_ptr() % 256 == 0
            self._base = self.buf.data_ptr()
        else:
            self.buf = host
            self._base = host.ctypes.data

    def view(self, name):
        first, stride, width, rows = self.fields[name]
        return View(self, name, self._base + 8 * first, stride, width, rows)

    def host_copy(self):
        return self.buf.cpu().numpy() if self.mem == MEM_DEVICE else self.buf

    def read(self, name, batch):
        """the logical [batch, width] array as the library addresses it: row b at pointer + b * stride"""
        first, stride, width, _ = self.fields[name]
        h = self.host_copy()
        return np.stack([h[first + b * stride:first + b * stride + width] for b in range(batch)])

    def unchanged(self):
        """pads, the doubles in front of an offset base and the guard bands still hold exactly the bits they were created with"""
        now = np.ascontiguousarray(self.host_copy()).view(np.uint64)
        return bool(np.array_equal(now[~self.logical], self.bits[~self.logical]))

    def spoil(self, names=None, value=np.nan):
        """overwrite the logical elements of the named arrays, default all (the caller `frees` them: a copy has been taken, or the borrow has ended)"""
        mask = self.logical if names is None else np.logical_or.reduce([self.where[k] for k in names])
        if self.mem == MEM_DEVICE:
            import torch
            self.buf[torch.from_numpy(mask).cuda()] = value
            torch.cuda.synchronize()
        else:
            self.buf[mask] = value


def _poisoned(count):
    return np.full(count, POISON, dtype=np.uint64).view(np.float64)


def _as_rows(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2, "logical arrays are [B, width]"
    return a


def lay(a, layout, mem=MEM_HOST, name="a"):
    """one logical [B, width] array in one of SINGLE or `shared` -> View"""
    a = _as_rows(a)
    B, width = a.shape
    if layout == "shared":
        if not all(np.array_equal(a[0].view(np.uint64), a[b].view(np.uint64)) for b in range(B)):
            raise ValueError("%s: rows differ, the array cannot be shared (stride 0)" % name)
        lead, stride, rows = 0, 0, 1
    else:
        lead, pad = _SHAPE[layout]
        stride, rows = width + pad, B
    first = GUARD + lead
    host = _poisoned(first + (rows - 1) * stride + width + GUARD)
    for b in range(rows):
        host[first + b * stride:first + b * stride + width] = a[b]
    return Backing(host, {name: (first, stride, width, rows)}, mem).view(name)


def lay_record(arrays, mem=MEM_HOST):
    """arrays: name -> [B, width], the five of FIELDS (or fewer) -> name -> View, all into one buffer, one stride"""
    arrays = {k: _as_rows(v) for k, v in arrays.items()}
    B = next(iter(arrays.values())).shape[0]
    off, at = {}, 0
    for k, v in arrays.items():
        assert v.shape[0] == B
        off[k] = at
        at += v.shape[1] + 1          # (one poisoned double behind every field: the next one starts at another alignment)
    length = at if at % 2 else at + 1
    host = _poisoned(GUARD + B * length + GUARD)
    for k, v in arrays.items():
        for b in range(B):
            host[GUARD + b * length + off[k]:GUARD + b * length + off[k] + v.shape[1]] = v[b]
    bk = Backing(host, {k: (GUARD + off[k], length, v.shape[1], B) for k, v in arrays.items()}, mem)
    return {k: bk.view(k) for k in arrays}


def lay_all(arrays, layout, mem=MEM_HOST, shared=()):
    """name -> [B, width]  ->  name -> View in `layout` (one of SINGLE, or `record`); the names in `shared` at stride 0 instead"""
    if layout == "record":
        assert not shared
        return lay_record(arrays, mem)
    return {k: lay(v, "shared" if k in shared else layout, mem, k) for k, v in arrays.items()}


def backings(views):
    out = []
    for v in views.values() if isinstance(views, dict) else views:
        if v is not None and not any(v.backing is o for o in out):
            out.append(v.backing)
    return out


def unchanged(views):
    return all(b.unchanged() for b in backings(views))


def spoil(views):
    """overwrite the arrays behind these Views, and nothing else of a backing they share with others"""
    for v in views.values() if isinstance(views, dict) else views:
        if v is not None:
            v.backing.spoil([v.name])


# ---------------------------------------------------------------------------------------------- the C ABI with these pointers
def _args(views):
    out = []
    for v in views:
        out += [None, 0] if v is None else [v.ptr, v.stride]
    return out


def _mem_of(views, mem):
    for v in views:
        assert v is None or v.backing.mem == mem
    return mem


def raw_update(qp, entry, P, q, A, l, u, mem):
    """mpcqp_update / mpcqp_update_matrices (entry: "update" | "update_matrices") on qp's handle with the Views' pointers and strides (None: NULL, stride 0)
    -> the return code.  The backings are parked in qp._keep: borrowed memory outlives the call."""
    from optimal_control_problem_amd import _lib
    views = [P, q, A, l, u]
    fn = {"update": _lib.lib().mpcqp_update, "update_matrices": _lib.lib().mpcqp_update_matrices}[entry]
    rc = fn(qp._h, *_args(views), _mem_of(views, mem))
    qp._keep = [views]
    return rc


def raw_update_vectors(qp, q, l, u, mem):
    """mpcqp_update_vectors likewise; the backings join what qp._keep holds (a reduced handle reads P and A of the last update again)"""
    from optimal_control_problem_amd import _lib
    views = [q, l, u]
    rc = _lib.lib().mpcqp_update_vectors(qp._h, *_args(views), _mem_of(views, mem))
    qp._keep = list(qp._keep or []) + [views]
    return rc


def raw_create_presolved(ls, l, u, mem, **settings):
    """mpcqp_create_presolved with the Views' pointers and strides -> (return code, a BatchQP around the handle or None)"""
    from optimal_control_problem_amd import _lib
    from optimal_control_problem_amd.batch_qp import BatchQP
    qp = BatchQP.__new__(BatchQP)
    qp.n, qp.m, qp.batch = int(ls.n), int(ls.m), int(ls.batch)
    qp.Pp, qp.Pi, qp.Ap, qp.Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai))
    qp.settings = _lib.default_settings(**settings)
    qp._h, qp._keep, qp.nfixed, qp.polish = C.c_void_p(), [[l, u]], 0, False
    nf = C.c_int(0)
    rc = _lib.lib().mpcqp_create_presolved(qp.n, qp.m, qp.batch, qp.Pp.ctypes.data, qp.Pi.ctypes.data, qp.Ap.ctypes.data, qp.Ai.ctypes.data,
                                           l.ptr, l.stride, u.ptr, u.stride, _mem_of([l, u], mem), C.byref(qp.settings), C.byref(qp._h), C.byref(nf))
    qp.nfixed = int(nf.value)
    if rc:
        assert not qp._h.value
        return rc, None
    return rc, qp


_OUT = {"x": ("n", np.float64), "y": ("m", np.float64), "z": ("m", np.float64), "status": (1, np.int32), "iters": (1, np.int32), "info": (4, np.float64),
        "polish_status": (1, np.int32), "polish_info": (4, np.float64)}


def raw_get_device(qp, want, lead=1):
    """mpcqp_get / mpcqp_get_polish with MPCQP_MEM_DEVICE into device buffers that start `lead` elements behind a GUARD band and end in front of another, NULL
    for what is not in `want` -> (name -> the region written, as [B, per instance]; True iff every guard element of every buffer kept its bits)"""
    import torch
    from optimal_control_problem_amd import _lib
    bufs, ptr = {}, {}
    for k in want:
        per, dt = _OUT[k]
        per = getattr(qp, per) if isinstance(per, str) else per
        count = qp.batch * per
        host = np.full(GUARD + lead + count + GUARD, POISON if dt is np.float64 else POISON32, dtype=np.uint64 if dt is np.float64 else np.int32).view(dt)
        dev = torch.from_numpy(host).cuda()
        bufs[k] = (dev, host.copy(), count, per)
        ptr[k] = dev.data_ptr() + (GUARD + lead) * host.itemsize
    p = lambda k: ptr.get(k)
    if any(k in want for k in ("x", "y", "z", "status", "iters", "info")):
        _lib.check(_lib.lib().mpcqp_get(qp._h, p("x"), p("y"), p("z"), p("status"), p("iters"), p("info"), MEM_DEVICE))
    if "polish_status" in want or "polish_info" in want:
        _lib.check(_lib.lib().mpcqp_get_polish(qp._h, p("polish_status"), p("polish_info"), MEM_DEVICE))
    qp.sync(); torch.cuda.synchronize()
    out, intact = {}, True
    for k, (dev, before, count, per) in bufs.items():
        now = dev.cpu().numpy()
        a, b = GUARD + lead, GUARD + lead + count
        raw = np.uint64 if now.dtype == np.float64 else np.int32
        intact = intact and np.array_equal(now[:a].view(raw), before[:a].view(raw)) and np.array_equal(now[b:].view(raw), before[b:].view(raw))
        out[k] = now[a:b].reshape(qp.batch, per) if per != 1 else now[a:b].copy()
    return out, bool(intact)


def device_at_offset(a, lead):
    """a float64 array in device memory, its first element `lead` doubles behind a GUARD band -> (pointer, the tensor that owns the memory)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    host = _poisoned(GUARD + lead + a.size + GUARD)
    host[GUARD + lead:GUARD + lead + a.size] = a
    dev = torch.from_numpy(host).cuda()
    return dev.data_ptr() + 8 * (GUARD + lead), dev


def materialised(ls):
    """the five value arrays of a models.LocalSystem as [B, width] each (a matrix the workload shares is repeated)"""
    B = ls.batch
    width = dict(P=len(ls.Pi), q=ls.n, A=len(ls.Ai), l=ls.m, u=ls.m)
    return {k: np.array(np.broadcast_to(getattr(ls, k), (B, width[k])), dtype=np.float64) for k in FIELDS}


def shared_vector_batch(ls, name):
    """the batch with instance 0's `name` (one of q, l, u) for every instance and everything else the instances' own: what a caller passes `name` at
    stride 0 for.  The pinned rows (l = u = the instance's own value) would cross under another instance's bound, so the bound that stays the
    instance's own gives way there: u_b = max(u_b, l_0) under a shared l, l_b = min(l_b, u_0) under a shared u -- the pinned rows become ranges.
    -> the five arrays, `name` with repeated rows (the dense control's input).  tests/test_layouts.py holds the CPU oracle's statuses on these batches
    to a mix of solved and not solved."""
    a = materialised(ls)
    boxed = np.argwhere((a["l"] == 50.0) & (a["u"] == 60.0))          # problems.hard_stage_batch's primal-infeasible row, [50, 60]: out of reach from below ...
    a[name] = np.repeat(a[name][:1], ls.batch, axis=0)
    if name == "l":
        a["u"] = np.maximum(a["u"], a["l"])
        for b, i in boxed:                                            # ... under a shared l it is out of reach from above: u = max(l_0, -50)
            a["u"][b, i] = max(a["l"][b, i], -50.0)
    elif name == "u":
        a["l"] = np.minimum(a["l"], a["u"])
    return a
