"""GPU: strided, offset, shared and borrowed caller arrays on every kernel family -- the layout of the input must not change one bit of the output.

include/mpcqp.h promises that value arrays are instance-major with an arbitrary stride in doubles (0 shares one array across the batch), that MPCQP_MEM_HOST
values are copied (the caller may free them at once), that MPCQP_MEM_DEVICE pointers are borrowed until the next solve has completed, and that of P only the
entries with row <= col are used.  Every other GPU test reaches the C ABI through BatchQP, which hands over whole allocations at stride 0 or stride = width.
Here tests/support/layouts.py lays the arrays out as a caller may -- rows padded by 1 and 7 doubles, bases 1 and 3 doubles into an allocation, single arrays
shared, one record [P | q | A | l | u] per instance with one stride for all five -- in host and in device memory, with NaN in every double that is not a
logical element, and the C entry points are called with those pointers and strides.  The read sites this aims at: the five `io.X + b * io.sX` of
kernel_stream / kernel_resident / kernel_oc_split / kernel_oc_rescale / reduced.hpp, gather8 and rz_fill_p of the set-up kernel, the polish kernel's q,
mpcqp_validate_kernel, and the per-instance compaction branch of stage() in mpcqp.hip.

Inputs: problems.hard_stage_batch (8 / 6 / 4 / 4 instances, one primal and one dual infeasible) under default settings on the rows of
tests/test_gpu_settings.py ROWS, whose parity with the oracle that module asserts; so every comparison here is bitwise (NaN equal to NaN) against a control:
a fresh handle fed dense host arrays through BatchQP.  One test per row loops over the layouts on one handle.

Exclusions -- the combinations the header documents a refusal for; each is asserted with its error code, none is skipped:

  what                                                   refusal                              asserted in
  stream x mpcqp_keep_workspace / mpcqp_update_vectors   MPCQP_ERR_LIMIT at keep_workspace    test_update_vectors_on_a_kept_workspace[stream-*]
  mpcqp_update_matrices off the two-kernel on-chip form  MPCQP_ERR_LIMIT, handle as it was    test_update_matrices_elsewhere_is_refused_and_harmless
  mpcqp_solve_host x stride != width                     MPCQP_ERR_ARG                        test_solve_host_takes_dense_arrays_only
  shared P / A x batches whose matrices differ           the caller's data do not allow it    test_update_layout_changes_no_bit (lo.lay raises; the shared matrices run
                                                         (layouts.lay refuses)                on the double integrator in test_shared_matrices)

Found by reading, before the first run: with MPCQP_MEM_DEVICE a NULL P (nnz(P) = 0) or A went to the kernels as it was, while the set-up kernel's gathers load
element 0 for a phantom slot before discarding it (gather8, rz_fill_p: `in[max(src, 0)]`).  No pattern the on-chip families take today has an empty P, and the
other kernels load under the `src >= 0` test only, so nothing faulted; the device path now substitutes q as the host path always did (mpcqp.hip
set_problem_data, host code only) and test_null_pointers_for_empty_arrays_on_the_device_path runs the two edge problems.

FIRST RUN ON AN MI355X: 122 passed in 8.4 s (the slowest test 0.36 s, 1.6 s of set-up once).  Combinations compared bit for bit, as
test_zz_combinations_compared prints them with -s: a 450 (25 rows x 18) + 36 with shared matrices, b 322 (23 rows x 14) + 24 on reduced handles, c 48, d 20,
e 20, f 54, g 40: 1014 (leg, layout, memory) combinations, next to the refusals of the table above.  No comparison failed: no kernel and no branch of stage()
was found to read where it must not.  Before that run the module's logic was rehearsed on the CPU against a stand-in for the library that reads the caller's
memory through (pointer, stride) and solves with the oracle; with a stand-in that reads q at b * n whatever the stride, 97 of 120 tests fail there, tests a, b
and e among them.  The wall time of the whole `-m gpu` suite next to the commit before is not recorded here: see the commit message for what could be run.
"""
import functools
import itertools

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import layouts as lo
from tests.support import problems
from tests.test_gpu_rho_resume import BITS, _bitwise
from tests.test_gpu_settings import ALL_KNOBS, ROWS, _handle

pytestmark = pytest.mark.gpu

HOST, DEVICE = lo.MEM_HOST, lo.MEM_DEVICE
MEMS = (("host", HOST), ("device", DEVICE))
LAYOUTS = lo.SINGLE + ("record",)
LEG_ROWS = [(leg, wid) for leg, wid, _ in ROWS]
TWO_KERNEL = [("oc4", "q20"), ("oc4", "cp30"), ("oc8", "q50"), ("oc8", "cp100")]
NO_MATRICES = [(leg, wid) for leg, wid in LEG_ROWS if leg.startswith(("res", "gres")) or leg.endswith("-mono")]
REDUCED = [("oc4", "q20"), ("oc4", "cp30")]
POLISH_BITS = BITS + ("polish_status", "polish_info")

_CONTROL = {}        # key -> a control's results: computed once, never changed
_COMPARED = {}       # test -> (leg, layout, memory) combinations compared bit for bit


def _count(test, k=1):
    _COMPARED[test] = _COMPARED.get(test, 0) + k


def _frozen(r):
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _batch(wid):
    """-> (model, LocalSystem, its five arrays as [B, width] each)"""
    mdl, ls, _ = problems.hard_stage_batch(wid)
    return mdl, ls, _frozen(lo.materialised(ls))


@functools.lru_cache(maxsize=None)
def _shared_batch(wid, name):
    return _frozen(lo.shared_vector_batch(_batch(wid)[1], name))


@functools.lru_cache(maxsize=None)
def _second(wid):
    """the next linearisation of the workload, at x + 0.7 dx with dx from the CPU oracle (as tests/support/kept_scaling.py builds its sequences), with the
    primal-infeasible box of hard_stage_batch on it: new P, q, A, l, u on the same pattern"""
    name, N, B = problems.HARD_WORKLOADS[wid]
    mdl, ls, meta = models.make_workload(name, B, N=N)
    dx = problems.oracle_solve(ls, nthreads=8)["x"][:, mdl.np:]
    ls2 = mdl.local_system(meta["p"], meta["x_iterate"] + 0.7 * dx, meta["lbx"], meta["ubx"], meta["lbg"], meta["ubg"])
    a = lo.materialised(ls2)
    row = mdl.np + mdl.f
    a["l"][problems.PRIMAL_INFEASIBLE, row], a["u"][problems.PRIMAL_INFEASIBLE, row] = 50.0, 60.0
    assert not np.array_equal(a["A"], _batch(wid)[2]["A"]) and not np.array_equal(a["q"], _batch(wid)[2]["q"])
    return _frozen(a)


def _five(views):
    return [views[k] for k in lo.FIELDS]


def _vec(views):
    return [views[k] for k in ("q", "l", "u")]


def _ok(rc):
    from optimal_control_problem_amd import _lib
    _lib.check(rc)


def _dense(qp, a, entry="update"):
    {"update": qp.update, "update_matrices": qp.update_matrices}[entry](a["P"], a["q"], a["A"], a["l"], a["u"])


def _raw(qp, views, mem, entry="update"):
    """the entry point with the Views' pointers and strides; host arrays are overwritten with NaN as soon as it returns (`the caller may free at once`)"""
    _ok(lo.raw_update(qp, entry, *_five(views), mem))
    if mem == HOST:
        lo.spoil(views)


def _raw_vectors(qp, views, mem):
    _ok(lo.raw_update_vectors(qp, *_vec(views), mem))
    if mem == HOST:
        lo.spoil(views)


def _solved(qp):
    qp.solve()
    return qp.get()


def _control(monkeypatch, leg, wid, key, run, **kw):
    """what `run(fresh handle of the leg)` returns, once per (leg, wid, key)"""
    k = (leg, wid, key)
    if k not in _CONTROL:
        qp = _handle(monkeypatch, leg, wid, {}, _batch(wid)[1], **kw)
        try:
            out = run(qp)
        finally:
            qp.close()
        _CONTROL[k] = tuple(_frozen(r) for r in out) if isinstance(out, tuple) else _frozen(out)
    return _CONTROL[k]


def _plain(monkeypatch, leg, wid, arrays=None, key="plain", **kw):
    a = _batch(wid)[2] if arrays is None else arrays
    return _control(monkeypatch, leg, wid, key, lambda qp: (_dense(qp, a), _solved(qp))[1], **kw)


def _mixed(status):
    """statuses other than `solved` next to `solved`: a comparison that means something for certificates and for ordinary runs"""
    s = set(np.asarray(status).tolist())
    return 1 in s and len(s) > 1


# ---------------------------------------------------------------------------------------------- a. mpcqp_update
@pytest.mark.parametrize("leg,wid", LEG_ROWS)
def test_update_layout_changes_no_bit(built, monkeypatch, leg, wid):
    """every layout x {host, device} through mpcqp_update on one handle of the row: x, y, z, status, iters, info bitwise the dense host control's, pads and
    guards untouched; q, l, u each shared in turn on the batch that allows it (tests/test_layouts.py holds the oracle's statuses on those batches)"""
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    assert _mixed(want["status"]) and 3 in want["status"], want["status"]
    for k in ("P", "A"):                  # the exclusion: these matrices differ by instance, a caller cannot share them
        with pytest.raises(ValueError):
            lo.lay(arrays[k], "shared")
    shared = {name: (_shared_batch(wid, name), _plain(monkeypatch, leg, wid, _shared_batch(wid, name), key="shared " + name)) for name in ("q", "l", "u")}
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        for (mname, mem), layout in itertools.product(MEMS, LAYOUTS):
            views = lo.lay_all(arrays, layout, mem)
            _raw(qp, views, mem)
            _bitwise(_solved(qp), want, "%s %s: %s, %s" % (leg, wid, layout, mname))
            assert lo.unchanged(views), (leg, wid, layout, mname)
            _count("a")
        for (mname, mem), name in itertools.product(MEMS, ("q", "l", "u")):
            a, want_s = shared[name]
            assert _mixed(want_s["status"]), (name, want_s["status"])
            views = lo.lay_all(a, "padded1", mem, shared=(name,))
            assert views[name].stride == 0
            _raw(qp, views, mem)
            _bitwise(_solved(qp), want_s, "%s %s: %s shared, %s" % (leg, wid, name, mname))
            assert lo.unchanged(views), (leg, wid, name, mname)
            _count("a")
    finally:
        qp.close()


FAMILIES = [("rule", {}, 20, 32, 2), ("stream", dict(MPCQP_VARIANT="stream"), 20, 32, 0), ("res4", dict(MPCQP_VARIANT="res4"), 20, 32, 4),
            ("gres4", dict(MPCQP_VARIANT="gres4"), 20, 32, 104), ("oc4", dict(MPCQP_VARIANT="oc4"), 20, 32, 204), ("oc8", dict(MPCQP_VARIANT="oc8"), 6, 8, 208)]


@pytest.mark.parametrize("fam,env,N,B,variant", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_shared_matrices(built, monkeypatch, fam, env, N, B, variant):
    """P and A at stride 0, each alone and both, next to padded q, l, u: on the double integrator, whose instances have equal matrices"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    _, ls, _ = models.make_workload("double_integrator", B, N=N)
    arrays = lo.materialised(ls)
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = []
    for _ in range(2):
        qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
        assert qp.plan_info()["variant"] == variant
        out.append(qp)
    ctl, qp = out
    try:
        _dense(ctl, arrays); want = _solved(ctl)
        assert (want["status"] == 1).any()
        for (mname, mem), which in itertools.product(MEMS, (("P",), ("A",), ("P", "A"))):
            views = lo.lay_all(arrays, "padded1", mem, shared=which)
            _raw(qp, views, mem)
            _bitwise(_solved(qp), want, "%s: %s shared, %s" % (fam, "+".join(which), mname))
            assert lo.unchanged(views)
            _count("a, shared matrices")
    finally:
        ctl.close(); qp.close()


# ---------------------------------------------------------------------------------------------- b. kept workspace
def _kept_control(qp, a, q2):
    """full solve -> vectors (q2) -> vectors (the first q again): the three results"""
    qp.keep_workspace(True)
    _dense(qp, a); r1 = _solved(qp)
    qp.update_vectors(q2, a["l"], a["u"]); r2 = _solved(qp)
    qp.update_vectors(a["q"], a["l"], a["u"]); r3 = _solved(qp)
    return r1, r2, r3


@pytest.mark.parametrize("leg,wid", LEG_ROWS)
def test_update_vectors_on_a_kept_workspace(built, monkeypatch, leg, wid):
    """a full solve from device arrays; once it has completed the borrow has ended: all five arrays are overwritten with NaN.  Then q, l, u in every layout and
    both memory spaces: bitwise the control's kept solve.  Every layout starts from a full solve again (a kept solve starts from the rho the one before left).
    Last, on the same handle: device update -> host vectors -> device vectors against the control's same chain."""
    from optimal_control_problem_amd import _lib
    _, ls, arrays = _batch(wid)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        if leg == "stream":              # the exclusion: the streaming kernel keeps no workspace
            with pytest.raises(_lib.MpcqpError) as e:
                qp.keep_workspace(True)
            assert e.value.code == _lib.ERR_LIMIT
            views = lo.lay_all(arrays, "padded1", DEVICE)
            _raw(qp, views, DEVICE); first = _solved(qp)
            assert lo.raw_update_vectors(qp, *_vec(views), DEVICE) == _lib.ERR_STATE          # (not kept: the call order is refused, and the handle goes on)
            _bitwise(_solved(qp), first, "stream: solve after the refusals"); _bitwise(first, _plain(monkeypatch, leg, wid), "stream")
            return
        q2 = problems.kept_q(ls)
        w1, w2, w3 = _control(monkeypatch, leg, wid, "kept", lambda c: _kept_control(c, arrays, q2))
        assert _mixed(w2["status"]) and not np.array_equal(w1["x"], w2["x"], equal_nan=True)
        vectors = dict(q=q2, l=arrays["l"], u=arrays["u"])
        qp.keep_workspace(True)
        for (mname, mem), layout in itertools.product(MEMS, LAYOUTS):
            full = lo.lay_all(arrays, "dense", DEVICE)
            _raw(qp, full, DEVICE); r1 = _solved(qp); qp.sync()
            lo.spoil(full)               # the borrow has ended: P and A are not the caller's to keep valid, the old q, l, u neither
            views = lo.lay_all(vectors, layout, mem)
            _raw_vectors(qp, views, mem)
            tag = "%s %s kept: %s, %s" % (leg, wid, layout, mname)
            _bitwise(r1, w1, tag + " (full solve)"); _bitwise(_solved(qp), w2, tag)
            assert lo.unchanged(views) and lo.unchanged(full), tag
            _count("b")
        full = lo.lay_all(arrays, "offset1", DEVICE)
        _raw(qp, full, DEVICE); _bitwise(_solved(qp), w1, "chain, device update"); qp.sync(); lo.spoil(full)
        v2 = lo.lay_all(vectors, "padded7", HOST)
        _raw_vectors(qp, v2, HOST); _bitwise(_solved(qp), w2, "chain, host vectors")
        v3 = lo.lay_all(dict(vectors, q=arrays["q"]), "record", DEVICE)
        _raw_vectors(qp, v3, DEVICE); _bitwise(_solved(qp), w3, "chain, device vectors")
        assert lo.unchanged(full) and lo.unchanged(v2) and lo.unchanged(v3)
        _count("b", 2)
    finally:
        qp.close()


@pytest.mark.parametrize("leg,wid", REDUCED)
def test_reduced_handle_reads_strided_matrices_again(built, monkeypatch, leg, wid):
    """mpcqp_create_reduced: mpcqp_presolve_kernel and mpcqp_postsolve_kernel read the caller's five arrays with their strides, and mpcqp_update_vectors reads
    P and A of the last update AGAIN -- those stay valid (device memory: borrowed on), only the old q, l, u are overwritten"""
    mdl, ls, arrays = _batch(wid)
    rows = list(range(mdl.np))
    q2 = problems.kept_q(ls)
    w1, w2, _ = _control(monkeypatch, leg, wid, "reduced kept", lambda c: _kept_control(c, arrays, q2), fixed_rows=rows)
    assert _mixed(w1["status"]) and _mixed(w2["status"])
    vectors = dict(q=q2, l=arrays["l"], u=arrays["u"])
    qp = _handle(monkeypatch, leg, wid, {}, ls, fixed_rows=rows)
    try:
        qp.keep_workspace(True)
        for (mname, mem), layout in itertools.product(MEMS, LAYOUTS):
            tag = "%s %s reduced: %s, %s" % (leg, wid, layout, mname)
            full = lo.lay_all(arrays, layout, mem)
            _raw(qp, full, mem); _bitwise(_solved(qp), w1, tag + " (full solve)"); qp.sync()
            if mem == DEVICE:
                lo.spoil(_vec(full))
            views = lo.lay_all(vectors, layout, mem)
            _raw_vectors(qp, views, mem); _bitwise(_solved(qp), w2, tag)
            assert lo.unchanged(views) and lo.unchanged(full), tag
            _count("b, reduced")
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- c. mpcqp_update_matrices
def _matrices_control(qp, a1, a2, q3):
    qp.keep_workspace(True)
    _dense(qp, a1); r1 = _solved(qp)
    _dense(qp, a2, "update_matrices"); r2 = _solved(qp)
    qp.update_vectors(q3, a2["l"], a2["u"]); r3 = _solved(qp)
    return r1, r2, r3


@pytest.mark.parametrize("leg,wid", TWO_KERNEL)
def test_update_matrices_layouts(built, monkeypatch, leg, wid):
    """new P, q, A, l, u on the kept scaling (mpcqp_oc_rescale_kernel reads the caller's arrays) in every layout and both memory spaces, mpcqp_update_vectors
    in a padded layout on top: bitwise the control's same chain from dense arrays"""
    _, ls, a1 = _batch(wid)
    a2 = _second(wid)
    q3 = a2["q"] * (1.0 + 0.1 * np.random.default_rng(17).standard_normal(a2["q"].shape))          # (problems.kept_q's rule on the second QP)
    w1, w2, w3 = _control(monkeypatch, leg, wid, "matrices", lambda c: _matrices_control(c, a1, a2, q3))
    assert _mixed(w2["status"]) and not np.array_equal(w1["x"], w2["x"], equal_nan=True) and not np.array_equal(w2["x"], w3["x"], equal_nan=True)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        qp.keep_workspace(True)
        for (mname, mem), layout in itertools.product(MEMS, LAYOUTS):
            tag = "%s %s update_matrices: %s, %s" % (leg, wid, layout, mname)
            _dense(qp, a1); _bitwise(_solved(qp), w1, tag + " (full solve)")
            views = lo.lay_all(a2, layout, mem)
            _raw(qp, views, mem, "update_matrices"); _bitwise(_solved(qp), w2, tag)
            qp.sync()
            if mem == DEVICE:
                lo.spoil(views)          # the borrow has ended
            v3 = lo.lay_all(dict(q=q3, l=a2["l"], u=a2["u"]), "padded7", mem)
            _raw_vectors(qp, v3, mem); _bitwise(_solved(qp), w3, tag + ", vectors on top")
            assert lo.unchanged(views) and lo.unchanged(v3), tag
            _count("c")
    finally:
        qp.close()


@pytest.mark.parametrize("leg,wid", NO_MATRICES)
def test_update_matrices_elsewhere_is_refused_and_harmless(built, monkeypatch, leg, wid):
    """the exclusion: off the two-kernel on-chip form mpcqp_update_matrices answers MPCQP_ERR_LIMIT and leaves the handle as it was -- the next plain solve is
    the control's, although the arrays offered were all NaN"""
    from optimal_control_problem_amd import _lib
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        qp.keep_workspace(True)
        _dense(qp, arrays); _bitwise(_solved(qp), want, "%s %s" % (leg, wid))
        for mname, mem in MEMS:
            views = lo.lay_all({k: np.full_like(v, np.nan) for k, v in arrays.items()}, "padded1", mem)
            assert lo.raw_update(qp, "update_matrices", *_five(views), mem) == _lib.ERR_LIMIT
            _bitwise(_solved(qp), want, "%s %s after the refusal, %s" % (leg, wid, mname))
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- d. Ruiz registers
@pytest.mark.parametrize("regs", ("registers", "MPCQP_NO_RUIZ_REGS=1"))
@pytest.mark.parametrize("leg,wid", [("oc4", "q20"), ("oc8", "q50")])
def test_ruiz_registers_on_and_off(built, monkeypatch, leg, wid, regs):
    """rz_fill_p gathers P straight from the caller's array; with the switch every wave walks the staged copy instead.  Both read padded, offset and record
    device layouts to the control's bits (tests/test_gpu_ruiz_registers.py holds on and off to each other on dense input)"""
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    if regs != "registers":
        monkeypatch.setenv("MPCQP_NO_RUIZ_REGS", "1")
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        for layout in ("padded1", "padded7", "offset1", "offset3", "record"):
            views = lo.lay_all(arrays, layout, DEVICE)
            _raw(qp, views, DEVICE)
            _bitwise(_solved(qp), want, "%s %s %s: %s" % (leg, wid, regs, layout))
            assert lo.unchanged(views)
            _count("d")
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- e. polish
def _polished(qp, a):
    qp.set_polish(True)
    _dense(qp, a)
    return _solved(qp)


@pytest.mark.parametrize("leg,wid", [("res4", "q20"), ("oc4", "q20")])
def test_polish_reads_q_with_its_stride(built, monkeypatch, leg, wid):
    """the polish kernel reads the caller's q (po.q + b * po.sq) behind the solve: padded, offset and shared q, host and device"""
    _, ls, arrays = _batch(wid)
    want = _control(monkeypatch, leg, wid, "polish", lambda c: _polished(c, arrays))
    sh = _shared_batch(wid, "q")
    want_s = _control(monkeypatch, leg, wid, "polish, shared q", lambda c: _polished(c, sh))
    for w in (want, want_s):
        assert (w["polish_status"] != 0).any() and (w["polish_status"] == 0).any(), w["polish_status"]          # polish attempts next to certificates
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        qp.set_polish(True)
        for (mname, mem), layout in itertools.product(MEMS, ("padded1", "padded7", "offset1", "offset3", "shared")):
            a, w = (sh, want_s) if layout == "shared" else (arrays, want)
            views = lo.lay_all(a, "dense", mem)
            views["q"] = lo.lay(a["q"], layout, mem, "q")
            _raw(qp, views, mem)
            _bitwise(_solved(qp), w, "%s %s polish: q %s, %s" % (leg, wid, layout, mname), keys=POLISH_BITS)
            assert lo.unchanged(views)
            _count("e")
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- f. P's lower triangle
def _lower_nan(ls, arrays):
    cols = np.repeat(np.arange(ls.n), np.diff(ls.Pp))
    lower = np.asarray(ls.Pi) > cols
    assert lower.sum() >= ls.n // 2          # the stage patterns carry both triangles: without entries below the diagonal this would test nothing
    P = arrays["P"].copy(); P[:, lower] = np.nan
    return dict(arrays, P=P)


@pytest.mark.parametrize("leg,wid", LEG_ROWS)
def test_lower_triangle_of_P_is_never_read(built, monkeypatch, leg, wid):
    """`only entries with row <= col are used`: NaN in every entry of P with row > col, host and device"""
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    spoilt = _lower_nan(ls, arrays)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        for mname, mem in MEMS:
            views = lo.lay_all(spoilt, "padded1", mem)
            _raw(qp, views, mem)
            _bitwise(_solved(qp), want, "%s %s: lower triangle NaN, %s" % (leg, wid, mname))
            _count("f")
    finally:
        qp.close()


@pytest.mark.parametrize("leg,wid", REDUCED)
def test_lower_triangle_of_P_on_a_reduced_handle(built, monkeypatch, leg, wid):
    mdl, ls, arrays = _batch(wid)
    rows = list(range(mdl.np))
    want = _plain(monkeypatch, leg, wid, key="reduced plain", fixed_rows=rows)
    spoilt = _lower_nan(ls, arrays)
    qp = _handle(monkeypatch, leg, wid, {}, ls, fixed_rows=rows)
    try:
        for mname, mem in MEMS:
            views = lo.lay_all(spoilt, "padded1", mem)
            _raw(qp, views, mem)
            _bitwise(_solved(qp), want, "%s %s reduced: lower triangle NaN, %s" % (leg, wid, mname))
            _count("f")
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- g. mpcqp_create_presolved
@pytest.mark.parametrize("wid", ("q20", "cp30"))
def test_create_presolved_reads_strided_bounds(built, monkeypatch, wid):
    """l, u of the first update in every layout, host and device, with different strides for the two and with one of them at stride 0: the rows found and the
    plan are the dense call's; a record-layout update and solve on the handle equals the dense presolved control"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    _, ls, arrays = _batch(wid)
    data = {"own": arrays, "l shared": _shared_batch(wid, "l"), "u shared": _shared_batch(wid, "u")}
    want = {}
    for key, a in data.items():
        ctl = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, presolve_bounds=(a["l"], a["u"]))
        try:
            assert 0 < ctl.nfixed < ls.n
            _dense(ctl, a); want[key] = (ctl.nfixed, ctl.plan_info(), _frozen(_solved(ctl)))
        finally:
            ctl.close()
    assert _mixed(want["own"][2]["status"])
    cases = [("own", layout, layout, ()) for layout in lo.SINGLE] + [("own", "record", "record", ()), ("own", "padded1", "padded7", ()), ("own", "offset3", "padded1", ()),
                                                                     ("l shared", "shared", "padded1", ("l",)), ("u shared", "offset1", "shared", ("u",))]
    for (mname, mem), (key, ll, lu, shared) in itertools.product(MEMS, cases):
        a = data[key]
        nfixed, plan, res = want[key]
        b = lo.lay_record(dict(l=a["l"], u=a["u"]), mem) if ll == "record" else dict(l=lo.lay(a["l"], ll, mem, "l"), u=lo.lay(a["u"], lu, mem, "u"))
        rc, qp = lo.raw_create_presolved(ls, b["l"], b["u"], mem)
        _ok(rc)
        try:
            tag = "%s presolved: l %s, u %s, %s" % (wid, ll, lu, mname)
            assert (qp.nfixed, qp.plan_info()) == (nfixed, plan), tag
            assert lo.unchanged(b), tag
            if mem == HOST:
                lo.spoil(b)              # `read once, here`
            views = lo.lay_all(a, "record", mem)
            _raw(qp, views, mem)
            _bitwise(_solved(qp), res, tag)
            assert lo.unchanged(views), tag
            _count("g")
        finally:
            qp.close()


# ---------------------------------------------------------------------------------------------- h. outputs and the other pointers
OUTPUTS = ("x", "y", "z", "status", "iters", "info")


def test_get_into_guarded_offset_device_buffers(built, monkeypatch):
    """mpcqp_get and mpcqp_get_polish with MPCQP_MEM_DEVICE in every combination of NULL and non-NULL outputs, the buffers 1 or 3 elements into an allocation:
    what is written equals the host get, and not one bit around it changes"""
    leg, wid = "oc4", "q20"
    _, ls, arrays = _batch(wid)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        qp.set_polish(True)
        _dense(qp, arrays); host = _solved(qp)
        host["info"] = np.stack([host[k] for k in ("obj", "prim_res", "dual_res", "rho")], axis=1)
        assert _mixed(host["status"])
        subsets = [s for r in range(1, len(OUTPUTS) + 1) for s in itertools.combinations(OUTPUTS, r)]
        assert len(subsets) == 63
        subsets += [("polish_status",), ("polish_info",), ("polish_status", "polish_info"), OUTPUTS + ("polish_status", "polish_info")]
        for k, want in enumerate(subsets):
            got, intact = lo.raw_get_device(qp, want, lead=1 + 2 * (k % 2))
            assert intact, want
            for name in want:
                assert np.array_equal(got[name], host[name], equal_nan=True), (want, name)
    finally:
        qp.close()


def test_warm_start_and_rho_from_offset_device_pointers(built, monkeypatch):
    """mpcqp_warm_start and mpcqp_set_rho borrow device pointers too: one double into an allocation against whole allocations"""
    import torch
    from optimal_control_problem_amd import _lib
    leg, wid = "oc4", "q20"
    _, ls, arrays = _batch(wid)
    rng = np.random.default_rng(23)
    x0, y0 = 0.1 * rng.standard_normal((ls.batch, ls.n)), 0.1 * rng.standard_normal((ls.batch, ls.m))
    rho0 = problems.split_rho(ls.batch)
    cold = _plain(monkeypatch, leg, wid)
    out = []
    for offset in (False, True):
        qp = _handle(monkeypatch, leg, wid, dict(warm_start=1), ls)
        try:
            _dense(qp, arrays)
            if offset:
                (px, kx), (py, ky), (pr, kr) = (lo.device_at_offset(a, 1) for a in (x0, y0, rho0))
                assert px % 16 == 8 and pr % 16 == 8
                _ok(_lib.lib().mpcqp_warm_start(qp._h, px, py, DEVICE)); _ok(_lib.lib().mpcqp_set_rho(qp._h, pr, DEVICE))
            else:
                keep = [torch.from_numpy(a).cuda() for a in (x0, y0, rho0)]
                qp.warm_start(keep[0], keep[1]); qp.set_rho(keep[2])
            out.append(_solved(qp))
        finally:
            qp.close()
    _bitwise(out[1], out[0], "warm start and rho from offset device pointers")
    assert not np.array_equal(out[0]["iters"], cold["iters"])          # (the start and the rho were used)


# ---------------------------------------------------------------------------------------------- i. argument checks
def _bad_strides(width):
    return (-1, -width, 1, width - 1)


def test_bad_strides_are_refused_and_harmless(built, monkeypatch):
    """a negative stride, or one between 0 and the width, on each array of each update entry: MPCQP_ERR_ARG, and the handle solves what it held before"""
    from optimal_control_problem_amd import _lib
    leg, wid = "oc4", "q20"
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    junk = {k: np.full_like(v, np.nan) for k, v in arrays.items()}
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        qp.keep_workspace(True)
        _dense(qp, arrays); _bitwise(_solved(qp), want, "before")
        for mname, mem in MEMS:
            views = lo.lay_all(junk, "padded1", mem)
            for entry in ("update", "update_matrices", "update_vectors"):
                names = ("q", "l", "u") if entry == "update_vectors" else lo.FIELDS
                for name in names:
                    for s in _bad_strides(views[name].width):
                        bad = dict(views, **{name: views[name].with_stride(s)})
                        rc = lo.raw_update_vectors(qp, *_vec(bad), mem) if entry == "update_vectors" else lo.raw_update(qp, entry, *_five(bad), mem)
                        assert rc == _lib.ERR_ARG, (entry, name, s, mname, rc)
                _bitwise(_solved(qp), want, "after the refusals of %s, %s" % (entry, mname))
    finally:
        qp.close()


def test_create_presolved_refuses_bad_strides(built, monkeypatch):
    from optimal_control_problem_amd import _lib
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    _, ls, arrays = _batch("q20")
    for mname, mem in MEMS:
        l, u = lo.lay(arrays["l"], "padded1", mem, "l"), lo.lay(arrays["u"], "padded1", mem, "u")
        for s in _bad_strides(ls.m):
            for pair in ((l.with_stride(s), u), (l, u.with_stride(s))):
                rc, qp = lo.raw_create_presolved(ls, pair[0], pair[1], mem)
                assert rc == _lib.ERR_ARG and qp is None, (s, mname, rc)


def test_solve_host_takes_dense_arrays_only(built, monkeypatch):
    """the exclusion: mpcqp_solve_host documents dense instance-major arrays; a padded stride on any of them is MPCQP_ERR_ARG, and the handle goes on"""
    from optimal_control_problem_amd import _lib
    leg, wid = "res4", "q20"
    _, ls, arrays = _batch(wid)
    want = _plain(monkeypatch, leg, wid)
    qp = _handle(monkeypatch, leg, wid, {}, ls)
    try:
        dense = lo.lay_all(arrays, "dense")
        for name in lo.FIELDS:
            views = dict(dense, **{name: lo.lay(arrays[name], "padded1", HOST, name)})
            args = []
            for v in _five(views):
                args += [v.ptr, v.stride]
            assert _lib.lib().mpcqp_solve_host(qp._h, *args, None, None, None, None, 0) == _lib.ERR_ARG, name
        got = qp.solve_host(arrays["P"], arrays["q"], arrays["A"], arrays["l"], arrays["u"])
        for k in ("x", "y", "status", "iters"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
    finally:
        qp.close()


# ---------------------------------------------------------------------------------------------- NULL for an empty array, device path
@pytest.mark.parametrize("name", ("lp", "no_constraints"))
def test_null_pointers_for_empty_arrays_on_the_device_path(built, name):
    """set_problem_data accepts P == NULL when nnz(P) = 0 and A (l, u) == NULL when there are none: with MPCQP_MEM_DEVICE as with host arrays"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    from tests.test_gpu_parity import _edge_problems
    prob = next(p for p in _edge_problems() if p["name"] == name)
    n, m = prob["n"], prob["m"]
    out = []
    for mem in (None, HOST, DEVICE):
        qp = BatchQP(n, m, 1, prob["Pp"], prob["Pi"], prob["Ap"], prob["Ai"])
        try:
            if mem is None:
                qp.update(prob["P"], prob["q"], prob["A"], prob["l"], prob["u"])
            else:
                views = {k: (lo.lay(prob[k], "offset1", mem, k) if prob[k].size else None) for k in lo.FIELDS}
                assert sum(v is None for v in views.values()) == (1 if name == "lp" else 3)
                _ok(lo.raw_update(qp, "update", *_five(views), mem))
            out.append(_solved(qp))
        finally:
            qp.close()
    assert out[0]["status"][0] == 1
    for got in out[1:]:
        _bitwise(got, out[0], name)


def test_zz_combinations_compared(built):
    """prints what the module docstring records (run with -s)"""
    for k in sorted(_COMPARED):
        print("%-22s %4d (leg, layout, memory) combinations compared bit for bit" % (k, _COMPARED[k]))
    print("%-22s %4d" % ("all", sum(_COMPARED.values())))
