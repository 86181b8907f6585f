"""GPU: the set-up kernel's factorisation with its operands on chip -- the T tiles of the assembly scattered into LDS and multiplied
from there, a part of the blocks at a time, and the diagonal term from the list of singleton rows -- against the same kernel with MPCQP_NO_T_LDS=1 and
MPCQP_NO_SING_LIST=1, the paths of the commit before (tiles through the slab, a full pass over A'): two fresh handles in one process, x, y, z, status,
iterations and info bit for bit; and the new path against the CPU oracle at the bar tests/test_gpu_parity.py holds the on-chip kernels to, with equal
iteration counts.  Shapes: three parts (quadrotor N = 20, with and without arrow head), two parts on two chain pairs (cart-pole N = 30), the fallback
to the slab with the list alone (quadrotor N = 50, cart-pole N = 100); the resume-mode factorisation and the <RF = 1> kernels, which never take the
LDS path (the smallest rho recipe at MPCQP_RESUME_ROUNDS 1 and 0); the kept-workspace entry re-factorising after a row changed class; and
mpcqp_update_matrices (the rescale kernel shares the factorisation)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import kept_scaling as ks
from tests.support import problems
from tests.test_gpu_parity import _close

pytestmark = pytest.mark.gpu

BITS = ("x", "y", "z", "status", "iters", "obj", "prim_res", "dual_res", "rho")
OFF = ("MPCQP_NO_T_LDS", "MPCQP_NO_SING_LIST")
SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "libt_lds_interp.so")


def _env(mp, off, family=None, **extra):
    for k in OFF:
        mp.delenv(k, raising=False)
    if family:
        mp.setenv("MPCQP_VARIANT", family)
    for k, v in extra.items():
        mp.setenv(k, v)
    if off:
        for k in OFF:
            mp.setenv(k, "1")


def _parts(ls, batch, cus):
    """(parts of the T tiles in LDS, entries per column of the singleton list) of the handle the library makes of this pattern under the environment as it stands"""
    L = C.CDLL(SO)
    L.t_lds_describe.restype = C.c_long
    info = np.zeros(18, np.int64); buf = np.zeros(1 << 22, np.int32)
    p = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    arrs = [p(a) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai)]
    fam = os.environ.get("MPCQP_VARIANT")
    w = L.t_lds_describe(ls.n, ls.m, batch, *[a.ctypes.data_as(C.c_void_p) for a in arrs], cus, fam.encode() if fam else None, info.ctypes.data_as(C.c_void_p),
                         buf.ctypes.data_as(C.c_void_p), C.c_long(buf.size))
    assert w > 0, w
    return int(info[3]), int(info[4])


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same_bits(on, off, tag=""):
    for k in BITS:
        assert np.array_equal(on[k], off[k], equal_nan=True), (tag, k)


def _against_oracle(got, ref):
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    assert (got["iters"] == ref["iters"]).all(), (got["iters"], ref["iters"])
    for k in ("x", "y", "z"):
        _close(got, ref, k)


@functools.lru_cache(maxsize=None)
def _workload(name, batch, N):
    return models.make_workload(name, batch, N=N)


@functools.lru_cache(maxsize=None)
def _plain_case(name, N, batch, reduced):
    """-> (LocalSystem, fixed rows or None, oracle result on the QP the handle iterates on, its free variables / kept rows or None)"""
    mdl, ls, _ = _workload(name, batch, N)
    if not reduced:
        return ls, None, problems.oracle_solve(ls), None
    fixed = list(range(mdl.np))
    red, free, kept, _, _ = problems.reduce_qp(ls, fixed)
    return ls, fixed, problems.oracle_solve(red), (free, kept)


def _solve(monkeypatch, ls, off, family, variant, want_parts, fixed=None, inner=None, **settings):
    from optimal_control_problem_amd.batch_qp import BatchQP
    with monkeypatch.context() as mp:
        _env(mp, off, family)
        qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, fixed_rows=fixed, **settings)
        got = _parts(inner or ls, ls.batch, _cus())
    try:
        assert qp.plan_info()["variant"] == variant
        assert got == ((0, 0) if off else want_parts), got        # which path this handle's set-up kernel takes
        qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve()
        return qp.get()
    finally:
        qp.close()


# (workload, N, batch, reduced form, family, variant, (parts, list entries per column) of the new path)
PLAIN = [("quadrotor", 20, 3, False, "oc4", 204, (3, 2)), ("quadrotor", 50, 2, False, "oc8", 208, (0, 2)), ("cartpole", 30, 4, False, "oc4", 204, (2, 2)),
         ("cartpole", 100, 2, False, "oc8", 208, (0, 2)), ("quadrotor", 20, 3, True, "oc4", 204, (3, 2))]


@pytest.mark.parametrize("name,N,batch,reduced,family,variant,parts", PLAIN, ids=["%s-N%d%s" % (c[0], c[1], "-reduced" if c[3] else "") for c in PLAIN])
def test_on_chip_operands_give_the_bits_of_the_slab_path(built, monkeypatch, name, N, batch, reduced, family, variant, parts):
    ls, fixed, ref, sub = _plain_case(name, N, batch, reduced)
    inner = problems.reduce_qp(ls, fixed)[0] if reduced else None
    on = _solve(monkeypatch, ls, False, family, variant, parts, fixed, inner)
    off = _solve(monkeypatch, ls, True, family, variant, parts, fixed, inner)
    _same_bits(on, off)
    if sub is not None:
        on = dict(on, x=on["x"][:, sub[0]], y=on["y"][:, sub[1]], z=on["z"][:, sub[1]])
    _against_oracle(on, ref)


@pytest.mark.parametrize("rounds", [0, 1])
def test_rho_updates_refactorise_on_the_same_bits(built, monkeypatch, rounds):
    """cart-pole N = 30 under its rho recipe: at MPCQP_RESUME_ROUNDS = 1 the first update is served by the set-up kernel in resume mode (LDS path, two
    parts), later ones by the iteration kernel <RF = 1> in place; at 0 every update is served in place -- the slab path, whatever the switches say"""
    from tests.test_gpu_rho_resume import _handle, _recipe, _same_as_oracle
    ls, st, ref, stable, updates = _recipe("cp30")
    assert (updates >= rounds + 1).any()
    res = []
    for off in (False, True):
        with monkeypatch.context() as mp:
            _env(mp, off)
            qp = _handle(mp, "cp30", ls, st, rounds)
            assert _parts(ls, ls.batch, _cus()) == ((0, 0) if off else (2, 2))
        qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); res.append(qp.get()); qp.close()
    _same_bits(res[0], res[1], "rounds=%d" % rounds)
    _same_as_oracle(res[0], ref, stable, "cp30 rounds=%d, operands on chip" % rounds, rho_at_the_bar=True)


def test_kept_workspace_refactorises_when_a_row_changes_class(built, monkeypatch):
    """keep_workspace + update_vectors with one equality row of every second instance released into an inequality: rho_i changes, the REUSE entry of
    the set-up kernel re-factorises on the kept scaling"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    from oracle import oracle as orc
    B = 4
    mdl, ls, _ = _workload("quadrotor", B, 20)
    l2, u2 = ls.l.copy(), ls.u.copy()
    l2[::2, mdl.np + 1] -= 0.25; u2[::2, mdl.np + 1] += 0.25
    st = orc.State(orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai), B, orc.default_settings())
    refs = [st.solve(ls.P, ls.q, ls.A, ls.l, ls.u), st.solve_vectors(ls.q, l2, u2)]

    def run(off):
        with monkeypatch.context() as mp:
            _env(mp, off, "oc4")
            qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
        try:
            assert qp.plan_info()["variant"] == 204
            qp.keep_workspace(True)
            qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); first = qp.get()
            qp.update_vectors(ls.q, l2, u2); qp.solve(); second = qp.get()
            return first, second
        finally:
            qp.close()

    on, off = run(False), run(True)
    for a, b, ref in zip(on, off, refs):
        _same_bits(a, b)
        _against_oracle(a, ref)
    assert not np.array_equal(on[0]["x"][::2], on[1]["x"][::2])          # (the released row moved those instances)


def test_update_matrices_factorises_on_the_same_bits(built, monkeypatch):
    """QP1 in full, then mpcqp_update_matrices(QP2): the rescale kernel's factorisation, against the reference on the kept scaling
    (tests/test_gpu_update_matrices.py's bar)"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    from tests.test_gpu_update_matrices import _against, _data, _scaling
    q1, q2, _ = ks.sequence("q20")

    def run(off):
        with monkeypatch.context() as mp:
            _env(mp, off, "oc4")
            qp = BatchQP(q1.n, q1.m, q1.batch, q1.Pp, q1.Pi, q1.Ap, q1.Ai)
        try:
            assert qp.plan_info()["variant"] == 204
            qp.keep_workspace(True)
            qp.update(*_data(q1)); qp.solve(); r1 = qp.get(); sc = _scaling(qp)
            qp.update_matrices(*_data(q2)); qp.solve(); r2 = qp.get()
            return r1, r2, sc
        finally:
            qp.close()

    on, off = run(False), run(True)
    _same_bits(on[0], off[0]); _same_bits(on[1], off[1])
    _against(on[1], q2, {}, on[2], on[0]["rho"])
