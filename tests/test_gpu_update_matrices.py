"""GPU: mpcqp_update_matrices -- new P, q, A, l, u on a kept workspace (OSQP's osqp_update_data_mat): D, E, c of the handle's last full set-up and every
instance's rho stay, the new data are scaled with them by mpcqp_oc_rescale_kernel (csrc/kernel_oc_rescale.hpp) and the KKT matrix is factorised again.

The reference is tests/support/osqp_ref.py (held to the CPU oracle by tests/test_osqp_ref.py) fed the D, E, c and rho the handle reports after its full
solve; with scaled_termination = 1 the unchanged oracle on the problem scaled by hand is a second, independent one.  The bar is the one tests/test_gpu_parity.py
holds the on-chip kernels to: status equal, x, y, z within 1e-6 (1 + |.|_inf), final rho to 1e-6; iteration counts equal on the instances whose decisions do
not hang on rounding (kept_scaling.stable_mask, at least three quarters of every batch).  Shapes: tests/support/kept_scaling.py."""
import contextlib
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import kept_scaling as ks
from tests.support import osqp_ref, problems
from tests.test_gpu_parity import _close

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "status", "iters")
GPU_SHAPES = ("q20", "q25", "di6", "ltv")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _open(sid, ls=None, **kw):
    """a handle on the shape's pattern in the shape's kernel family; the variant is asserted"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    ls = ls or ks.sequence(sid)[0]
    fam, want = ks.SHAPES[sid][3:]
    with _env(MPCQP_VARIANT=fam):
        qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **kw)
    assert qp.plan_info()["variant"] == want
    return qp


def _data(ls):
    return ls.P, ls.q, ls.A, ls.l, ls.u


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _scaling(qp):
    return [qp.debug_scaling(b) for b in range(qp.batch)]


def _with_q(ls, q):
    return models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, ls.P, q, ls.A, ls.l, ls.u, ls.np)


@functools.lru_cache(maxsize=None)
def _chain(sid, eps, extra=()):
    """One handle through the whole call order, once per (shape, tolerance): QP1 in full -> update_matrices(QP2) -> update_matrices(QP3) ->
    update_vectors(perturbed q) -> update(QP3) in full.  -> the five results, the scaling read after the first solve and again after the fourth"""
    st = dict(ks.EPS[eps], **dict(extra))
    q1, q2, q3 = ks.sequence(sid)
    qp = _open(sid, **st)
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); r1 = qp.get(); sc = _scaling(qp)
        qp.update_matrices(*_data(q2)); qp.solve(); r2 = qp.get()
        qp.update_matrices(*_data(q3)); qp.solve(); r3 = qp.get()
        qp.update_vectors(problems.kept_q(q3), q3.l, q3.u); qp.solve(); r4 = qp.get(); sc4 = _scaling(qp)
        qp.update(*_data(q3)); qp.solve(); r5 = qp.get()
    finally:
        qp.close()
    return tuple(_frozen(r) for r in (r1, r2, r3, r4, r5)) + (sc, sc4)


def _against(got, ls, settings, scaling, rho0, x0=None, y0=None):
    mask, ref = ks.stable_mask(ls, settings, scaling, rho0, x0, y0)
    print("iters gpu", got["iters"], "ref", ref["iters"], "stable", mask, "rho gpu", got["rho"], "ref", ref["rho"])
    for k in ("x", "y", "z"):
        ok = np.isfinite(ref[k])
        print(k, "err", np.abs(got[k][ok] - ref[k][ok]).max() if ok.any() else None, "scale", 1.0 + np.abs(ref[k][ok]).max() if ok.any() else None)
    assert 4 * int(mask.sum()) >= 3 * len(mask), mask
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    assert (got["iters"][mask] == ref["iters"][mask]).all(), (got["iters"], ref["iters"], mask)
    for k in ("x", "y", "z"):
        _close(got, ref, k)
    assert (np.abs(got["rho"] - ref["rho"]) <= 1e-6 * np.abs(ref["rho"])).all(), (got["rho"], ref["rho"])


# ---------------------------------------------------------------------------------------------- 1. parity, default termination
@pytest.mark.parametrize("eps", list(ks.EPS))
@pytest.mark.parametrize("sid", GPU_SHAPES)
def test_parity_with_the_reference_on_the_kept_scaling(built, sid, eps):
    r1, r2 = _chain(sid, eps)[:2]; sc = _chain(sid, eps)[5]
    _against(r2, ks.sequence(sid)[1], ks.EPS[eps], sc, r1["rho"])


def test_rho_updates_behind_the_rescale_kernel(built):
    """settings under which every instance adapts rho inside the kept-scaling solve (problems.RHO_RECIPES "q20"'s, on the eight-wave shape): the leave /
    resume launches of the two-kernel form run behind the new kernel, on the slab it left"""
    st = dict(problems._Q_RHO)
    q1, q2, _ = ks.sequence("q25")
    qp = _open("q25", **st)
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); r1 = qp.get(); sc = _scaling(qp)
        qp.update_matrices(*_data(q2)); qp.solve(); r2 = qp.get()
    finally:
        qp.close()
    assert (r2["rho"] != r1["rho"]).all(), (r1["rho"], r2["rho"])
    _against(r2, q2, st, sc, r1["rho"])


# ---------------------------------------------------------------------------------------------- 2. parity, scaled termination: the unchanged oracle
@pytest.mark.parametrize("sid", GPU_SHAPES)
def test_scaled_termination_is_the_oracle_on_the_prescaled_problem(built, sid):
    extra = (("scaled_termination", 1),)
    r1, r2 = _chain(sid, "1e-3", extra)[:2]; sc = _chain(sid, "1e-3", extra)[5]
    pre = osqp_ref.prescaled(ks.sequence(sid)[1], sc)
    st = dict(scaling=0, scaled_termination=1)
    ref = osqp_ref.unscaled(problems.oracle_solve(pre, nthreads=8, rho0=r1["rho"], **st), sc)
    mask = problems.oracle_stable_mask(pre, rho0=r1["rho"], **st)
    print("iters gpu", r2["iters"], "oracle", ref["iters"], "stable", mask)
    assert 4 * int(mask.sum()) >= 3 * len(mask), mask
    assert (r2["status"] == ref["status"]).all() and (r2["iters"][mask] == ref["iters"][mask]).all(), (r2["iters"], ref["iters"])
    for k in ("x", "y", "z"):
        _close(r2, ref, k)
    assert (np.abs(r2["rho"] - ref["rho"]) <= 1e-6 * np.abs(ref["rho"])).all()


# ---------------------------------------------------------------------------------------------- 3. same data
@pytest.mark.parametrize("sid", GPU_SHAPES)
def test_same_data_gives_the_full_solves_result(built, sid):
    """update_matrices with QP1's own arrays: the scaling is QP1's own, so this is the full solve again (the products are formed in another order: not bitwise)"""
    q1 = ks.sequence(sid)[0]
    qp = _open(sid)
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); full = qp.get()
        assert (full["rho"] == 0.1).all()        # (no instance adapted rho at this tolerance: the second solve starts where the first did)
        qp.update_matrices(*_data(q1)); qp.solve(); again = qp.get()
    finally:
        qp.close()
    assert np.array_equal(again["status"], full["status"]) and np.array_equal(again["iters"], full["iters"]), (again["iters"], full["iters"])
    for k in ("x", "y", "z"):
        _close(again, full, k)


# ---------------------------------------------------------------------------------------------- 4. sequence
@pytest.mark.parametrize("sid,eps", [(s, "1e-3") for s in GPU_SHAPES] + [("q25", "1e-5")])      # (at 1e-5 the full solve of QP1 adapts rho: the later solves start from carried values that differ per instance)
def test_sequence_of_updates_on_one_handle(built, sid, eps):
    r1, r2, r3, r4, r5, sc, sc4 = _chain(sid, eps)
    q3 = ks.sequence(sid)[2]
    for a, b in zip(sc, sc4):                  # D, E, c are still QP1's after two matrix updates and a vector update
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    _against(r3, q3, ks.EPS[eps], sc, r2["rho"])                                              # scaling QP1's, rho carried from solve 2
    _against(r4, _with_q(q3, problems.kept_q(q3)), ks.EPS[eps], sc, r3["rho"])                # vectors alone, on the factor solve 3 left
    fresh = _open(sid, **ks.EPS[eps])
    try:
        fresh.update(*_data(q3)); fresh.solve(); want = fresh.get()
    finally:
        fresh.close()
    for k in KEYS:                             # mpcqp_update returns to a full set-up: the mode leaves nothing behind
        assert np.array_equal(r5[k], want[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------- 5. warm start
@pytest.mark.parametrize("sid", ("q20", "q25"))
def test_warm_start_on_the_kept_scaling(built, sid):
    q1, q2, _ = ks.sequence(sid)
    x0, y0, st = problems.warm_point(q2, {})
    qp = _open(sid, **st)
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); r1 = qp.get(); sc = _scaling(qp)
        qp.update_matrices(*_data(q2)); qp.warm_start(x0, y0); qp.solve(); got = qp.get()
    finally:
        qp.close()
    cold = _chain(sid, "1e-3")[1]
    assert not np.array_equal(got["x"], cold["x"])        # (the start was used)
    _against(got, q2, st, sc, r1["rho"], x0, y0)


# ---------------------------------------------------------------------------------------------- 6. device pointers and the SQP loop
def test_device_sqp_loop_keeps_the_scaling(built, monkeypatch):
    from optimal_control_problem_amd.batch_qp import BatchQP
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    B = 8
    mdl, ls, meta = models.make_workload("quadrotor", B, N=20)
    arg = dict(lbx=meta["lbx"], ubx=meta["ubx"], lbg=meta["lbg"], ubg=meta["ubg"], p=meta["p"])
    calls = []
    plain = BatchQP.update_matrices
    monkeypatch.setattr(BatchQP, "update_matrices", lambda self, *a: (calls.append(1), plain(self, *a))[1])
    with _env(MPCQP_VARIANT="oc4"):
        a = DeviceSQPOptimizationSolver(mdl, {"max_iter": 1, "alpha": 0.7}, batch=B)
        b = DeviceSQPOptimizationSolver(mdl, {"max_iter": 2, "alpha": 0.7, "keep_scaling": True}, batch=B)
    try:
        assert a.qp.plan_info()["variant"] == 204 and b.qp.plan_info()["variant"] == 204
        a.setInitialGuess(meta["x_iterate"]); b.setInitialGuess(meta["x_iterate"])
        a.getOptimalSolution(arg)
        assert not calls
        sc = _scaling(a.qp); rho = a.info[:, 3].cpu().numpy()
        b.getOptimalSolution(arg)
        assert len(calls) == 1
        host = lambda k: b.ls[k].cpu().numpy()
        qp2 = models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, host("P"), host("q"), host("A"), host("l"), host("u"), ls.np)
        assert not np.array_equal(qp2.A, np.broadcast_to(ls.A, qp2.A.shape))
        mask, ref = ks.stable_mask(qp2, {}, sc, rho)
        got = dict(x=b.dw.cpu().numpy(), status=b.status.cpu().numpy(), iters=b.iters.cpu().numpy())
        print("iters gpu", got["iters"], "ref", ref["iters"], "stable", mask)
        assert 4 * int(mask.sum()) >= 3 * len(mask)
        assert (got["status"] == ref["status"]).all() and (got["iters"][mask] == ref["iters"][mask]).all(), (got["iters"], ref["iters"])
        _close(got, ref, "x")
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 7. reduced handle
def test_reduced_handle_forwards(built):
    from optimal_control_problem_amd.batch_qp import BatchQP
    mdl = models.make_workload("quadrotor", 8, N=20)[0]
    q1, q2, _ = ks.sequence("q20")
    tight = dict(eps_abs=1e-7, eps_rel=1e-7)
    out = []
    for rows in (list(range(mdl.np)), None):
        with _env(MPCQP_VARIANT="oc4"):
            qp = BatchQP(q1.n, q1.m, q1.batch, q1.Pp, q1.Pi, q1.Ap, q1.Ai, fixed_rows=rows, **tight)
        try:
            assert qp.plan_info()["variant"] == 204             # (the reduced handle reports its inner handle's plan: an on-chip one)
            qp.keep_workspace(True)
            qp.update(*_data(q1)); qp.solve(); qp.get()
            qp.update_matrices(*_data(q2)); qp.solve(); out.append(qp.get())
        finally:
            qp.close()
    red, full = out
    assert (red["status"] == 1).all() and (full["status"] == 1).all()
    for k in ("x", "y"):        # (the bar test_gpu_parity.py test_reduced_form holds its leg (b) to)
        err = np.abs(red[k] - full[k]).max()
        print(k, "err", err, "scale", 1.0 + np.abs(full[k]).max())
        assert err <= 1e-4 * (1.0 + np.abs(full[k]).max())


# ---------------------------------------------------------------------------------------------- 8. refusals and per-instance outcomes
def test_call_order_is_enforced(built):
    from optimal_control_problem_amd import _lib
    q1, q2, _ = ks.sequence("q20")
    qp = _open("q20")
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1))
        with pytest.raises(_lib.MpcqpError) as e:           # kept, but nothing solved yet
            qp.update_matrices(*_data(q2))
        assert e.value.code == _lib.ERR_STATE
        qp.solve(); qp.get()
        qp.keep_workspace(False)
        with pytest.raises(_lib.MpcqpError) as e:           # solved, but not kept
            qp.update_matrices(*_data(q2))
        assert e.value.code == _lib.ERR_STATE
    finally:
        qp.close()


def test_other_kernel_families_answer_err_limit_and_stay_usable(built):
    from optimal_control_problem_amd import _lib
    from optimal_control_problem_amd.batch_qp import BatchQP
    mdl, ls, _ = models.make_workload("double_integrator", 8, N=20)
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
    try:
        assert qp.plan_info()["variant"] < 100              # an LDS-resident family
        qp.keep_workspace(True)
        qp.update(*_data(ls)); qp.solve(); first = qp.get()
        with pytest.raises(_lib.MpcqpError) as e:
            qp.update_matrices(*_data(ls))
        assert e.value.code == _lib.ERR_LIMIT
        qp.update(*_data(ls)); qp.solve(); got = qp.get()
    finally:
        qp.close()
    ref = problems.oracle_solve(ls)
    assert (got["status"] == ref["status"]).all() and (got["iters"] == ref["iters"]).all()
    for k in ("x", "y", "z"):
        _close(got, ref, k)
        assert np.array_equal(got[k], first[k])


def test_crossed_bounds_are_refused_per_instance(built):
    q1, q2, _ = ks.sequence("q20")
    l = q2.l.copy(); l[3, 40] = q2.u[3, 40] + 1.0
    qp = _open("q20")
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); qp.get()
        qp.update_matrices(q2.P, q2.q, q2.A, l, q2.u); qp.solve(); got = qp.get()
    finally:
        qp.close()
    assert got["status"][3] == 11 and got["iters"][3] == 0 and np.isnan(got["x"][3]).all() and np.isnan(got["y"][3]).all()
    rest = np.delete(np.arange(q2.batch), 3)
    assert (got["status"][rest] == 1).all()
    want = _chain("q20", "1e-3")[1]
    for k in KEYS:
        assert np.array_equal(got[k][rest], want[k][rest]), k


def test_non_convex_instance_alone_and_not_for_good(built):
    """double integrator N=6: an input's diagonal entry of P at -1 leaves P + sigma I + A' R A indefinite in the kept scaling (on the quadrotor no single
    entry does: rho A' A outweighs it, and OSQP would not notice either)"""
    q1, q2, _ = ks.sequence("di6")
    j, b = 7, 2
    cols = np.repeat(np.arange(q2.n), np.diff(q2.Pp))
    k = int(np.flatnonzero((np.asarray(q2.Pi) == j) & (cols == j))[0])
    P = np.array(np.broadcast_to(q2.P, (q2.batch, len(q2.Pi)))); P[b, k] = -1.0
    qp = _open("di6")
    try:
        qp.keep_workspace(True)
        qp.update(*_data(q1)); qp.solve(); r1 = qp.get(); sc = _scaling(qp)
        qp.update_matrices(P, q2.q, q2.A, q2.l, q2.u); qp.solve(); bad = qp.get()
        qp.update_matrices(*_data(q2)); qp.solve(); good = qp.get()
    finally:
        qp.close()
    spoilt = models.LocalSystem(q2.n, q2.m, q2.Pp, q2.Pi, q2.Ap, q2.Ai, P, q2.q, q2.A, q2.l, q2.u, q2.np)
    ref = osqp_ref.solve_batch(spoilt, {}, sc, r1["rho"])
    assert ref["status"][b] == 9 and (np.delete(ref["status"], b) == 1).all()
    assert np.array_equal(bad["status"], ref["status"]) and np.isnan(bad["x"][b]).all()
    assert (good["status"] == 1).all()
    ref2 = osqp_ref.solve_batch(q2, {}, sc, bad["rho"])
    assert np.array_equal(good["iters"], ref2["iters"])
    _close(good, ref2, "x")


# ---------------------------------------------------------------------------------------------- 9. facades
def _facade(keep):
    from optimal_control_problem_amd.cucaqp import CuCaQP
    q1, q2, _ = ks.sequence("q20")
    qp = CuCaQP(batch=q1.batch)
    try:
        assert qp.setDimension(q1.n, q1.m)
        qp.setSystem(q1)
        with _env(MPCQP_VARIANT="oc4"):
            assert qp.initSolver()
        assert qp._qp.plan_info()["variant"] == 204
        assert qp.solve()
        qp.setKeepScaling(keep)
        assert qp.updateHessianMatrix((q2.Pp, q2.Pi, q2.P)) and qp.updateLinearConstraintsMatrix((q2.Ap, q2.Ai, q2.A))
        assert qp.updateGradient(q2.q) and qp.updateLowerBound(q2.l) and qp.updateUpperBound(q2.u)
        assert qp.solve()
        return {k: np.array(v) for k, v in qp.getInfo().items()}
    finally:
        qp.close()


def _full_qp2():
    qp = _open("q20")
    try:
        qp.update(*_data(ks.sequence("q20")[1])); qp.solve()
        return qp.get()
    finally:
        qp.close()


def test_python_facade_keep_scaling(built):
    kept, full = _facade(True), _facade(False)
    want_kept, want_full = _chain("q20", "1e-3")[1], _full_qp2()
    for k in KEYS:
        assert np.array_equal(kept[k], want_kept[k], equal_nan=True), k
        assert np.array_equal(full[k], want_full[k], equal_nan=True), k
    assert not np.array_equal(kept["x"], full["x"])


EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "cucaqp_keep_scaling_test")


def test_cpp_facade_keep_scaling(built, tmp_path):
    q1, q2, _ = ks.sequence("q20")
    B = q1.batch
    path = str(tmp_path / "qps.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("5i", q1.n, q1.m, B, len(q1.Pi), len(q1.Ai)))
        for a in (q1.Pp, q1.Pi, q1.Ap, q1.Ai):
            f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
        for q in (q1, q2):
            for a, w in ((q.P, len(q.Pi)), (q.q, q.n), (q.A, len(q.Ai)), (q.l, q.m), (q.u, q.m)):
                f.write(np.ascontiguousarray(np.broadcast_to(a, (B, w)), dtype=np.float64).tobytes())
    r = subprocess.run([EXE, path], capture_output=True, text=True, timeout=300, env=dict(os.environ, MPCQP_VARIANT="oc4"))
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    rows = {tuple(line.split()[:3]): line.split()[3:] for line in r.stdout.splitlines() if line.startswith("keep")}
    for keep, want in (("1", _chain("q20", "1e-3")[1]), ("0", _full_qp2())):
        assert [int(v) for v in rows[("keep", keep, "status")]] == want["status"].tolist()
        assert [int(v) for v in rows[("keep", keep, "iters")]] == want["iters"].tolist()
        x = np.array([float.fromhex(v) for v in rows[("keep", keep, "x")]]).reshape(B, -1)
        assert np.array_equal(x, want["x"])
