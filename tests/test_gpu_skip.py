"""GPU: solving a subset of the batch (mpcqp_set_skip).

The contract of include/mpcqp.h: under a skip array an active instance gets, bit for bit, the result of the same solve without one, and nothing of a skipped
instance is read or written.  So every comparison here is of bits (_bitwise / BITS of tests/test_gpu_rho_resume.py), the reference is the existing unskipped
path -- which tests/test_gpu_instances.py holds to the oracle --, and no tolerance is introduced.

"Nothing is written" is made visible by a second solve: a handle first solves OTHER data unskipped (R2), then takes the original data under a mask; the
active instances must then carry the unskipped result of the original data (R) and the skipped ones must still carry R2.
  1. the compaction kernel against its NumPy statement batch_qp.skip_list, exactly, at batches around the wave, the pass (1024) and two passes;
  2. every compiled kernel instance (tests/support/instance_cases.py ROWS, reduced rows included) under the default and the rho leg (the resume launches);
  3. the kept workspace: a skipped instance's slab is untouched by a vectors-only solve, and serves its next one as if that solve had not happened;
  4. the ticket loop of the eight-wave iteration kernel at more instances than resident workgroups;
  5. the state rules of the kept-workspace entries, each error code;
  6. polish, and warm start + per-instance rho, under a mask;
  7. the dispatch hint composes: the list is the hint's order without the skipped instances;
  8. a captured solve follows the contents of a borrowed device skip array at replay;
  9. the loops: options["skip_converged_qps"] changes no bit of x, converged_at, kkt_history -- device loop, four option combinations, ClosedLoopMPC, C++.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from optimal_control_problem_amd.batch_qp import skip_list
from tests.support import instance_cases as ic
from tests.support import kkt_cases as kc
from tests.support import problems
from tests.test_gpu_instances import KEPT_ROWS, ROW_IDS, _handle, _key, _solve
from tests.test_gpu_rho_resume import BITS, _bitwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -2 ** 31
OC4_ROW = ic.INSTANCE_CASES[ic._admm(4, 5, 3)][0]          # cart-pole N=6 on the four-wave two-kernel on-chip form: takes matrix updates
OC8_ROW = ic.INSTANCE_CASES[ic._admm(8, 4, 4)][0]          # cart-pole N=6 on the eight-wave form: the ticket loop


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _mask(B, idx):
    m = np.zeros(B, np.int32)
    m[np.asarray(idx, int)] = 1
    return m


def _rows(res, sel, keys=BITS):
    return {k: res[k][sel] for k in keys if k in res}


def _check(got, active_ref, skipped_ref, mask, tag, keys=BITS):
    sk = np.asarray(mask) != 0
    _bitwise(_rows(got, ~sk, keys), _rows(active_ref, ~sk, keys), tag + ": active instances", keys)
    _bitwise(_rows(got, sk, keys), _rows(skipped_ref, sk, keys), tag + ": skipped instances", keys)


def _differs(a, b):
    """R and R2 must not coincide, or 'kept the bits of R2' would say nothing"""
    return not np.array_equal(a["x"], b["x"], equal_nan=True)


def _err(code, fn, *a):
    with pytest.raises(_lib.MpcqpError) as e:
        fn(*a)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


# ------------------------------------------------------------------------------------------------ 1. the list kernel = the statement
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_list_kernel_equals_the_statement(built, monkeypatch, B):
    from optimal_control_problem_amd.batch_qp import BatchQP
    for name in [n for n in os.environ if n.startswith("MPCQP_")]:
        monkeypatch.delenv(name)
    mdl, ls, _ = models.make_workload("double_integrator", B, N=3)
    qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
    qp.set_dispatch_hint(False)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); full = qp.get()
    _err(_lib.ERR_STATE, qp.debug_skip_list)                         # the last solve ran without a skip array
    rng = np.random.default_rng(100 + B)
    half = np.where(rng.random(B) < 0.5, rng.choice(np.array([-1, 2, INT_MIN, 1]), size=B), 0)
    masks = {"none": np.zeros(B), "all": np.full(B, 2), "first only": _mask(B, [0]) * -1, "last only": _mask(B, [B - 1]) * INT_MIN,
             "every second": (np.arange(B) % 2) * 2, "all but one": np.where(np.arange(B) == B // 2, 0, -1), "random half": half}
    for tag, mk in masks.items():
        mk = np.asarray(mk, np.int64).astype(np.int32)
        qp.set_skip(mk); qp.solve()
        got = qp.debug_skip_list()
        assert np.array_equal(got, skip_list(mk)), (B, tag, got[:16], skip_list(mk)[:16])
        assert got.dtype == np.int32 and (got[int((mk == 0).sum()):] == -1).all()
        res = qp.get()                                                # same data: every instance, skipped or not, still carries the full solve
        _bitwise(res, full, "B=%d %s" % (B, tag))
    qp.set_skip(None); qp.solve()
    _err(_lib.ERR_STATE, qp.debug_skip_list)
    qp.close()


# ------------------------------------------------------------------------------------------------ 2. every compiled instance
def _masks_of(B):
    return [("0", [0]), ("the infeasible two", [problems.DUAL_INFEASIBLE, problems.PRIMAL_INFEASIBLE]), ("all but 3", [b for b in range(B) if b != 3]),
            ("all", list(range(B))), ("none", [])]


@pytest.mark.parametrize("leg", ["default", "rho"])
@pytest.mark.parametrize("k,r", ic.ROWS, ids=ROW_IDS)
def test_every_compiled_instance(built, monkeypatch, k, r, leg):
    key = _key(r)
    ls = ic.row_data(*key).ls
    st = ic.leg_settings(*key, leg)
    q2, l2, u2 = ic.kept_vectors(*key)
    qa = _handle(monkeypatch, r, st)
    R = _solve(qa, ls); qa.close()
    qb = _handle(monkeypatch, r, st)
    for tag, idx in _masks_of(ls.batch):
        qb.set_skip(None)
        qb.update(ls.P, q2, ls.A, l2, u2); qb.solve(); R2 = qb.get()
        assert _differs(R, R2)
        mk = _mask(ls.batch, idx)
        qb.update(ls.P, ls.q, ls.A, ls.l, ls.u); qb.set_skip(mk); qb.solve()
        _check(qb.get(), R, R2, mk, "%s %s, skip %s" % (ic.row_id(r), leg, tag))
    qb.close()


# ------------------------------------------------------------------------------------------------ 3. the kept workspace
@pytest.mark.parametrize("k,r", KEPT_ROWS, ids=[ic.row_id(r) for _, r in KEPT_ROWS])
def test_kept_workspace(built, monkeypatch, k, r):
    key = _key(r)
    ls = ic.row_data(*key).ls
    q2, l2, u2 = ic.kept_vectors(*key)
    q3 = ls.q * (1.0 + 0.1 * np.random.default_rng(29).standard_normal(ls.q.shape))
    sh = 0.01 * np.random.default_rng(31).standard_normal(ls.l.shape)
    l3, u3 = ls.l + sh, ls.u + sh
    mk = _mask(ls.batch, [1, 3])
    # a: full -> q2 -> q3 (the three-step history); c: full -> q3; b: full -> q2 under the mask -> q3 unskipped
    qa = _handle(monkeypatch, r, {}); qa.keep_workspace(True)
    F1 = _solve(qa, ls)
    qa.update_vectors(q2, l2, u2); qa.solve(); K2 = qa.get()
    qa.update_vectors(q3, l3, u3); qa.solve(); three = qa.get(); qa.close()
    qc = _handle(monkeypatch, r, {}); qc.keep_workspace(True)
    _solve(qc, ls)
    qc.update_vectors(q3, l3, u3); qc.solve(); direct = qc.get(); qc.close()
    qb = _handle(monkeypatch, r, {}); qb.keep_workspace(True)
    _bitwise(_solve(qb, ls), F1, "%s: full solve" % ic.row_id(r))
    qb.set_skip(mk)
    qb.update_vectors(q2, l2, u2); qb.solve()
    _check(qb.get(), K2, F1, mk, "%s: vectors-only solve under a mask" % ic.row_id(r))
    qb.set_skip(None)
    qb.update_vectors(q3, l3, u3); qb.solve()
    # (a formerly skipped instance's slab was untouched: it is where `direct` was; the others went through q2)
    _check(qb.get(), three, direct, mk, "%s: the vectors-only solve after the mask" % ic.row_id(r))
    qb.close()
    assert _differs(F1, K2)          # (`three` and `direct` may coincide: where rho never moved, a vectors-only solve does not depend on the one before)


# ------------------------------------------------------------------------------------------------ 4. the ticket loop
@functools.lru_cache(maxsize=None)
def _tiled():
    base = ic.row_data(*_key(OC8_ROW)).ls
    B = 2 * ic.CUS + 44
    ls = problems.take(base, np.arange(B) % base.batch)
    rng = np.random.default_rng(41)
    return ls, problems.kept_q(ls), rng.random(B) < 0.5


def _oc8_handle(monkeypatch, ls, st):
    from optimal_control_problem_amd.batch_qp import BatchQP
    for name in [n for n in os.environ if n.startswith("MPCQP_")]:
        monkeypatch.delenv(name)
    for name, v in OC8_ROW.env.items():
        monkeypatch.setenv(name, v)
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **st)
    assert qp.plan_info()["variant"] == 208, qp.plan_info()
    return qp


@pytest.mark.parametrize("leg", ["default", "rho"])
def test_ticket_loop(built, monkeypatch, leg):
    ls, q2, half = _tiled()
    B = ls.batch
    st = ic.leg_settings(*_key(OC8_ROW), leg)
    qa = _oc8_handle(monkeypatch, ls, st)
    R = _solve(qa, ls); qa.close()
    qb = _oc8_handle(monkeypatch, ls, st)
    for tag, mk in (("random half", half.astype(np.int32)), ("all but the last", _mask(B, range(B - 1))), ("only the first", _mask(B, [0]))):
        qb.set_skip(None)
        qb.update(ls.P, q2, ls.A, ls.l, ls.u); qb.solve(); R2 = qb.get()
        assert _differs(R, R2)
        qb.update(ls.P, ls.q, ls.A, ls.l, ls.u); qb.set_skip(mk); qb.solve()
        _check(qb.get(), R, R2, mk, "ticket loop %s, skip %s" % (leg, tag))
        lst = qb.debug_skip_list()
        n_act = int((mk == 0).sum())
        assert sorted(lst[:n_act].tolist()) == np.flatnonzero(mk == 0).tolist() and (lst[n_act:] == -1).all()
    qb.close()


# ------------------------------------------------------------------------------------------------ 5. the state rules
def test_state_rules(built, monkeypatch):
    r = OC4_ROW
    ls = ic.row_data(*_key(r)).ls
    q2, l2, u2 = ic.kept_vectors(*_key(r))
    data = (ls.P, ls.q, ls.A, ls.l, ls.u)
    mk = _mask(ls.batch, [0, 3])
    qp = _handle(monkeypatch, r, {})
    qp.keep_workspace(True)
    qp.update(*data)
    _err(_lib.ERR_STATE, qp.debug_skip_list)                         # nothing solved yet
    # a full set-up under a skip array: both kept-workspace entries are refused, with the reason
    qp.set_skip(mk); qp.solve()
    assert "skip" in _err(_lib.ERR_STATE, qp.update_vectors, q2, l2, u2)
    assert "skip" in _err(_lib.ERR_STATE, qp.update_matrices, *data)
    qp.set_skip(None)                                                # clearing the array does not repair the slabs
    _err(_lib.ERR_STATE, qp.update_vectors, q2, l2, u2)
    _err(_lib.ERR_STATE, qp.update_matrices, *data)
    qp.update(*data); qp.solve()                                     # a full set-up without one does
    qp.update_vectors(q2, l2, u2); qp.solve()
    # an update_vectors solve under a skip array leaves everything valid
    qp.set_skip(mk)
    qp.update_vectors(ls.q, ls.l, ls.u); qp.solve()
    qp.update_vectors(q2, l2, u2); qp.solve()
    qp.update_matrices(*data); qp.solve()                            # ... and this one is an update_matrices solve under a skip array:
    assert "skip" in _err(_lib.ERR_STATE, qp.update_vectors, q2, l2, u2)
    qp.update_matrices(*data)                                        # update_matrices still works (D, E, c are the unskipped set-up's)
    qp.update_vectors(q2, l2, u2)                                    # (between update_matrices and its solve: the vectors of that solve)
    qp.set_skip(None); qp.solve()                                    # an update_matrices solve without a skip array repairs the factors
    qp.update_vectors(ls.q, ls.l, ls.u); qp.solve()
    assert np.isfinite(qp.get()["x"][0]).all()
    # solve_host solves the whole batch
    qp.set_skip(mk)
    dense = lambda a, w: np.ascontiguousarray(np.broadcast_to(a, (ls.batch, w)))
    host = (dense(ls.P, qp.nnzP), dense(ls.q, ls.n), dense(ls.A, qp.nnzA), dense(ls.l, ls.m), dense(ls.u, ls.m))
    assert "skip" in _err(_lib.ERR_STATE, qp.solve_host, *host)
    qp.set_skip(None)
    qp.solve_host(*host)
    _err(_lib.ERR_STATE, qp.debug_skip_list)
    with pytest.raises(ValueError):
        qp.set_skip(np.zeros(ls.batch + 1, np.int32))
    qp.close()
    # a reduced handle keeps the same books
    red = ic.INSTANCE_CASES[ic._admm(4, 5, 0)][0]
    lr = ic.row_data(*_key(red)).ls
    qr = _handle(monkeypatch, red, {})
    qr.keep_workspace(True)
    qr.update(lr.P, lr.q, lr.A, lr.l, lr.u); qr.set_skip(_mask(lr.batch, [0])); qr.solve()
    _err(_lib.ERR_STATE, qr.update_vectors, lr.q, lr.l, lr.u)
    qr.set_skip(None); qr.update(lr.P, lr.q, lr.A, lr.l, lr.u); qr.solve()
    qr.update_vectors(lr.q, lr.l, lr.u); qr.solve()
    qr.close()


# ------------------------------------------------------------------------------------------------ 6. polish; warm start + rho
POLISH_KEYS = BITS + ("polish_status", "polish_info")


def test_polish_under_a_mask(built, monkeypatch):
    r = OC4_ROW
    ls = ic.row_data(*_key(r)).ls
    q2, l2, u2 = ic.kept_vectors(*_key(r))
    mk = _mask(ls.batch, [0, 4])
    qa = _handle(monkeypatch, r, {}); qa.set_polish(True)
    R = _solve(qa, ls); qa.close()
    assert (R["polish_status"] != _lib.POLISH_NOT_PERFORMED).any()
    qb = _handle(monkeypatch, r, {}); qb.set_polish(True)
    qb.update(ls.P, q2, ls.A, l2, u2); qb.solve(); R2 = qb.get()
    assert _differs(R, R2) and not np.array_equal(R["polish_info"], R2["polish_info"], equal_nan=True)
    qb.update(ls.P, ls.q, ls.A, ls.l, ls.u); qb.set_skip(mk); qb.solve()
    _check(qb.get(), R, R2, mk, "polish under a mask", POLISH_KEYS)
    qb.close()


def test_warm_start_and_rho_under_a_mask(built, monkeypatch):
    r = OC4_ROW
    ls = ic.row_data(*_key(r)).ls
    q2, l2, u2 = ic.kept_vectors(*_key(r))
    B = ls.batch
    mk = _mask(B, [2, 5])
    rng = np.random.default_rng(43)
    x0, y0 = 0.1 * rng.standard_normal((B, ls.n)), 0.1 * rng.standard_normal((B, ls.m))
    rho0 = np.linspace(0.05, 0.4, B)

    def run(qp, q, l, u, x0, y0, rho0):
        qp.update(ls.P, q, ls.A, l, u); qp.warm_start(x0, y0); qp.set_rho(rho0); qp.solve()
        return qp.get()
    qa = _handle(monkeypatch, r, dict(warm_start=1))
    R = run(qa, ls.q, ls.l, ls.u, x0, y0, rho0); qa.close()
    qc = _handle(monkeypatch, r, {})
    cold = _solve(qc, ls); qc.close()
    assert not np.array_equal(R["iters"], cold["iters"])             # the start and the rho are used
    qb = _handle(monkeypatch, r, dict(warm_start=1))
    R2 = run(qb, q2, l2, u2, x0, y0, rho0)
    # none of a skipped instance's inputs is read: NaN in its q, bounds, start and rho leaves no trace
    sk = mk != 0
    poison = lambda a: np.where(sk.reshape((B,) + (1,) * (a.ndim - 1)), np.nan, a)
    qb.set_skip(mk)
    got = run(qb, poison(np.array(np.broadcast_to(ls.q, (B, ls.n)))), poison(np.array(np.broadcast_to(ls.l, (B, ls.m)))),
              poison(np.array(np.broadcast_to(ls.u, (B, ls.m)))), poison(x0), poison(y0), poison(rho0))
    _check(got, R, R2, mk, "warm start + rho under a mask")
    qb.close()


# ------------------------------------------------------------------------------------------------ 7. the hint composes
def test_hint_on(built, monkeypatch):
    ls, q2, half = _tiled()
    B = ls.batch
    st = ic.leg_settings(*_key(OC8_ROW), "default")
    qp = _oc8_handle(monkeypatch, ls, st)                            # (the hint is on by default)
    R = _solve(qp, ls)
    assert len(np.unique(R["iters"])) > 1                            # the hint has something to order
    qp.update(ls.P, q2, ls.A, ls.l, ls.u); qp.solve(); R2 = qp.get()
    mk = half.astype(np.int32)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.set_skip(mk); qp.solve()
    _check(qp.get(), R, R2, mk, "hint on")
    lst = qp.debug_skip_list()
    n_act = int((mk == 0).sum())
    assert sorted(lst[:n_act].tolist()) == np.flatnonzero(mk == 0).tolist() and (lst[n_act:] == -1).all()
    # the base was the hint's order (longest first by the iteration counts of the solve before: R2's), not the identity
    assert lst[:n_act].tolist() != np.flatnonzero(mk == 0).tolist()
    unit = 25                                                        # (check_termination: the bin width of mpcqp_order_kernel)
    assert len(np.unique(R2["iters"] // unit)) > 1
    rank = R2["iters"][lst[:n_act]] // unit
    assert (np.diff(rank) <= 0).all(), rank[:32]
    qp.close()


# ------------------------------------------------------------------------------------------------ 8. capture
def test_captured_solve_follows_the_device_array(built, monkeypatch):
    import torch
    r = OC4_ROW
    ls = ic.row_data(*_key(r)).ls
    q2, l2, u2 = ic.kept_vectors(*_key(r))
    B = ls.batch
    qa = _handle(monkeypatch, r, {})
    R = _solve(qa, ls); qa.close()
    qb = _handle(monkeypatch, r, {})
    mA, mB = _mask(B, [0, 3]), _mask(B, [1, 6, 7])
    t = torch.as_tensor(mA, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream(); g = torch.cuda.CUDAGraph()

    def other():                                                      # the handle's buffers at R2, then the original data in place again
        qb.set_skip(None)
        qb.update(ls.P, q2, ls.A, l2, u2); qb.solve(stream=s.cuda_stream); res = qb.get()
        qb.update(ls.P, ls.q, ls.A, ls.l, ls.u); qb.set_skip(t)
        return res
    with torch.cuda.stream(s):
        other()
        qb.solve(stream=s.cuda_stream); s.synchronize()
        with torch.cuda.graph(g, stream=s):
            qb.solve(stream=s.cuda_stream)
        R2 = other()
        g.replay(); s.synchronize()
        _check(qb.get(), R, R2, mA, "replay under the captured contents")
        R2 = other()
        t.copy_(torch.as_tensor(mB, dtype=torch.int32)); s.synchronize()      # in place: no set_skip, no new capture
        g.replay(); s.synchronize()
        _check(qb.get(), R, R2, mB, "replay after the contents changed")
    assert _differs(R, R2)
    qb.close()


# ------------------------------------------------------------------------------------------------ 9. the loops
def _loop(mdl, arg, options, B, x0=None):
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    dev = DeviceSQPOptimizationSolver(mdl, options, batch=B)
    out = dev.getOptimalSolution(arg)
    rep = dict(x=out["x"], f=out["f"], converged=dev.converged.cpu().numpy(), converged_at=dev.converged_at.cpu().numpy(), done=dev.iterations_done,
               history=[h.cpu().numpy() for h in dev.kkt_history], admm=[a.cpu().numpy() for a in dev.admm_iterations])
    dev.close()
    return rep


def _same_loop(on, off, tag):
    assert np.array_equal(on["converged_at"], off["converged_at"]) and np.array_equal(on["converged"], off["converged"]), (tag, on["converged_at"], off["converged_at"])
    assert on["done"] == off["done"] and len(on["history"]) == len(off["history"]), tag
    assert np.array_equal(bits(on["x"]), bits(off["x"])) and np.array_equal(bits(on["f"]), bits(off["f"])), tag
    for a, b in zip(on["history"], off["history"]):
        assert np.array_equal(bits(a), bits(b)), tag
    at = on["converged_at"]
    skipped = 0
    for i, (a, b) in enumerate(zip(on["admm"], off["admm"])):
        frozen = (at >= 0) & (at <= i)
        assert (a[frozen] == 0).all() and np.array_equal(a[~frozen], b[~frozen]) and (b[~frozen] > 0).all(), (tag, i, a, b)
        skipped += int(frozen.sum())
    return skipped


def test_device_loop_with_the_option_is_the_loop_without_it(built):
    mdl, arg = kc.recipe()
    off = _loop(mdl, arg, kc.recipe_options(), kc.RECIPE_BATCH)
    on = _loop(mdl, arg, kc.recipe_options(skip_converged_qps=True), kc.RECIPE_BATCH)
    assert off["converged_at"].tolist() == [1, 1, 1, 2, 2, 2, 3, 6]
    assert _same_loop(on, off, "recipe") == 3 * 5 + 3 * 4 + 3          # QPs left out: instances frozen at 1, 2, 3 over the iterations up to 5


@pytest.mark.parametrize("extra", [{"line_search": True, "warm_start_admm": True}, {"keep_scaling": True, "sqp_tol": 1e-12},
                                   {"presolve_fixed_rows": True, "skip_failed_steps": True}], ids=["line_search+warm_start", "keep_scaling+sqp_tol", "presolve_fixed_rows"])
def test_option_combinations(built, extra):
    mdl, arg = kc.recipe()
    off = _loop(mdl, arg, kc.recipe_options(**extra), kc.RECIPE_BATCH)
    on = _loop(mdl, arg, kc.recipe_options(skip_converged_qps=True, **extra), kc.RECIPE_BATCH)
    assert _same_loop(on, off, str(extra)) > 0 and on["converged"].all()


def test_constant_matrices_under_damping(built):
    """the recipe of tests/test_gpu_kkt.py test_constant_matrices_and_damping: every QP after the first is a vectors-only solve on the kept workspace, the later ones
    under the frozen mask (converged_at = 7 7 7 7 7 8 8 8)"""
    B = 8
    mdl = models.DoubleIntegrator(20, 0.05)
    frame0 = np.zeros((B, 3)); frame0[:, 0] = np.linspace(0.05, 2.5, B); frame0[:, 1] = 0.3
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    arg = dict(p=np.zeros((B, mdl.np)), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    opt = {"max_iter": 30, "alpha": 0.5, "kkt_tol": 1.25e-2, "constant_matrices": True}
    off = _loop(mdl, arg, opt, B)
    on = _loop(mdl, arg, dict(opt, skip_converged_qps=True), B)
    assert off["converged_at"].tolist() == [7, 7, 7, 7, 7, 8, 8, 8]
    assert _same_loop(on, off, "constant_matrices") == 5


def test_host_loop_on_the_gpu_backend(built):
    """the host loop with its default backend (cucaqp.CuCaQP on the GPU: setSkip -> mpcqp_set_skip with a host array, every QP a full set-up): the option changes
    no bit of x, converged_at, kkt_history, and a frozen instance's rows of last_qp_info are finite (those of its last solved QP)"""
    from optimal_control_problem_amd.sqp import SQPOptimizationSolver
    mdl, arg = kc.recipe()
    out = {}
    for key, extra in (("off", {}), ("on", {"skip_converged_qps": True})):
        sol = SQPOptimizationSolver(mdl, kc.recipe_options(**extra), batch=kc.RECIPE_BATCH)
        res = sol.getOptimalSolution(arg)
        out[key] = (sol, res)
    (on, ron), (off, roff) = out["on"], out["off"]
    assert np.array_equal(on.converged_at, off.converged_at) and off.converged_at.tolist() == [1, 1, 1, 2, 2, 2, 3, 6]
    assert np.array_equal(bits(ron["x"]), bits(roff["x"])) and len(on.kkt_history) == len(off.kkt_history)
    for a, b in zip(on.kkt_history, off.kkt_history):
        assert np.array_equal(bits(a), bits(b))
    for i, (a, b) in enumerate(zip(on.admm_iterations, off.admm_iterations)):
        frozen = (on.converged_at >= 0) & (on.converged_at <= i)
        assert (a[frozen] == 0).all() and np.array_equal(a[~frozen], b[~frozen])
    assert np.isfinite(on.last_qp_info["x"]).all() and (np.asarray(on.last_qp_info["status"]) == 1).all()
    on.qpSolver_.close(); off.qpSolver_.close()


def test_cucaqp_wrapper_after_a_set_up_under_a_skip_array(built, monkeypatch):
    """cucaqp.CuCaQP: after initSolver + solve under a skip array the library refuses the vectors-only update (MPCQP_ERR_STATE); the wrapper's solve() after
    updateGradient then runs the full set-up -- under the array still set, and, once it is cleared, for every instance: the bits of a fresh object's solve"""
    from optimal_control_problem_amd.cucaqp import CuCaQP
    for name in [n for n in os.environ if n.startswith("MPCQP_")]:
        monkeypatch.delenv(name)
    r = OC4_ROW
    ls = ic.row_data(*_key(r)).ls
    q2 = problems.kept_q(ls)
    B = ls.batch
    mk = _mask(B, [0, 5])

    def fresh(q):
        qp = CuCaQP(batch=B)
        assert qp.setDimension(ls.n, ls.m)
        qp.setSystem([(ls.Pp, ls.Pi, ls.P), q, (ls.Ap, ls.Ai, ls.A), ls.l, ls.u])
        return qp
    ref = fresh(q2); assert ref.initSolver() and ref.solve()
    want = {k: np.array(v) for k, v in ref.getInfo().items()}; ref.close()
    qp = fresh(ls.q)
    assert qp.initSolver()
    qp.setSkip(mk)
    assert qp.solve()
    first = {k: np.array(v) for k, v in qp.getInfo().items()}
    assert qp.updateGradient(q2) and qp.solve()                      # (update_vectors is refused behind the wrapper: the full set-up, under the mask)
    _check(qp.getInfo(), want, first, mk, "wrapper: solve after updateGradient under the mask", ("x", "y", "status", "iters"))
    qp.setSkip(None)
    assert qp.updateGradient(q2) and qp.solve()                      # (still refused: the skipped instances hold no factor; the full set-up repairs them)
    _bitwise(qp.getInfo(), want, "wrapper: solve after the mask was cleared", ("x", "y", "status", "iters"))
    assert qp.updateGradient(ls.q) and qp.solve()                    # (and from here the kept workspace serves again)
    qp.close()


def test_option_is_refused_without_kkt_tol(built):
    from optimal_control_problem_amd.sqp import SKIP_NEEDS_KKT, DeviceSQPOptimizationSolver
    mdl, _ = kc.recipe()
    with pytest.raises(ValueError) as e:
        DeviceSQPOptimizationSolver(mdl, {"max_iter": 2, "alpha": 1.0, "skip_converged_qps": True}, batch=2)
    assert str(e.value) == SKIP_NEEDS_KKT


def test_closed_loop_mpc_three_ticks(built):
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    mdl, _ = kc.recipe()
    B = kc.RECIPE_BATCH
    frame0 = np.zeros((B, mdl.f)); frame0[:, 1] = kc.recipe_angles()
    out = {}
    for key, extra in (("off", {}), ("on", {"skip_converged_qps": True})):
        mpc = ClosedLoopMPC(mdl, kc.recipe_options(max_iter=6, **extra), batch=B)
        mpc.reset(frame0)
        ticks = []
        for _ in range(3):
            rr = mpc.tick()
            ticks.append((rr["applied"].cpu().numpy().copy(), mpc.sol.converged_at.cpu().numpy().copy(), mpc.sol.iterations_done,
                          [a.cpu().numpy() for a in mpc.sol.admm_iterations]))
        out[key] = (ticks, mpc.x.cpu().numpy().copy())
        mpc.close()
    assert np.array_equal(bits(out["on"][1]), bits(out["off"][1]))
    for (a_on, at_on, d_on, _), (a_off, at_off, d_off, _) in zip(out["on"][0], out["off"][0]):
        assert np.array_equal(bits(a_on), bits(a_off)) and np.array_equal(at_on, at_off) and d_on == d_off
    admm = out["on"][0][-1][3]
    assert any((a == 0).any() for a in admm)                          # some QP of some tick was left out


def test_cpp_program_equals_the_python_loop(built):
    mdl, arg = kc.recipe()
    rep = _loop(mdl, arg, kc.recipe_options(skip_converged_qps=True), kc.RECIPE_BATCH)
    exe = os.path.join(ROOT, "tests", "support", "stagesqp_skip_test")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.splitlines() if ln.strip()}
    assert int(out["iterations_done"][0]) == rep["done"]
    assert [int(v) for v in out["converged_at"]] == rep["converged_at"].tolist() == [1, 1, 1, 2, 2, 2, 3, 6]
    vec = lambda key: np.array([float(v) for v in out[key]]).reshape(rep["x"].shape)
    assert np.array_equal(bits(vec("x")), bits(rep["x"])) and np.array_equal(bits(vec("x_plain")), bits(rep["x"]))
    # second leg: the KKT stop switched off again with the skip option still set -- no verdict of the first call may skip a QP: the fixed twelve iterations
    # of the whole batch, bit for bit those of a twin that never had the option (and they do move x)
    assert [int(v) for v in out["iterations_off"]] == [12, 12]
    assert np.array_equal(bits(vec("x_off")), bits(vec("x_off_plain"))) and not np.array_equal(bits(vec("x_off")), bits(vec("x")))
