"""CPU: the NumPy reference of the kept-scaling tests (tests/support/osqp_ref.py) against the CPU oracle, where the oracle has an answer.

(a) a full set-up + solve: the reference restates scale_data, the rho rule, the iteration, the termination test and the adaptive-rho schedule, so
    status, iteration counts and final rho agree with the oracle and x, y, z meet the bar of tests/test_gpu_parity.py;
(b) a solve on a scaling handed in from outside -- what mpcqp_update_matrices does, and what the oracle has no entry for -- with scaled_termination = 1
    is the unchanged oracle run with scaling = 0 on the problem scaled by hand (c D P D, c D q, E A D, E l, E u; rho carried; x = D xbar, y = E ybar / c,
    z = zbar / E): a second yardstick that shares no code with the reference;
(c) the stability mask the GPU tests use (iteration counts are only asked of instances whose decisions do not hang on rounding) leaves at least three
    quarters of every batch in, at both tolerances, so that it cannot hide a failure."""
import functools

import numpy as np
import pytest

from tests.support import kept_scaling as ks
from tests.support import osqp_ref, problems
from tests.test_gpu_parity import _close

WORKLOADS = ("q20", "cp30")


def _agree(got, ref):
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    assert (got["iters"] == ref["iters"]).all(), (got["iters"], ref["iters"])
    assert (np.abs(got["rho"] - ref["rho"]) <= 1e-6 * np.abs(ref["rho"])).all(), (got["rho"], ref["rho"])
    for k in ("x", "y", "z"):
        _close(got, ref, k)


@functools.lru_cache(maxsize=None)
def _full(sid, eps):
    return ks.ref(("full", sid, eps), ks.sequence(sid)[0], ks.EPS[eps])


@pytest.mark.parametrize("eps", list(ks.EPS))
@pytest.mark.parametrize("sid", WORKLOADS)
def test_reference_against_the_oracle_full_setup(built, sid, eps):
    ls = ks.sequence(sid)[0]
    _agree(_full(sid, eps), problems.oracle_solve(ls, nthreads=8, **ks.EPS[eps]))


@pytest.mark.parametrize("eps", list(ks.EPS))
@pytest.mark.parametrize("sid", WORKLOADS)
def test_kept_scaling_against_the_prescaled_oracle(built, sid, eps):
    first = _full(sid, eps)
    qp2 = ks.sequence(sid)[1]
    st = dict(ks.EPS[eps], scaled_termination=1)
    got = osqp_ref.solve_batch(qp2, st, first["scaling"], first["rho"])
    for b in range(qp2.batch):      # (the scaling that came in is the scaling that was used)
        assert all(np.array_equal(a, c) for a, c in zip(got["scaling"][b], first["scaling"][b]))
    want = problems.oracle_solve(osqp_ref.prescaled(qp2, first["scaling"]), nthreads=8, rho0=first["rho"], **dict(st, scaling=0))
    _agree(got, osqp_ref.unscaled(want, first["scaling"]))


def test_scale_data_is_the_oracles(built):
    """D, E, c alone: a scaling = 0 run of the oracle on the reference's scaled data equals the oracle's own scaled run, iteration for iteration"""
    ls = ks.sequence("q20")[0]
    sc = [osqp_ref.scale_data(*_sym(ls, b), 10) for b in range(ls.batch)]
    a = osqp_ref.unscaled(problems.oracle_solve(osqp_ref.prescaled(ls, sc), nthreads=8, scaling=0), sc)
    b = problems.oracle_solve(ls, nthreads=8, scaled_termination=1)
    assert (a["iters"] == b["iters"]).all() and (a["status"] == b["status"]).all()
    _close(a, b, "x")


def _sym(ls, b):
    P, A = osqp_ref.dense_instance(ls, b)
    return np.triu(P) + np.triu(P, 1).T, ls.q[b], A


@pytest.mark.parametrize("eps", list(ks.EPS))
@pytest.mark.parametrize("sid", ("q20", "q25", "cp30"))
def test_stability_mask_keeps_three_quarters(built, sid, eps):
    first = ks.ref(("full", sid, eps), ks.sequence(sid)[0], ks.EPS[eps])
    mask, _ = ks.stable_mask(ks.sequence(sid)[1], ks.EPS[eps], first["scaling"], first["rho"])
    assert 4 * int(mask.sum()) >= 3 * len(mask), mask


def test_reference_reports_a_non_convex_instance():
    P = np.diag([1.0, -1.0]); A = np.eye(2)
    r = osqp_ref.solve(P, np.zeros(2), A, -np.ones(2), np.ones(2))
    assert r[3] == osqp_ref.NON_CVX and np.isnan(r[0]).all()
