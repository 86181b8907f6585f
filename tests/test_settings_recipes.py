"""CPU: the inputs of tests/test_gpu_settings.py -- problems.hard_stage_batch x problems.SETTINGS_MATRIX -- on the oracle alone.  The GPU module asks every
kernel family for the oracle's status, iteration count, iterates and info under every setting; what that is worth depends on what the oracle does with
these inputs: whether the certificates of infeasibility are found, whether they are found in the code after the loop (the runs that end off a termination
check), whether the decisions hang on rounding.  These tests hold the inputs to what the GPU tests rely on, so that a change of the oracle, of a model or
of a seed shows up here and not as a GPU mystery."""
import functools

import numpy as np
import pytest

from tests.support import problems

WORKLOADS = list(problems.HARD_WORKLOADS)
SETTINGS = list(problems.SETTINGS_MATRIX)
UNSTABLE_CAP = 0.10          # share of a batch that may be left out of the comparison of iteration counts (the cap of tests/test_rho_recipes.py)
CERTIFICATES = (3, 4, 5, 6)

# oracle statuses / iteration counts, measured when the matrix was drawn up (8 threads; the thread count changes no result)
PINNED_STATUS = {
    ("q20", "default"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "max_iter=24"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "check=0,max_iter=40"): [1, 5, 3, 1, 1, 1, 1, 1],
    ("q20", "check=7,max_iter=30"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "check=1"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "alpha=1.0"): [1, 5, 3, 1, 1, 1, 1, 1],
    ("q20", "scaling=0"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "scaled_termination=1"): [1, 5, 3, 1, 1, 1, 1, 1], ("q20", "eps_dual_inf=1e-7"): [1, 5, 3, 1, 1, 1, 1, 1],
    ("q20", "eps_prim_inf=1e-7,eps_dual_inf=1e-2"): [1, 5, 3, 1, 1, 1, 1, 1],
    ("cp30", "max_iter=37"): [2, 2, 4, 2, 7, 7], ("cp30", "max_iter=60"): [2, 2, 4, 2, 2, 2], ("cp30", "check=7,max_iter=30"): [7, 2, 3, 7, 7, 2],
    ("cp30", "scaling=0"): [1, 5, 3, 1, 1, 1], ("cp30", "default"): [1, 1, 3, 1, 1, 1], ("cp30", "scaled_termination=1"): [1, 5, 3, 1, 1, 1],
    ("q50", "max_iter=24"): [2, 5, 4, 1], ("q50", "max_iter=37"): [2, 5, 3, 1], ("q50", "check=7,max_iter=30"): [1, 5, 3, 1],
    ("cp100", "max_iter=60"): [2, 2, 4, 2], ("cp100", "check=7,max_iter=30"): [2, 1, 4, 2],
}
PINNED_ITERS = {
    ("q20", "default"): [25] * 8, ("q20", "max_iter=24"): [24] * 8, ("q20", "check=0,max_iter=40"): [40] * 8,
    ("q20", "check=7,max_iter=30"): [21, 14, 28, 21, 21, 28, 28, 21], ("q20", "check=1"): [21, 24, 21, 21, 21, 22, 22, 21],
    ("q20", "alpha=1.0"): [50, 25, 50, 25, 25, 25, 25, 25], ("q20", "scaling=0"): [125, 25, 125, 75, 75, 75, 75, 75],
    ("q20", "scaled_termination=1"): [50, 25, 50, 25, 50, 50, 50, 50],
    ("cp30", "max_iter=37"): [37] * 6, ("cp30", "max_iter=60"): [60] * 6, ("cp30", "check=7,max_iter=30"): [30] * 6, ("cp30", "scaling=0"): [125, 25, 125, 125, 125, 125],
    ("q50", "max_iter=24"): [24] * 4, ("q50", "max_iter=37"): [37, 25, 25, 25], ("q50", "check=7,max_iter=30"): [21, 21, 30, 28],
    ("cp100", "max_iter=60"): [60] * 4, ("cp100", "check=7,max_iter=30"): [30] * 4,
}


@functools.lru_cache(maxsize=None)
def _oracle(wid, sid):
    """-> (oracle result, stable mask) of one workload under one entry of the matrix"""
    _, ls, _ = problems.hard_stage_batch(wid)
    st = problems.SETTINGS_MATRIX[sid]
    return problems.oracle_solve(ls, nthreads=8, **st), problems.oracle_stable_mask(ls, nthreads=8, **st)


def test_the_matrix_is_what_the_gpu_module_expects():
    assert len(SETTINGS) >= 17 and SETTINGS[0] == "default" and problems.SETTINGS_MATRIX["default"] == {}
    from oracle import oracle as orc
    d = orc.default_settings()
    named = set()
    for sid, st in problems.SETTINGS_MATRIX.items():
        for k, v in st.items():
            assert getattr(d, k) != v or k == "max_iter", (sid, k)          # (a setting at its default value tests nothing)
            named.add(k)
        if st.get("check_termination", 1) == 0:
            assert st["max_iter"] <= 200, sid
    assert named >= {"alpha", "sigma", "rho", "check_termination", "eps_prim_inf", "eps_dual_inf", "scaling", "scaled_termination", "adaptive_rho", "max_iter"}
    assert {problems.SETTINGS_MATRIX[s].get("scaling") for s in SETTINGS} >= {0, 3}
    assert set(problems.TAIL_CASES) == {"max_iter=24", "max_iter=37", "max_iter=60", "check=0,max_iter=40", "check=7,max_iter=30"}
    assert set(problems.NEVER_SAVED) <= set(problems.TAIL_CASES)


@pytest.mark.parametrize("wid", WORKLOADS)
def test_the_two_spoilt_instances_are_what_they_are_meant_to_be(built, wid):
    """the recipe itself: one row of A in the column of the last input (its box), nothing of the dynamics; the other instances untouched"""
    from optimal_control_problem_amd import models
    name, N, B = problems.HARD_WORKLOADS[wid]
    mdl, ls, meta = problems.hard_stage_batch(wid)
    _, plain, _ = models.make_workload(name, B, N=N)
    assert ls.batch == B and ls.P.shape == (B, len(ls.Pi)) and len(meta["dual_rows"]) == 1
    assert int(meta["dual_rows"][0]) == {"q20": 331, "cp30": 153, "q50": 811, "cp100": 503}[wid]
    keep = np.setdiff1d(np.arange(B), [problems.DUAL_INFEASIBLE, problems.PRIMAL_INFEASIBLE])
    for a, b in ((ls.P, np.broadcast_to(plain.P, ls.P.shape)), (ls.q, plain.q), (ls.l, plain.l), (ls.u, plain.u)):
        assert np.array_equal(a[keep], b[keep])
    assert np.array_equal(ls.A, plain.A)
    Pd, _ = ls.dense(problems.DUAL_INFEASIBLE)
    assert not Pd[-1].any() and not Pd[:, -1].any() and ls.q[problems.DUAL_INFEASIBLE, -1] == -1.0
    _, _, only_primal = problems.hard_stage_batch(wid, dual=False)
    assert len(only_primal["dual_rows"]) == 0


def test_every_status_but_the_inaccurate_dual_certificate_is_reached(built):
    """1, 2, 3, 4, 5 and 7 occur; 6 (dual infeasible, inaccurate) does not on these inputs, and is not constructed: the GPU module asserts whatever the oracle says"""
    seen = set()
    for wid in WORKLOADS:
        for sid in SETTINGS:
            seen |= set(_oracle(wid, sid)[0]["status"].tolist())
    print("oracle statuses over the matrix:", sorted(seen))
    assert seen >= {1, 2, 3, 4, 5, 7}, seen
    assert seen <= {1, 2, 3, 4, 5, 6, 7}, seen          # (never non-convex or refused: ordinary inputs)


@pytest.mark.parametrize("wid", WORKLOADS)
def test_every_workload_finds_a_certificate_in_the_code_after_the_loop(built, wid):
    """in at least one tail case an instance ends with a certificate status and iters == max_iter: found by the test behind the loop, from the steps of the
    last iteration"""
    hits = []
    for sid in problems.TAIL_CASES:
        ref, _ = _oracle(wid, sid)
        mi = problems.SETTINGS_MATRIX[sid]["max_iter"]
        if (np.isin(ref["status"], CERTIFICATES) & (ref["iters"] == mi)).any():
            hits.append(sid)
    assert hits, wid
    if wid == "q20":          # the two cases in which nothing in the loop ever looks at the steps
        assert set(problems.NEVER_SAVED) <= set(hits), hits
        for sid in problems.NEVER_SAVED:
            st = problems.SETTINGS_MATRIX[sid]
            check, interval = st.get("check_termination", 25), 4 * st.get("check_termination", 25) or 100
            assert (check == 0 or st["max_iter"] < check) and st["max_iter"] < interval


@pytest.mark.parametrize("sid", SETTINGS)
@pytest.mark.parametrize("wid", WORKLOADS)
def test_decisions_do_not_hang_on_rounding(built, wid, sid):
    ref, ok = _oracle(wid, sid)
    assert (~ok).sum() <= UNSTABLE_CAP * len(ok), (wid, sid, np.flatnonzero(~ok))


@pytest.mark.parametrize("wid,sid", sorted(PINNED_STATUS))
def test_pinned_outcomes(built, wid, sid):
    ref, _ = _oracle(wid, sid)
    assert ref["status"].tolist() == PINNED_STATUS[(wid, sid)], (wid, sid, ref["status"])
    if (wid, sid) in PINNED_ITERS:
        assert ref["iters"].tolist() == PINNED_ITERS[(wid, sid)], (wid, sid, ref["iters"])


def test_the_cart_pole_certificate_depends_on_the_scaling(built):
    """the cart-pole's dual-infeasible instance ends `solved` under the default scaling and with the certificate without scaling or with the scaled termination
    test: OSQP's behaviour, which the GPU has to reproduce"""
    b = problems.DUAL_INFEASIBLE
    assert _oracle("cp30", "default")[0]["status"][b] == 1
    assert _oracle("cp30", "scaling=0")[0]["status"][b] == 5 and _oracle("cp30", "scaled_termination=1")[0]["status"][b] == 5


def test_reduced_and_kept_legs(built):
    """what the smaller legs of the GPU module rely on: the reduced form of q20 still reports both certificates, and a kept workspace still sees them after
    a change of q"""
    mdl, ls, _ = problems.hard_stage_batch("q20")
    red = problems.reduce_qp(ls, list(range(mdl.np)))[0]
    for sid in problems.REDUCED_CASES:
        r = problems.oracle_solve(red, nthreads=8, **problems.SETTINGS_MATRIX[sid])
        assert r["status"][problems.PRIMAL_INFEASIBLE] == 3 and r["status"][problems.DUAL_INFEASIBLE] == 5, (sid, r["status"])
        assert (~problems.oracle_stable_mask(red, **problems.SETTINGS_MATRIX[sid])).sum() <= UNSTABLE_CAP * ls.batch
    for wid in ("q20", "q50"):
        _, ls, _ = problems.hard_stage_batch(wid)
        for sid in problems.KEPT_CASES:
            st = problems.SETTINGS_MATRIX[sid]
            first, second = problems.oracle_kept_solves(ls, problems.kept_q(ls), **st)
            assert np.array_equal(first["status"], _oracle(wid, sid)[0]["status"])
            assert second["status"][problems.PRIMAL_INFEASIBLE] in (3, 4) and second["status"][problems.DUAL_INFEASIBLE] in (5, 6), (wid, sid, second["status"])
            assert np.abs(second["x"][0] - first["x"][0]).max() > 1e-3, (wid, sid)      # (the new q changes the answer)
            for ok in problems.oracle_kept_stable_mask(ls, problems.kept_q(ls), **st):
                assert (~ok).sum() <= UNSTABLE_CAP * ls.batch, (wid, sid, np.flatnonzero(~ok))
