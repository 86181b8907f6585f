"""GPU: what follows an adaptive-rho update in the two-kernel on-chip form (kernel_oc_split.hpp, launch_oc_split in mpcqp.hip).

A rho change makes the iteration kernel <RF=0> park x, z, y, the iteration number and the new rho and leave; MPCQP_RESUME_ROUNDS (default 1) pairs of
{set-up kernel in resume mode, iteration kernel in resume mode} follow, and a last pair whose iteration kernel <RF=1> re-factorises in place.  An
instance runs that re-factorisation from its (rounds + 2)-th update on, which the MPC workloads never reach at the reference's settings.  The recipes of
tests/support/problems.py RHO_RECIPES do (tests/test_rho_recipes.py holds them to it on the oracle): q20 -> the four-wave instance, cp30 / di60 -> the four-wave
instance with two chain pairs, q50 / cp100 -> the eight-wave queued instances.

Bar against the oracle: the module-wide one of tests/test_gpu_parity.py (RTOL relative to 1 + |ref|_inf for x, y, z; equal status; equal iteration counts
for the instances whose decisions do not hang on rounding, problems.oracle_stable_mask) and the final rho to the same relative bar -- the one output that
tells whether every update was applied.  Everything else is bitwise: a run resumed is the run continued.

Measured on an MI355X with this module's first run:
  * bitwise equality holds for every pair of settings: MPCQP_RESUME_ROUNDS 0 / 1 / 2 / 8 and the single-kernel form on all five recipes (for cp30 and di60, whose
    default order has two chain pairs and no single-kernel instance, the single kernel against the two-kernel form in the one-pair order), 700 queued instances
    against batches of 12, the pipelined host step, two graph replays;
  * largest |x_gpu - x_oracle| / (1 + |x_oracle|_inf) at eps 1e-7 through the <RF=1> kernels: 9.45e-11 (q20, four waves), 9.07e-11 (q50, eight waves); at eps 1e-6
    8.26e-09 (cp30), 2.16e-12 (di60); cp100 (default eps) 9.50e-09; the 64-instance sample of q50 x 700: 6.60e-09.  Final rho over 1 + |rho|_inf: 3.41e-07 (q20) at most;
  * rho alone, relative, is a looser story than x: 2.0e-05 on q20 cold, 2.0e-04 warm-started, 7.9e-04 in the q50 x 700 sample, the same in the single-kernel form --
    see _same_as_oracle;
  * mutants, built by hand and not kept: the last launch pair without the in-place re-factorisation leaves status 100 with the caller, and a park that does not
    store the new rho changes iteration counts -- either fails every test of (a) and (b);
  * iteration limits on an update: parked on the limit (first update at MPCQP_RESUME_ROUNDS = 0, second at 1) and served in place on the limit (second at 0)
    all give status 7, iters == max_iter and x within 2.9e-09 of the oracle's over 1 + |x|_inf, rho within 4e-09 relative;
  * wall time, each figure pytest's own total for one invocation: this module run alone 11.4 s (29 tests; 1.3 s of it the session's build check, and the oracle
    runs, which the module caches per recipe); the whole GPU suite 64.5 s for 266 tests with this module and the two new on-chip fuzz legs; the other 235 tests
    without them 41.1 s when run right after in the same visit and 53.4 s in a visit of their own -- the suite's time moves by that much from run to run, so the
    cost of the new tests is the 11 - 13 s they take themselves (GPUTEST_r04: 48.6 s for 234 tests).
"""
import functools

import numpy as np
import pytest

from tests.support import problems
from tests.test_gpu_parity import RTOL, _close      # noqa: F401 (RTOL: the bar _close applies)

pytestmark = pytest.mark.gpu

FAMILY = {"q20": "oc4", "cp30": "oc4", "di60": "oc4", "q50": "oc8", "cp100": "oc8"}
CHAIN_PAIRS = {"q20": 1, "cp30": 2, "di60": 2, "q50": 1, "cp100": 4}          # twisted pairs of chains: 1 = the twisted order, more = the dissected order (plan.hpp ordering 4)
KNOBS = ("MPCQP_RESUME_ROUNDS", "MPCQP_VARIANT", "MPCQP_OC_MONO", "MPCQP_NO_DISSECT")
BITS = ("x", "y", "z", "status", "iters", "obj", "prim_res", "dual_res", "rho")


@functools.lru_cache(maxsize=None)
def _recipe(rid):
    """-> (LocalSystem, settings, oracle result, stable mask, rho updates per instance)"""
    _, ls, _, st = problems.rho_recipe(rid)
    return ls, st, problems.oracle_solve(ls, nthreads=8, **st), problems.oracle_stable_mask(ls, **st), problems.oracle_rho_updates(ls, **st)


def _handle(monkeypatch, rid, ls, st, rounds, mono=False, dissect=True, batch=None):
    """a handle of the recipe's family at MPCQP_RESUME_ROUNDS = rounds (mono: the single-kernel form), checked to be what it is meant to be"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPCQP_VARIANT", FAMILY[rid])
    if rounds is not None:
        monkeypatch.setenv("MPCQP_RESUME_ROUNDS", str(rounds))
    if mono:
        monkeypatch.setenv("MPCQP_OC_MONO", "1")
    if not dissect:
        monkeypatch.setenv("MPCQP_NO_DISSECT", "1")
    qp = BatchQP(ls.n, ls.m, batch or ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **st)
    info, oc = qp.plan_info(), qp.oc_info()
    assert info["variant"] == {"oc4": 204, "oc8": 208}[FAMILY[rid]], info
    assert oc["launch_pairs_for_rho_updates"] == (0 if mono else 1 + (1 if rounds is None else rounds)), oc
    if not mono:
        want = CHAIN_PAIRS[rid] if dissect else 1
        assert oc["chain_pairs"] == want and (info["ordering"] == 4) == (want > 1), (oc, info)
    return qp


def _solve(qp, ls):
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve()
    return qp.get()


RHO_DECISIONS = 1e-2


def _same_as_oracle(got, ref, stable, tag, rho_at_the_bar=False):
    """status, iteration counts of the stable instances, x / y / z and the final rho against the oracle; -> the figures.
    rho: at the bar of x, y, z in the parity tests (a).  Elsewhere to RHO_DECISIONS, relative: every update multiplies rho by a factor beyond
    adaptive_rho_tolerance (1.5 here) either way, so a decision that fell differently, an update lost or a stale rho handed to the next launch moves it
    by a third or more, while the value itself is sqrt(primal / dual residual) -- for an update a few iterations before termination a ratio of two
    numbers at their rounding floor (q20 warm-started, instance 0, iteration 60: residuals 1e-8 and 3e-9, 1e-3 apart between GPU and oracle with x
    1e-10 apart; rho 2e-4 apart, the same in the single-kernel form)."""
    assert (got["status"] == ref["status"]).all(), (tag, got["status"], ref["status"])
    assert (got["iters"][stable] == ref["iters"][stable]).all(), (tag, got["iters"], ref["iters"])
    same = stable | (got["iters"] == ref["iters"])       # (an instance that stops a check apart is a tolerance apart: its iterates are not compared)
    assert same.sum() >= 0.9 * len(same), (tag, np.flatnonzero(~same))           # (the cap tests/test_rho_recipes.py puts on the unstable ones)
    g, r = ({k: res[k][same] for k in ("x", "y", "z", "rho")} for res in (got, ref))
    fig = {k: float(np.abs(g[k] - r[k])[np.isfinite(r[k])].max() / (1.0 + np.abs(r[k][np.isfinite(r[k])]).max())) for k in g}
    print("%s: difference to the oracle over 1 + |ref|_inf: x %.2e y %.2e z %.2e rho %.2e (rho alone, relative: %.2e); iterations compared for %d of %d instances, "
          "iterates for %d" % (tag, fig["x"], fig["y"], fig["z"], fig["rho"], np.abs(g["rho"] / r["rho"] - 1.0).max(), stable.sum(), len(stable), same.sum()))
    for k in ("x", "y", "z"):
        _close(g, r, k)
    if rho_at_the_bar:
        _close(g, r, "rho")
    assert (np.abs(g["rho"] / r["rho"] - 1.0) <= RHO_DECISIONS).all(), (tag, g["rho"], r["rho"])
    return fig


def _bitwise(a, b, tag, keys=BITS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k, np.flatnonzero((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1)))


PARITY = [(rid, r) for rid in ("q20", "q50", "cp30", "cp100", "di60") for r in problems.RHO_RECIPES[rid][4]]


@pytest.mark.parametrize("rid,rounds", PARITY)
def test_oracle_parity_through_the_in_place_refactorisation(built, monkeypatch, rid, rounds):
    """(a) every recipe at the MPCQP_RESUME_ROUNDS values at which its instances reach the last launch pair: the iteration kernels <RF=1> of the four-wave
    instance, of the two-pair four-wave instance, and of the two eight-wave instances against the oracle, final rho included"""
    ls, st, ref, stable, updates = _recipe(rid)
    assert (updates >= rounds + 2).any()
    qp = _handle(monkeypatch, rid, ls, st, rounds)
    got = _solve(qp, ls); qp.close()
    _same_as_oracle(got, ref, stable, "%s rounds=%d" % (rid, rounds), rho_at_the_bar=True)
    if CHAIN_PAIRS[rid] > 1:
        # the same pattern in the plain twisted order: the one-pair instances of the same family
        qp = _handle(monkeypatch, rid, ls, st, rounds, dissect=False)
        got = _solve(qp, ls); qp.close()
        _same_as_oracle(got, ref, stable, "%s rounds=%d, one pair" % (rid, rounds), rho_at_the_bar=True)


@pytest.mark.parametrize("rid", sorted(problems.RHO_RECIPES))
def test_a_run_resumed_is_the_run_continued(built, monkeypatch, rid):
    """(b) MPCQP_RESUME_ROUNDS = 0, 1, 2, 8 (the edge of launch_oc_split's tables: ten launches, ten ticket counters) give the same bits, and those of the
    single-kernel form, which re-factorises where it stands.  The single-kernel form has no instance for the order with several chain pairs, so
    for those patterns it is compared with the two-kernel form in the one-pair order, and the rounds with one another in theirs."""
    ls, st, ref, stable, updates = _recipe(rid)
    assert (updates >= 2).any() and (ref["status"] == 1).all()
    runs = {}
    for rounds in (0, 1, 2, 8):
        qp = _handle(monkeypatch, rid, ls, st, rounds)
        runs[rounds] = _solve(qp, ls); qp.close()
        assert (runs[rounds]["status"] == ref["status"]).all(), rounds          # (never a parked instance's 100 / 101)
    for rounds in (1, 2, 8):
        _bitwise(runs[rounds], runs[0], "%s rounds %d against 0" % (rid, rounds))
    split = runs[0]
    if CHAIN_PAIRS[rid] > 1 and FAMILY[rid] == "oc4":
        qp = _handle(monkeypatch, rid, ls, st, 0, dissect=False)
        split = _solve(qp, ls); qp.close()
    qp = _handle(monkeypatch, rid, ls, st, None, mono=True)
    mono = _solve(qp, ls); qp.close()
    _bitwise(split, mono, "%s two kernels against one" % rid)


@pytest.mark.parametrize("rounds,which,parks", problems.UPDATE_LIMIT_CASES, ids=["first-update-parks", "second-update-parks", "second-update-in-place"])
@pytest.mark.parametrize("rid", ["q20", "q50"])
def test_iteration_limit_on_an_update(built, monkeypatch, rid, rounds, which, parks):
    """(c) max_iter on the iteration of a rho update, and one beyond (problems.UPDATE_LIMIT_CASES; tests/test_rho_recipes.py: the update falls there for at least
    half of the batch).  parks: the update is one that <RF=0> leaves on -- the first at MPCQP_RESUME_ROUNDS = 0, the second at 1, where the first resumed launch
    is <RF=0> too -- so the instance is parked with iters == max_iter, the set-up kernel re-factorises, and the launch that picks it up (<RF=1>, the last) has no
    iteration left, or one, and finishes in the kernel's tail from the state in the slab.  Not parks: the second update at MPCQP_RESUME_ROUNDS = 0 comes in <RF=1>,
    which re-factorises in place in its last iteration, or last but one.  Either way the caller sees MPCQP_MAX_ITER_REACHED, iters == max_iter and the oracle's
    iterates, info and rho, never a parked instance's status."""
    ls, st, _, _, _ = _recipe(rid)
    for mi in problems.update_limits(ls, st, which):
        s = dict(st, max_iter=mi)
        ref = problems.oracle_solve(ls, nthreads=8, **s)
        assert (ref["status"] == 7).all() and (ref["iters"] == mi).all()
        qp = _handle(monkeypatch, rid, ls, s, rounds)
        got = _solve(qp, ls); qp.close()
        tag = "%s rounds=%d max_iter=%d (%s)" % (rid, rounds, mi, "parked on the limit" if parks else "in place on the limit")
        _same_as_oracle(got, ref, problems.oracle_stable_mask(ls, **s), tag)
        assert (got["iters"] == mi).all(), tag
        for k in ("obj", "prim_res", "dual_res"):
            _close(got, ref, k)


@pytest.mark.parametrize("rid", ["q20", "q50"])
def test_neighbours_leave_at_different_iterations(built, monkeypatch, rid):
    """(c) per-instance starting rho (mpcqp_set_rho), half the batch at 0.1 and half at 10: neighbouring instances need different numbers of launches"""
    ls, st, _, _, _ = _recipe(rid)
    rho0 = problems.split_rho(ls.batch)
    ref = problems.oracle_solve(ls, nthreads=8, rho0=rho0, **st)
    qp = _handle(monkeypatch, rid, ls, st, 0)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.set_rho(rho0); qp.solve(); got = qp.get(); qp.close()
    _same_as_oracle(got, ref, problems.oracle_stable_mask(ls, rho0=rho0, **st), "%s rho0 0.1 | 10" % rid)


@pytest.mark.parametrize("rid", ["q20", "q50"])
def test_warm_start_through_the_hand_over(built, monkeypatch, rid):
    """(c) mpcqp_warm_start from the oracle's solution of a perturbed q: fewer updates than the cold run (tests/test_rho_recipes.py), both as the oracle's"""
    ls, st, cold, stable, _ = _recipe(rid)
    x0, y0, sw = problems.warm_point(ls, st)
    ref = problems.oracle_solve(ls, nthreads=8, x0=x0, y0=y0, **sw)
    assert ref["iters"].sum() < cold["iters"].sum()
    qp = _handle(monkeypatch, rid, ls, sw, 0)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.warm_start(x0, y0); qp.solve(); got = qp.get()
    _same_as_oracle(got, ref, problems.oracle_stable_mask(ls, x0=x0, y0=y0, **sw), "%s warm" % rid)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.warm_start(np.zeros((ls.batch, ls.n)), np.zeros((ls.batch, ls.m))); qp.solve(); got = qp.get(); qp.close()
    _same_as_oracle(got, cold, stable, "%s cold on the warm-start handle" % rid)


@pytest.mark.parametrize("rid", ["q20", "q50"])
def test_kept_workspace_after_in_place_refactorisations(built, monkeypatch, rid):
    """(c) mpcqp_keep_workspace, solve, mpcqp_update_vectors, solve: the kept factor is the one of the last rho, which the in-place path produced; against the
    oracle's kept workspaces, as tests/test_gpu_parity.py test_kept_workspace_vectors_vs_oracle runs them"""
    from oracle import oracle as orc
    mdl, ls, meta, st = problems.rho_recipe(rid)
    _, _, _, stable, _ = _recipe(rid)
    B = ls.batch
    state = orc.State(orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai), B, orc.default_settings(**st))
    qp = _handle(monkeypatch, rid, ls, st, 0)
    qp.keep_workspace(True)
    _same_as_oracle(_solve(qp, ls), state.solve(ls.P, ls.q, ls.A, ls.l, ls.u, nthreads=8), stable, "%s kept workspace, full solve" % rid)
    rng = np.random.default_rng(11)
    frame0 = meta["frame0"].copy(); frame0[:, :mdl.nx] += rng.normal(0, 0.05, (B, mdl.nx))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    ls2 = mdl.local_system(meta["p"] + 0.1, meta["x_iterate"], lbx, ubx, lbg, ubg)       # same iterate -> same A, P; new q, l, u
    assert np.array_equal(ls2.A, ls.A)
    ref2 = state.solve_vectors(ls2.q, ls2.l, ls2.u, nthreads=8)
    qp.update_vectors(ls2.q, ls2.l, ls2.u); qp.solve(); got2 = qp.get(); qp.close()
    # (every instance is held to equal iteration counts: the mask of the first solve says nothing about this one)
    _same_as_oracle(got2, ref2, np.ones(B, bool), "%s kept workspace, vectors only" % rid)


@pytest.mark.parametrize("rid", ["q50", "cp100"])
def test_queue_of_more_instances_than_resident_workgroups(built, monkeypatch, rid):
    """(d) the eight-wave instances as resident workgroups drawing tickets, with more instances than workgroups, over the launches of a rho update
    (one ticket counter per launch): every instance solved once, the bits of the same instances solved in batches of 12, a sample against the oracle"""
    B = problems.BIG_BATCH
    _, ls, _, st = problems.rho_recipe(rid, B)
    sub, idx, _ = problems.big_batch_sample(rid)
    ref = problems.oracle_solve(sub, nthreads=8, **st)
    stable = problems.oracle_stable_mask(sub, **st)
    runs = {}
    for rounds in (0, 1):
        qp = _handle(monkeypatch, rid, ls, st, rounds)
        runs[rounds] = _solve(qp, ls); qp.close()
        assert (runs[rounds]["status"] == 1).all(), np.unique(runs[rounds]["status"])
        _same_as_oracle({k: v[idx] for k, v in runs[rounds].items()}, ref, stable, "%s batch %d rounds=%d, sample of %d" % (rid, B, rounds, len(idx)))
    _bitwise(runs[1], runs[0], "%s batch %d rounds 1 against 0" % (rid, B))
    qp = _handle(monkeypatch, rid, ls, st, 0, batch=12)
    for lo in list(range(0, B - 12, 12)) + [B - 12]:
        part = _solve(qp, problems.take(ls, np.arange(lo, lo + 12)))
        _bitwise({k: v[lo:lo + 12] for k, v in runs[0].items()}, part, "%s instances %d.. in a batch of 12" % (rid, lo))
    qp.close()


def test_pipelined_host_step_through_the_hand_over(built, monkeypatch):
    """(e) mpcqp_solve_host (pipelined slices, each with its own launches) on q20, MPCQP_RESUME_ROUNDS = 0: the bits of mpcqp_solve"""
    ls, st, ref, stable, _ = _recipe("q20")
    qp = _handle(monkeypatch, "q20", ls, st, 0)
    got = _solve(qp, ls)
    _same_as_oracle(got, ref, stable, "q20 before the host step")
    for chunks in (0, 1, 5):
        host = qp.solve_host(ls.P, ls.q, ls.A, ls.l, ls.u, chunks=chunks)
        _bitwise(host, got, "q20 host step, chunks=%d" % chunks, keys=("x", "y", "status", "iters"))
        _bitwise(qp.get(), got, "q20 after the host step, chunks=%d" % chunks)
    qp.close()


def test_graph_replay_through_the_hand_over(built, monkeypatch):
    """(e) the q50 solve at MPCQP_RESUME_ROUNDS = 0 captured in a HIP graph (its launches and the memset of their ticket counters) and replayed twice:
    the bits of the eager solve"""
    import torch
    ls, st, ref, stable, _ = _recipe("q50")
    qp = _handle(monkeypatch, "q50", ls, st, 0)
    got = _solve(qp, ls)
    _same_as_oracle(got, ref, stable, "q50 before the capture")
    s = torch.cuda.Stream(); g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        qp.solve(stream=s.cuda_stream); s.synchronize()
        with torch.cuda.graph(g, stream=s):
            qp.solve(stream=s.cuda_stream)
        for replay in (1, 2):
            g.replay(); s.synchronize()
            _bitwise(qp.get(), got, "q50 graph replay %d" % replay)
    qp.close()
