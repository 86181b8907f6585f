"""GPU: every solver setting and every exit status on every kernel family.

mpcqp_settings has fifteen numeric fields and the library several copies of the ADMM loop (kernel_stream.hpp; kernel_resident.hpp, which also hosts the
global-block and the single-kernel on-chip instances; kernel_oc_split.hpp with its <RF=0> / <RF=1> / tile / two-pair instantiations), each with its own
relaxation step, termination bookkeeping and code behind the loop.  This module runs problems.SETTINGS_MATRIX -- alpha, sigma, rho, check_termination,
eps_prim_inf / eps_dual_inf, scaling 0 / 3 / 25, scaled_termination, adaptive_rho = 0 and iteration limits that end a run off a termination check -- on
problems.hard_stage_batch: the MPC workloads with one instance made dual infeasible and one primal infeasible, which every family takes, the on-chip ones
included.  tests/test_settings_recipes.py holds the oracle's outcomes on these inputs to what is relied on here.

Bar against the oracle per solve: the module-wide one of tests/test_gpu_parity.py (RTOL relative to 1 + |ref|_inf for x, y, z; obj, prim_res, dual_res per
instance to the same bar, +-Q_INFTY of a certificate equal), equal status and NaN pattern on every instance, equal iteration counts on the instances whose
decisions do not hang on rounding (problems.oracle_stable_mask), the final rho to RHO_DECISIONS of tests/test_gpu_rho_resume.py.  Relations that need no
oracle are bitwise: (a) a used handle against a fresh one, (b) the two-kernel against the single-kernel on-chip form and MPCQP_RESUME_ROUNDS 0 against 1,
(c) a setting given at its default value against the default run.

What the module is aimed at (found by reading, fixed in the same change).  Every copy of the loop stored the iteration's steps dx, dy -- what the certificates of
infeasibility are computed from -- in the slab only in an iteration with a termination check or a rho update, while the code behind the loop, which runs OSQP's
last check when the iteration limit does not fall on a check iteration (oracle/osqp_oracle.c solve_one, behind its loop), read them from the slab: the steps of the
last check iteration, or, when nothing had been stored yet -- max_iter < check_termination, or check_termination = 0 below the rho interval --, the zeros the slab
is created with.  With zeros no certificate is ever found: on the quadrotor N=20 at max_iter=24 and at check_termination=0, max_iter=40 (problems.NEVER_SAVED) the
oracle's [1 5 3 1 1 1 1 1] can only come back with 2 or 7 in the places of 5 and 3; with stale steps the cart-pole's primal_infeasible_inaccurate (4) at max_iter
37 / 60 hangs on iteration 25's or 50's steps.  The fix makes the last iteration one that stores (save = can_check || do_rho || iter == max_iter) in the three copies of the
loop.  A launch of the two-kernel form that resumes with iterations left ends in the same loop; one parked on the limit itself stored its steps in the iteration of the
rho update that parked it, and the set-up kernel's resume mode, which runs in between, writes the factor, its temp tiles and the status word only (nothing but the Ruiz
passes of a pattern with m < n ever uses the dx region as scratch, and those run before the loop).  Runs that end on a check iteration store what they stored before.
Relation (a) is not expected to tell the two builds apart, and the reading that it would was wrong: the settings belong to the handle, so a handle whose runs never store
never holds another solve's steps either -- its slab stays zero -- and one whose runs do store overwrites them in every solve before the tail reads them.  It guards
the property all the same: nothing a solve reads may be left over from the one before.

NOT YET MEASURED.  This module, the fix and the whole GPU suite with them have not been run on an MI355X: no GPU could be had while they were written.  The test code
was rehearsed on the CPU with the oracle standing in for the library (every test passes in that rehearsal, which says nothing about the kernels).  Still to be recorded
here from the first GPU run, which test_zz_figures_of_the_matrix prints with -s: per workload the largest difference to the oracle in x, y, z and rho over the matrix, the
number of instances compared for iterations out of the total, the statuses that occurred (the oracle's side: 1, 2, 3, 4, 5, 7; 6 -- dual infeasible, inaccurate -- does not
occur on these inputs and is not constructed, it would be asserted like every other status); which tests fail against the kernels of the commit before, with which
statuses; the wall time of this module (766 tests) and of the whole `-m gpu` run next to the commit before.
"""
import functools
from collections import OrderedDict

import numpy as np
import pytest

from tests.support import problems
from tests.test_gpu_parity import RTOL, _close      # noqa: F401 (RTOL: the bar _close applies)
from tests.test_gpu_rho_resume import BITS, KNOBS, RHO_DECISIONS, _bitwise

pytestmark = pytest.mark.gpu

ALL_KNOBS = KNOBS + ("MPCQP_VTILES", "MPCQP_TILES")
CERTIFICATES = (3, 4, 5, 6)
SETTINGS = list(problems.SETTINGS_MATRIX)

# leg -> (environment, plan_info()["variant"], single-kernel form)
LEGS = OrderedDict([
    ("stream", (dict(MPCQP_VARIANT="stream"), 0, False)), ("res1", (dict(MPCQP_VARIANT="res1"), 1, False)), ("res2", (dict(MPCQP_VARIANT="res2"), 2, False)),
    ("res4", (dict(MPCQP_VARIANT="res4"), 4, False)), ("res8", (dict(MPCQP_VARIANT="res8"), 8, False)),
    ("gres4", (dict(MPCQP_VARIANT="gres4"), 104, False)), ("gres2", (dict(MPCQP_VARIANT="gres2"), 102, False)),
    ("oc4", (dict(MPCQP_VARIANT="oc4"), 204, False)), ("oc4-one-pair", (dict(MPCQP_VARIANT="oc4", MPCQP_NO_DISSECT="1"), 204, False)),
    ("oc8", (dict(MPCQP_VARIANT="oc8"), 208, False)), ("oc8-one-pair", (dict(MPCQP_VARIANT="oc8", MPCQP_NO_DISSECT="1"), 208, False)),
    ("oc4-mono", (dict(MPCQP_VARIANT="oc4", MPCQP_OC_MONO="1"), 204, True)), ("oc8-mono", (dict(MPCQP_VARIANT="oc8", MPCQP_OC_MONO="1"), 208, True)),
    ("oc8-mono-one-pair", (dict(MPCQP_VARIANT="oc8", MPCQP_OC_MONO="1", MPCQP_NO_DISSECT="1"), 208, True)),
    ("vtiles", (dict(MPCQP_VARIANT="oc4", MPCQP_VTILES="1"), 204, False)),
])
# (leg, workload, twisted pairs of chains of the on-chip plan -- None: not an on-chip family).  The LDS-resident families and the four-wave on-chip instances
# refuse the two long horizons (ERR_LIMIT): those rows are not in the table.
ROWS = [(leg, wid, None) for leg in ("stream", "res1", "res2", "res4", "res8", "gres4", "gres2") for wid in ("q20", "cp30")] + [
    ("gres4", "q50", None), ("gres2", "q50", None), ("gres4", "cp100", None),
    ("oc4", "q20", 1), ("oc4", "cp30", 2), ("oc4-one-pair", "cp30", 1),
    ("oc8", "q50", 1), ("oc8", "cp100", 4), ("oc8-one-pair", "cp100", 1),
    ("oc4-mono", "q20", 1), ("oc8-mono", "q50", 1)]
PAIRS = {(leg, wid): pairs for leg, wid, pairs in ROWS}
PAIRS.update({("oc4-mono", "cp30"): 1, ("oc8-mono", "cp100"): 4, ("oc8-mono-one-pair", "cp100"): 1, ("vtiles", "q20"): 1})      # (the partners of relation (b); the tile sweeps)
MATRIX = [(leg, wid, sid) for leg, wid, _ in ROWS for sid in SETTINGS]
VTILES = [("vtiles", "q20", sid) for sid in problems.TAIL_CASES + ("alpha=1.0",)]
# relation (b): the two-kernel form and the single-kernel form it has to equal bit for bit.  The four-wave single kernel has no instance for the order with two
# chain pairs: it is compared with the two-kernel form in the one-pair order.
TWO_AND_ONE = [("oc4", "oc4-mono", "q20"), ("oc4-one-pair", "oc4-mono", "cp30"), ("oc8", "oc8-mono", "q50"), ("oc8", "oc8-mono", "cp100"),
               ("oc8-one-pair", "oc8-mono-one-pair", "cp100")]
ROUNDS = [("oc4", "q20"), ("oc4", "cp30"), ("oc8", "q50"), ("oc8", "cp100")]

_GOT = {}           # (leg, workload, setting) -> a fresh handle's single solve: computed once, never changed
_FIGURES = {}       # workload -> the largest differences to the oracle met so far; instances compared; statuses seen


@functools.lru_cache(maxsize=None)
def _batch(wid, dual=True):
    return problems.hard_stage_batch(wid, dual)


@functools.lru_cache(maxsize=None)
def _oracle(wid, sid):
    """-> (oracle result, stable mask) of one workload under one entry of the matrix"""
    _, ls, _ = _batch(wid)
    st = problems.SETTINGS_MATRIX[sid]
    return problems.oracle_solve(ls, nthreads=8, **st), problems.oracle_stable_mask(ls, nthreads=8, **st)


@functools.lru_cache(maxsize=None)
def _kept_oracle(wid, sid):
    """-> (the second solve's q, the oracle's kept workspaces' two solves, their stable masks)"""
    _, ls, _ = _batch(wid)
    q2 = problems.kept_q(ls)
    st = problems.SETTINGS_MATRIX[sid]
    return q2, problems.oracle_kept_solves(ls, q2, **st), problems.oracle_kept_stable_mask(ls, q2, **st)


def _handle(monkeypatch, leg, wid, st, ls, rounds=None, **kw):
    """a handle of the leg for the workload's pattern, checked to be what the leg means"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    env, variant, mono = LEGS[leg]
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if rounds is not None:
        monkeypatch.setenv("MPCQP_RESUME_ROUNDS", str(rounds))
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **dict(st, **kw))
    if "fixed_rows" in kw:
        return qp
    info, oc = qp.plan_info(), qp.oc_info()
    assert info["variant"] == variant, (leg, wid, info)
    pairs = PAIRS[(leg, wid)]
    if pairs is None:
        assert oc["chain_pairs"] == 0 and oc["launch_pairs_for_rho_updates"] == 0, (leg, wid, oc)
    else:
        assert oc["chain_pairs"] == pairs and (info["ordering"] == 4) == (pairs > 1), (leg, wid, oc, info)
        assert oc["launch_pairs_for_rho_updates"] == (0 if mono else 1 + (1 if rounds is None else rounds)), (leg, wid, oc)
        assert info["tiles"] == (problems.HARD_WORKLOADS[wid][1] - 1 if leg == "vtiles" else 0), (leg, wid, info)
    return qp


def _solve(qp, ls, order=None):
    pick = (lambda a: a) if order is None else (lambda a: a if a.ndim == 1 else np.ascontiguousarray(a[order]))
    qp.update(pick(ls.P), pick(ls.q), pick(ls.A), pick(ls.l), pick(ls.u)); qp.solve()
    return qp.get()


def _fresh(monkeypatch, leg, wid, sid):
    """a fresh handle's single solve of the workload under the setting (kept for the relations that compare with it)"""
    key = (leg, wid, sid)
    if key not in _GOT:
        _, ls, _ = _batch(wid)
        qp = _handle(monkeypatch, leg, wid, problems.SETTINGS_MATRIX[sid], ls)
        got = _solve(qp, ls); qp.close()
        for v in got.values():
            v.setflags(write=False)
        _GOT[key] = got
    return _GOT[key]


def _same_as_oracle(got, ref, stable, tag, wid=None, keys=("x", "y", "z"), info=True):
    """the bar of the module docstring; -> the instances whose iterates were compared"""
    print("%s: status %s iters %s (oracle %s %s)" % (tag, got["status"].tolist(), got["iters"].tolist(), ref["status"].tolist(), ref["iters"].tolist()))
    assert (got["status"] == ref["status"]).all(), (tag, got["status"], ref["status"])
    for k in keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (tag, "NaN pattern of %s" % k)
    assert (got["iters"][stable] == ref["iters"][stable]).all(), (tag, got["iters"], ref["iters"])
    same = got["iters"] == ref["iters"]
    assert same.sum() >= 0.9 * len(same), (tag, np.flatnonzero(~same))           # (the cap tests/test_settings_recipes.py puts on the unstable ones)
    g, r = ({k: res[k][same] for k in keys + ("rho", "obj", "prim_res", "dual_res", "status")} for res in (got, ref))
    fig = {k: float(np.abs(g[k] - r[k])[np.isfinite(r[k])].max(initial=0.0) / (1.0 + np.abs(r[k][np.isfinite(r[k])]).max(initial=0.0))) for k in keys}
    fig["rho"] = float(np.abs(g["rho"] / r["rho"] - 1.0).max())
    print("%s: difference to the oracle over 1 + |ref|_inf: %s, rho alone, relative: %.2e; iterations compared for %d of %d instances, iterates for %d" % (
        tag, " ".join("%s %.2e" % (k, fig[k]) for k in keys), fig["rho"], stable.sum(), len(stable), same.sum()))
    if wid is not None:
        acc = _FIGURES.setdefault(wid, dict(x=0.0, y=0.0, z=0.0, rho=0.0, compared=0, total=0, gpu=set(), oracle=set()))
        for k in keys + ("rho",):
            acc[k] = max(acc[k], fig[k])
        acc["compared"] += int(stable.sum()); acc["total"] += len(stable); acc["gpu"] |= set(got["status"].tolist()); acc["oracle"] |= set(ref["status"].tolist())
    for k in keys:
        _close(g, r, k)
    if info:
        cert = np.isin(r["status"], CERTIFICATES)
        assert np.array_equal(g["obj"][cert], r["obj"][cert]) and (np.abs(r["obj"][cert]) == 1e30).all(), (tag, g["obj"], r["obj"])          # +-Q_INFTY
        for b in range(len(cert)):
            for k in ("obj", "prim_res", "dual_res"):
                if k != "obj" or not cert[b]:
                    _close({k: g[k][b:b + 1]}, {k: r[k][b:b + 1]}, k)
    assert (np.abs(g["rho"] / r["rho"] - 1.0) <= RHO_DECISIONS).all(), (tag, g["rho"], r["rho"])
    return same


# ---------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("leg,wid,sid", MATRIX + VTILES)
def test_settings_matrix_vs_oracle(built, monkeypatch, leg, wid, sid):
    """every leg x workload x setting against the oracle.  vtiles: the two sweeps of the two-kernel form on dense tiles (MPCQP_VTILES=1) -- another text of the
    sweeps in front of the same bookkeeping -- on the cases that end behind the loop and on alpha = 1"""
    ref, stable = _oracle(wid, sid)
    _same_as_oracle(_fresh(monkeypatch, leg, wid, sid), ref, stable, "%s %s %s" % (leg, wid, sid), wid=wid)


def test_the_cart_pole_certificate_depends_on_the_scaling(built, monkeypatch):
    """OSQP's behaviour, reproduced and not "fixed": the cart-pole's dual-infeasible instance is `solved` under the default scaling and `dual infeasible` without
    scaling or with the scaled termination test (on the default family of the size, four waves on chip, two pairs)"""
    b = problems.DUAL_INFEASIBLE
    assert _fresh(monkeypatch, "oc4", "cp30", "default")["status"][b] == 1
    assert _fresh(monkeypatch, "oc4", "cp30", "scaling=0")["status"][b] == 5 and _fresh(monkeypatch, "oc4", "cp30", "scaled_termination=1")["status"][b] == 5


# ---------------------------------------------------------------------------------------------- relations that need no oracle
@pytest.mark.parametrize("leg,wid,sid", [(leg, wid, sid) for leg, wid, _ in ROWS for sid in problems.TAIL_CASES] + [r for r in VTILES if r[2] in problems.TAIL_CASES])
def test_used_handle_equals_fresh_handle(built, monkeypatch, leg, wid, sid):
    """(a) a handle that has solved the batch with its instances in reverse order -- so that the slab of instance b holds what instance B - 1 - b left, the steps of
    the certificate instances among it -- then solves the batch in order: the bits of a fresh handle's single solve.  A run that ends behind the loop must not
    read anything an earlier solve left."""
    _, ls, _ = _batch(wid)
    fresh = _fresh(monkeypatch, leg, wid, sid)
    qp = _handle(monkeypatch, leg, wid, problems.SETTINGS_MATRIX[sid], ls)
    rev = _solve(qp, ls, order=np.arange(ls.batch)[::-1])
    used = _solve(qp, ls); qp.close()
    _bitwise({k: v[::-1] for k, v in rev.items()}, fresh, "%s %s %s: reversed batch on a fresh handle" % (leg, wid, sid))
    _bitwise(used, fresh, "%s %s %s: used handle against fresh handle" % (leg, wid, sid))


@pytest.mark.parametrize("sid", SETTINGS)
@pytest.mark.parametrize("split,mono,wid", TWO_AND_ONE)
def test_two_kernels_equal_one(built, monkeypatch, split, mono, wid, sid):
    """(b) the two-kernel on-chip form against the single-kernel form of the same order, under every setting"""
    _bitwise(_fresh(monkeypatch, split, wid, sid), _fresh(monkeypatch, mono, wid, sid), "%s against %s, %s %s" % (split, mono, wid, sid))


@pytest.mark.parametrize("sid", SETTINGS)
@pytest.mark.parametrize("leg,wid", ROUNDS)
def test_resume_rounds_change_no_bit(built, monkeypatch, leg, wid, sid):
    """(b) MPCQP_RESUME_ROUNDS = 0 -- every rho update beyond the first is served in place by <RF=1> -- against the default 1"""
    _, ls, _ = _batch(wid)
    qp = _handle(monkeypatch, leg, wid, problems.SETTINGS_MATRIX[sid], ls, rounds=0)
    got = _solve(qp, ls); qp.close()
    _bitwise(got, _fresh(monkeypatch, leg, wid, sid), "%s %s %s: MPCQP_RESUME_ROUNDS 0 against 1" % (leg, wid, sid))


def test_settings_at_their_default_values_are_the_default_run(built, monkeypatch):
    """(c) every field of the matrix given explicitly at the value mpcqp_default_settings puts there: the default run, bit for bit (the Python -> struct plumbing)"""
    from optimal_control_problem_amd import _lib
    d = _lib.default_settings()
    named = sorted({k for st in problems.SETTINGS_MATRIX.values() for k in st})
    explicit = {k: getattr(d, k) for k in named}
    assert (explicit["alpha"], explicit["check_termination"], explicit["scaling"], explicit["max_iter"]) == (1.6, 25, 10, 10000)
    _, ls, _ = _batch("q20")
    qp = _handle(monkeypatch, "oc4", "q20", explicit, ls)
    got = _solve(qp, ls); qp.close()
    _bitwise(got, _fresh(monkeypatch, "oc4", "q20", "default"), "explicit defaults")


# ---------------------------------------------------------------------------------------------- smaller legs
@pytest.mark.parametrize("sid", problems.KEPT_CASES)
@pytest.mark.parametrize("leg,wid", [("res4", "q20"), ("oc4", "q20"), ("oc8", "q50")])
def test_kept_workspace_under_settings(built, monkeypatch, leg, wid, sid):
    """mpcqp_keep_workspace, solve, mpcqp_update_vectors with another q, solve: the kept path scales with parked D, E, c and has its own entry into the loop;
    against the oracle's kept workspaces"""
    _, ls, _ = _batch(wid)
    st = problems.SETTINGS_MATRIX[sid]
    q2, (ref1, ref2), (ok1, ok2) = _kept_oracle(wid, sid)
    qp = _handle(monkeypatch, leg, wid, st, ls)
    qp.keep_workspace(True)
    _same_as_oracle(_solve(qp, ls), ref1, ok1, "%s %s %s kept workspace, full solve" % (leg, wid, sid))
    qp.update_vectors(q2, ls.l, ls.u); qp.solve(); got2 = qp.get(); qp.close()
    _same_as_oracle(got2, ref2, ok2, "%s %s %s kept workspace, vectors only" % (leg, wid, sid))


@pytest.mark.parametrize("sid", problems.REDUCED_CASES)
def test_reduced_handle_under_settings(built, monkeypatch, sid):
    """mpcqp_create_reduced with the parameter rows fixed: the settings reach the inner handle -- against the oracle on the reduced QP (problems.reduce_qp).  The
    dual-infeasible recipe touches no fixed row; tests/test_settings_recipes.py holds the reduced oracle to both certificates."""
    mdl, ls, _ = _batch("q20")
    rows = list(range(mdl.np))
    st = problems.SETTINGS_MATRIX[sid]
    red, free, kept, fvars, xfix = problems.reduce_qp(ls, rows)
    ref = problems.oracle_solve(red, nthreads=8, **st)
    assert ref["status"][problems.PRIMAL_INFEASIBLE] == 3 and ref["status"][problems.DUAL_INFEASIBLE] == 5
    plain = problems.oracle_solve(red, nthreads=8)          # (a handle that ignored the settings would not pass: other iteration counts, or an x far beyond the bar)
    assert not np.array_equal(ref["iters"], plain["iters"]) or np.abs(plain["x"][0] - ref["x"][0]).max() > 1e3 * RTOL * (1.0 + np.abs(ref["x"][0]).max())
    qp = _handle(monkeypatch, "oc4", "q20", st, ls, fixed_rows=rows)
    info = qp.plan_info()
    assert (info["variant"], info["n"], info["m"]) == (204, red.n, red.m), info
    got = _solve(qp, ls); qp.close()
    inner = dict(got, x=got["x"][:, free], y=got["y"][:, kept], z=got["z"][:, kept])
    same = _same_as_oracle(inner, ref, problems.oracle_stable_mask(red, **st), "reduced q20 %s" % sid, info=False)
    ok = same & ~np.isin(ref["status"], CERTIFICATES)
    assert np.array_equal(got["x"][ok][:, fvars], xfix[ok]) and np.array_equal(got["z"][ok][:, rows], ls.l[ok][:, rows])


def test_polish_without_scaling(built):
    """the polish kernel's `unscale` switch off (scaling = 0: D = E = 1, c = 1 are never written as such): the double-integrator golden fixture at the bars of
    tests/test_gpu_polish.py against the dense reference polish"""
    from tests import test_gpu_polish as tp
    from tests.support import golden, polish_ref as pr
    fx = golden.load()["double_integrator"]; ls = fx["ls"]
    got, _ = tp._run(ls, polish=True, scaling=0)
    base, _ = tp._run(ls, scaling=0)
    ref = tp._reference(ls, base)
    tp._check_against_reference(ls, got, base, ref, "double_integrator, scaling=0")
    done = [b for b, r in ref.items() if r["status"] == pr.SUCCESS and max(r["pri"], r["dua"]) < 1e-9]
    assert len(done) >= 0.9 * ls.batch          # (so that this cannot pass with polishing silently failing)
    for b in done:
        ex, ey = np.abs(got["x"][b] - fx["x_star"][b]).max(), np.abs(got["y"][b] - fx["y_star"][b]).max()
        assert ex <= tp.X_TOL and ey <= tp.Y_TOL, (b, ex, ey)


def test_zz_figures_of_the_matrix(built):
    """prints what the module docstring records (run with -s): per workload the largest differences to the oracle, the instances compared, the statuses met"""
    for wid, acc in _FIGURES.items():
        print("%-6s x %.2e  y %.2e  z %.2e  rho (relative) %.2e   iterations compared for %d of %d instances; statuses: GPU %s oracle %s" % (
            wid, acc["x"], acc["y"], acc["z"], acc["rho"], acc["compared"], acc["total"], sorted(acc["gpu"]), sorted(acc["oracle"])))
        assert acc["gpu"] == acc["oracle"]
