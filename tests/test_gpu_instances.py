"""GPU: every compiled instance of the QP kernels against the oracle.

A kernel family is several separately compiled instances -- mpcqp_res_kernel at a 128-, 168- or 256-VGPR budget with the factor in LDS or streamed from the slab, with
z and y in LDS or in the slab, each with its kept-workspace twin; mpcqp_admm_kernel with 4 or 8 blocks in flight; the set-up, iteration and in-place re-factorisation
kernels of the two-kernel on-chip form in four- and eight-wave shapes, with and without hub blocks -- and which one a handle launches follows from the pattern's LDS
footprint (csrc/select.hpp kernel_id_of).  The other GPU modules sit at five problem sizes and reach some of them.  tests/support/instance_cases.py sweeps the selection
on the CPU and keeps INSTANCE_CASES, a row for every reachable instance at the smallest problem that launches it and, where the rule itself picks the instance at a
batch of 64 ... 16384, a row at the rule's own selection (tests/test_instance_census_host.py holds the table to the sweep).  This module runs the rows.

Every test creates its handle under the row's environment and first asserts that plan_info() and oc_info() are the CPU selection of the row: the library runs the same
select_kernel and the same kernel_id_of, so equal numbers (family code, LDS bytes, ordering, chain shape) under the same environment mean the instance the test is
named for.  What this cannot tell apart is two register budgets of one family on one pattern -- plan_info() does not carry minw: the register-budget test relies on
the handle reading the knob at create (Knobs::from_env), as every other knob test of the suite does.

Second tier (ic.SETUP_BRANCH_CASES): the run-time branches of the set-up kernel's shape that none of those rows takes -- which values are staged in LDS, whether the
16-bit index tables exist and whether each sits in the factorisation's scratch or in the z region -- each at the smallest problem whose default handle takes it, through
legs 1 and 4.  These handles are created with MPCQP_VERBOSE set, and the first assertion also holds the line the library prints about its set-up shape to the CPU selection's.

Data: the row's workload at 8 instances (4 for the quadrotor from N = 100), instance 1 dual infeasible and instance 2 primal infeasible (problems.hard_stage_batch).
Legs, each against the oracle at the module-wide bar of tests/test_gpu_parity.py -- equal status and NaN pattern on every instance, equal iteration counts on the
instances whose decisions do not hang on rounding (problems.oracle_stable_mask), x, y, z, obj, prim_res, dual_res to RTOL relative to 1 + |ref|_inf, the final rho to
RHO_DECISIONS of tests/test_gpu_rho_resume.py; no tolerance of this module's own:
  1. default settings (statuses 1, 3, 5);
  2. the rho recipe of the row: repeated rho updates, i.e. the in-kernel re-factorisation of the instance (two-kernel form: the <RF=1> kernel);
  3. an iteration limit one short of the first termination check (status 7 and the code behind the loop);
  4. the kept workspace where the family has one (not the streaming kernels): a full solve, then update_vectors with another q and shifted bounds -- the _r1 twin of
     the instance, the set-up kernel's reuse instance in the two-kernel form;
  5. bitwise, without the oracle: a second solve on the same handle equals the first, the batch reversed gives the reversed result, and the register-budget relation below.
A reduced row (mpcqp_create_reduced with the parameter rows fixed) is compared on the reduced QP's variables and rows (problems.reduce_qp); prim_res, dual_res and rho
are the inner handle's, which the postsolve kernel passes through (csrc/reduced.hpp), and obj is the caller's objective: the reduced QP's plus the constant of the
eliminated variables, q_f'x_f + 1/2 x_f'P_ff x_f, which the oracle's side adds in NumPy (instance_cases._callers_info).

Register budgets (ic.KNOB_PAIRS).  MPCQP_NO_RES1X, MPCQP_NO_RES3, MPCQP_GB_OCC2 and MPCQP_GB_OCC3 move a pattern between instances of ONE source text that differ in
__launch_bounds__'s second argument and, for the 168-VGPR global-block instance, in the number of factor blocks in flight (a ring of loads consumed in program order:
kernel_resident.hpp seg_each_g).  Neither changes the order of any sum, so x, y, z, iters, status and the info block are expected to be equal bit for bit between the
two instances, and that is asserted -- it would catch a spill that corrupts a value and a budget-dependent difference in the compiler's contraction alike.

Measured on one MI355X (DESIGN.md section 6.24 has the table per instance): all 160 tests pass in 10 s; over every instance and leg x, y, z are at most 3.9e-10 from
the oracle in units of the bar's scale (bar 1e-6), obj / prim_res / dual_res at most 9.8e-9 per instance, the final rho at most 5.9e-4 relative (bar 1e-2), iteration
counts were compared on all but one instance, and the six register-budget pairs agree bit for bit.  Nothing was found to fix.
"""
import functools
import os

import numpy as np
import pytest

from tests.support import instance_cases as ic
from tests.support import problems
from tests.test_gpu_parity import RTOL, _close      # noqa: F401 (RTOL: the bar _close applies)
from tests.test_gpu_rho_resume import BITS, RHO_DECISIONS, _bitwise

pytestmark = pytest.mark.gpu

CERTIFICATES = (3, 4, 5, 6)
ROW_IDS = [ic.row_id(r) for _, r in ic.ROWS]
KEPT_ROWS = [(k, r) for k, r in ic.ROWS if k.kind != "stream"]          # (the streaming kernels keep no workspace: mpcqp_keep_workspace answers ERR_LIMIT)
_FIGURES = {}       # KernelId of the rows' plain solve -> rows, largest differences to the oracle, instances compared, statuses


def _key(r):
    return (r.workload, r.N, r.form)


def _handle(monkeypatch, r, st, knob=None, capfd=None):
    """a handle for the row's pattern under the row's environment, checked to be the CPU selection of the row (capfd: and to say so itself, under MPCQP_VERBOSE)"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    for name in [n for n in os.environ if n.startswith("MPCQP_")]:
        monkeypatch.delenv(name)
    for name, v in dict(r.env, **({knob: "1"} if knob else {})).items():
        monkeypatch.setenv(name, v)
    d = ic.row_data(*_key(r))
    ls = d.ls
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, fixed_rows=d.fixed_rows, **st)
    sel = ic.row_selection(r, knob)
    info, oc = qp.plan_info(), qp.oc_info()
    assert {k: info[k] for k in ic.PLAN_KEYS} == sel.plan, (ic.row_id(r), knob, info, sel.plan)
    assert oc == sel.oc, (ic.row_id(r), knob, oc, sel.oc)
    if capfd is not None:      # (the line ends with what only the device knows: ", <n> resident workgroups")
        said = [ln.rsplit(",", 1)[0] for ln in capfd.readouterr().err.splitlines() if ln.startswith("mpcqp: set-up kernel shape")]
        assert sel.shape and said == [sel.shape], (ic.row_id(r), said, sel.shape)
    return qp


def _solve(qp, ls, order=None):
    pick = (lambda a: a) if order is None else (lambda a: a if a.ndim == 1 else np.ascontiguousarray(a[order]))
    qp.update(pick(ls.P), pick(ls.q), pick(ls.A), pick(ls.l), pick(ls.u)); qp.solve()
    return qp.get()


def _inner(r, got):
    """the handle's result on the variables and rows of the QP the oracle solves"""
    d = ic.row_data(*_key(r))
    return got if d.free is None else dict(got, x=got["x"][:, d.free], y=got["y"][:, d.kept], z=got["z"][:, d.kept])


def _same_as_oracle(k, r, got, ref, stable, tag):
    """the bar of the module docstring"""
    got = _inner(r, got)
    print("%s: status %s iters %s (oracle %s %s)" % (tag, got["status"].tolist(), got["iters"].tolist(), ref["status"].tolist(), ref["iters"].tolist()))
    assert (got["status"] == ref["status"]).all(), (tag, got["status"], ref["status"])
    for key in ("x", "y", "z"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), (tag, "NaN pattern of %s" % key)
    assert (got["iters"][stable] == ref["iters"][stable]).all(), (tag, got["iters"], ref["iters"])
    same = got["iters"] == ref["iters"]           # (an instance that stops a check apart is a tolerance apart: its iterates are not compared)
    assert same.sum() >= 0.75 * len(same), (tag, np.flatnonzero(~same))        # (the cap tests/test_instance_census_host.py puts on the unstable ones)
    keys = ("x", "y", "z", "obj", "prim_res", "dual_res")
    g, o = ({key: res[key][same] for key in keys + ("rho", "status")} for res in (got, ref))
    fig = {key: float(np.abs(g[key] - o[key])[np.isfinite(o[key])].max(initial=0.0) / (1.0 + np.abs(o[key][np.isfinite(o[key])]).max(initial=0.0))) for key in ("x", "y", "z")}
    fig["rho"] = float(np.abs(g["rho"] / o["rho"] - 1.0).max())
    point = ~np.isin(o["status"], CERTIFICATES)
    fig["info"] = max(float((np.abs(g[key] - o[key]) / (1.0 + np.abs(o[key])))[point if key == "obj" else np.isfinite(o[key])].max(initial=0.0)) for key in ("obj", "prim_res", "dual_res"))
    print("%s: difference to the oracle over 1 + |ref|_inf: %s, rho alone, relative: %.2e; iterations compared for %d of %d instances, iterates for %d" % (
        tag, " ".join("%s %.2e" % (key, fig[key]) for key in ("x", "y", "z")), fig["rho"], stable.sum(), len(stable), same.sum()))
    acc = _FIGURES.setdefault(k, dict(rows=set(), x=0.0, y=0.0, z=0.0, rho=0.0, info=0.0, compared=0, total=0, gpu=set(), oracle=set()))
    acc["rows"].add(ic.row_id(r))
    for key in ("x", "y", "z", "rho", "info"):
        acc[key] = max(acc[key], fig[key])
    acc["compared"] += int(stable.sum()); acc["total"] += len(stable); acc["gpu"] |= set(got["status"].tolist()); acc["oracle"] |= set(ref["status"].tolist())
    for key in ("x", "y", "z"):
        _close(g, o, key)
    cert = np.isin(o["status"], CERTIFICATES)
    assert np.array_equal(g["obj"][cert], o["obj"][cert]) and (np.abs(o["obj"][cert]) == 1e30).all(), (tag, g["obj"], o["obj"])          # +-Q_INFTY
    for b in range(len(cert)):
        for key in ("obj", "prim_res", "dual_res"):
            if key != "obj" or not cert[b]:
                _close({key: g[key][b:b + 1]}, {key: o[key][b:b + 1]}, key)
    assert (np.abs(g["rho"] / o["rho"] - 1.0) <= RHO_DECISIONS).all(), (tag, g["rho"], o["rho"])


@functools.lru_cache(maxsize=None)
def _oracle(key, leg):
    """the oracle's result and stable mask of a row's batch under a leg: computed once per (workload, N, form), shared by the rows on it, never changed"""
    return ic.oracle_leg(*key, leg)


@functools.lru_cache(maxsize=None)
def _kept_oracle(key):
    return ic.oracle_kept(*key)


def _leg(monkeypatch, k, r, leg):
    ref, stable = _oracle(_key(r), leg)
    qp = _handle(monkeypatch, r, ic.leg_settings(*_key(r), leg))
    got = _solve(qp, ic.row_data(*_key(r)).ls); qp.close()
    _same_as_oracle(k, r, got, ref, stable, "%s %s" % (ic.row_id(r), leg))
    return got


@pytest.mark.parametrize("k,r", ic.ROWS, ids=ROW_IDS)
def test_default_settings(built, monkeypatch, k, r):
    """leg 1: a solved, a dual infeasible and a primal infeasible instance on every compiled instance"""
    got = _leg(monkeypatch, k, r, "default")
    assert got["status"][0] == 1 and got["status"][problems.DUAL_INFEASIBLE] == 5 and got["status"][problems.PRIMAL_INFEASIBLE] == 3


@pytest.mark.parametrize("k,r", ic.ROWS, ids=ROW_IDS)
def test_repeated_rho_updates(built, monkeypatch, k, r):
    """leg 2: the row's rho recipe -- at least one instance changes rho twice or more (held on the oracle by the CPU module), so the instance's in-kernel
    re-factorisation runs, and in the two-kernel form the last launch's <RF=1> kernel re-factorises in place"""
    _leg(monkeypatch, k, r, "rho")


@pytest.mark.parametrize("k,r", ic.ROWS, ids=ROW_IDS)
def test_iteration_limit_off_a_check(built, monkeypatch, k, r):
    """leg 3: max_iter = 24, not on a termination check: the code behind the loop makes the run's only check"""
    got = _leg(monkeypatch, k, r, "tail")
    assert (got["status"] == 7).any() and (got["iters"] == 24).all()


@pytest.mark.parametrize("k,r", KEPT_ROWS, ids=[ic.row_id(r) for _, r in KEPT_ROWS])
def test_kept_workspace(built, monkeypatch, k, r):
    """leg 4: keep_workspace, a full solve, update_vectors with problems.kept_q and shifted bounds, a vectors-only solve: the _r1 twin of the instance against the
    oracle's kept workspace"""
    key = _key(r)
    (ref1, ref2), (ok1, ok2) = _kept_oracle(key)
    q2, l2, u2 = ic.kept_vectors(*key)
    qp = _handle(monkeypatch, r, {})
    qp.keep_workspace(True)
    _same_as_oracle(k, r, _solve(qp, ic.row_data(*key).ls), ref1, ok1, "%s kept workspace, full solve" % ic.row_id(r))
    qp.update_vectors(q2, l2, u2); qp.solve(); got2 = qp.get(); qp.close()
    _same_as_oracle(k._replace(reuse=1), r, got2, ref2, ok2, "%s kept workspace, vectors only" % ic.row_id(r))


@pytest.mark.parametrize("k,r", ic.ROWS, ids=ROW_IDS)
def test_second_solve_and_reversed_batch(built, monkeypatch, k, r):
    """leg 5: on one handle, under the rho recipe (every kernel of the handle runs): the batch, the batch again, the batch reversed -- the second equals the first bit
    for bit, the third is the first reversed.  Nothing a solve reads is left over from the one before, and no result depends on the workgroup that computed it."""
    ls = ic.row_data(*_key(r)).ls
    qp = _handle(monkeypatch, r, ic.leg_settings(*_key(r), "rho"))
    first, second = _solve(qp, ls), _solve(qp, ls)
    rev = _solve(qp, ls, order=np.arange(ls.batch)[::-1]); qp.close()
    _bitwise(second, first, "%s: second solve on the same handle" % ic.row_id(r))
    _bitwise({key: v[::-1] for key, v in rev.items()}, first, "%s: reversed batch" % ic.row_id(r))


@pytest.mark.parametrize("r,knob,k2", ic.KNOB_PAIRS, ids=["%s+%s" % (ic.row_id(r), knob.replace("MPCQP_", "")) for r, knob, _ in ic.KNOB_PAIRS])
def test_register_budgets_of_one_source_agree(built, monkeypatch, r, knob, k2):
    """leg 5, the register-budget relation of the module docstring: the row's pattern on the instance the knob moves it to -- held to the oracle like the row itself --
    gives the bits of the row's own instance, under the default settings and under the rho recipe"""
    ls = ic.row_data(*_key(r)).ls
    for leg in ("default", "rho"):
        st = ic.leg_settings(*_key(r), leg)
        ref, stable = _oracle(_key(r), leg)
        qa = _handle(monkeypatch, r, st); a = _solve(qa, ls); qa.close()
        qb = _handle(monkeypatch, r, st, knob); b = _solve(qb, ls); qb.close()
        _same_as_oracle(k2, r, b, ref, stable, "%s %s under %s" % (ic.row_id(r), leg, knob))
        _bitwise(b, a, "%s %s: %s against the row's own instance" % (ic.row_id(r), leg, knob), keys=BITS)


SETUP_IDS = [ic.row_id(r) for _, r in ic.SETUP_ROWS]


@pytest.mark.parametrize("branch,r", ic.SETUP_ROWS, ids=SETUP_IDS)
def test_set_up_branch_default_settings(built, monkeypatch, capfd, branch, r):
    """second tier, leg 1: the set-up kernel's branch of the row (checked on the CPU selection and on the library's own MPCQP_VERBOSE line) under the default settings"""
    assert ic.setup_branch(ic.row_selection(r)) == branch
    ref, stable = _oracle(_key(r), "default")
    capfd.readouterr()
    qp = _handle(monkeypatch, r, {}, capfd=capfd)
    got = _solve(qp, ic.row_data(*_key(r)).ls); qp.close()
    _same_as_oracle(ic.primary(ic.row_selection(r)), r, got, ref, stable, "%s set-up branch %s default" % (ic.row_id(r), branch))
    assert got["status"][0] == 1 and got["status"][problems.DUAL_INFEASIBLE] == 5 and got["status"][problems.PRIMAL_INFEASIBLE] == 3


@pytest.mark.parametrize("branch,r", ic.SETUP_ROWS, ids=SETUP_IDS)
def test_set_up_branch_kept_workspace(built, monkeypatch, capfd, branch, r):
    """second tier, leg 4: the same branch, then the set-up kernel's reuse instance on the kept workspace"""
    key, k = _key(r), ic.primary(ic.row_selection(r))
    assert ic.setup_branch(ic.row_selection(r)) == branch
    (ref1, ref2), (ok1, ok2) = _kept_oracle(key)
    q2, l2, u2 = ic.kept_vectors(*key)
    capfd.readouterr()
    qp = _handle(monkeypatch, r, {}, capfd=capfd)
    qp.keep_workspace(True)
    _same_as_oracle(k, r, _solve(qp, ic.row_data(*key).ls), ref1, ok1, "%s set-up branch %s kept workspace, full solve" % (ic.row_id(r), branch))
    qp.update_vectors(q2, l2, u2); qp.solve(); got2 = qp.get(); qp.close()
    _same_as_oracle(k._replace(reuse=1), r, got2, ref2, ok2, "%s set-up branch %s kept workspace, vectors only" % (ic.row_id(r), branch))


def test_zz_figures_per_instance(built):
    """prints (run with -s) one line per compiled instance: the rows that ran it, the largest differences to the oracle, the instances compared for iterations, the statuses"""
    for k, acc in _FIGURES.items():
        print("%s | rows %s | x %.2e y %.2e z %.2e obj / prim_res / dual_res (per instance, over 1 + |ref|) %.2e rho (relative) %.2e | iterations compared for %d of %d instances | statuses: GPU %s oracle %s" % (
            "%s nw=%d minw=%d zyg=%d ng=%d nh=%d pd=%d reuse=%d" % (k.kind, k.nw, k.minw, k.zyg, k.ng, k.nh, k.pd, k.reuse), ", ".join(sorted(acc["rows"])),
            acc["x"], acc["y"], acc["z"], acc["info"], acc["rho"], acc["compared"], acc["total"], sorted(acc["gpu"]), sorted(acc["oracle"])))
        assert acc["gpu"] == acc["oracle"]
