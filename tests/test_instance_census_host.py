"""CPU: the census of the compiled QP kernel instances (tests/support/instance_cases.py) and the table of cases tests/test_gpu_instances.py runs.

select_kernel (csrc/select.hpp) is swept at 256 CUs over the three workloads x N = 3 ... 150 x {full, reduced form} x {the rule at 64 / 1024 / 8192 / 16384, every forced
family}, plain and under each occupancy knob, plus the random patterns of tests/test_gpu_fuzz.py; the kernels of every selection come from kernel_id_of, the mapping
mpcqp.hip launches through.  Held here: every reachable instance is a kernel of some row's handle, every row launches what it is filed under and is the smallest problem
that does, every instance the rule itself picks has a row at the rule's own selection, and deleting any row fails by name.  The oracle's outcomes on every row's data are
held to what the GPU module relies on (statuses, stable instances, rho updates).  Needs no GPU.
"""
import collections

import numpy as np
import pytest

from tests.support import instance_cases as ic
from tests.support import problems

DATA_KEYS = sorted({(r.workload, r.N, r.form) for _, r in ic.ROWS}, key=lambda k: (ic.WORKLOADS.index(k[0]), k[1], k[2]))
SETUP_KEYS = [(r.workload, r.N, r.form) for _, r in ic.SETUP_ROWS]


@pytest.fixture(scope="module")
def census(built):
    return ic.census()


def test_every_reachable_instance_has_a_row(census):
    reached, _, _ = census
    bad = ic.check_table(ic.INSTANCE_CASES, reached, ic.natural_ids())
    print("%d reachable instances, %d of them picked by the rule itself; %d rows; instances without a row: %d" % (
        len(reached), len(ic.natural_ids()), len(ic.ROWS), sum("no row runs" in b for b in bad)))
    assert not bad, "\n".join(bad)


def test_deleting_any_row_fails_by_name(census):
    """the table has no row to spare: without any one of them an instance is left without a row, or without one at the rule's own selection, and the complaint names it"""
    reached, natural = census[0], ic.natural_ids()
    for k, rows in ic.INSTANCE_CASES.items():
        for r in rows:
            table = collections.OrderedDict((kk, [x for x in rr if x is not r]) for kk, rr in ic.INSTANCE_CASES.items())
            bad = ic.check_table(table, reached, natural)
            assert bad, "the table passes without %s" % ic.row_id(r)
            lost = {kid for kid in ic.ids_of(ic.row_selection(r)) if any(str(kid) in b for b in bad)}
            assert lost, (ic.row_id(r), bad)


def test_the_random_patterns_reach_nothing_else(census):
    """the fuzz gate's patterns are part of the reachable set: every instance they reach is one the sweep of the workloads reaches (and so has a row)"""
    reached, _, fuzz = census
    assert fuzz and not [k for k in fuzz if k not in reached]


def test_no_single_kernel_on_chip_instance_and_no_experiment_is_reachable(census):
    """the rule, the forced families and the occupancy knobs never arrive at the single-kernel on-chip form or at the tile experiment's kernels (those have their own
    switches and tests: tests/test_gpu_settings.py), nor at the kernel of mpcqp_update_matrices, which is not a kernel of a solve (tests/test_gpu_update_matrices.py)"""
    assert {k.kind for k in census[0]} == {"stream", "lds", "gb", "oc_setup", "oc_admm", "oc_admm_rf", "oc_admm_p4"}
    assert not any(k.tiles for k in census[0])


def test_single_kernel_lookup_of_a_plan_without_an_arrow_head(built):
    """the eight-wave single-kernel lookup asks the table with nh = 0 for a plan without an arrow head, as the iteration kernel's lookup does: the table has no such
    single-kernel instance, so such a handle would fail at create instead of running a hub instance on a hub-less plan"""
    for form, nh in (("full", 7), ("reduced", 0)):
        s = ic.select(ic.pattern("quadrotor", 35, form), 8, {"MPCQP_VARIANT": "oc8"})
        assert s.oc["has_hub"] == (form == "full") and s.split
        assert (s.mono.kind, s.mono.nw, s.mono.ng, s.mono.nh, s.mono.hub) == ("oc_mono", 8, 7, nh, int(form == "full"))
        assert (s.ids["plain"].nh, s.ids["rf"].nh, s.ids["setup"].hub) == (nh, nh, int(form == "full"))


def test_what_the_family_table_reached(census):
    """report (-s): the instances the broadest older case table runs -- tests/test_gpu_settings.py's family x workload rows, whose sizes (quadrotor N=20 / 50, cart-pole
    N=30 / 100) are with the double integrator N=20 the sizes of nearly every GPU case -- and the rule at those sizes, against the reachable set"""
    from tests import test_gpu_settings as ts
    reached, old = census[0], set()
    for leg, wid in list(ts.PAIRS) + [(None, w) for w in problems.HARD_WORKLOADS]:
        name, N, B = problems.HARD_WORKLOADS[wid]
        s = ic.select(ic.pattern(name, N), B, ts.LEGS[leg][0] if leg else {})
        old |= ic.ids_of(s) & set(reached) if isinstance(s, ic.Sel) else set()
    for b in ic.RULE_BATCHES:
        old |= ic.ids_of(ic.select(ic.pattern("double_integrator", 20), b, {}))
    new = sorted(set(reached) - old)
    print("%d of %d reachable instances in the family table of tests/test_gpu_settings.py; not reached there:" % (len(old), len(reached)))
    for k in new:
        print("   ", k, "  smallest:", min(reached[k], key=lambda r: r.n)[:5], "  random patterns of the fuzz gate: %d" % census[2].get(k, 0))
    for k in (ic._stream(8), ic._gb(4, 3, 0), ic._gb(4, 2, 1), ic._gb(4, 2, 0), ic._lds(1, 4), ic._lds(4, 3)):
        assert k in new, k


def test_set_up_branches(census):
    """second tier: every run-time branch of the set-up kernel's shape that the sweep reaches is taken by a row's handle or by a handle of SETUP_BRANCH_CASES; each of the
    latter takes the branch it is filed under, is the smallest problem of the sweep that does, and is the rule's own choice with the same kernels and the same set-up
    shape at every batch of RULE_BATCHES.  Printed (-s): the branches and who takes them."""
    branches = census[1]
    by_rows = collections.defaultdict(list)
    for _, r in ic.ROWS:
        b = ic.setup_branch(ic.row_selection(r))
        if b:
            by_rows[b].append(ic.row_id(r))
    for b, r in ic.SETUP_ROWS:
        s = ic.row_selection(r)
        assert ic.setup_branch(s) == b and b not in by_rows, (b, ic.row_id(r))
        assert s.plan["n"] == min(x.n for x in branches[b]), (b, ic.row_id(r))
        assert s.shape.startswith("mpcqp: set-up kernel shape: 4 waves, %d B of LDS" % s.setup["lds"])
        for batch in ic.RULE_BATCHES:
            t = ic.select(ic.pattern(r.workload, r.N, r.form), batch, {})
            assert (t.ids, t.setup, t.plan["lds_bytes"]) == (s.ids, s.setup, s.plan["lds_bytes"]), (ic.row_id(r), batch)
    second = {b: ic.row_id(r) for b, r in ic.SETUP_ROWS}
    for b in sorted(branches):
        print("(A staged %d, P staged %d, 16-bit tables %d, A's table %s, P's %s): %d selections, smallest %s; taken by: %s" % (
            b + (len(branches[b]), min(branches[b], key=lambda r: r.n)[:4], ", ".join(by_rows.get(b, []) + ([second[b]] if b in second else [])))))
    assert set(by_rows) | set(second) == set(branches) and {b[2] for b in branches} == {0, 1, 3}


def test_knob_pairs(built):
    """the pairs of tests/test_gpu_instances.py's register-budget relation: the knob moves the row's pattern to the named instance and changes nothing else of the plan"""
    for row, knob, k in ic.KNOB_PAIRS:
        a, b = ic.row_selection(row), ic.row_selection(row, knob)
        assert ic.primary(b) == k != ic.primary(a), (ic.row_id(row), knob)
        assert a.plan == b.plan and a.oc == b.oc


@pytest.mark.parametrize("key", DATA_KEYS, ids=lambda k: "%s-N%d-%s" % k)
def test_oracle_outcomes_on_a_rows_data(built, key):
    """what tests/test_gpu_instances.py relies on, on the oracle: a solved, a primal infeasible and a dual infeasible instance under the default settings, an instance
    that ends on the iteration limit in the tail leg, at least three quarters of the batch stable in every leg (the cap of tests/test_osqp_ref.py), and in the rho leg an
    instance that changes rho at least twice (counted as tests/test_rho_recipes.py counts)"""
    d = ic.row_data(*key)
    B = d.ref_ls.batch
    for leg in ic.LEGS:
        ref, stable = ic.oracle_leg(*key, leg)
        print(key, leg, ic.leg_settings(*key, leg), "status", ref["status"].tolist(), "iters", ref["iters"].tolist(), "stable %d of %d" % (stable.sum(), B))
        assert stable.sum() >= 0.75 * B, (key, leg, stable)
        if leg == "default":
            assert ref["status"][0] == 1 and ref["status"][problems.PRIMAL_INFEASIBLE] == 3 and ref["status"][problems.DUAL_INFEASIBLE] == 5, ref["status"]
        if leg == "tail":
            assert (ref["status"] == 7).any() and ref["iters"].max() <= 24, (ref["status"], ref["iters"])
    updates = problems.oracle_rho_updates(d.ref_ls, **ic.leg_settings(*key, "rho"))
    print(key, "rho updates", updates.tolist())
    assert updates.max() >= 2 and ic.oracle_leg(*key, "rho")[0]["iters"].max() <= 1500
    (first, second), (ok1, ok2) = ic.oracle_kept(*key)
    assert ok1.sum() >= 0.75 * B and ok2.sum() >= 0.75 * B
    assert np.array_equal(first["status"], ic.oracle_leg(*key, "default")[0]["status"]) and (second["status"] == 1).any()


@pytest.mark.parametrize("key", SETUP_KEYS, ids=lambda k: "%s-N%d-%s" % k)
def test_oracle_outcomes_on_a_set_up_branch_rows_data(built, key):
    """the same for the rows of SETUP_BRANCH_CASES, which run the default and the kept-workspace leg only"""
    B = ic.row_data(*key).ref_ls.batch
    ref, stable = ic.oracle_leg(*key, "default")
    assert stable.sum() >= 0.75 * B and ref["status"][0] == 1 and ref["status"][problems.PRIMAL_INFEASIBLE] == 3 and ref["status"][problems.DUAL_INFEASIBLE] == 5, ref["status"]
    (first, second), (ok1, ok2) = ic.oracle_kept(*key)
    assert ok1.sum() >= 0.75 * B and ok2.sum() >= 0.75 * B and np.array_equal(first["status"], ref["status"]) and (second["status"] == 1).any()


def test_reduced_objective_constant(built):
    """the constant instance_cases adds to the reduced oracle's objective is the caller's objective at the lifted point minus the reduced QP's at the reduced point"""
    key = ("double_integrator", 6, "reduced")
    d = ic.row_data(*key)
    plain = problems.oracle_solve(d.ref_ls, nthreads=8)
    ref = ic.oracle_leg(*key, "default")[0]
    mdl = __import__("optimal_control_problem_amd.models", fromlist=["x"]).make_workload(key[0], 1, N=key[1])[0]
    _, free, _, fvars, xfix = problems.reduce_qp(d.ls, list(range(mdl.np)))
    for b in np.flatnonzero(plain["status"] == 1):
        x = np.zeros(d.ls.n); x[free] = plain["x"][b]; x[fvars] = xfix[b]
        Pd = d.ls.dense(b)[0]; Pd = np.triu(Pd) + np.triu(Pd, 1).T
        assert abs(0.5 * x @ Pd @ x + d.ls.q[b] @ x - ref["obj"][b]) <= 1e-9 * (1.0 + abs(ref["obj"][b]))
    cert = np.isin(plain["status"], (3, 4, 5, 6))
    assert cert.any() and np.array_equal(ref["obj"][cert], plain["obj"][cert])
