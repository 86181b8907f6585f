"""The compiled instances of the QP kernels, who reaches them, and the table of cases that runs each of them -- TEST INFRASTRUCTURE ONLY.

A kernel family is several separately compiled instances: mpcqp_res_kernel at three register budgets, its kept-workspace twins, two streaming kernels, the
set-up / iteration / in-place re-factorisation kernels of the two-kernel on-chip form in four- and eight-wave shapes with and without hub blocks.  Which one a
handle launches is csrc/select.hpp kernel_id_of (and its siblings), read here through tests/support/plan_interp.cpp plan_select_kernels -- the mapping
mpcqp.hip itself goes through, not a restatement.

  * census(): select_kernel at 256 CUs over the three workloads x N_GRID x {full, reduced form} x {the rule at RULE_BATCHES, every forced family}, once plain
    and once under each occupancy knob, plus the random patterns of tests/test_gpu_fuzz.py -> the reachable KernelIds and who reaches them.
  * INSTANCE_CASES: the rows tests/test_gpu_instances.py runs, each filed under the KernelId its handle launches for a plain solve.
  * tests/test_instance_census_host.py holds the table to the census: every reachable id has a row, every row selects what it is filed under.
"""
import collections
import contextlib
import ctypes as C
import functools
import os

import numpy as np

from tests.support import problems

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libplan_interp.so")
CUS = 256                                              # compute units of an MI355X
KINDS = ("stream", "lds", "gb", "oc_mono", "oc_setup", "oc_admm", "oc_admm_rf", "oc_admm_p4", "oc_admm_tl", "oc_rescale")      # csrc/select.hpp KernelKind
KernelId = collections.namedtuple("KernelId", "kind nw minw zyg ng nh hub pd reuse rf tiles")
ROLES = ("plain", "kept", "rf", "setup", "setup_kept")                  # the kernels of a handle that the legs of tests/test_gpu_instances.py run
Sel = collections.namedtuple("Sel", "plan oc setup flags ids mono pd8 split shape")
PLAN_KEYS = ["n", "m", "batch", "npad", "mpad", "n_blocks", "L_blocks", "lds_bytes", "workspace_bytes_per_qp", "ordering", "nnzP_triu", "nnzA", "T_blocks",
             "factor_ops", "ell_slots", "variant"]
OC_KEYS = ["chain_blocks", "has_hub", "chain_e", "chain_f", "lds_blocks", "positions_per_wave", "hub_blocks_in_registers", "launch_pairs_for_rho_updates",
           "slots_A", "slots_At", "slots_P", "chain_pairs"]
FAMILY_OF_VARIANT = {0: "stream", 1: "res1", 2: "res2", 4: "res4", 8: "res8", 102: "gres2", 104: "gres4", 204: "oc4", 208: "oc8"}

WORKLOADS = ("double_integrator", "quadrotor", "cartpole")
# every horizon README.md and DESIGN.md section 3 quote a figure for (5, 6, 10, 15, 20, 22, 24, 25, 26, 30, 40, 50, 55, 56, 57, 60, 80, 100, 120, 150), every N up to 26, and
# steps of at most 10 between them up to 60
N_GRID = tuple(range(3, 27)) + (28, 30, 35, 40, 45, 50, 55, 56, 57, 60, 70, 80, 100, 120, 150)
RULE_BATCHES = (64, 1024, 8192, 16384)
FAMILIES = ("stream", "res1", "res2", "res4", "res8", "gres4", "gres2", "oc4", "oc8")
OCCUPANCY_KNOBS = ("MPCQP_GB_OCC2", "MPCQP_GB_OCC3", "MPCQP_NO_ZYG", "MPCQP_NO_RES1X", "MPCQP_NO_RES3", "MPCQP_PD4")
FORCED_BATCH = 8                                       # a forced family's instance does not depend on the batch (select.hpp occupancy_instances reads the footprint only)


def gpu_batch(workload, N):
    """instances a row is run with: each test is a few seconds, most of it the oracle"""
    return 4 if workload == "quadrotor" and N >= 100 else 8


@contextlib.contextmanager
def environment(env):
    """the MPCQP_* variables of the process replaced by env (Knobs::from_env reads them at every selection)"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("MPCQP_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


@functools.lru_cache(maxsize=None)
def pattern(workload, N, form="full"):
    """(n, m, Pp, Pi, Ap, Ai) of a workload; form "reduced": the pattern mpcqp_create_reduced hands to its inner handle with the parameter rows fixed"""
    n, m, Pp, Pi, Ap, Ai, _ = problems.selection_pattern(dict(workload=workload, N=N, reduced=form == "reduced"), inner=True)
    return (n, m) + tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (Pp, Pi, Ap, Ai))


@functools.lru_cache(maxsize=None)
def _lib():
    L = C.CDLL(SO)
    L.plan_select_kernels.restype = C.c_int
    L.plan_select_shape.restype = C.c_char_p
    return L


def select(pat, batch, env=None, forced=None, knob_mask=0):
    """select_kernel on a pattern under the environment env -> Sel, or the error code.  forced: mpcqp_create_tuned's way of naming a family, knob_mask: bit i =
    OCCUPANCY_KNOBS[i] switched on -- the same selection as with MPCQP_VARIANT and the knob in env, without touching the environment (the census runs on threads)"""
    n, m, Pp, Pi, Ap, Ai = pat
    out = np.zeros(48, np.int64); kid = np.zeros(8 * 12, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    def call():      # (the MPCQP_VERBOSE line of the selection is kept per thread: read on the thread that selected)
        rc = _lib().plan_select_kernels(n, m, int(batch), p(Pp), p(Pi), p(Ap), p(Ai), CUS, forced, int(knob_mask), p(out), p(kid))
        return rc, _lib().plan_select_shape().decode()
    if env is None:
        rc, shape = call()
    else:
        with environment(env):
            rc, shape = call()
    if rc:
        return rc
    o, k = out.tolist(), kid.reshape(8, 12).tolist()
    ident = lambda r: KernelId(KINDS[r[0]], *r[1:11]) if r[11] else None
    setup = dict(zip(["waves", "lds", "stage", "a_lds", "p_lds", "ix16", "zpad", "ixo_a", "ixo_p", "split"], o[28:38]))
    flags = dict(zip(["zyg", "occ3", "occ4", "res1x", "res3", "wide", "oc8", "waves_a"], o[40:48]))
    return Sel(dict(zip(PLAN_KEYS, o[:16])), dict(zip(OC_KEYS, o[16:28])), setup, flags, dict(zip(ROLES, map(ident, k[:5]))), ident(k[6]), bool(k[7][0]), bool(k[7][1]), shape)


def ids_of(sel):
    """the compiled instances a handle of this selection launches in the legs of the GPU module (the kernel of mpcqp_update_matrices is not among them:
    tests/test_gpu_update_matrices.py runs both of its instances)"""
    return {k for k in sel.ids.values() if k is not None}


def setup_branch(sel):
    """second tier: the run-time branch of the set-up kernel a two-kernel handle takes -- (values of A staged, of P staged, 16-bit index tables 0 / 1 = A / 3 = A and P,
    where A's table sits, where P's) with "scratch" = the factorisation's scratch, "z" = the z region, "-" = no table.  None: no set-up kernel"""
    if not isinstance(sel, Sel) or not sel.split:
        return None
    u = sel.setup
    staged = u["a_lds"] and u["p_lds"]
    where = lambda on, off: "-" if not on else "z" if staged or off else "scratch"
    return (u["a_lds"], u["p_lds"], u["ix16"], where(u["ix16"] & 1, u["ixo_a"]), where(u["ix16"] & 2, u["ixo_p"]))


# ---------------------------------------------------------------------------------------------- the census
Reach = collections.namedtuple("Reach", "workload N form batch env n")       # batch None: a forced family (env names it)


# the families whose instance a knob can change (where select.hpp reads it: occupancy_instances, the streaming kernel's blocks in flight; MPCQP_NO_ZYG also in the
# rule's footprint test).  Under a knob the other forced families select what they select without it, so the knob's sweep forces only these -- and runs the rule.
KNOB_FAMILIES = {"MPCQP_GB_OCC2": ("gres4", "gres2"), "MPCQP_GB_OCC3": ("gres4", "gres2"), "MPCQP_NO_ZYG": ("gres4", "gres2"), "MPCQP_NO_RES1X": ("res1",),
                 "MPCQP_NO_RES3": ("res4",), "MPCQP_PD4": ("stream",)}


def _sweep_pattern(key):
    w, N, form = key
    pat = pattern(w, N, form)
    found = []
    for knob in (None,) + OCCUPANCY_KNOBS:
        mask = 1 << OCCUPANCY_KNOBS.index(knob) if knob else 0
        for batch, fam in [(b, None) for b in RULE_BATCHES] + [(None, f) for f in (KNOB_FAMILIES[knob] if knob else FAMILIES)]:
            s = select(pat, batch or FORCED_BATCH, None, fam.encode() if fam else b"", mask)      # (b"": the rule whatever the environment says)
            if isinstance(s, Sel):
                env = ((("MPCQP_VARIANT", fam),) if fam else ()) + (((knob, "1"),) if knob else ())
                found.append((Reach(w, N, form, batch, tuple(sorted(env)), pat[0]), ids_of(s), setup_branch(s)))
    return found


@functools.lru_cache(maxsize=None)
def census():
    """-> (reached: KernelId -> [Reach, ...] over the sweep of the module docstring, branches: set-up branch -> [Reach, ...], fuzz: KernelId -> number of random patterns)"""
    from concurrent.futures import ThreadPoolExecutor
    reached, branches, fuzz = collections.defaultdict(list), collections.defaultdict(list), collections.Counter()
    keys = [(w, N, form) for N in reversed(N_GRID) for w in WORKLOADS for form in ("full", "reduced")]      # (longest first)
    for key in keys:
        pattern(*key)                   # (NumPy work, cached: before the threads start)
    # (the selection is C++ behind ctypes, which releases the interpreter lock)
    with environment({}), ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for found in pool.map(_sweep_pattern, keys):
            for r, ids, branch in found:
                for k in ids:
                    reached[k].append(r)
                if branch:
                    branches[branch].append(r)
    for pat, B, fam in fuzz_patterns():
        s = select(pat, B, {"MPCQP_VARIANT": fam} if fam else {})
        if isinstance(s, Sel):
            for k in ids_of(s):
                fuzz[k] += 1
    return dict(reached), dict(branches), fuzz


def fuzz_patterns():
    """the patterns, batches and families of tests/test_gpu_fuzz.py: 60 random sparse patterns x {the rule, res1, res4, gres4, stream}, and the random stage
    problems of its on-chip gate (the first 20 per family that the family takes)"""
    from tests import test_gpu_fuzz as fz
    as_pat = lambda ls: (ls.n, ls.m) + tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai))
    for c in range(fz.NPAT):
        n, m, B, dens = problems.fuzz_pattern_draw(c)
        pat = as_pat(problems.sparse_batch(n, m, 1, c, dens))        # (the pattern is drawn before any instance's values: the same for every batch)
        for fam in fz.FAMILIES:
            yield pat, B, fam
    for fam, _ in fz.OC_FAMILIES:
        taken = c = 0
        while taken < fz.OC_NPAT and c < 4 * fz.OC_NPAT:
            ls, _, _ = problems.random_stage_ocp(c, fam); c += 1
            pat = as_pat(ls)
            if isinstance(select(pat, ls.batch, {"MPCQP_VARIANT": fam}), Sel):
                taken += 1
                yield pat, ls.batch, fam


def natural_ids():
    """KernelId -> [Reach, ...]: what the rule itself picks (no knob, no forced family) at the batches of RULE_BATCHES"""
    return {k: [r for r in rs if r.batch is not None and not r.env] for k, rs in census()[0].items() if any(r.batch is not None and not r.env for r in rs)}


# ---------------------------------------------------------------------------------------------- the case table
# A row: the workload, horizon and form whose pattern the handle is created on, and the environment it is created under, at gpu_batch() instances.
#   rule_batch = None: the row is there because it is the smallest problem (by n) of the sweep whose handle launches the id it is filed under with nothing but a
#     forced family set -- or, with an occupancy knob in env, a small problem that a knob moves to that instance.
#   rule_batch = B: the rule itself picks this instance for this pattern at batch B.  A handle is created for one batch and solved at that batch only, so the
#     row creates it at gpu_batch() under the family the rule chose, and the CPU module asserts that this selects the same kernels and the same lds_bytes.
Row = collections.namedtuple("Row", "workload N form env rule_batch")


def row_id(r):
    return "%s-N%d%s%s%s" % (r.workload, r.N, "" if r.form == "full" else "-reduced", "".join("-%s=%s" % (k.replace("MPCQP_", ""), v) for k, v in sorted(r.env.items())),
                             "-rule@%d" % r.rule_batch if r.rule_batch else "")


_SELECTED = {}


def row_selection(r, knob=None):
    """the CPU selection of the handle tests/test_gpu_instances.py creates for the row (knob: with that occupancy knob set besides the row's environment)"""
    key = (row_id(r), knob)
    if key not in _SELECTED:
        _SELECTED[key] = select(pattern(r.workload, r.N, r.form), gpu_batch(r.workload, r.N), dict(r.env, **({knob: "1"} if knob else {})))
    return _SELECTED[key]


def row_rule_selection(r):
    """what the rule picks at the row's rule_batch"""
    key = (row_id(r), "rule")
    if key not in _SELECTED:
        _SELECTED[key] = select(pattern(r.workload, r.N, r.form), r.rule_batch, {})
    return _SELECTED[key]


def primary(sel):
    return sel.ids["plain"]


def _lds(nw, minw, **kw):
    return KernelId("lds", nw, minw, 0, 0, 0, 0, 0, 0, 0, 0)._replace(**kw)


def _gb(nw, minw, zyg):
    return KernelId("gb", nw, minw, zyg, 0, 0, 0, 0, 0, 0, 0)


def _stream(pd):
    return KernelId("stream", 1, 0, 0, 0, 0, 0, pd, 0, 0, 0)


def _admm(nw, ng, nh):
    return KernelId("oc_admm", nw, 0, 0, ng, nh, 1 if nh else 0, 0, 0, 0, 0)


def _p4(hub=1):
    return KernelId("oc_admm_p4", 4, 0, 0, 5, 3 if hub else 0, hub, 0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------- a row's data and the oracle's side of its legs
# The legs of tests/test_gpu_instances.py and their settings.  tests/test_instance_census_host.py holds the oracle's outcomes on every row to what the GPU module relies
# on: statuses 1, 3, 5 in the default leg and a 7 in the tail leg, at least three quarters of every batch stable, an instance with two rho updates in the rho leg.
LEGS = ("default", "rho", "tail")
# tail: problems.TAIL_CASES' "max_iter=24", a limit one iteration short of the first termination check, so that the code behind the loop makes the only check of the run.
# The quadrotor and the problems of up to six stages are solved to the default 1e-3 by then (status 1 from the tail as well): they run the same limit at 1e-6, where the
# tail finds them unfinished (7) -- the number of the recipe changed for those rows, not the case.
TAIL = "max_iter=24"
assert TAIL in problems.TAIL_CASES


def _tail_settings(workload, N):
    st = dict(problems.SETTINGS_MATRIX[TAIL])
    return dict(st, eps_abs=1e-6, eps_rel=1e-6) if workload == "quadrotor" or N <= 6 else st


# rho: the settings under which a workload changes rho repeatedly (the in-kernel re-factorisation of the instance): problems' recipes for the quadrotor and the cart-pole,
# and per row where those give fewer than two updates on that size or run for thousands of iterations: a start at rho = 1e-3 (the cart-pole N=100 recipe of problems,
# tests/test_gpu_fuzz.py's interval of 25), for the smallest problems with a look every 10 iterations and a tolerance that keeps them running long enough
_SMALL_RHO = dict(adaptive_rho_interval=10, rho=1e-3, eps_abs=1e-8, eps_rel=1e-8)
RHO_RECIPE = {"quadrotor": dict(problems._Q_RHO), "cartpole": dict(problems.RHO_RECIPES["cp30"][3]), "double_integrator": dict(_SMALL_RHO)}
RHO_RECIPE_OF_ROW = {
    ("double_integrator", 6, "reduced"): dict(adaptive_rho_interval=10, rho=1e-3),       # (at 1e-8 only half of the batch is stable)
    ("cartpole", 6, "full"): dict(_SMALL_RHO), ("cartpole", 19, "full"): dict(_SMALL_RHO),
    ("cartpole", 55, "reduced"): dict(problems.RHO_RECIPES["cp100"][3]), ("cartpole", 120, "reduced"): dict(problems.RHO_RECIPES["cp100"][3]),
    ("cartpole", 150, "full"): dict(adaptive_rho_interval=25, rho=1e-3),
}
# the dual-infeasible instance's q (problems.hard_stage_batch: -1): the cart-pole N=150 is `solved` at -1 under the default scaling, as tests/test_gpu_settings.py notes for N=30
DUAL_Q_OF_ROW = {("cartpole", 150): -10.0, ("cartpole", 100): -10.0}


def leg_settings(workload, N, form, leg):
    if leg == "rho":
        return dict(RHO_RECIPE_OF_ROW.get((workload, N, form), RHO_RECIPE[workload]))
    return _tail_settings(workload, N) if leg == "tail" else {}


Data = collections.namedtuple("Data", "ls fixed_rows ref_ls free kept const")


def _reduced(mdl, ls):
    """problems.reduce_qp with the parameter rows fixed -> (reduced QP, its variables, its rows, the constant the eliminated variables contribute to the caller's
    objective per instance: q_f'x_f + 1/2 x_f'P_ff x_f -- what mpcqp_postsolve_kernel adds to the inner handle's objective, csrc/reduced.hpp)"""
    red, free, kept, fvars, xfix = problems.reduce_qp(ls, list(range(mdl.np)))
    const = np.zeros(ls.batch)
    for b in range(ls.batch):
        Pd = ls.dense(b)[0]
        Pd = np.triu(Pd) + np.triu(Pd, 1).T
        const[b] = ls.q[b, fvars] @ xfix[b] + 0.5 * xfix[b] @ Pd[np.ix_(fvars, fvars)] @ xfix[b]
    return red, free, kept, const


def _callers_info(ref, const):
    """the oracle's result on the reduced QP with the objective the handle reports: the caller's, i.e. plus the eliminated variables' constant wherever the run ends
    at a point (statuses 1, 2, 7; a certificate's +-1e30 stays).  prim_res, dual_res and rho are the inner handle's, which the postsolve passes through."""
    if const is None:
        return ref
    return dict(ref, obj=np.where(np.isin(ref["status"], (1, 2, 7)), ref["obj"] + const, ref["obj"]))


@functools.lru_cache(maxsize=None)
def row_data(workload, N, form):
    """the batch a row is run on: problems.hard_stage_batch at gpu_batch() instances -- instance 1 dual infeasible, instance 2 primal infeasible.  -> Data(the
    batch the handle is given, the rows mpcqp_create_reduced fixes or None, the QP the oracle solves, the handle's variables / rows that QP keeps or None, the
    objective's constant or None)"""
    mdl, ls, _ = problems.hard_stage_batch((workload, N, gpu_batch(workload, N)), dual_q=DUAL_Q_OF_ROW.get((workload, N), -1.0))
    if form == "full":
        return Data(ls, None, ls, None, None, None)
    red, free, kept, const = _reduced(mdl, ls)
    return Data(ls, list(range(mdl.np)), red, free, kept, const)


def _frozen(*results):
    for r in results:
        for v in r.values():
            v.setflags(write=False)
    return results if len(results) > 1 else results[0]


@functools.lru_cache(maxsize=None)
def oracle_leg(workload, N, form, leg):
    """-> (oracle result, stable mask) of a row's batch under a leg's settings: computed once, shared, never changed"""
    d, st = row_data(workload, N, form), leg_settings(workload, N, form, leg)
    return _frozen(_callers_info(problems.oracle_solve(d.ref_ls, nthreads=8, **st), d.const)), problems.oracle_stable_mask(d.ref_ls, nthreads=8, **st)


@functools.lru_cache(maxsize=None)
def kept_vectors(workload, N, form):
    """(q, l, u) of the vectors-only solve of the kept-workspace leg: problems.kept_q and every finite bound shifted (l and u of a row by the same amount)"""
    ls = row_data(workload, N, form).ls
    shift = 0.01 * np.random.default_rng(23).standard_normal(ls.l.shape)
    return problems.kept_q(ls), ls.l + shift, ls.u + shift


@functools.lru_cache(maxsize=None)
def oracle_kept(workload, N, form):
    """-> ((full solve, vectors-only solve), (their stable masks)) of the oracle's kept workspace on the row's batch, default settings"""
    from optimal_control_problem_amd import models
    d = row_data(workload, N, form)
    q2, l2, u2 = kept_vectors(workload, N, form)
    const2 = None
    if form == "reduced":           # (the reduced statement of the second solve: P and A of the reduced QP do not depend on q, l, u)
        mdl = models.make_workload(workload, 1, N=N)[0]
        ls = d.ls
        r2, _, _, const2 = _reduced(mdl, models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, ls.P, q2, ls.A, l2, u2, ls.np))
        q2, l2, u2 = r2.q, r2.l, r2.u
    first, second = problems.oracle_kept_solves(d.ref_ls, q2, l2=l2, u2=u2)
    return _frozen(_callers_info(first, d.const), _callers_info(second, const2)), problems.oracle_kept_stable_mask(d.ref_ls, q2, l2=l2, u2=u2)


def _row(workload, N, form="full", family=None, rule_batch=None):
    return Row(workload, N, form, {"MPCQP_VARIANT": family} if family else {}, rule_batch)


# KernelId of a plain solve -> rows.  The kept-workspace twin (reuse = 1), the in-place re-factorisation kernel and the set-up kernels of a two-kernel handle are the other
# kernels of the same rows' handles (Sel.ids): tests/test_instance_census_host.py counts them as reached through these rows.
INSTANCE_CASES = collections.OrderedDict([
    (_stream(4), [_row("double_integrator", 3, "reduced", "stream")]),
    (_stream(8), [_row("cartpole", 120, "reduced", "stream")]),
    (_lds(1, 4), [_row("double_integrator", 3, "reduced", "res1", 8192)]),
    (_lds(1, 2), [_row("cartpole", 6, "full", "res1", 8192)]),
    (_lds(2, 3), [_row("double_integrator", 3, "reduced", "res2"), _row("double_integrator", 13, "full", "res2", 64)]),
    (_lds(4, 4), [_row("double_integrator", 3, "reduced", "res4", 64)]),
    (_lds(4, 3), [_row("quadrotor", 4, "full", "res4", 64)]),
    (_lds(4, 2), [_row("cartpole", 19, "full", "res4"), _row("cartpole", 45, "reduced", "res4", 64)]),
    (_lds(4, 1), [_row("quadrotor", 10, "full", "res4"), _row("cartpole", 55, "reduced", "res4", 64)]),
    (_lds(8, 2), [_row("double_integrator", 3, "reduced", "res8")]),
    (_gb(2, 3, 0), [_row("double_integrator", 3, "reduced", "gres2")]),
    (_gb(4, 4, 0), [_row("double_integrator", 3, "reduced", "gres4")]),
    (_gb(4, 3, 0), [_row("quadrotor", 28, "full", "gres4")]),
    (_gb(4, 3, 1), [_row("cartpole", 150, "full", "gres4"), _row("quadrotor", 55, "reduced", "gres4", 64)]),
    (_gb(4, 2, 1), [_row("quadrotor", 100, "reduced", "gres4", 64)]),
    (_gb(4, 2, 0), [_row("quadrotor", 150, "reduced", "gres4", 64)]),
    (_admm(4, 5, 3), [_row("cartpole", 6, "full", "oc4", 64)]),
    (_admm(4, 5, 0), [_row("double_integrator", 6, "reduced", "oc4", 64)]),
    (_p4(), [_row("cartpole", 26, "full", "oc4", 64)]),
    (_admm(8, 4, 4), [_row("cartpole", 6, "full", "oc8"), _row("quadrotor", 21, "full", "oc8", 1024)]),
    (_admm(8, 4, 0), [_row("double_integrator", 6, "reduced", "oc8"), _row("cartpole", 55, "reduced", "oc8", 1024)]),
    (_admm(8, 7, 7), [_row("quadrotor", 35, "full", "oc8", 64)]),
    (_admm(8, 7, 0), [_row("quadrotor", 35, "reduced", "oc8", 64)]),
])
ROWS = [(k, r) for k, rows in INSTANCE_CASES.items() for r in rows]

# Knobs that move a pattern between two register budgets of the same code: (row, knob, the instance the row's pattern runs under the knob)
KNOB_PAIRS = [
    (INSTANCE_CASES[_lds(1, 4)][0], "MPCQP_NO_RES1X", _lds(1, 2)),
    (INSTANCE_CASES[_lds(4, 4)][0], "MPCQP_NO_RES3", _lds(4, 2)),
    (INSTANCE_CASES[_lds(4, 3)][0], "MPCQP_NO_RES3", _lds(4, 2)),
    (INSTANCE_CASES[_gb(4, 4, 0)][0], "MPCQP_GB_OCC3", _gb(4, 3, 0)),
    (INSTANCE_CASES[_gb(4, 4, 0)][0], "MPCQP_GB_OCC2", _gb(4, 2, 0)),
    (INSTANCE_CASES[_gb(4, 3, 0)][0], "MPCQP_GB_OCC2", _gb(4, 2, 0)),
]


# Second tier: the run-time branches of the set-up kernel's shape that no row above takes, each at the smallest problem of the sweep that takes it -- the rule's own
# choice at every batch of RULE_BATCHES, and at gpu_batch() too (the CPU module asserts both).  tests/test_gpu_instances.py runs them through the default and the
# kept-workspace leg with MPCQP_VERBOSE set, and first holds the library's own line about the shape to the CPU selection's.
SETUP_BRANCH_CASES = collections.OrderedDict([
    ((1, 1, 1, "z", "-"), _row("double_integrator", 55)),
    ((1, 0, 0, "-", "-"), _row("double_integrator", 70)),
    ((0, 0, 1, "scratch", "-"), _row("quadrotor", 24)),
    ((0, 0, 3, "z", "scratch"), _row("cartpole", 100)),
    ((0, 0, 0, "-", "-"), _row("quadrotor", 45, "reduced")),
])
SETUP_ROWS = [(b, r._replace(env={"MPCQP_VERBOSE": "1"})) for b, r in SETUP_BRANCH_CASES.items()]


def check_table(table, reached, natural):
    """the conditions the table is held to (tests/test_instance_census_host.py) -> list of complaints, each naming the instance.
    (a) every reachable id is a kernel of some row's handle; (b) every row's handle launches the id it is filed under for a plain solve, and is the smallest problem (by n) of
    the sweep that does with at most a forced family set -- or, for a row with a rule_batch, the smallest the rule itself picks the id for -- and every id rows are filed
    under has its row at that smallest size; (c) every id the rule picks at a
    batch of RULE_BATCHES has such a row, and creating the handle at gpu_batch() under the rule's family selects the same kernels and the same lds_bytes."""
    bad, covered = [], set()
    plain_min = {k: min(r.n for r in rs if all(name == "MPCQP_VARIANT" for name, _ in r.env)) for k, rs in reached.items()}
    natural_min = {k: min(r.n for r in rs) for k, rs in natural.items()}
    for k, rows in table.items():
        for r in rows:
            s = row_selection(r)
            if not isinstance(s, Sel) or primary(s) != k:
                bad.append("%s: filed under %s, selects %s" % (row_id(r), k, primary(s) if isinstance(s, Sel) else "error %s" % s)); continue
            covered |= ids_of(s)
            n = s.plan["n"]
            if any(name != "MPCQP_VARIANT" for name in r.env):
                bad.append("%s: a knob in the environment of a row" % row_id(r))
            if r.rule_batch:
                t = row_rule_selection(r)
                if not isinstance(t, Sel) or t.ids != s.ids or t.plan["lds_bytes"] != s.plan["lds_bytes"] or FAMILY_OF_VARIANT[t.plan["variant"]] != r.env.get("MPCQP_VARIANT"):
                    bad.append("%s: the rule at batch %d does not select what the row runs (%s)" % (row_id(r), r.rule_batch, k))
            if not (n == plain_min.get(k) or (r.rule_batch and n == natural_min.get(k))):
                bad.append("%s: n = %d is not the smallest of the sweep for %s (%s forced, %s by the rule)" % (row_id(r), n, k, plain_min.get(k), natural_min.get(k)))
    for k, rows in table.items():
        if rows and not any(isinstance(row_selection(r), Sel) and row_selection(r).plan["n"] == plain_min.get(k) for r in rows):
            bad.append("no row runs %s at the smallest size of the sweep (n = %s)" % (k, plain_min.get(k)))
    for k in sorted(reached):
        if k not in covered:
            bad.append("no row runs the reachable instance %s (smallest: %s)" % (k, min(reached[k], key=lambda r: r.n),))
    for k in sorted(natural):
        prim = [kk for kk, rows in table.items() for r in rows if r.rule_batch and isinstance(row_selection(r), Sel) and k in ids_of(row_selection(r))]
        if not prim:
            bad.append("the rule picks %s (smallest: %s) and no row runs it at the rule's own selection" % (k, min(natural[k], key=lambda r: r.n),))
    return bad
