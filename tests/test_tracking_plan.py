"""CPU: what the QP engine makes of the per-frame-reference ("tracking") patterns -- the library's own selection rule (csrc/select.hpp through
tests/support/plan_interp.cpp plan_select, 256 CUs, rule defaults) on the full form and on the presolved inner pattern (the parameter rows and the
pinned first frame eliminated: tests/support/problems.reduce_qp, the NumPy statement of mpcqp_create_presolved), and the lane-accurate emulations
of the on-chip solve (plan_execute_oc, plan_execute_oc_nw) on the inner patterns.  These patterns are new to the QP kernels: this runs before
anything touches a GPU.

Found (DESIGN 6.10 has the table): the full form leaves the on-chip families (N nx pinned parameters, each a leaf of its own stage), the inner
pattern returns to them without a hub.  Cart-pole N = 30 is the exception the selection rule itself makes: its inner pattern (n = 145) gets
variant 4, the on-chip plan does not apply to it (rc 5 from both emulation entries, "plan refused", as for every pattern it does not take), so
for that pattern the emulation that is checked at the bound is the one of the family it runs on (plan_execute); cart-pole N = 100, which does go
on chip, runs the on-chip emulation in its place."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "libplan_interp.so")
PLAN_KEYS = ["n", "m", "batch", "npad", "mpad", "n_blocks", "L_blocks", "lds_bytes", "workspace_bytes_per_qp", "ordering", "nnzP_triu", "nnzA", "T_blocks",
             "factor_ops", "ell_slots", "variant"]
OC_KEYS = ["chain_blocks", "has_hub", "chain_e", "chain_f", "lds_blocks", "positions_per_wave", "hub_blocks_in_registers", "launch_pairs_for_rho_updates",
           "slots_A", "slots_At", "slots_P", "chain_pairs"]
ZOO = {"double_integrator": models.DoubleIntegrator, "quadrotor": models.Quadrotor, "cartpole": models.CartPole}
BOUND = 1e-9          # tests/test_plan.py: |sol - dense solve| / |dense solve|, hub-less plans included (test_onchip_plan_without_hub_and_limits)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def patterns(name, N):
    """(model, full tracking local system, presolved inner system) at a perturbed iterate, two instances; computed once and shared"""
    m = type("Tracking" + ZOO[name].__name__, (ZOO[name],), {"per_frame_reference": True})(N)
    rng = np.random.default_rng(17)
    p = rng.normal(0.0, 0.5, size=(2, m.np)); x = rng.normal(0.0, 0.1, size=(2, m.nvar))
    lbx, ubx, lbg, ubg = m.stacked_bounds(x[:, :m.f].copy())
    ls = m.local_system(p, x, lbx, ubx, lbg, ubg)
    fixed = list(range(m.np + m.f))                     # the rows p - p and the first frame's lbx = ubx: what mpcqp_create_presolved finds
    assert np.array_equal(ls.l[:, fixed], ls.u[:, fixed]) and not np.array_equal(ls.l[:, m.np + m.f:m.n], ls.u[:, m.np + m.f:m.n])
    red, free, kept, fvars, _ = problems.reduce_qp(ls, fixed)
    assert np.array_equal(np.sort(fvars), np.arange(m.np + m.f)) and red.n == m.n - m.np - m.f
    return m, ls, red


def select(ls, batch):
    L = C.CDLL(SO)
    out = np.zeros(48, np.int64)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai))
    rc = L.plan_select(ls.n, ls.m, batch, _p(Pp), _p(Pi), _p(Ap), _p(Ai), 256, None, _p(out))
    o = out.tolist()
    return rc, dict(zip(PLAN_KEYS, o[:16])), dict(zip(OC_KEYS, o[16:28]))


@pytest.fixture
def rule_defaults(monkeypatch):
    for k in [k for k in os.environ if k.startswith("MPCQP_")]:
        monkeypatch.delenv(k)


# (name, N, batch, full-form variant, inner n, inner variant, inner chain blocks, inner L-blocks): DESIGN 6.10
TABLE = [("quadrotor", 10, 8192, 104, 144, 204, 9, 17), ("quadrotor", 20, 8192, 104, 304, 204, 19, 37), ("quadrotor", 50, 8192, 0, 784, 208, 49, 97),
         ("cartpole", 100, 16384, 104, 495, 208, 31, 61), ("cartpole", 30, 8192, 104, 145, 4, 0, 18), ("double_integrator", 20, 4096, 4, 57, 2, 0, 7)]


@pytest.mark.parametrize("name,N,batch,vfull,n_in,vin,chain,lblk", TABLE, ids=["%s_N%d" % r[:2] for r in TABLE])
def test_selection_of_the_full_and_the_presolved_pattern(built, rule_defaults, name, N, batch, vfull, n_in, vin, chain, lblk):
    m, ls, red = patterns(name, N)
    rc, plan, oc = select(ls, batch)
    assert rc == 0 and plan["n"] == m.n and plan["variant"] == vfull
    rc, plan, oc = select(red, batch)
    assert rc == 0
    assert (plan["n"], plan["variant"], oc["chain_blocks"], plan["L_blocks"]) == (n_in, vin, chain, lblk)
    assert oc["has_hub"] == 0
    if (name, N) in (("quadrotor", 10), ("quadrotor", 20), ("quadrotor", 50), ("cartpole", 100)):
        assert plan["variant"] >= 200 and oc["has_hub"] == 0          # on chip, no hub
    if vfull < 200 and vin >= 200:
        mdl, sls, _ = models.make_workload(name, 1, N=N)               # fewer factor blocks than today's single-reference QP
        assert plan["L_blocks"] < select(sls, batch)[1]["L_blocks"]


def _emulate(ls, nw, NG, NH, ldl, b=1, seed=0):
    L = C.CDLL(SO)
    L.plan_execute_oc_nw.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 3
    rng = np.random.default_rng(seed)
    n, m = ls.n, ls.m
    Pd, Ad = ls.dense(b)
    Pd = np.triu(Pd) + np.triu(Pd, 1).T
    rho = rng.choice([0.1, 100.0, 1e-6], size=m); sigma = 1e-6
    M = Pd + sigma * np.eye(n) + Ad.T @ (rho[:, None] * Ad)
    rhs = rng.normal(size=n); sol = np.zeros(n); info = np.zeros(8, np.int64)
    Pv = np.ascontiguousarray(ls.P[b]); Av = np.ascontiguousarray(ls.A[b])
    if nw == 4:
        rc = L.plan_execute_oc(n, m, _p(ls.Pp), _p(ls.Pi), _p(ls.Ap), _p(ls.Ai), NG, NH, ldl, _p(Pv), _p(Av), _p(rho), C.c_double(sigma), _p(rhs), _p(sol), _p(info))
    else:
        rc = L.plan_execute_oc_nw(n, m, _p(ls.Pp), _p(ls.Pi), _p(ls.Ap), _p(ls.Ai), 8, NG, NH, ldl, 0, _p(Pv), _p(Av), _p(rho), C.c_double(sigma), _p(rhs), _p(sol), _p(info))
    err = None
    if rc == 0:
        ref = np.linalg.solve(M, rhs)
        err = np.abs(sol - ref).max() / np.abs(ref).max()
    return rc, err, dict(nbc=info[0], has_hub=info[1], junc=info[2], nlds=info[3], lds=info[5])


@pytest.mark.parametrize("ldl", [0, 1])
@pytest.mark.parametrize("name,N,nw,inst", [("quadrotor", 10, 4, (5, 0)), ("quadrotor", 10, 8, (7, 0)), ("quadrotor", 20, 4, (5, 0)),
                                            ("quadrotor", 50, 8, (7, 0)), ("cartpole", 100, 8, (4, 0))])
def test_onchip_emulation_of_the_presolved_pattern(built, name, N, nw, inst, ldl):
    """two chains meeting in their last element (quadrotor) or one chain (cart-pole), no hub phases"""
    m, ls, red = patterns(name, N)
    rc, err, info = _emulate(red, nw, *inst, ldl)
    assert rc == 0, (rc, info)
    assert err < BOUND, err
    assert info["has_hub"] == 0 and info["nbc"] == (N - 1 if name == "quadrotor" else 31) and info["lds"] <= 160 * 1024


@pytest.mark.parametrize("ldl", [0, 1])
def test_cartpole_n30_inner_pattern_runs_on_the_family_it_is_given(built, rule_defaults, ldl):
    """n = 145: the selection rule gives it variant 4 and the on-chip plan refuses it (rc 5) in both emulation entries -- never mis-executes it;
    the plan of the family it runs on solves it at the bound"""
    m, ls, red = patterns("cartpole", 30)
    assert select(red, 8192)[1]["variant"] < 200
    for nw, inst in ((4, (5, 0)), (8, (4, 0)), (8, (7, 0))):
        assert _emulate(red, nw, *inst, ldl)[0] == 5
    L = C.CDLL(SO)
    rng = np.random.default_rng(ldl)
    n, mm, b = red.n, red.m, 1
    Pd, Ad = red.dense(b)
    Pd = np.triu(Pd) + np.triu(Pd, 1).T
    rho = rng.choice([0.1, 100.0, 1e-6], size=mm); sigma = 1e-6
    M = Pd + sigma * np.eye(n) + Ad.T @ (rho[:, None] * Ad)
    rhs = rng.normal(size=n); xin = rng.normal(size=n); win = rng.normal(size=mm)
    sol = np.zeros(n); Ax = np.zeros(mm); Atw = np.zeros(n); Px = np.zeros(n)
    Pv = np.ascontiguousarray(red.P[b]); Av = np.ascontiguousarray(red.A[b])
    rc = L.plan_execute(n, mm, _p(red.Pp), _p(red.Pi), _p(red.Ap), _p(red.Ai), -1, _p(Pv), _p(Av), _p(rho), C.c_double(sigma),
                        _p(rhs), _p(sol), _p(xin), _p(win), _p(Ax), _p(Atw), _p(Px))
    assert rc == 0
    ref = np.linalg.solve(M, rhs)
    assert np.abs(sol - ref).max() / np.abs(ref).max() < BOUND
    assert np.abs(Ax - Ad @ xin).max() / np.abs(Ad @ xin).max() < 1e-13


@pytest.mark.parametrize("name,N", [("quadrotor", 10), ("cartpole", 30), ("double_integrator", 20)])
def test_full_tracking_pattern_through_the_generic_plan(built, name, N):
    """the full form (what a handle without presolve gets): ordering, assembly and factor plan against dense linear algebra"""
    m, ls, red = patterns(name, N)
    L = C.CDLL(SO)
    info = np.zeros(8, np.int64); pos = np.zeros(ls.n, np.int32)
    assert L.plan_describe(ls.n, ls.m, _p(ls.Pp), _p(ls.Pi), _p(ls.Ap), _p(ls.Ai), -1, _p(info), _p(pos)) == 0
    assert sorted(pos.tolist()) == list(range(ls.n))
    rng = np.random.default_rng(2)
    n, mm, b = ls.n, ls.m, 1
    Pd, Ad = ls.dense(b)
    Pd = np.triu(Pd) + np.triu(Pd, 1).T
    rho = rng.choice([0.1, 100.0, 1e-6], size=mm); sigma = 1e-6
    M = Pd + sigma * np.eye(n) + Ad.T @ (rho[:, None] * Ad)
    rhs = rng.normal(size=n); xin = rng.normal(size=n); win = rng.normal(size=mm)
    sol = np.zeros(n); Ax = np.zeros(mm); Atw = np.zeros(n); Px = np.zeros(n)
    Pv = np.ascontiguousarray(ls.P[b]); Av = np.ascontiguousarray(ls.A[b])
    assert L.plan_execute(n, mm, _p(ls.Pp), _p(ls.Pi), _p(ls.Ap), _p(ls.Ai), -1, _p(Pv), _p(Av), _p(rho), C.c_double(sigma),
                          _p(rhs), _p(sol), _p(xin), _p(win), _p(Ax), _p(Atw), _p(Px)) == 0
    ref = np.linalg.solve(M, rhs)
    assert np.abs(sol - ref).max() / np.abs(ref).max() < BOUND
