"""CPU: transition data -- the stage data in F / cdyn, kfun and llink (models.StageOCP.transition_data).  The generated source (unchanged
without the flag: hashes and kernel instances of the parent commit; the signatures and the host build of a flagged functor against the NumPy
statement), the pattern of a flagged model against its constants-baked twin, the properties of the statement, the refusals, and the inputs the GPU
tests rely on (tests/support/transition_data_cases.py).  The bar is that of tests/test_stage_data_host.py: 1e-12 max(1, |ref|), bits where nothing is
computed differently."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, codegen, models
from tests.support import kernel_instances as ki
from tests.support import linesearch_cases as lc
from tests.support import stage_data_cases as sdc
from tests.support import transition_data_cases as tdc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12

# sha256 of codegen's device source (up to mpcqp_user_eval, as tests/test_stage_data_host.py pins it) and host source at commit 3fcff66, the parent
# of transition data, for the three plain models of stage_data_cases and its data models without the flag
PARENT_SOURCE = {
    "plain_pendulum": ("48872b73ab86c62599bbffce4b4cfd3c6ef2fd7799c29216c23644fc66b999cd", "f88fcf7e6e913feb594afe5c7d43d180b6cc4f3f69f5f23965e72202d4adbffc"),
    "param_pendulum": ("4ee6e62730d624944a16ddcf78d2ed796e7059984dda26a8cc4d69d86f33c8bd", "805bfb358df263f25c86cd6d4eea42185356da50e2191f498b5acea0125f4db5"),
    "cartpole_general_link": ("cc4ad6b04ad11f901e3567c2c03dd1da210890079ae4078ef57f6bf2cf4c4266", "b8cd110ee308e8d871fc0898e3e597a862a3d429be5bf0a85f38b62b026f9566"),
    "pendulum3": ("95f02f31f80f3fb15a156a0aa50e5fc212963859a38d05e6f9642d0b6704b161", "de0fbdb3f938809b64ff00bc645d33f7ecc0752c903d98f49bc77e6de168c405"),
    "theta3": ("9e86bf7654de0589dda4cbc5bb237142fb32c96aa900edb4712d817aa922387b", "39029b67b802b9971b28bbe426bce21a590d00d026b6dfb36b8c4a8c593bfa46"),
    "tracking3": ("5b78e18f72c22338b7aee0a24062caa83f1827c1de9f97cda97b91933ad41ffe", "1b3dcf0965733129cadec2b9c853da107905b5e076825208418d7f1696d873de"),
}
# the stage_*_kernel instances of those libraries at the parent (nm -C): (per-frame references, the trailing packs)
PARENT_KERNELS = {
    "plain_pendulum": (False, [()]), "param_pendulum": (False, [(), ("StageTheta",)]), "cartpole_general_link": (False, [()]),
    "pendulum3": (False, [("StageData",)]), "theta3": (False, [("StageData",), ("StageTheta", "StageData")]), "tracking3": (True, [("StageData",)]),
}


def _instances(pf, packs):
    out = set()
    for pack in packs:
        out |= ki.four(pf, *pack) | {"stage_rollout_kernel<%s>" % ", ".join(("SmUser",) + pack)}
    return out


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _close(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))).all())


# ------------------------------------------------------------------------------------------------ the source
@pytest.mark.parametrize("name", sorted(PARENT_SOURCE))
def test_source_without_the_flag_is_the_parents(name):
    tape = sdc.trace_of(tdc.flagless_models()[name])
    dev, host = codegen.device_source(tape), codegen.host_source(tape)
    head = dev[:dev.index("int mpcqp_user_eval(")]
    assert (hashlib.sha256(head.encode()).hexdigest(), hashlib.sha256(host.encode()).hexdigest()) == PARENT_SOURCE[name]
    for word in ("tdata", "transition_data", "_d("):
        assert word not in dev and word not in host.replace("user_host_path_d(", "").replace("user_host_cost_d(", "").replace("host_cost_d(", ""), word
    got = {n for n in ki.kernel_instances(codegen.build_device_library(tape)) if n.startswith("stage_")}
    assert got == _instances(*PARENT_KERNELS[name]), sorted(got)


def test_source_with_the_flag():
    for kind in ("pendulum3", "theta3", "tracking3", "fonly3", "exact3"):
        m = tdc.model(kind)
        tape = tdc.trace_of(m)
        dev, host = codegen.device_source(tape), codegen.host_source(tape)
        par = "par" if m.ntheta else ""
        words = ["static constexpr int tdata = 1;", "int mpcqp_user_transition_data() { return SmUser::tdata; }",
                 "F(const double *%s, double, const T *s, const T *u, const double *d, T *out)" % par,
                 "K(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out)"]
        if m.link_cost:
            words += ["LK(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out)",
                      "LKG(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out)"]
        if m.exact_hessian:
            words.append("FG(const double *%s, double, const T *s, const T *u, const double *lam, const double *d, T *out)" % par)
        for w in words:
            assert w in dev and (w in host or w.startswith("int mpcqp_user")), (kind, w)
        for w in ("user_host_transition_data", "user_host_eval_d(", "user_host_link_d(") + (("user_host_link_cost_d(",) if m.link_cost else ()):
            assert w in host and w not in dev, (kind, w)
        # a node of data and constants only is a plain double (the step's half in the RK4), as for par[i]
        assert re.search(r"const double w\d+ = 0\.5 \* d\[0\];", dev), kind
        assert "STAGE_ABI_VERSION" in dev and "#define STAGE_ABI_VERSION 8" in open(os.path.join(codegen.CSRC, "stage_kernels.hpp")).read()
    # the flag changes no size, mask or bound of the traced model
    a, b = tdc.trace_of(tdc.model("pendulum3")), tdc.trace_of(tdc.model("pendulum3", twin=True))
    assert np.array_equal(a.cost["mask"], b.cost["mask"]) and np.array_equal(a.link_cost["mask"], b.link_cost["mask"]) and (a.k_lo, a.k_hi) == (b.k_lo, b.k_hi)


@pytest.mark.parametrize("kind", ["pendulum3", "theta3", "fonly3", "exact3"])
def test_host_build_matches_the_statement(kind):
    """dynamics with Jacobian, link rows, link cost with gradient and Hessian and the curvature of the host build with a data row, against the
    statement (complex step) on the one transition of a two-frame model; the defaults handed over as a row give the bits of the forms without one"""
    m = tdc.model(kind)
    L = C.CDLL(codegen.build_host_library(tdc.trace_of(m)))
    assert L.user_host_transition_data() == 1 and L.user_host_nsd() == 2
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(23)
    one = tdc.make(type(m), 2)
    nx, f = one.nx, one.f
    for trial in range(4):
        d = np.asarray(m.sdata) * rng.uniform(0.6, 1.6, 2) if trial else np.asarray(m.sdata, float).copy()
        th = np.asarray(m.theta) * rng.uniform(0.7, 1.4, 2) if m.ntheta else None
        x = rng.normal(0.0, 0.6, size=(1, one.nvar))
        rows = np.stack([d, d + 7.0])[None]              # frame 1's row is never read by the transition 0 -> 1
        one.set_stage_data(rows)
        if th is not None:
            one.set_instance_params(th[None])
        try:
            s, u = one.frames(x)
            s0, u0, s1, u1 = s[0, 0].copy(), u[0, 0].copy(), s[0, 1].copy(), u[0, 1].copy()
            ls = one.local_system(np.zeros((1, one.np)), x, x, x, np.zeros((1, one.ng)), np.zeros((1, one.ng)))
            F_ref = s1 + ls.l[0, one.n:one.n + nx]       # l = lbg - (s_1 - F)
            J_ref = -ls.A[0, one._A_blk[0]]
            out = np.zeros(nx); jac = np.zeros(nx * f)
            L.user_host_eval_d(vp(th), vp(s0), vp(u0), vp(d), vp(out), vp(jac))
            assert _close(out, F_ref) and _close(jac.reshape(nx, f), J_ref), (kind, trial)
            if trial == 0 and th is None:
                o2 = np.zeros(nx); j2 = np.zeros(nx * f)
                L.user_host_eval(vp(s0), vp(u0), vp(o2), vp(j2))
                assert _bits(o2, out) and _bits(j2, jac)
            if one.nk:
                k_ref = one.link_values(x)[0]; dk_ref = one.dk(s[:, :1], u[:, :1], s[:, 1:], u[:, 1:])[0, 0]
                ko = np.zeros(one.nk); kj = np.zeros(one.nk * 2 * f)
                L.user_host_link_d(vp(s0), vp(u0), vp(s1), vp(u1), vp(d), vp(ko), vp(kj))
                assert _close(ko, k_ref) and _close(kj.reshape(one.nk, 2 * f), dk_ref), (kind, trial)
                if trial == 0:
                    k2 = np.zeros(one.nk); kj2 = np.zeros(one.nk * 2 * f)
                    L.user_host_link(vp(s0), vp(u0), vp(s1), vp(u1), vp(k2), vp(kj2))
                    assert _bits(k2, ko) and _bits(kj2, kj)
            if one.link_cost:
                v_ref = one.link_cost_values(x)[0]; g_ref, H_ref = one.link_cost_derivatives(x)
                v = np.zeros(1); g = np.zeros(2 * f); H = np.zeros(4 * f * f)
                L.user_host_link_cost_d(vp(s0), vp(u0), vp(s1), vp(u1), vp(d), vp(v), vp(g), vp(H))
                assert _close(v, v_ref) and _close(g, g_ref[0, 0]) and _close(H.reshape(2 * f, 2 * f), H_ref[0, 0]), (kind, trial)
                if trial == 0:
                    v2 = np.zeros(1); g2 = np.zeros(2 * f); H2 = np.zeros(4 * f * f)
                    L.user_host_link_cost(vp(s0), vp(u0), vp(s1), vp(u1), vp(v2), vp(g2), vp(H2))
                    assert _bits(v2, v) and _bits(g2, g) and _bits(H2, H)
            if one.exact_hessian:
                y = rng.normal(0.0, 1.0, size=(1, one.m))
                C_ref = one.constraint_curvature(x, y)[0, 0]
                lam = y[0, one.n:one.n + nx].copy(); mu = y[0, one.n + one.ngd:one.n + one.ngd + one.nh].copy()
                Cv = np.zeros(f * f)
                L.user_host_curvature(vp(th), vp(s0), vp(u0), vp(lam), vp(mu), vp(d), 1, vp(Cv))
                assert _close(Cv.reshape(f, f), C_ref), (kind, trial)
                other = np.zeros(f * f)
                L.user_host_curvature(vp(th), vp(s0), vp(u0), vp(lam), vp(mu), vp(d * 1.3), 1, vp(other))
                assert np.abs(other - Cv).max() > 1e-3           # the curvature depends on the row
        finally:
            one.set_stage_data(None)
            if th is not None:
                one.set_instance_params()


# ------------------------------------------------------------------------------------------------ pattern and sizes
@pytest.mark.parametrize("kind", tdc.KINDS)
def test_pattern_and_sizes_are_those_of_the_baked_twin(kind):
    m, t = tdc.model(kind), tdc.model(kind, twin=True)
    assert m.nsd == 2 and m.transition_data and t.nsd == 0 and not t.transition_data
    assert (m.n, m.m, m.np, m.ng, m.nvar) == (t.n, t.m, t.np, t.ng, t.nvar)
    for k in ("Pp", "Pi", "Ap", "Ai"):
        assert np.array_equal(getattr(m, k), getattr(t, k)), (kind, k)
    c = tdc.kernel_case(kind)
    a = tdc.statement(c, "local_system", d=None)
    if c["theta"] is not None:
        t.set_instance_params(c["theta"])
    b = t.local_system(c["p"], c["x"], c["lbx"], c["ubx"], c["lbg"], c["ubg"])
    for k in ("P", "q", "A", "l", "u"):
        assert _close(getattr(a, k), getattr(b, k)), (kind, k)
    # rollout with constant rows is the twin's rollout
    ra = tdc.statement(c, "rollout", d=tdc.constant_rows(c["model"]))
    rb = t.rollout(c["x"], c["lbx"], c["ubx"])
    assert _close(ra["x"], rb["x"]) and np.array_equal(ra["diverged"], rb["diverged"]), kind


# ------------------------------------------------------------------------------------------------ the statement
def _everything(c, d, idx=None):
    mu0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])
    ls = tdc.statement(c, "local_system", d=d, idx=idx)
    f, g = tdc.statement(c, "merit", d=d, idx=idx)
    se = tdc.statement(c, "line_search", d=d, idx=idx, mu=(mu0 if idx is None else mu0[idx]).copy())
    out = {k: getattr(ls, k) for k in ("P", "q", "A", "l", "u")}
    out.update(f=f, g=g, **{"ls_" + k: se[k] for k in ("x", "alpha", "step_max", "f", "gmax", "phi", "mu")})
    for tail in ("rollout", "repeat"):
        adv = tdc.statement(c, "advance", d=d, idx=idx, tail=tail)
        out.update({"adv_%s_%s" % (tail, k): adv[k] for k in ("x", "lbx", "ubx", "applied", "dw", "y", "stage_cost")})
    for inputs in ("iterate", "hold"):
        out["roll_" + inputs] = tdc.statement(c, "rollout", d=d, idx=idx, inputs=inputs)["x"]
    if c["model"].exact_hessian:
        P = ls.P
        out["lag"] = tdc.statement(c, "lagrangian", d=d, idx=idx, P=P)[0]
        out["lag_project"] = tdc.statement(c, "lagrangian", d=d, idx=idx, P=P, mode="project")[0]
    return out


@pytest.mark.parametrize("kind", tdc.KINDS)
def test_statement_properties(kind):
    """rows equal to the defaults = no stored set; instance b alone with its rows = row b of the batch run; both bit for bit, in every method"""
    c = tdc.kernel_case(kind)
    mdl = c["model"]
    unset, explicit, batch = _everything(c, None), _everything(c, tdc.constant_rows(mdl)), _everything(c, "case")
    for k in unset:
        assert _bits(unset[k], explicit[k]), (kind, k)
    blk = mdl._A_blk.ravel()
    assert not _bits(batch["A"][:, blk], unset["A"][:, blk]) and not _bits(batch["roll_iterate"], unset["roll_iterate"])
    for b in range(tdc.BATCH):
        one = _everything(c, "case", idx=slice(b, b + 1))
        for k in one:
            assert _bits(one[k], batch[k][b:b + 1]), (kind, b, k)


@pytest.mark.parametrize("kind", tdc.KINDS)
def test_the_data_matter_in_the_statement(kind):
    """two instances that differ in their rows only differ by more than 1e-3 in the dynamics blocks of A and in the dynamics rows of l and u"""
    mdl, d, p, x, lbx, ubx, lbg, ubg = tdc.matters_case(kind)
    mdl.set_stage_data(d)
    try:
        ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
    finally:
        mdl.set_stage_data(None)
    blk = mdl._A_blk.ravel(); rows = tdc.dynamics_rows(mdl)
    assert tdc.gap(ls.A[0, blk], ls.A[1, blk]) > 1e-3, kind
    assert tdc.gap(ls.l[0, rows], ls.l[1, rows]) > 1e-3 and tdc.gap(ls.u[0, rows], ls.u[1, rows]) > 1e-3, kind


@pytest.mark.parametrize("kind", ["pendulum2", "pendulum3", "theta3"])
def test_advance_reads_rows_0_and_last(kind):
    """each row perturbed alone: row 0 moves the plant step only, row N-1 the rollout tail only, a row between them nothing"""
    c = tdc.kernel_case(kind)
    mdl = c["model"]
    N, nx, f = mdl.N, mdl.nx, mdl.f
    base = tdc.statement(c, "advance")["x"].reshape(tdc.BATCH, N, f)
    for k in range(N):
        d = c["d"].copy(); d[:, k, 0] *= 1.5; d[:, k, 1] += 0.3
        got = tdc.statement(c, "advance", d=d)["x"].reshape(tdc.BATCH, N, f)
        plant = not _bits(got[:, 0, :nx], base[:, 0, :nx]); tail = not _bits(got[:, N - 1, :nx], base[:, N - 1, :nx])
        assert (plant, tail) == (k == 0, k == N - 1), (kind, k)
        if k == 0:
            assert tdc.gap(got[:, 0, :nx], base[:, 0, :nx]) > 1e-3
        if k == N - 1:
            assert tdc.gap(got[:, N - 1, :nx], base[:, N - 1, :nx]) > 1e-3
        assert _bits(got[:, :, nx:], base[:, :, nx:]) and _bits(got[:, 1:N - 1], base[:, 1:N - 1])
    # the rollout takes row k at step k: perturbing row k alone leaves the states up to k as they were and moves state k + 1
    roll = tdc.statement(c, "rollout")["x"].reshape(tdc.BATCH, N, f)
    for k in range(N - 1):
        d = c["d"].copy(); d[:, k, 0] *= 1.5
        got = tdc.statement(c, "rollout", d=d)["x"].reshape(tdc.BATCH, N, f)
        assert _bits(got[:, :k + 1], roll[:, :k + 1]) and tdc.gap(got[:, k + 1, :nx], roll[:, k + 1, :nx]) > 1e-4, (kind, k)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(ValueError, match="transition_data needs stage data"):
        tdc.make(tdc.FlagWithoutData, 3)
    m = tdc.model("pendulum3")
    with pytest.raises(ValueError, match="transition_data needs stage data"):
        codegen.trace(m.F, m.nx, m.nu, transition_data=True)
    # a model without the flag is refused as before (beside tests/test_stage_data_host.py::test_refusals, which holds the three messages)
    bad = tdc.make(tdc.Flagless, 3)
    with pytest.raises(ValueError, match="F reads self.sdata: stage data are supported in hfun, lcost and lterm only"):
        tdc.trace_of(bad)
    assert _bits(bad.sdata, tdc.TdPendulum.sdata)
    for cls, word in ((sdc.SdataInF, "F reads self.sdata"), (sdc.SdataInK, "kfun reads self.sdata"), (sdc.SdataInLink, "llink reads self.sdata")):
        with pytest.raises(ValueError, match=word + ": stage data are supported in hfun, lcost and lterm only"):
            sdc.trace_of(sdc.make(cls, 3))
    # shift_data=False with d_new: refused before anything else of the tick (no device is needed to see it)
    from optimal_control_problem_amd.mpc import ClosedLoopMPC
    loop = object.__new__(ClosedLoopMPC)
    loop.shift_data = False
    with pytest.raises(ValueError, match="d_new with shift_data=False"):
        loop.tick(d_new=np.zeros((1, 2)))
    # theta in hfun stays refused with the flag

    class ThetaInPath(tdc.ThetaTdPendulum):
        def hfun(self, s, u):
            return np.stack([self.theta[0] * s[..., 0] + self.sdata[1] * u[..., 0]], axis=-1)
    with pytest.raises(ValueError, match="hfun reads self.theta"):
        tdc.trace_of(tdc.make(ThetaInPath, 3))


def test_header_exports_and_library_agree(built):
    hdr = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"int mpcqp_stage_has_transition_data\(const mpcqp_stage \*s\);", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    assert "mpcqp_stage_has_transition_data" in _lib.EXPORTS and re.search(r" T mpcqp_stage_has_transition_data$", syms, re.M)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("kind", tdc.KINDS)
def test_line_search_inputs_have_no_undecided_instance(kind):
    c = tdc.kernel_case(kind)
    for K in (1, 4):
        out = tdc.statement(c, "line_search", candidates=K)
        assert not lc.undecided(out).any(), (kind, K)


def test_grid_recipe_is_solved_on_the_oracle():
    """pins the inputs of the GPU loop test: every QP of the non-uniform-grid recipe ends solved on the CPU oracle, with and without the search, no
    decision of the search sits on its threshold, and the grid matters: the uniform grid of the same first step ends elsewhere"""
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, d, arg, x0 = tdc.recipe()
    B = d.shape[0]
    assert np.allclose(d[0, :, 0], tdc.RECIPE_H0 * tdc.RECIPE_GROWTH ** np.arange(mdl.N)) and d[0, -1, 0] > 5 * d[0, 0, 0]
    for search in (False, True):
        sol, log = tdc.host_loop(mdl, d, arg, x0, OracleCuCaQP(batch=B, nthreads=4), line_search=search)
        assert all((it["status"] == 1).all() for it in log), [it["status"] for it in log]
        if search:
            assert not any(lc.undecided(it["ls"]).any() for it in log)
    uni = models.GridCartPole(mdl.N, tdc.RECIPE_H0, 1.0)
    _, ulog = tdc.host_loop(uni, uni.grid_rows(B), arg, x0, OracleCuCaQP(batch=B, nthreads=4))
    assert np.abs(ulog[-1]["x"] - log[-1]["x"]).max() > 1e-2
