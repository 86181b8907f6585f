"""CPU: stage data -- the generated source (unchanged without data; the host build of a data functor against the NumPy statement), the pattern of a
data model against its constants-baked twin, the refusals, the exported symbols, the properties of the statement (models.StageOCP.set_stage_data,
shift_stage_data), and the inputs the GPU tests rely on (tests/support/stage_data_cases.py)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mpcqp_stage_data_count", "mpcqp_stage_set_stage_data", "mpcqp_stage_shift_data")
TOL = 1e-12

# sha256 of codegen's device and host source at commit d7e05e5 (the parent of stage data), for three models without nsd.  The device text up to the
# launchers -- the functor, its tables and the descriptive exports; the launchers themselves have since become one per operation (STAGE_ABI_VERSION 8)
PARENT_SOURCE = {
    "plain_pendulum": ("48872b73ab86c62599bbffce4b4cfd3c6ef2fd7799c29216c23644fc66b999cd", "f88fcf7e6e913feb594afe5c7d43d180b6cc4f3f69f5f23965e72202d4adbffc"),
    "param_pendulum": ("4ee6e62730d624944a16ddcf78d2ed796e7059984dda26a8cc4d69d86f33c8bd", "805bfb358df263f25c86cd6d4eea42185356da50e2191f498b5acea0125f4db5"),
    "cartpole_general_link": ("cc4ad6b04ad11f901e3567c2c03dd1da210890079ae4078ef57f6bf2cf4c4266", "b8cd110ee308e8d871fc0898e3e597a862a3d429be5bf0a85f38b62b026f9566"),
}


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _close(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin]) and bool((np.abs(a[fin] - b[fin]) <= TOL * np.maximum(1.0, np.abs(b[fin]))).all())


@pytest.mark.parametrize("name", sorted(PARENT_SOURCE))
def test_source_without_data_is_the_parents(name):
    tape = sdc.trace_of(sdc.plain_models()[name])
    dev, host = codegen.device_source(tape), codegen.host_source(tape)
    head = dev[:dev.index("int mpcqp_user_eval(")]
    assert (hashlib.sha256(head.encode()).hexdigest(), hashlib.sha256(host.encode()).hexdigest()) == PARENT_SOURCE[name]
    for word in ("nsd", "sdata", "StageData", "_sd("):
        assert word not in dev and word not in host, word


def test_source_with_data():
    for kind, pp in (("pendulum3", False), ("theta3", True), ("tracking3", False)):
        src = codegen.device_source(sdc.trace_of(sdc.model(kind)))
        for word in ("static constexpr int nsd = 2;", "static constexpr double sdata0[2] = {0.4, 1.3};", "SmUser_sdata0[]", "mpcqp_user_nsd", "mpcqp_user_sdata0",
                     "H(const T *s, const T *u, const double *d, T *out)",
                     "LG(const T *s, const T *u, const T *r, const double *d, T *out)", "d[0]", "d[1]"):
            assert word in src, (kind, word)
        assert ("static constexpr int ntheta" in src) == ("mpcqp_user_ntheta" in src) == pp, kind
        # the instances that take the data rows, with the parameter rows in front only in a library that has both: only the combinations the model needs
        got = ki.kernel_instances(codegen.build_device_library(sdc.trace_of(sdc.model(kind))))
        pf = kind == "tracking3"
        assert {n for n in got if n.split("_kernel<")[0] in ("stage_eval", "stage_merit", "stage_advance", "stage_linesearch")} \
            == ki.four(pf, "StageData") | (ki.four(pf, "StageTheta", "StageData") if pp else set()), (kind, sorted(got))
    plain = ki.kernel_instances(codegen.build_device_library(sdc.trace_of(sdc.plain_models()["plain_pendulum"])))
    assert ki.four(False) <= plain and not [n for n in plain if "StageTheta" in n or "StageData" in n], sorted(plain)
    src =codegen.device_source(sdc.trace_of(sdc.model("path3")))
    assert "has_cost = 0" in src and "d[0]" in src and "d[1]" not in src


@pytest.mark.parametrize("kind", ["pendulum3", "tracking3", "path3"])
def test_host_build_matches_the_statement(kind):
    """H, dH and the cost's value, gradient and Hessian of the host build with a data row, against the statement (complex step) at one frame"""
    m = sdc.model(kind)
    L = C.CDLL(codegen.build_host_library(sdc.trace_of(m)))
    assert L.user_host_nsd() == 2
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d0 = np.zeros(2); L.user_host_sdata0(vp(d0))
    assert _bits(d0, m.sdata)
    rng = np.random.default_rng(11)
    one = sdc.make(type(m), 2)                        # two frames: frame 0 takes lcost, frame 1 lterm
    for trial in range(4):
        d = m.sdata + rng.normal(0.0, 0.4, 2) if trial else m.sdata.copy()
        x = rng.normal(0.0, 0.6, size=(1, one.nvar)); p = rng.normal(0.0, 0.3, size=(1, one.np))
        one.set_stage_data(np.tile(d, (1, 2, 1)))
        s, u = one.frames(x)
        h_ref = one.path_values(x).reshape(2, 1); dh_ref = one.dh(s, u)[0]
        out = np.zeros(1); jac = np.zeros(3)
        for k in range(2):
            L.user_host_path_d(vp(s[0, k].copy()), vp(u[0, k].copy()), vp(d), vp(out), vp(jac))
            assert _close(out, h_ref[k]) and _close(jac, dh_ref[k].ravel()), (kind, trial, k)
            if trial == 0:                            # the defaults are what the form without the row uses
                o2 = np.zeros(1); j2 = np.zeros(3)
                L.user_host_path(vp(s[0, k].copy()), vp(u[0, k].copy()), vp(o2), vp(j2))
                assert _bits(o2, out) and _bits(j2, jac)
        if one.general_cost:
            grad, hess = one.cost_derivatives(p, x)
            val = one._cost_eval(one._ltape, one._lttape, one._cost_inputs(p, x))[0]
            r = p.reshape(1, 2, 2) if one.pref else np.broadcast_to(p[:, None, :], (1, 2, 2))
            for k in range(2):
                v = np.zeros(1); g = np.zeros(5); H = np.zeros(25)
                L.user_host_cost_d(vp(s[0, k].copy()), vp(u[0, k].copy()), vp(r[0, k].copy()), vp(d), k, vp(v), vp(g), vp(H))
                assert _close(v, val[0, k:k + 1]) and _close(g, grad[0, k]) and _close(H.reshape(5, 5), hess[0, k]), (kind, trial, k)
        else:
            assert L.user_host_has_cost() == 0
        one.set_stage_data(None)


@pytest.mark.parametrize("kind", sdc.KINDS)
def test_pattern_and_sizes_are_those_of_the_baked_twin(kind):
    m, t = sdc.model(kind), sdc.model(kind, twin=True)
    assert m.nsd == 2 and t.nsd == 0
    assert (m.n, m.m, m.np, m.ng, m.nvar) == (t.n, t.m, t.np, t.ng, t.nvar)
    for k in ("Pp", "Pi", "Ap", "Ai"):
        assert np.array_equal(getattr(m, k), getattr(t, k)), (kind, k)
    ta, tb = sdc.trace_of(m), sdc.trace_of(t)
    if m.general_cost:
        assert np.array_equal(ta.cost["mask"], tb.cost["mask"]) and ta.cost["mask"].shape == (5, 5)
    # and with the defaults in force the data model computes what the twin computes (not bit for bit: the twin folds its constants)
    c = sdc.kernel_case(kind)
    a = sdc.statement(c, "local_system", d=None)
    if c["theta"] is not None:
        t.set_instance_params(c["theta"])
    b = t.local_system(c["p"], c["x"], c["lbx"], c["ubx"], c["lbg"], c["ubg"])
    for k in ("P", "q", "A", "l", "u"):
        assert _close(getattr(a, k), getattr(b, k)), (kind, k)


def test_refusals():
    for cls, word in ((sdc.SdataInF, "F reads self.sdata"), (sdc.SdataInK, "kfun reads self.sdata"), (sdc.SdataInLink, "llink reads self.sdata")):
        bad = sdc.make(cls, 3)
        with pytest.raises(ValueError, match=word):
            sdc.trace_of(bad)
        assert _bits(bad.sdata, sdc.DataPendulum.sdata)             # the model's values are back in place after the refused trace
    bad = sdc.make(sdc.ThetaInPathData, 3)
    with pytest.raises(ValueError, match="hfun reads self.theta"):
        sdc.trace_of(bad)
    from tests.support import instance_params_cases as ipc
    bad = ipc.param_pendulum(cls=ipc.ThetaInPath)
    with pytest.raises(ValueError, match="hfun reads self.theta"):
        codegen.trace(bad.F, bad.nx, bad.nu, bad.hfun, 1, bad.h_lo, bad.h_hi, ntheta=2)
    m = sdc.model("pendulum3")
    with pytest.raises(ValueError, match="at most 8"):
        codegen.trace(m.F, m.nx, m.nu, nsd=9, sdata0=np.zeros(9))

    class TooMany(sdc.DataPendulum):
        nsd = 9; sdata = np.zeros(9)
    with pytest.raises(ValueError, match="at most 8"):
        sdc.make(TooMany, 3)
    for shape in ((2, 3), (2, 4, 2), (2, 3, 3), (0, 3, 2)):
        with pytest.raises(ValueError, match="expected an array"):
            m.set_stage_data(np.zeros(shape))
    with pytest.raises(ValueError, match="no stage data"):
        models.DoubleIntegrator(3).set_stage_data(np.zeros((2, 3, 1)))
    with pytest.raises(ValueError, match="no stage data are stored"):
        m.shift_stage_data()
    m.set_stage_data(np.tile(m.sdata, (2, 3, 1)))
    x = np.zeros((3, m.nvar)); p = np.zeros((3, m.np))
    for call in (lambda: m.path_values(x), lambda: m.objective(p, x), lambda: m.violation(x, x, x)):
        with pytest.raises(ValueError, match="larger than the stored"):
            call()                                                  # three instances, two stored
    assert m.path_values(x[:1]).shape == (1, 3)                     # a smaller batch uses the first rows
    m.set_stage_data(None)


def test_header_exports_and_library_agree(built):
    hdr = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"int mpcqp_stage_data_count\(const mpcqp_stage \*s\);", hdr)
    assert re.search(r"int mpcqp_stage_set_stage_data\(mpcqp_stage \*s, int batch, const double \*d, int mem\);", hdr)
    assert re.search(r"int mpcqp_stage_shift_data\(mpcqp_stage \*s, int batch, const double \*d_new( /\*[^/]*\*/)?, void \*stream\);", hdr)
    assert re.search(r"#define MPCQP_STAGE_MAXSD 8\b", hdr)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    for e in ENTRIES:
        assert e in _lib.EXPORTS and re.search(r" T %s$" % e, syms, re.M), e


@pytest.mark.parametrize("kind", sdc.KINDS)
def test_statement_properties(kind):
    """the defaults tiled = the unset model; instance b alone with its rows = row b of the batch run; both bit for bit, in every method"""
    c = sdc.kernel_case(kind)
    mdl = c["model"]
    B = sdc.BATCH
    tiled = np.tile(np.asarray(mdl.sdata, float), (B, mdl.N, 1))
    mu0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])

    def everything(d, idx=None):
        ls = sdc.statement(c, "local_system", d=d, idx=idx)
        f, g = sdc.statement(c, "merit", d=d, idx=idx)
        se = sdc.statement(c, "line_search", d=d, idx=idx, mu=(mu0 if idx is None else mu0[idx]).copy())
        adv = sdc.statement(c, "advance", d=d, idx=idx)
        out = {k: getattr(ls, k) for k in ("P", "q", "A", "l", "u")}
        out.update(f=f, g=g, **{"ls_" + k: se[k] for k in ("x", "alpha", "step_max", "f", "gmax", "phi", "mu")},
                   **{"adv_" + k: adv[k] for k in ("x", "lbx", "ubx", "applied", "dw", "y", "stage_cost")})
        return out
    unset, explicit, batch = everything(None), everything(tiled), everything("case")
    for k in unset:
        assert _bits(unset[k], explicit[k]), (kind, k)
    assert not _bits(batch["A"], unset["A"]) and not _bits(batch["l"], unset["l"])
    if mdl.general_cost:
        assert not _bits(batch["P"], unset["P"]) and not _bits(batch["adv_stage_cost"], unset["adv_stage_cost"])
    for b in range(B):
        one = everything("case", idx=slice(b, b + 1))
        for k in one:
            assert _bits(one[k], batch[k][b:b + 1]), (kind, b, k)
    fresh = sdc.model(kind)                             # a model that never had the call
    if c["theta"] is not None:
        fresh.set_instance_params(c["theta"])
    a = fresh.local_system(c["p"], c["x"], c["lbx"], c["ubx"], c["lbg"], c["ubg"])
    assert all(_bits(getattr(a, k), unset[k]) for k in ("P", "q", "A", "l", "u"))


def test_shift_statement():
    m = sdc.model("pendulum2")
    rng = np.random.default_rng(5)
    d = rng.normal(size=(3, 2, 2)); dn = rng.normal(size=(3, 2))
    m.set_stage_data(d)
    m.shift_stage_data()
    assert _bits(m._sdata_rows, np.stack([d[:, 1], d[:, 1]], axis=1)) and _bits(m._sdata_rows, sdc.shift_reference(d))
    m.shift_stage_data(dn)
    assert _bits(m._sdata_rows, np.stack([d[:, 1], dn], axis=1))
    x = rng.normal(size=(3, m.nvar))
    h = m.path_values(x)
    s, u = m.frames(x)
    assert _bits(h[:, 0], (s[:, 0, 0] - d[:, 1, 0]) ** 2 + 0.5 * u[:, 0, 0]) and _bits(h[:, 1], (s[:, 1, 0] - dn[:, 0]) ** 2 + 0.5 * u[:, 1, 0])
    m.set_stage_data(None)
    assert m._sdata_rows is None


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("kind", sdc.KINDS)
def test_the_data_matter_in_the_statement(kind):
    """the two instances of the GPU `matters` test differ by more than 1e-3 in A, l and u"""
    mdl, d, p, x, lbx, ubx, lbg, ubg = sdc.matters_case(kind)
    mdl.set_stage_data(d)
    try:
        ls = mdl.local_system(p, x, lbx, ubx, lbg, ubg)
    finally:
        mdl.set_stage_data(None)
    for k in ("A", "l", "u"):
        assert sdc.gap(getattr(ls, k)[0], getattr(ls, k)[1]) > 1e-3, (kind, k)
    blk = mdl._A_blk.ravel()
    assert _bits(ls.A[0, blk], ls.A[1, blk])                        # the dynamics take no data


@pytest.mark.parametrize("kind", sdc.KINDS)
def test_line_search_inputs_have_no_undecided_instance(kind):
    c = sdc.kernel_case(kind)
    for K in (1, 4):
        out = sdc.statement(c, "line_search", candidates=K)
        assert not lc.undecided(out).any(), (kind, K)


def test_obstacle_recipe_is_solved_on_the_oracle():
    """pins the inputs of the GPU loop test: every QP of the recipe ends solved on the CPU oracle, with and without the search, no decision of the
    search sits on its threshold, and the discs matter: the four instances end on different paths"""
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, d, arg, x0 = sdc.recipe()
    B = d.shape[0]
    for search in (False, True):
        sol, log = sdc.host_loop(mdl, d, arg, x0, OracleCuCaQP(batch=B, nthreads=4), line_search=search)
        assert all((it["status"] == 1).all() for it in log), [it["status"] for it in log]
        if search:
            assert not any(lc.undecided(it["ls"]).any() for it in log)
    Y = log[-1]["x"].reshape(B, mdl.N, mdl.f)[:, :, 1]
    print(Y[:, mdl.N // 2])
    assert np.abs(Y[0] - Y[-1]).max() > 1e-2
