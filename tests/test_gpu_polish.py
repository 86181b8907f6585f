"""Solution polishing on the GPU (mpcqp_set_polish; csrc/kernel_polish.hpp) against the dense reference tests/support/polish_ref.py.

Bars.  The reference polish, fed the oracle's ADMM output, reaches |x - x*| <= 1.9e-9, |y - y*| <= 2.9e-7 and residuals <= 1e-10 on the golden
fixtures it accepts (tests/test_polish_reference.py prints them).  The kernel does the same arithmetic in Ruiz-scaled space with blocked explicit
16 x 16 inverses; two orders of margin are left for that: |x - x*| <= 1e-7, |y - y*| <= 1e-5, host-recomputed residuals <= 1e-8.  ADMM alone at the
tolerances used here is >= 1e-5 on every multi-stage problem, so none of the bars is met without the polish.  Where the acceptance rule takes a
candidate built on a wrong active set (random_3) the comparison is with the reference's candidate, 1e-6 relative.
Measured maxima are recorded in DESIGN.md section 6.7."""
import os
import subprocess

import numpy as np
import pytest

from optimal_control_problem_amd import _lib, models
from tests.support import golden, polish_ref as pr, problems

pytestmark = pytest.mark.gpu

RES_TOL, X_TOL, Y_TOL, CAND_RTOL = 1e-8, 1e-7, 1e-5, 1e-6
KEYS = ("x", "y", "z", "status", "iters", "obj", "prim_res", "dual_res", "rho")


def _run(ls, polish=None, **settings):
    """one handle, one solve; polish: None = never touched, False = switched on and off again, True / dict(delta=, refine_iter=) = on"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **settings)
    if polish is False:
        qp.set_polish(True); qp.set_polish(False)
    elif polish:
        qp.set_polish(True, **(polish if isinstance(polish, dict) else {}))
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); got = qp.get()
    info = qp.plan_info(); qp.close()
    return got, info


def _same_bits(a, b, keys=KEYS, rows=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), k


def _reference(ls, base, rows=None, **kw):
    """the reference polish fed the GPU's own pre-polish result, per instance"""
    out = {}
    for b in (range(ls.batch) if rows is None else rows):
        P, A, q, l, u = pr.dense_qp(ls, b)
        out[b] = pr.polish_ref(P, A, q, l, u, base["x"][b], base["y"][b], base["z"][b], base["prim_res"][b], base["dual_res"][b],
                               status=int(base["status"][b]), **kw)
    return out


def _host_residuals(ls, got, b):
    return pr.residuals(*pr.dense_qp(ls, b), got["x"][b], got["y"][b])


def _check_against_reference(ls, got, base, ref, tag, residual_bar=True):
    """decision equal for every instance; unpolished instances bitwise the ADMM result; accepted ones at the residual bar (candidates the reference
    itself leaves with a large residual: compared with its candidate).  Returns the measured maxima."""
    worst = dict(res=0.0, cand=0.0)
    for b, r in ref.items():
        assert got["polish_status"][b] == r["status"], (tag, b, got["polish_status"][b], r["status"], got["polish_info"][b], r["pri"], r["dua"])
        assert got["status"][b] == base["status"][b] and got["iters"][b] == base["iters"][b] and np.array_equal(got["rho"][b], base["rho"][b], equal_nan=True)
        if r["status"] != pr.SUCCESS:
            _same_bits(got, base, rows=b)
            continue
        cand = np.abs(got["x"][b] - r["x"]).max() / (1.0 + np.abs(r["x"]).max())
        worst["cand"] = max(worst["cand"], cand)
        if max(r["pri"], r["dua"]) < 1e-9:
            pri, dua = _host_residuals(ls, got, b)
            worst["res"] = max(worst["res"], pri, dua)
            if residual_bar:
                assert pri <= RES_TOL and dua <= RES_TOL, (tag, b, pri, dua)
                assert abs(got["prim_res"][b] - pri) <= 1e-9 and abs(got["dual_res"][b] - dua) <= 1e-9      # info[1..2] are the candidate's
        if not residual_bar or max(r["pri"], r["dua"]) >= 1e-9:
            assert cand <= CAND_RTOL, (tag, b, cand)
    print("%s: host-recomputed residual max %.3e, |x - x_ref| rel max %.3e, accepted %d of %d" % (
        tag, worst["res"], worst["cand"], sum(r["status"] == pr.SUCCESS for r in ref.values()), len(ref)))
    return worst


# ---------------------------------------------------------------------------------------------- 1. golden fixtures
@pytest.mark.parametrize("name", golden.NAMES)
def test_golden_fixtures_polished(built, name):
    fx = golden.load()[name]; ls = fx["ls"]
    got, _ = _run(ls, polish=True)
    base, _ = _run(ls, polish=False)
    fresh, _ = _run(ls)
    _same_bits(base, fresh)
    assert "polish_status" not in base and "polish_status" in got
    ref = _reference(ls, base)
    _check_against_reference(ls, got, base, ref, name)
    for b, r in ref.items():
        if r["status"] == pr.SUCCESS and max(r["pri"], r["dua"]) < 1e-9:
            ex, ey = np.abs(got["x"][b] - fx["x_star"][b]).max(), np.abs(got["y"][b] - fx["y_star"][b]).max()
            print("%s[%d]: |x - x*| %.3e (ADMM %.3e)  |y - y*| %.3e" % (name, b, ex, np.abs(base["x"][b] - fx["x_star"][b]).max(), ey))
            assert ex <= X_TOL and ey <= Y_TOL, (name, b, ex, ey)
    if name == "cartpole":
        assert (got["polish_status"] == _lib.POLISH_FAILED).all()
    if name == "random_3":
        assert (got["polish_status"] == _lib.POLISH_SUCCESS).all() and max(max(r["pri"], r["dua"]) for r in ref.values()) > 1e-4


# ---------------------------------------------------------------------------------------------- 2. every kernel family
FAMILIES = {"stream": 0, "res1": 1, "res2": 2, "res4": 4, "res8": 8, "gres4": 104, "gres2": 102, "oc4": 204}


@pytest.mark.parametrize("variant", list(FAMILIES))
@pytest.mark.parametrize("name,eps", [("quadrotor", 1e-4), ("double_integrator", 1e-5)])
def test_polish_on_every_kernel_family(built, monkeypatch, variant, name, eps):
    """every family leaves the scaled A, A', P, l, u, D, E the polish reads in its slab"""
    monkeypatch.setenv("MPCQP_VARIANT", variant)
    _, ls, _ = models.make_workload(name, 64)
    got, info = _run(ls, polish=True, eps_abs=eps, eps_rel=eps)
    assert info["variant"] == FAMILIES[variant]
    base, _ = _run(ls, eps_abs=eps, eps_rel=eps)
    ref = _reference(ls, base)
    _check_against_reference(ls, got, base, ref, "%s/%s" % (variant, name))
    assert (got["polish_status"] == _lib.POLISH_SUCCESS).sum() >= 0.9 * ls.batch      # (so that this cannot pass with polishing silently failing)


@pytest.mark.parametrize("name,B,N,pairs", [("quadrotor", 12, 50, 1), ("cartpole", 6, 100, 2)])
def test_polish_on_the_eight_wave_and_dissected_plans(built, monkeypatch, name, B, N, pairs):
    """the eight-wave on-chip instances, plain (quadrotor N = 50) and in the dissected order (cart-pole N = 100): decision and candidate as the reference's"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    monkeypatch.setenv("MPCQP_VARIANT", "oc8")
    _, ls, _ = models.make_workload(name, B, N=N)
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai); oc = qp.oc_info(); qp.close()
    assert (oc["chain_pairs"] > 1) == (pairs > 1)
    got, info = _run(ls, polish=True)
    assert info["variant"] == 208
    base, _ = _run(ls)
    _check_against_reference(ls, got, base, _reference(ls, base), "oc8/%s N=%d" % (name, N), residual_bar=False)


# ---------------------------------------------------------------------------------------------- 3. off means off
def test_off_means_off(built):
    _, ls, _ = models.make_workload("quadrotor", 48)
    fresh, _ = _run(ls)
    toggled, _ = _run(ls, polish=False)
    _same_bits(fresh, toggled)
    on, _ = _run(ls, polish=True)
    for k in ("status", "iters", "rho"):
        assert np.array_equal(on[k], fresh[k])
    kept = on["polish_status"] != _lib.POLISH_SUCCESS
    print("quadrotor x 48, default tolerance: %d accepted, %d kept" % ((~kept).sum(), kept.sum()))
    assert (~kept).any()
    if kept.any():
        _same_bits(on, fresh, rows=np.nonzero(kept)[0])
    changed = np.nonzero(~kept)[0]
    assert all(not np.array_equal(on["x"][b], fresh["x"][b]) for b in changed)


# ---------------------------------------------------------------------------------------------- 4. not performed
def test_not_performed(built):
    fxs = golden.load()
    for name in ("primal_infeasible", "dual_infeasible", "testcpp_case8"):
        ls = fxs[name]["ls"]
        got, _ = _run(ls, polish=True); base, _ = _run(ls)
        assert (got["status"] != 1).all() and (got["polish_status"] == _lib.POLISH_NOT_PERFORMED).all()
        assert np.isnan(got["x"]).all()
        _same_bits(got, base)
    mdl, ls, _ = models.make_workload("double_integrator", 24)
    l = ls.l.copy(); u = ls.u.copy(); bad = np.array([3, 10]); l[bad, mdl.n + 5] = 1.0; u[bad, mdl.n + 5] = -1.0
    crossed = models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, ls.P, ls.q, ls.A, l, u)
    got, _ = _run(crossed, polish=True)
    assert (got["status"][bad] == 11).all() and (got["polish_status"][bad] == _lib.POLISH_NOT_PERFORMED).all() and np.isnan(got["x"][bad]).all()
    ok = np.setdiff1d(np.arange(ls.batch), bad)
    assert (got["polish_status"][ok] != _lib.POLISH_NOT_PERFORMED).all()
    got, _ = _run(ls, polish=True, max_iter=25, eps_abs=1e-9, eps_rel=1e-9)
    assert (got["status"] == 7).all() and (got["polish_status"] == _lib.POLISH_NOT_PERFORMED).all()


# ---------------------------------------------------------------------------------------------- 5. kept workspace
@pytest.mark.parametrize("variant,name,B,N", [("res4", "double_integrator", 24, 20), ("oc4", "quadrotor", 10, 20)])
def test_kept_workspace_survives_the_polish(built, monkeypatch, variant, name, B, N):
    """the polish factor lives in scratch of its own: the factor a kept workspace parks in the slab serves the next solve, whose status and
    iteration counts are the oracle's solve_vectors (as in test_gpu_parity.py::test_kept_workspace_vectors_vs_oracle)"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    from oracle import oracle as orc
    monkeypatch.setenv("MPCQP_VARIANT", variant)
    mdl, ls, meta = models.make_workload(name, B, N=N)
    st = orc.State(orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai), B, orc.default_settings())
    qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
    qp.keep_workspace(True); qp.set_polish(True)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); g1 = qp.get(); r1 = st.solve(ls.P, ls.q, ls.A, ls.l, ls.u)
    assert np.array_equal(g1["status"], r1["status"]) and np.array_equal(g1["iters"], r1["iters"])
    assert (g1["polish_status"] == _lib.POLISH_SUCCESS).any()
    rng = np.random.default_rng(11)
    frame0 = meta["frame0"].copy(); frame0[:, :mdl.nx] += rng.normal(0, 0.05, (B, mdl.nx))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    ls2 = mdl.local_system(meta["p"] + 0.1, meta["x_iterate"], lbx, ubx, lbg, ubg)
    qp.update_vectors(ls2.q, ls2.l, ls2.u); qp.solve(); g2 = qp.get(); qp.close()
    r2 = st.solve_vectors(ls2.q, ls2.l, ls2.u)
    assert np.array_equal(g2["status"], r2["status"]) and np.array_equal(g2["iters"], r2["iters"])
    ok = g2["polish_status"] == _lib.POLISH_SUCCESS
    assert ok.any()
    for b in np.nonzero(ok)[0]:
        pri, dua = _host_residuals(ls2, g2, b)
        assert pri <= RES_TOL and dua <= RES_TOL


# ---------------------------------------------------------------------------------------------- 6. mpcqp_solve_host
def test_solve_host_with_polish_equals_update_solve_get(built):
    from optimal_control_problem_amd.batch_qp import BatchQP
    _, ls, _ = models.make_workload("quadrotor", 100)
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai); qp.set_polish(True)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); ref = qp.get()
    assert (ref["polish_status"] == _lib.POLISH_SUCCESS).any()
    for chunks in (0, 7):
        out = qp.solve_host(ls.P, ls.q, ls.A, ls.l, ls.u, chunks=chunks)
        for k in ("x", "y", "status", "iters"):
            assert np.array_equal(out[k], ref[k], equal_nan=True), (chunks, k)
        after = qp.get()
        _same_bits(after, ref, keys=KEYS + ("polish_status", "polish_info"))
    qp.close()


# ---------------------------------------------------------------------------------------------- 7. reduced handle
def test_presolved_handle_forwards_the_polish(built):
    from optimal_control_problem_amd.batch_qp import BatchQP
    _, ls, _ = models.make_workload("quadrotor", 32)
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, presolve_bounds=(ls.l, ls.u))
    assert qp.nfixed > 0
    qp.set_polish(True)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); got = qp.get(); qp.close()
    ok = got["polish_status"] == _lib.POLISH_SUCCESS
    print("presolved quadrotor x 32: %d accepted" % ok.sum())
    assert ok.sum() >= 16
    worst = 0.0
    for b in np.nonzero(ok)[0]:
        pri, dua = _host_residuals(ls, got, b)
        worst = max(worst, pri, dua)
        assert pri <= RES_TOL and dua <= RES_TOL, (b, pri, dua)
    print("presolved: full-size host-recomputed residual max %.3e" % worst)


# ---------------------------------------------------------------------------------------------- 8. warm start
def test_polished_point_as_warm_start_ends_at_the_first_check(built):
    from optimal_control_problem_amd.batch_qp import BatchQP
    _, ls, _ = models.make_workload("quadrotor", 32)
    got, _ = _run(ls, polish=True)
    ok = got["polish_status"] == _lib.POLISH_SUCCESS
    assert ok.sum() >= 16
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, warm_start=1)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.warm_start(got["x"], got["y"]); qp.solve(); again = qp.get(); qp.close()
    assert (again["status"][ok] == 1).all() and (again["iters"][ok] == qp.settings.check_termination).all(), again["iters"]


# ---------------------------------------------------------------------------------------------- 9. C++ facade
def test_cpp_cucaqp_set_polish(built, tmp_path):
    """cpp/CuCaQP.hpp: setPolish(true) survives the handle re-creation in initSolver; one golden fixture against x_star"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fx = golden.load()["double_integrator"]; ls = fx["ls"]
    arr = lambda a, fmt: "{" + ", ".join(fmt % v for v in np.asarray(a).ravel()) + "}"
    src = tmp_path / "polish_cpp_test.cpp"
    src.write_text("""
#include <cmath>
#include <cstdio>
#include <vector>
#include "CuCaQP.hpp"
int main() {
  const int n = %d, m = %d;
  std::vector<int> Pp = %s, Pi = %s, Ap = %s, Ai = %s;
  std::vector<double> P = %s, q = %s, A = %s, l = %s, u = %s, xs = %s;
  CuCaQP qp;
  qp.setPolish(true);
  if (qp.getPolishStatus() != 0) return 2;
  if (!qp.setDimension(n, m)) return 3;
  for (int round = 0; round < 2; round++) {      // (the second round goes through setSystem + initSolver again)
    qp.setSystem(CuCaQP::CscView{n, n, Pp.data(), Pi.data(), P.data()}, q.data(), CuCaQP::CscView{m, n, Ap.data(), Ai.data(), A.data()}, l.data(), u.data());
    if (!qp.initSolver() || !qp.solve()) return 4;
    if (qp.getPolishStatus() != 1) { std::printf("polish status %%d\\n", qp.getPolishStatus()); return 5; }
    const std::vector<double> &x = qp.getSolutionVector();
    double err = 0.0;
    for (int j = 0; j < n; j++) err = std::fmax(err, std::fabs(x[j] - xs[j]));
    std::printf("round %%d: |x - x*| = %%.3e\\n", round, err);
    if (!(err <= 1e-7)) return 6;
  }
  qp.setPolish(false);
  qp.setSystem(CuCaQP::CscView{n, n, Pp.data(), Pi.data(), P.data()}, q.data(), CuCaQP::CscView{m, n, Ap.data(), Ai.data(), A.data()}, l.data(), u.data());
  if (!qp.initSolver() || !qp.solve() || qp.getPolishStatus() != 0) return 7;
  return 0;
}
""" % (ls.n, ls.m, arr(ls.Pp, "%d"), arr(ls.Pi, "%d"), arr(ls.Ap, "%d"), arr(ls.Ai, "%d"), arr(ls.P[0], "%.17g"), arr(ls.q[0], "%.17g"),
       arr(ls.A[0], "%.17g"), arr(np.maximum(ls.l[0], -1e30), "%.17g"), arr(np.minimum(ls.u[0], 1e30), "%.17g"), arr(fx["x_star"][0], "%.17g")))
    exe = tmp_path / "polish_cpp_test"
    pkg = os.path.join(root, "optimal_control_problem_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "include"), "-I", os.path.join(pkg, "cpp"), "-o", str(exe), str(src),
                           "-L", pkg, "-lmpcqp", "-Wl,-rpath," + pkg])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------- 10. full size
def test_full_size_quadrotor_polished(built):
    from optimal_control_problem_amd.batch_qp import BatchQP
    B = 8192
    _, ls, _ = models.make_workload("quadrotor", B)
    qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai); qp.set_polish(True)
    qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); got = qp.get()
    ms, pms = qp.last_kernel_ms(), qp.last_polish_ms()
    qp.solve(); second = qp.get(); qp.close()                 # (the second solve dispatches longest-first: another order)
    qn = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai); qn.set_polish(True); qn.set_dispatch_hint(False)
    qn.update(ls.P, ls.q, ls.A, ls.l, ls.u); qn.solve(); qn.solve(); plain = qn.get(); qn.close()
    _same_bits(got, second, keys=KEYS + ("polish_status", "polish_info"))
    _same_bits(got, plain, keys=KEYS + ("polish_status", "polish_info"))
    ps = got["polish_status"]
    assert np.isin(ps, (_lib.POLISH_SUCCESS, _lib.POLISH_FAILED, _lib.POLISH_LINSYS_ERROR)).all() and (got["status"] == 1).all()
    sample = np.arange(0, B, B // 256)
    base, _ = _run(problems.take(ls, sample))
    ref = _reference(problems.take(ls, sample), base)
    ref_frac = np.mean([r["status"] == pr.SUCCESS for r in ref.values()])
    frac = (ps == _lib.POLISH_SUCCESS).mean()
    print("quadrotor x %d: solve %.2f ms + polish %.2f ms, accepted %.2f %% (reference on 256: %.2f %%)" % (B, ms, pms, 100 * frac, 100 * ref_frac))
    assert frac >= ref_frac - 0.02
    worst = 0.0
    for b in sample[::4]:
        if ps[b] == _lib.POLISH_SUCCESS:
            pri, dua = _host_residuals(ls, got, b)
            worst = max(worst, pri, dua)
            assert pri <= RES_TOL and dua <= RES_TOL, (b, pri, dua)
    print("full size: host-recomputed residual max %.3e on %d sampled instances" % (worst, len(sample[::4])))


def test_polish_example_runs(built):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "polish_qp.py"), "128"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "polishing on" in r.stdout and "polished" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
