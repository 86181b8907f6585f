"""CPU: the cases of tests/support/reduced_cases.py are what tests/test_gpu_reduced_general.py takes them for.

The 60-digit restatement of the reduced form against the NumPy statement problems.reduce_qp; every built QP's x*, y* as a KKT point at 60 digits; the
planted pattern features; and the conditions under which the GPU module's bars cannot pass by accident: the dropped objective constant is large, every
correction map (qc, lc, yp, ya of csrc/reduced.hpp) is exercised by non-zero values, the status recipes reach their status on the oracle for the reduced and the
full QP, and the chosen seeds leave no instance out of the iteration-count comparison.
"""
import numpy as np
import pytest

from tests.support import problems
from tests.support import reduced_cases as rc

U = 2.0 ** -53


@pytest.mark.parametrize("name", rc.CASES + ("all_fixed",))
def test_restatement_against_the_numpy_statement(built, name):
    """patterns and value gathers equal; q_r, l_r, u_r and x_f to the rounding of reduce_qp's float64 sums: (k + 1) 2^-53 sum|terms| with k <= nfix + 1 terms,
    the sum of absolute values bounded by (k + 1) (1 + |ref|_inf) max(1, |x_f|_inf)"""
    c = rc.case(name)
    R = rc.Restated(c.ls, c.fixed_rows)
    red = R.reduced_system()
    ref, free, kept, fvars, xfix = problems.reduce_qp(c.ls, c.fixed_rows)
    assert sorted(R.free) == list(free) and sorted(R.kept) == list(kept) and R.fvars == list(fvars)
    for k in ("Pp", "Pi", "Ap", "Ai", "P", "A"):
        assert np.array_equal(getattr(red, k), getattr(ref, k)), k
    xf = np.array([[float(v) for v in r] for r in R.xf])
    assert np.abs(xf - xfix).max() <= 2 * U * np.abs(xfix).max()
    k = len(c.fixed_rows) + 1
    for key in ("q", "l", "u"):
        got, want = getattr(red, key), getattr(ref, key)
        fin = np.abs(want) < rc.INF
        assert np.array_equal(got[~fin], want[~fin]), key                      # an infinite bound stays what it was, whatever its spelling
        bar = (k + 1) ** 2 * U * (1.0 + np.abs(want[fin]).max()) * max(1.0, np.abs(xfix).max())
        err = np.abs(got[fin] - want[fin]).max()
        print("%s %s: restated against NumPy %.3e (bar %.3e)" % (name, key, err, bar))
        assert err <= bar, (name, key, err, bar)


@pytest.mark.parametrize("name", rc.CASES + ("all_fixed",))
def test_the_chosen_point_is_the_kkt_point(built, name):
    """x*, y* on the ROUNDED QP at 60 digits: stationarity to the rounding of q (2^-53 |q|_inf, doubled), feasibility to the rounding of the bounds, every
    multiplier's sign backed by an active bound of that side; strict complementarity as the module docstring states it"""
    c = rc.case(name)
    kv = rc.kkt_violation(c)
    fin = lambda a: np.abs(a[np.abs(a) < rc.INF]).max()
    bq, bl = 2 * U * np.abs(c.ls.q).max(), 2 * U * max(fin(c.ls.l), fin(c.ls.u))
    print("%s: stationarity %.3e (bar %.3e), feasibility %.3e (bar %.3e), sign violations %.1e" % (name, kv[:, 0].max(), bq, kv[:, 1].max(), bl, kv[:, 2].max()))
    assert kv[:, 0].max() <= bq and kv[:, 1].max() <= bl and kv[:, 2].max() == 0.0
    act = c.ystar != 0
    assert np.abs(c.ystar[act]).min() >= 0.3
    for i1, i2 in c.dup:
        act[:, i2] = True          # (the second singleton: an equality that carries no multiplier, see the support module)
    Ax = np.array([c.ls.dense(b)[1] @ c.xstar[b] for b in range(c.ls.batch)])
    assert (np.minimum(Ax - c.ls.l, c.ls.u - Ax)[~act] >= 0.49).all()
    assert np.abs(c.xstar[:, rc.Restated(c.ls, c.fixed_rows).fvars]).min() >= 0.3          # the fixed values: non-zero


def test_general_patterns_hold_what_they_are_meant_to(built):
    """between them (here: each of them) the general cases contain every feature the GPU module's docstring lists"""
    for name in rc.GENERAL:
        c = rc.case(name); ls = c.ls; R = rc.restated(name)
        fx = set(R.fvars)
        cols = np.repeat(np.arange(ls.n), np.diff(ls.Pp))
        up = [(int(i), int(j)) for i, j in zip(ls.Pi, cols) if i <= j]
        assert any(i == j and i in fx for i, j in up)                                       # a fixed variable with a diagonal entry
        assert any(i in fx and j not in fx for i, j in up) and any(i not in fx and j in fx for i, j in up)      # fixed - free, as row and as column
        assert any(i != j and i in fx and j in fx for i, j in up)                           # fixed - fixed off the diagonal
        assert c.rows["f_nop"] in fx and not any(c.rows["f_nop"] in e for e in zip(ls.Pi.tolist(), cols.tolist()))
        _, Ad = ls.dense(0)
        nz = lambda i: set(np.flatnonzero(Ad[i]).tolist())
        assert len(nz(c.rows["two_fixed"]) & fx) == 2 and nz(c.rows["two_fixed"]) - fx
        assert nz(c.rows["only_fixed"]) <= fx and len(nz(c.rows["only_fixed"])) == 2
        s = c.rows["shifted"]
        assert all(nz(i) & fx and nz(i) - fx for i in s)
        assert (ls.l[:, s[0]] == -np.inf).all() and (ls.u[:, s[1]] == np.inf).all() and (ls.l[:, s[2]] == -1e30).all() and (ls.u[:, s[3]] == 1e30).all()
        assert np.isfinite(ls.u[:, s[0]]).all() and np.isfinite(ls.l[:, s[1]]).all() and (np.abs(ls.u[:, s[2]]) < 1e3).all() and (np.abs(ls.l[:, s[3]]) < 1e3).all()
        assert sorted(set(np.round(np.abs(ls.A[0, R.fsrc]), 6))) == sorted(set(abs(a) for a in rc.COEFFS))
        assert c.find_all
        if c.rows["second"] is not None:
            i2 = c.rows["second"]
            assert nz(i2) == {R.fvars[2]} and (ls.l[:, i2] == ls.u[:, i2]).all() and i2 in R.kept and c.dup == ((2, i2),)
    assert sum(rc.case(n).rows["second"] is not None for n in rc.GENERAL) >= 1
    for name in rc.STAGE:
        c = rc.case(name)
        assert c.find_all and len(c.fixed_rows) == c.mdl.np + c.mdl.f
    a = rc.case("all_fixed")
    assert len(rc.found_rows(a.ls)) == 2 and a.ls.n == 3          # (three rows pin the three variables; the rule keeps one variable)


@pytest.mark.parametrize("name", rc.CASES)
def test_conditions(built, name):
    """the dropped objective constant against the obj bar; every correction map multiplies non-zero values; no instance left out of the iteration counts"""
    c = rc.case(name); ls = c.ls
    R, R0 = rc.restated(name), rc.Restated(c.ls, c.fixed_rows, zero_xf=True)
    red = R.reduced_system()
    # the objective's constant: at least 1e-2 (1 + |obj|), against a bar of 1e-6 (1 + |obj|)
    const = rc.dropped_constant(ls, R)
    obj = rc.objective_and_residuals(ls, c.xstar, c.ystar, np.zeros_like(c.ystar))["obj"]
    print("%s: dropped constant %s, objective %s" % (name, np.array2string(const, precision=2), np.array2string(obj, precision=2)))
    assert (np.abs(const) >= 1e-2 * (1.0 + np.abs(obj))).all()
    # qc, lc: q_r and the shift of the bounds with x_f against x_f = 0, over 1e3 times the parity bar 1e-6 (1 + |ref|_inf) of what they feed
    f = lambda rows: np.array([[float(v) for v in r] for r in rows])
    dq = np.abs(f(R.qr) - f(R0.qr)).max(axis=1); dl = np.abs(f(R.shift)).max(axis=1)
    lr = f(R.lr); fin = np.abs(lr) < rc.INF
    print("%s: q_r moves by %.2e, the bounds by %.2e without x_f" % (name, dq.min(), dl.min()))
    assert (dq > 1e3 * 1e-6 * (1.0 + np.abs(f(R.qr)).max())).all() and (dl > 1e3 * 1e-6 * (1.0 + np.abs(lr[fin]).max())).all()
    # yp, ya: the multipliers of the eliminated rows at (x*, y*) move by far more than their rounding bar when x_f (yp), or y on the kept rows (ya), is zero
    xr, yr = c.xstar[:, R.free], c.ystar[:, R.kept]
    zr = np.zeros_like(yr)
    _, Y, _, mag, cnt = R.expand(xr, yr, zr); _, Y0, _, _, _ = R0.expand(xr, yr, zr); _, Ya, _, _, _ = R.expand(xr, np.zeros_like(yr), zr)
    for b in range(ls.batch):
        bar = np.array([4 * (k + 2) * U * float(m) for k, m in zip(cnt[b], mag[b])])
        dyp = np.array([abs(float(Y[b][i] - Y0[b][i])) for i in R.fixed_rows]); dya = np.array([abs(float(Y[b][i] - Ya[b][i])) for i in R.fixed_rows])
        assert (dyp > 1e3 * bar).sum() >= 0.8 * len(bar) and (dya > 1e3 * bar).sum() >= len(bar) / 3, (name, b, dyp / bar, dya / bar)
        err = max(abs(float(Y[b][i]) - c.ystar[b, i]) for i in R.fixed_rows)          # ... and the restated stationarity gives y* back
        assert err <= 1e3 * bar.max(), (name, b, err)
    # iteration counts: the chosen seeds leave no instance out
    assert problems.oracle_stable_mask(red).all()          # (the default-tolerance run: the one whose counts are compared)
    q2, l2, u2 = rc.new_pinned_values(name)
    red2 = rc.Restated(rc.with_vectors(ls, q=q2, l=l2, u=u2), c.fixed_rows).reduced_system()
    ok1, ok2 = _kept_stable(red, red2)
    assert ok1.all() and ok2.all()


def _kept_stable(red, red2, draws=3):
    """problems.oracle_stable_mask for the pair of solves of a kept workspace whose second solve has new q, l, u"""
    from oracle import oracle as orc

    def run(P, A, q, qq):
        st = orc.State(orc.Pattern(red.n, red.m, red.Pp, red.Pi, red.Ap, red.Ai), red.batch, orc.default_settings())
        return st.solve(P, q, A, red.l, red.u, nthreads=8), st.solve_vectors(qq, red2.l, red2.u, nthreads=8)
    ref = run(red.P, red.A, red.q, red2.q)
    assert (ref[0]["status"] == 1).all() and (ref[1]["status"] == 1).all(), (ref[0]["status"], ref[1]["status"])          # (the new pinned values leave every instance solvable)
    rng = np.random.default_rng(99)
    ok = [np.ones(red.batch, bool), np.ones(red.batch, bool)]
    for _ in range(draws):
        P, A, q, qq = (a * (1.0 + 1e-12 * rng.standard_normal(a.shape)) for a in (red.P, red.A, red.q, red2.q))
        got = run(P, A, q, qq)
        for k in (0, 1):
            ok[k] &= (got[k]["iters"] == ref[k]["iters"]) & (got[k]["status"] == ref[k]["status"])
    return ok


@pytest.mark.parametrize("name", rc.CASES)
def test_measured_optimum_distance(built, name):
    """the table the GPU module takes its optimum bar from (10 x) is what the oracle's full-form solve gives here, to a factor 2"""
    dx, dy = rc.measure_optimum_distance(name)
    tx, ty = rc.OPTIMUM_DISTANCE[name]
    print("%s: oracle full form at eps 1e-9: |x - x*| %.3e (table %.3e), |y - y*| %.3e (table %.3e)" % (name, dx, tx, dy, ty))
    assert tx / 2 <= dx <= 2 * tx and ty / 2 <= dy <= 2 * ty


@pytest.mark.parametrize("kind", rc.STATUS_KINDS)
@pytest.mark.parametrize("name", ("g1", "di20"))
def test_status_recipes(built, name, kind):
    """every recipe reaches its status on the oracle, for the reduced QP and for the full QP, next to healthy neighbours whose counts are stable"""
    c = rc.case(name)
    ls, st, want = rc.status_batch(name, kind)
    full = problems.oracle_solve(ls, nthreads=8, **st)
    others = np.arange(ls.batch) != rc.SPOILT
    print("%s %s: full %s" % (name, kind, full["status"].tolist()))
    assert (full["status"][others] == 1).all()
    if kind == "promise_open":          # a valid QP: the full form solves it, the reduced form has no statement of it
        assert full["status"][rc.SPOILT] == 1
        return
    assert full["status"][rc.SPOILT] == want
    if kind == "promise_crossed":
        return
    red = rc.Restated(ls, c.fixed_rows).reduced_system()
    r = problems.oracle_solve(red, nthreads=8, **st)
    print("%s %s: reduced %s iters %s" % (name, kind, r["status"].tolist(), r["iters"].tolist()))
    assert r["status"][rc.SPOILT] == want and (r["status"][others] == 1).all()
    assert problems.oracle_stable_mask(red, **st).all()
    assert np.array_equal(np.isnan(r["x"]).all(axis=1), np.isnan(full["x"]).all(axis=1))
