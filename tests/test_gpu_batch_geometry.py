"""GPU: the NLP-side kernels at batches that cross every launch boundary (cases, tiling and the restated launch arithmetic in
tests/support/geometry_cases.py, whose claims tests/test_batch_geometry_host.py checks on the CPU).

Every case is launched once at its own batch -- the launch tests/test_gpu_nlp_hp.py and its siblings hold to 1e-12 against their references -- and
then tiled to every batch of geometry_cases.BATCHES: instance b of the tiled launch is base instance idx[b].  Assertions, all bit for bit (bytes
compared, so NaN patterns count): row b of every output is row idx[b] of the base launch -- including what a kernel must leave alone: the NaN prefill
of an instance without a point, its x and mu, touched = 0, P where no frame is touched; every buffer a kernel writes is [B + 2, width] with a guard
row on either side that still holds its fill afterwards.  Three rows of the largest launch are also held to the 60-digit reference of their base
instance (hp_cases.TOL; convexify_cases.bar behind the eigen-solve), so that a failure names the kernel and not the tiling.  Then the state a handle
keeps between launches: one evaluator through the batches 5, 1031, 64, 1, 257.  Each test prints its largest measured distance."""
import contextlib

import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import convexify_cases as cc
from tests.support import geometry_cases as gc
from tests.support import hp_cases as hc
from tests.support import nlp_hp as hp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL = {np.dtype(np.float64): np.nan, np.dtype(np.int32): -99}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _i32(a):
    return None if a is None else _dev(a, torch.int32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class _Guarded:
    """the buffers a launch writes: [B + 2, ...] filled with NaN (int32: -99), the kernel gets the contiguous rows 1 .. B"""

    def __init__(self, B):
        self.B, self.bufs = B, {}

    def new(self, name, *width, init=None, dtype=np.float64):
        host = np.full((self.B + 2,) + tuple(width), FILL[np.dtype(dtype)], dtype)
        if init is not None:
            host[1:-1] = init
        full = torch.from_numpy(host).cuda()
        self.bufs[name] = full
        view = full[1:self.B + 1]
        assert view.is_contiguous() and view.shape[0] == self.B
        return view

    def collect(self):
        """{name: rows 1 .. B on the host}; both guard rows of every buffer still hold their fill"""
        out = {}
        for name, full in self.bufs.items():
            h = full.cpu().numpy()
            guard = np.full_like(h[:1], FILL[h.dtype])
            assert _same(h[:1], guard) and _same(h[-1:], guard), "guard row of %s written" % name
            out[name] = h[1:-1]
        return out


@contextlib.contextmanager
def _rows(ev, c, plant=False):
    """the case's parameter and stage-data rows on a stage evaluator for the duration of a block"""
    stage = hasattr(ev, "set_stage_data")
    try:
        if stage and c["d"] is not None:
            ev.set_stage_data(c["d"])
        if stage and c["theta"] is not None:
            ev.set_instance_params(c["theta"])
            if plant and c["plant"] is not None:
                ev.set_instance_params(c["plant"], plant=True)
        yield ev
    finally:
        if stage and c["d"] is not None:
            ev.set_stage_data(None)
        if stage and c["theta"] is not None:
            ev.set_instance_params(None)
            if plant and c["plant"] is not None:
                ev.set_instance_params(None, plant=True)


# ------------------------------------------------------------------------------------------------ one launch of every operation
def _system(ev, c, g):
    out = {k: g.new(k, w) for k, w in (("P", ev.nnzP), ("q", ev.n), ("A", ev.nnzA), ("l", ev.m), ("u", ev.m))}
    ev.eval(*[_dev(c[k]) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")], out=out)
    return out


def _op_eval(ev, c, g):
    _system(ev, c, g)


def _op_merit(ev, c, g):
    B = g.B
    f, gm = g.new("f"), g.new("gmax")
    p, x = _dev(c["p"]), _dev(c["x"])
    if hasattr(ev, "set_stage_data"):
        _lib.check(_lib.lib().mpcqp_stage_merit(ev._h, B, p.data_ptr(), x.data_ptr(), f.data_ptr(), gm.data_ptr(), None))
    else:
        lbg, ubg = _dev(c["lbg"]), _dev(c["ubg"])
        _lib.check(_lib.lib().mpcqp_nlp_merit(ev._h, B, p.data_ptr() or None, x.data_ptr(), lbg.data_ptr() or None, ubg.data_ptr() or None,
                                              f.data_ptr(), gm.data_ptr(), None))
        torch.cuda.synchronize()                                         # (lbg, ubg live until the kernel has run)


def _op_step(ev, c, g, alpha=0.75):
    x, sm = g.new("x", ev.nvar, init=c["x"]), g.new("step_max")
    dw, st = _dev(c["dw"]), _i32(c["status"])
    entry = _lib.lib().mpcqp_stage_step if hasattr(ev, "set_stage_data") else _lib.lib().mpcqp_nlp_step
    _lib.check(entry(ev._h, g.B, alpha, dw.data_ptr(), x.data_ptr(), sm.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()


def _op_linesearch(ev, c, g, candidates=hc.CANDIDATES):
    out = {k: g.new(k) for k in ("alpha", "step_max", "f", "gmax")}
    out["accepted"] = g.new("accepted", dtype=np.int32)
    x, mu, phi = g.new("x", ev.nvar, init=c["x"]), g.new("mu", init=c["mu"]), g.new("phi", 2)
    kw = dict(lbg=_dev(c["lbg"]), ubg=_dev(c["ubg"])) if not hasattr(ev, "set_stage_data") else {}
    ev.line_search(_dev(c["p"]), x, _dev(c["lbx"]), _dev(c["ubx"]), _dev(c["q"]), _dev(c["dw"]), _dev(c["y"]), status=_i32(c["status"]), mu=mu,
                   alpha0=1.0, candidates=candidates, out=out, phi=phi, **kw)


def _op_advance(ev, c, g):
    mdl = c["model"]
    o = dict(x_out=g.new("x_out", ev.nvar), applied=g.new("applied", mdl.f), stage_cost=g.new("stage_cost"))
    lb, ub = g.new("lbx", ev.nvar, init=c["lbx"]), g.new("ubx", ev.nvar, init=c["ubx"])
    kw = dict(p_in=_dev(c["p"]), p_out=g.new("p_out", ev.np)) if mdl.pref else dict(p=_dev(c["p"]))
    ev.advance(_dev(c["x"]), o["x_out"], lb, ub, status=_i32(c["status"]), tail="rollout", w=_dev(c["w"]), applied=o["applied"],
               stage_cost=o["stage_cost"], **kw)


def _op_convexify(ev, c, g, mode):
    out = _system(ev, c, g)
    ev.convexify(_dev(c["p"]), _dev(c["x"]), out["P"], mode, hc.EPS, touched=g.new("touched", dtype=np.int32), lam_min=g.new("lam_min", ev.horizon))


def _op_lagrangian(ev, c, g, mode):
    out = _system(ev, c, g)
    ev.lagrangian(_dev(c["p"]), _dev(c["x"]), _dev(c["y"]), out["P"], status=_i32(c["status"]), mode=mode, eps=hc.EPS,
                  touched=g.new("touched", dtype=np.int32), lam_min=g.new("lam_min", ev.horizon))


def _op_nlp_lagrangian(ev, c, g, mode, workspace):
    out = _system(ev, c, g)
    Cw = g.new("C", ev.nnzP) if workspace else None
    shift = g.new("shift", ev.n, init=0.0)                                # (the entry asks for a zeroed shift; the guard rows keep their NaN)
    ev.lagrangian(_dev(c["p"]), _dev(c["x"]), _dev(c["y"]), out["P"], status=_i32(c["status"]), mode=mode, C=Cw, shift=shift)


OPS = {"eval": _op_eval, "merit": _op_merit, "step": _op_step, "linesearch": _op_linesearch, "advance": _op_advance, "convexify": _op_convexify,
       "lagrangian": _op_lagrangian, "nlp_eval": _op_eval, "nlp_merit": _op_merit, "nlp_step": _op_step, "nlp_linesearch": _op_linesearch,
       "nlp_lagrangian": _op_nlp_lagrangian}


def _launch(ev, c, job, rows=True):
    """one launch of the job's operation on the case c (at whatever batch it has) with guarded, NaN-filled outputs: {name: [B, ...] host array}"""
    g = _Guarded(c["x"].shape[0])
    with (_rows(ev, c, plant=job.op == "advance") if rows else contextlib.nullcontext()):
        OPS[job.op](ev, c, g, **dict(job.kw))
        torch.cuda.synchronize()
    return g.collect()


def _differing(got, want):
    """the number of elements of a launch that are not the bits of the base launch's"""
    n = 0
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape)
        if a.size:
            n += int((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(axis=1).sum())
    return n


# ------------------------------------------------------------------------------------------------ evaluators and base launches, once per module
@pytest.fixture(scope="module")
def evaluators(built):
    """one evaluator (one generated library) per case for the whole module; every test leaves it with nothing set"""
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.stage_eval import StageEvaluator
    evs = {}

    def get(family, name, fresh=False):
        make = lambda: (GeneralEvaluator if family in ("general", "gls", "gexact") else StageEvaluator)(gc.base(family, name)["model"])
        if fresh:
            ev = make(); evs[(family, name, len(evs))] = ev
            return ev
        if (family, name) not in evs:
            evs[(family, name)] = make()
        return evs[(family, name)]
    yield get
    for ev in evs.values():
        ev.close()


@pytest.fixture(scope="module")
def base_launch(evaluators):
    """the launch of a job's base case at its own batch, once"""
    done = {}

    def get(job):
        if job not in done:
            done[job] = _launch(evaluators(job.family, job.name), gc.base(job.family, job.name), job)
        return done[job]
    return get


# ------------------------------------------------------------------------------------------------ 1. every kernel at every batch
@pytest.mark.parametrize("job", gc.JOBS, ids=gc.job_id)
def test_rows_of_every_batch_are_the_base_launch(evaluators, base_launch, job):
    c0 = gc.base(job.family, job.name)
    ev = evaluators(job.family, job.name)
    want = base_launch(job)
    worst, d = 0, None
    for B in gc.BATCHES:
        ct, idx = gc.tile(c0, B)
        got = _launch(ev, ct, job)
        n = _differing(got, {k: v[idx] for k, v in want.items()})
        worst = max(worst, n)
        assert n == 0, (gc.job_id(job), B, {k: int((got[k] != want[k][idx]).sum()) for k in want})
        if B == max(gc.BATCHES):
            d = _hp_distances(job, c0, got, idx, gc.probe_rows(job, B))
    # (the comparison can tell positions apart: against the neighbour's base instance rows do differ, and something was written)
    assert _differing(got, {k: v[np.roll(idx, 1)] for k, v in want.items()}) > 0 and any(np.isfinite(v).any() for v in want.values() if v.dtype.kind == "f")
    print(gc.job_id(job), "batches", gc.BATCHES, "elements that differ from the base launch:", worst,
          "" if d is None else "rows %s against the 60-digit reference: %s" % (d[0], " ".join("%s %.2e" % kv for kv in d[1].items())))
    if d is not None:
        for k, dist in d[1].items():
            assert dist <= 1.0, (gc.job_id(job), k, dist)


def _hp_distances(job, c0, got, idx, rows):
    """(rows, {quantity: distance / bar}) of three rows of a tiled launch against the high-precision reference of their base instances; None for a
    case outside hp_cases and for the step, which has no reference of its own"""
    if job.family not in ("hp", "general") or job.op in ("step", "nlp_step"):
        return None
    name, mdl, base = job.name, c0["model"], idx[rows]
    pick = lambda ref: {k: np.asarray(v)[base] for k, v in ref.items() if isinstance(v, np.ndarray) and v.shape[:1] == (c0["x"].shape[0],)}
    g = {k: v[rows] for k, v in got.items()}
    if job.op in ("eval", "nlp_eval"):
        ref = pick(hc.ref_system(name) if job.family == "hp" else hc.ref_general(name))
        d = hc.system_distances(mdl, g, ref)
    elif job.op in ("merit", "nlp_merit"):
        ref = pick(hc.ref_merit(name) if job.family == "hp" else hc.ref_general(name))
        d = dict(f=hp.distance(g["f"], ref["f"]), gmax=hp.distance(g["gmax"], ref["gmax"]))
    elif job.op == "linesearch":
        full = hc.ref_line_search(name)
        ref = pick(full)
        ok = np.isin(c0["status"][base], hp.OK)
        sel = np.zeros(len(rows), np.int64)
        for i in np.nonzero(ok)[0]:
            j = np.nonzero(full["alphas"] == g["alpha"][i])[0]
            assert len(j) == 1 and g["accepted"][i] in (j[0], -1), (name, rows[i], g["alpha"][i], g["accepted"][i])
            sel[i] = j[0] + 1
        r = np.arange(len(rows))
        d = dict(phi0=hp.distance(g["phi"][:, 0], ref["phis"][:, 0]), phi1=hp.distance(g["phi"][:, 1], ref["phis"][r, sel]),
                 f=hp.distance(g["f"], ref["fs"][r, sel]), gmax=hp.distance(g["gmax"], ref["gmaxs"][r, sel]), mu=hp.distance(g["mu"][ok], ref["mu"][ok]))
    elif job.op == "convexify":
        ref = pick(hc.ref_convexify(name, dict(job.kw)["mode"]))
        bar_frame, bar_inst = cc.bar({"hnorm": ref["hnorm"]})
        assert np.array_equal(g["touched"], ref["touched"])
        dP = np.array([np.abs(hp.dense(mdl.Pp, mdl.Pi, g["P"][i], mdl.n)[0] - ref["P"][i]).max() for i in range(len(rows))]) / bar_inst
        return rows, dict(P=dP.max(), lam_min=(np.abs(g["lam_min"] - ref["lam_min"]) / bar_frame).max())
    elif job.op == "advance":
        ref = pick(hc.ref_advance(name, "rollout", False))
        N, nx, f = mdl.N, mdl.nx, mdl.f
        G = g["x_out"].reshape(-1, N, f); R = ref["x"].reshape(-1, N, f)
        d = dict(first=hp.distance(G[:, 0, :nx], R[:, 0, :nx]), tail=hp.distance(G[:, N - 1, :nx], R[:, N - 1, :nx]),
                 stage_cost=hp.distance(g["stage_cost"], ref["stage_cost"]))
        assert _same(g["applied"], ref["applied"])
    else:
        return None
    return rows, {k: v / hc.TOL for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ 2. what a handle keeps between launches
def _sequence(ev, job, c0, want, **kw):
    for B in gc.SEQUENCE:
        ct, idx = gc.tile(c0, B)
        n = _differing(_launch(ev, ct, job, **kw), {k: v[idx] for k, v in want.items()})
        print(gc.job_id(job), "batch", B, "elements that differ from the base launch:", n)
        assert n == 0, (gc.job_id(job), B)


@pytest.mark.parametrize("job", [gc.Job("hp", "bump3", "convexify", (("mode", "project"),)), gc.Job("hp", "every3", "convexify", (("mode", "mirror"),)),
                                 gc.Job("exact", "cvx", "lagrangian", (("mode", "project"),)), gc.Job("exact", "wide7", "lagrangian", (("mode", "mirror"),))],
                         ids=gc.job_id)
def test_convexify_scratch_grows_and_is_reused(evaluators, base_launch, job):
    """the scratch of the convexification (the corrections of the shared block, then the flags, placed by the capacity) on one fresh handle through
    5, 1031, 64, 1, 257: a launch below the capacity finds its flags where the capacity puts them.  every3 also has parameter and stage-data rows
    that are set per launch: their buffers grow and are reused in the same order."""
    _sequence(evaluators(job.family, job.name, fresh=True), job, gc.base(job.family, job.name), base_launch(job))


def test_one_handle_convexifies_and_adds_on_the_same_scratch(evaluators, base_launch):
    """mpcqp_stage_convexify and mpcqp_stage_lagrangian with a mode share the scratch of one handle: alternated, at batches that go up and down"""
    ev = evaluators("exact", "cvx", fresh=True)
    c0 = gc.base("exact", "cvx")
    jobs = (gc.Job("exact", "cvx", "convexify", (("mode", "mirror"),)), gc.Job("exact", "cvx", "lagrangian", (("mode", "project"),)))
    want = [_launch(ev, c0, j) for j in jobs]
    for i, B in enumerate(gc.SEQUENCE + gc.SEQUENCE[::-1]):
        ct, idx = gc.tile(c0, B)
        j = jobs[i % 2]
        n = _differing(_launch(ev, ct, j), {k: v[idx] for k, v in want[i % 2].items()})
        print(gc.job_id(j), "batch", B, "elements that differ from the base launch:", n)
        assert n == 0, (gc.job_id(j), B)


@pytest.mark.parametrize("name", ["every3", "quadrotor2_pfw"])
def test_instance_params_rows_at_and_below_the_stored_batch(evaluators, base_launch, name):
    """model and plant rows through 5, 1031, 64, 1, 257 (eval reads the model's, advance both), then launches smaller than the stored rows: instance
    b reads row b"""
    ev = evaluators("hp", name, fresh=True)
    c0 = gc.base("hp", name)
    jobs = (gc.Job("hp", name, "eval", ()), gc.Job("hp", name, "advance", ()))
    for j in jobs:
        _sequence(ev, j, c0, base_launch(j))
    big, idx = gc.tile(c0, 1031)
    with _rows(ev, big, plant=True):
        for B in (257, 64, 5):
            head = {k: (v[:B] if k in gc.PER_INSTANCE and v is not None else v) for k, v in big.items()}
            for j in jobs:
                n = _differing(_launch(ev, head, j, rows=False), {k: v[idx[:B]] for k, v in base_launch(j).items()})
                print(gc.job_id(j), "batch", B, "of 1031 stored rows, elements that differ from the base launch:", n)
                assert n == 0, (gc.job_id(j), B)


@pytest.mark.parametrize("name", ["every_pf4", "data70"])
def test_stage_data_set_and_shifted_at_every_batch(evaluators, name):
    """mpcqp_stage_set_stage_data and mpcqp_stage_shift_data on one handle through 5, 1031, 64, 1, 257: what the kernels read after the device's
    shift is what they read from the NumPy shift of the same rows, bit for bit, and row b of it is the base case's shifted row idx[b]"""
    from tests.support import stage_data_cases as sdc
    ev = evaluators("hp", name, fresh=True)
    c0 = gc.base("hp", name)
    job = gc.Job("hp", name, "merit" if name == "data70" else "eval", ())
    shifted = lambda c: dict(c, d=sdc.shift_reference(sdc.shift_reference(c["d"], c["d_new"])))
    want = _launch(ev, shifted(c0), job)
    assert _differing(want, _launch(ev, c0, job)) > 0                      # the shift matters to what is read
    for B in gc.SEQUENCE:
        ct, idx = gc.tile(c0, B)
        with _rows(ev, ct):
            ev.shift_stage_data(_dev(ct["d_new"]))
            ev.shift_stage_data()
            got = _launch(ev, ct, job, rows=False)
        host = _launch(ev, shifted(ct), job)
        n = _differing(got, host) + _differing(got, {k: v[idx] for k, v in want.items()})
        print(gc.job_id(job), "batch", B, "elements that differ after the device's shift:", n)
        assert n == 0, (name, B)


@pytest.mark.parametrize("name", hc.GENERAL)
def test_general_evaluator_refuses_remembered_bounds_of_another_batch(evaluators, name):
    """merit and line_search without explicit bounds after an eval at another batch: refused by the shape check, before any launch -- the outputs
    keep their fill; with the bounds given they pass"""
    ev = evaluators("general", name, fresh=True)
    c0 = gc.base("general", name)
    for B_eval, B in ((1031, 64), (5, 1031)):
        big, _ = gc.tile(c0, B_eval)
        ev.eval(*[_dev(big[k]) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")])
        ct, idx = gc.tile(c0, B)
        t = {k: _dev(ct[k]) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg", "dw")}
        q, y = _dev(np.zeros((B, ev.n))), _dev(np.zeros((B, ev.m)))
        g = _Guarded(B)
        out = {k: g.new(k) for k in ("alpha", "step_max", "f", "gmax")}
        out["accepted"] = g.new("accepted", dtype=np.int32)
        x = g.new("x", ev.nvar, init=ct["x"])
        with pytest.raises(ValueError, match="dimension mismatch"):
            ev.merit(t["p"], t["x"])
        with pytest.raises(ValueError, match="dimension mismatch"):
            ev.line_search(t["p"], x, t["lbx"], t["ubx"], q, t["dw"], y, out=out)
        torch.cuda.synchronize()
        left = g.collect()
        assert _same(left["x"], ct["x"]) and all(np.isnan(left[k]).all() for k in ("alpha", "step_max", "f", "gmax")) and (left["accepted"] == -99).all()
        f, gm = ev.merit(t["p"], t["x"], lbg=t["lbg"], ubg=t["ubg"])
        ev.line_search(t["p"], x, t["lbx"], t["ubx"], q, t["dw"], y, out=out, lbg=t["lbg"], ubg=t["ubg"])
        torch.cuda.synchronize()
        want = _launch(ev, c0, gc.Job("general", name, "nlp_merit", ()))
        assert _same(f.cpu().numpy(), want["f"][idx]) and _same(gm.cpu().numpy(), want["gmax"][idx]), (name, B)
        after = g.collect()
        assert np.isfinite(after["alpha"]).all() and (after["accepted"] != -99).all(), (name, B)
