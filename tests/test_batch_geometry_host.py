"""CPU: the tables of tests/support/geometry_cases.py do what tests/test_gpu_batch_geometry.py relies on.

1. BATCHES, through the restated launch arithmetic `threads`, puts every kernel of the GPU module past four blocks, into a partial last block and --
   where an instance's thread count does not divide the block's -- an instance across a block boundary; both pass ranges of general_eval_kernel get
   more than one block; the line-search and convexify cases cover every group width.
2. `tile` gathers rows, stage data, parameters and statuses together: the NumPy statement at the tiled case is the gathered statement of the base
   case, to 1e-14 max(1, |ref|) (the statements work instance by instance; the bar allows a vectorised sum another order).
3. `index` puts every base instance into each of the four wave slots of a block."""
import numpy as np
import pytest

from tests.support import geometry_cases as gc
from tests.support import hp_cases as hc

TILED = 11                                           # prime, above every base batch
FLOAT_BAR = 1e-14


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("job", gc.JOBS, ids=gc.job_id)
def test_batches_cross_every_boundary_of_the_launch(job):
    ranges = {B: gc.job_threads(job, B) for B in gc.BATCHES}
    for i, r in enumerate(ranges[gc.BATCHES[0]]):
        over = [ranges[B][i] for B in gc.BATCHES]
        assert max(v.blocks for v in over) > 4, (r.name, [v.blocks for v in over])
        # (a range whose instance fills whole blocks -- a group count equal to the horizon -- never ends inside a block)
        if r.per % r.block:
            assert any(gc.last_block_partial(v, B) for v, B in zip(over, gc.BATCHES)), r
        if gc.can_straddle(r):
            assert any(len(gc.straddlers(v, B)) for v, B in zip(over, gc.BATCHES)), r
        else:
            assert not any(len(gc.straddlers(v, B)) for v, B in zip(over, gc.BATCHES)), r
    if job.op == "nlp_eval":
        h, j, _ = ranges[max(gc.BATCHES)]
        assert h.blocks > 1 and j.blocks > 1, (h, j)
    # the thread count of a launch covers the batch, and the last instance ends in the last block
    for B, rs in ranges.items():
        for r in rs:
            assert (r.blocks - 1) * r.block < B * r.per <= r.blocks * r.block, (B, r)


def test_every_group_width_occurs():
    widths = {gc.line_search_width(dict(j.kw)["candidates"]) for j in gc.JOBS if j.op == "nlp_linesearch"}
    assert widths == {2, 4, 8, 16}
    cvx = {gc.convexify_groups(gc.base("hp", name)["model"])[1] for name in gc.CONVEXIFY}
    assert cvx == {16, 32, 64}
    # some convexify launch has an instance's groups in two blocks, and the launch that follows a lagrangian add does too
    assert any(gc.can_straddle(gc.job_threads(j, 5)[0]) for j in gc.JOBS if j.op == "convexify")
    assert any(gc.can_straddle(gc.job_threads(j, 5)[1]) for j in gc.JOBS if j.op == "lagrangian" and dict(j.kw)["mode"])
    # both mappings of stage_eval_kernel, the cooperative one with and without the padded parameter group
    per = {name: gc.threads("stage_eval", gc.base("hp", name)["model"], 1)[0].per for name in gc.ZOO}
    mdl = gc.base("hp", "quadrotor2_pfw")["model"]
    assert per["cartpole3"] == gc.base("hp", "cartpole3")["model"].n and per["quadrotor2"] == 16 * 3 and per["quadrotor2_pfw"] == 32 + 16 * 2
    assert per["quadrotor2_pfw"] > mdl.n                               # padding lanes exist


def test_modes_and_statuses_of_the_cases():
    from tests.support import exact_hessian_cases as ec
    assert {m for _, m in gc.EXACT} == {None} | set(ec.MODES)
    assert {dict(j.kw)["mode"] for j in gc.JOBS if j.op == "convexify"} == set(hc.MODES)
    seen = set()
    for j in gc.JOBS:
        st = gc.base(j.family, j.name)["status"]
        if st is not None:
            seen |= set(int(s) for s in st)
    assert set(gc.NO_POINT) <= seen


# ------------------------------------------------------------------------------------------------ 2. tile
class _rows(hc.rows_on_statement):
    pass


def _statement(job, c):
    """the NumPy statement of the job's operation on the case c: a dict of per-instance arrays (None: the operation has no statement of its own)"""
    mdl, kw = c["model"], dict(job.kw)
    a = [c[k] for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")]
    p, x = c["p"], c["x"]
    system = lambda ls: dict(P=np.array(ls.P), q=np.array(ls.q), A=np.array(ls.A), l=np.array(ls.l), u=np.array(ls.u))
    search = ("alpha", "accepted", "step_max", "f", "gmax", "phi")
    if job.op in ("step", "nlp_step"):
        return None
    if job.op.startswith("nlp_"):
        if job.op == "nlp_eval":
            return system(mdl.local_system(*a))
        if job.op == "nlp_merit":
            return dict(f=mdl.objective(p, x), gmax=mdl.violation(*a)[1])
        if job.op == "nlp_linesearch":
            xs, mu = x.copy(), c["mu"].copy()
            out = mdl.line_search(p, xs, c["lbx"], c["ubx"], c["q"], c["dw"], c["y"], status=c["status"], mu=mu, candidates=kw["candidates"],
                                  lbg=c["lbg"], ubg=c["ubg"])
            return dict({k: np.asarray(out[k]) for k in search}, x=xs, mu=mu)
        P0 = np.array(mdl.local_system(*a).P)
        Pn, shift = mdl.lagrangian_system(p, x, c["y"], P0, c["status"], 1 if kw["mode"] == "dominant" else 0)
        return dict(P=Pn, shift=shift)
    with _rows(c, plant=job.op == "advance"):
        if job.op == "eval":
            return system(mdl.local_system(*a))
        if job.op == "merit":
            return dict(f=mdl.objective(p, x), gmax=mdl.violation(x, c["lbx"], c["ubx"])[1])
        if job.op == "linesearch":
            xs, mu = x.copy(), c["mu"].copy()
            out = mdl.line_search(p, xs, c["lbx"], c["ubx"], c["q"], c["dw"], c["y"], status=c["status"], mu=mu, candidates=hc.CANDIDATES)
            return dict({k: np.asarray(out[k]) for k in search}, x=xs, mu=mu)
        if job.op == "advance":
            out = mdl.advance(x, c["lbx"], c["ubx"], status=c["status"], w=c["w"], tail="rollout", p=p)
            return {k: np.asarray(v) for k, v in out.items()}
        P0 = np.array(mdl.local_system(*a).P)
        if job.op == "convexify":
            Pn, touched, lam = mdl.convexify_system(p, x, P0, kw["mode"], hc.EPS)
        else:
            Pn, touched, lam = mdl.lagrangian_system(p, x, c["y"], P0, c["status"], kw["mode"], hc.EPS)
        return dict(P=Pn, touched=np.asarray(touched), lam_min=np.asarray(lam))


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    fin = np.isfinite(b)
    same = np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    return same and bool((np.abs(a[fin] - b[fin]) <= FLOAT_BAR * np.maximum(1.0, np.abs(b[fin]))).all())


@pytest.mark.parametrize("job", [j for j in gc.JOBS if j.op not in ("step", "nlp_step")], ids=gc.job_id)
def test_tile_gathers_everything_together(job):
    c0 = gc.base(job.family, job.name)
    ct, idx = gc.tile(c0, TILED)
    B0 = c0["x"].shape[0]
    assert set(idx) == set(range(B0)) and ct["x"].shape[0] == TILED
    for k in gc.PER_INSTANCE:
        assert (ct[k] is None) == (c0[k] is None)
        if c0[k] is not None:
            assert ct[k].shape == (TILED,) + c0[k].shape[1:] and ct[k].flags["C_CONTIGUOUS"]
    before = {k: c0[k].copy() for k in gc.PER_INSTANCE if c0[k] is not None}
    want, got = _statement(job, c0), _statement(job, ct)
    for k in want:
        assert got[k].shape[0] == TILED and _close(got[k], want[k][idx]), (gc.job_id(job), k)
    assert all(np.array_equal(c0[k], v, equal_nan=True) for k, v in before.items())      # the shared base case is left as it was


# ------------------------------------------------------------------------------------------------ 3. index
def test_index_puts_every_base_instance_into_every_wave_slot():
    sizes = sorted({gc.base(j.family, j.name)["x"].shape[0] for j in gc.JOBS})
    assert sizes == [2, 3, 5, 7]
    for B0 in sizes:
        # a wave slot of a batch B holds B / 4 instances: all B0 of them fit from 4 B0 on (20 for the cases with up to five, 28 for those with seven)
        for B in sorted(set(range(max(20, 4 * B0), 300)) | {b for b in gc.BATCHES if b >= 4 * B0}):
            idx = gc.index(B, B0)
            for slot in range(4):
                assert set(idx[slot::4]) == set(range(B0)), (B0, B, slot)
    for B0 in (3, 5):                                    # the formula itself where it needs no correction
        assert np.array_equal(gc.index(40, B0), (7 * np.arange(40) + 3) % B0)
    # the no-point instances of a case with statuses reach every slot of a partial last block's batch
    c0 = gc.base("hp", "every3")
    for B in (63, 65, 257, 1031):
        ct, idx = gc.tile(c0, B)
        bad = np.isin(ct["status"], gc.NO_POINT)
        assert np.array_equal(ct["status"], c0["status"][idx]) and all(bad[slot::4].any() for slot in range(4))
