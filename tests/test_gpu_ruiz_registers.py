"""GPU: the set-up kernel's Ruiz passes with their fixed operands in registers (kernel_resident.hpp rz_*, kernel_oc_split.hpp scale_phase) against
the same kernel with MPCQP_NO_RUIZ_REGS=1 -- every wave reloads indices and P's values in every pass, the path of the commit before -- bit for
bit (x, y, z, status, iterations; fresh handles in one process), and against the CPU oracle at the bar tests/test_gpu_parity.py holds the on-chip
cases to.  The shapes are the smallest that reach each branch: every wave's list fits (quadrotor N = 20: the 21-slot chunk of P shares a wave
with another chunk), no wave's list fits (quadrotor N = 50: five or six chunks of A and three or four of P per wave), one wave of A and one of
P fall back beside three that do not (quadrotor N = 25), waves that own no chunk at all (double integrator N = 6, the smallest horizon the
four-wave on-chip plan accepts -- its set-up stages A and P and has no register form, so once more with nothing staged), zero / one / ten
passes, and the kept-workspace instances of the kernel."""
import functools
import os
import re

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems
from tests.test_gpu_parity import _close

pytestmark = pytest.mark.gpu

KEYS = ("x", "y", "z", "status", "iters")


def _capacities():
    """RUIZ_REG_* of csrc/plan.hpp (the device code's capacities are these constants)"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optimal_control_problem_amd", "csrc", "plan.hpp")).read()
    return {k: int(v) for k, v in re.findall(r"RUIZ_REG_(\w+) = (\d+)", src)}


@functools.lru_cache(maxsize=None)
def _workload(name, batch, N):
    return models.make_workload(name, batch, N=N)


@functools.lru_cache(maxsize=None)
def _oracle(name, batch, N, scaling):
    ref = problems.oracle_solve(_workload(name, batch, N)[1], scaling=scaling)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _solve(ls, monkeypatch, family, off, want_variant, env=(), **settings):
    from optimal_control_problem_amd.batch_qp import BatchQP
    with monkeypatch.context() as mp:
        mp.setenv("MPCQP_VARIANT", family)
        for k, v in env:
            mp.setenv(k, v)
        if off:
            mp.setenv("MPCQP_NO_RUIZ_REGS", "1")
        qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **settings)
    try:
        assert qp.plan_info()["variant"] == want_variant
        oc = qp.oc_info()
        qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve()
        return qp.get(), oc
    finally:
        qp.close()


def _same_bits(on, off):
    for k in KEYS:
        assert np.array_equal(on[k], off[k], equal_nan=True), k


def _against_oracle(got, ref):
    assert (got["status"] == ref["status"]).all(), (got["status"], ref["status"])
    assert (got["iters"] == ref["iters"]).all(), (got["iters"], ref["iters"])
    for k in ("x", "y", "z"):
        _close(got, ref, k)


def _on_off_oracle(monkeypatch, name, batch, N, family, variant, scaling=10, env=()):
    ls = _workload(name, batch, N)[1]
    on, oc = _solve(ls, monkeypatch, family, False, variant, env, scaling=scaling)
    off, _ = _solve(ls, monkeypatch, family, True, variant, env, scaling=scaling)
    _same_bits(on, off)
    _against_oracle(on, _oracle(name, batch, N, scaling))
    return oc


def test_headline_shape_every_wave_from_registers(built, monkeypatch):
    cap = _capacities()
    oc = _on_off_oracle(monkeypatch, "quadrotor", 8, 20, "oc4", 204)
    # the north-star plan: 73 slots of A and 31 of P over four waves; what the capacities were chosen for
    assert oc["slots_A"] <= 4 * cap["SLOTS_A"] and oc["slots_P"] <= 4 * cap["SLOTS_P"]


@pytest.mark.parametrize("N,batch", [(50, 4), (25, 4)])
def test_fallback_shapes_waves_keep_the_reloading_sweeps(built, monkeypatch, N, batch):
    """N = 50: 22 chunks of A and 13 of P, more per wave than a list holds: every wave falls back for both.  N = 25: chunk widths of A
    [1 x 6, 17 x 5] and of P [2 x 6, 26]: the wave with two 17-slot chunks of A and the wave with the 26-slot chunk of P fall back, the others
    run from registers, and P goes through the slab for all of them"""
    cap = _capacities()
    oc = _on_off_oracle(monkeypatch, "quadrotor", batch, N, "oc8", 208)
    # four waves, each with room for SLOTS_A slots: more slots than that in all means at least one wave's list of A does not fit
    assert oc["slots_A"] > 4 * cap["SLOTS_A"]


@pytest.mark.parametrize("env", [(), (("MPCQP_SETUP_CAP", "1"),)], ids=["staged", "nothing-staged"])
def test_waves_without_a_chunk(built, monkeypatch, env):
    """(MPCQP_SETUP_CAP=1: the set-up's shape with nothing staged, the one that has the register form)"""
    ls = _workload("double_integrator", 8, 6)[1]
    assert ls.n <= 64 and ls.m <= 64          # one chunk of P, one of A: three waves own nothing of either
    _on_off_oracle(monkeypatch, "double_integrator", 8, 6, "oc4", 204, env=env)


@pytest.mark.parametrize("scaling", [0, 1, 10])
def test_pass_counts(built, monkeypatch, scaling):
    """no pass at all (P still reaches the slab from the registers, unscaled by D but for c = 1) , a single pass, and the default ten"""
    _on_off_oracle(monkeypatch, "quadrotor", 8, 20, "oc4", 204, scaling=scaling)


def test_kept_workspace_instances(built, monkeypatch):
    """keep_workspace + update_vectors: the REUSE instances of the set-up kernel (full set-up through the register path, then a q / l / u solve on
    the kept scaling) agree with the oracle's kept workspace and with the reloading path"""
    from optimal_control_problem_amd.batch_qp import BatchQP
    from oracle import oracle as orc
    B = 8
    mdl, ls, meta = _workload("quadrotor", B, 20)
    rng = np.random.default_rng(11)
    frame0 = meta["frame0"].copy(); frame0[:, :mdl.nx] += rng.normal(0, 0.05, (B, mdl.nx))
    lbx, ubx, lbg, ubg = mdl.stacked_bounds(frame0)
    ls2 = mdl.local_system(meta["p"] + 0.1, meta["x_iterate"], lbx, ubx, lbg, ubg)       # same iterate -> same A, P; new q, l, u
    assert np.array_equal(ls2.A, ls.A)
    st = orc.State(orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai), B, orc.default_settings())
    refs = [st.solve(ls.P, ls.q, ls.A, ls.l, ls.u), st.solve_vectors(ls2.q, ls2.l, ls2.u)]

    def run(off):
        with monkeypatch.context() as mp:
            mp.setenv("MPCQP_VARIANT", "oc4")
            if off:
                mp.setenv("MPCQP_NO_RUIZ_REGS", "1")
            qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai)
        try:
            assert qp.plan_info()["variant"] == 204
            qp.keep_workspace(True)
            qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); first = qp.get()
            qp.update_vectors(ls2.q, ls2.l, ls2.u); qp.solve(); second = qp.get()
            return first, second
        finally:
            qp.close()

    on, off = run(False), run(True)
    for a, b, ref in zip(on, off, refs):
        _same_bits(a, b)
        _against_oracle(a, ref)
