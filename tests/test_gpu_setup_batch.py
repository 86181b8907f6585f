"""GPU: the set-up kernel's batched load and write-out phases -- the pattern's tables, then the gathers from the caller's arrays, in two
stages; q loaded by its owner; A' written out from the staged copy of A through the host's map; the bounds of several trips in flight -- against the same
kernel with MPCQP_NO_SETUP_BATCH=1, the paths of the commit before: two fresh handles in one process, x, y, z, status, iterations and info bit for bit;
and the new path against the CPU oracle at the bar tests/test_gpu_parity.py holds the on-chip kernels to, with equal iteration counts.  One case per
instantiation of scale_phase (kernel_oc_split.hpp): the shape is forced with MPCQP_SETUP_CAP / MPCQP_NO_IX16 where the rule does not give it, and read
back from the MPCQP_VERBOSE line of the handle."""
import functools
import re

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems
from tests.test_gpu_parity import _close
from tests.test_setup_batch_host import describe

pytestmark = pytest.mark.gpu

BITS = ("x", "y", "z", "status", "iters", "obj", "prim_res", "dual_res", "rho")
OFF = "MPCQP_NO_SETUP_BATCH"
SHAPE = re.compile(r"set-up kernel shape: 4 waves, \d+ B of LDS \(values of A (staged|in the slab), of P (staged|in the slab), 16-bit index tables (A and P|A|off);")
# the seven arms at the bottom of scale_phase, by what the shape line says: (A staged, P staged, 16-bit tables)
ARMS = {1: (True, True, 3), 2: (True, True, 1), 3: (True, True, 0), 4: (True, False, 0), 5: (False, False, 3), 6: (False, False, 1), 7: (False, False, 0)}

# (id, workload, N, batch, reduced, family, variant, extra environment, arm, A' from the staged copy)
CASES = [
    ("quadrotor-N20", "quadrotor", 20, 3, False, "oc4", 204, {}, 4, True),          # the north star: a 576-entry remainder of A, two trips of q, three of l / u, waves with two chunks of A'
    ("quadrotor-N20-reduced", "quadrotor", 20, 3, True, "oc4", 204, {}, 4, True),
    ("cartpole-N30", "cartpole", 30, 4, False, "oc4", 204, {}, 1, True),            # fully staged, 16-bit tables; npad < 256: a wave with no chunk of A'
    ("quadrotor-N50", "quadrotor", 50, 2, False, "oc8", 208, {}, 5, False),         # nothing staged: the slab-destination load, A' from the caller's array in hoisted batches
    ("cartpole-N100", "cartpole", 100, 2, False, "oc8", 208, {}, 5, False),
    ("cartpole-N30-tables-of-A", "cartpole", 30, 2, False, "oc4", 204, {"MPCQP_SETUP_CAP": "45056"}, 2, True),
    ("cartpole-N30-no-tables", "cartpole", 30, 2, False, "oc4", 204, {"MPCQP_NO_IX16": "1"}, 3, True),
    ("cartpole-N30-slab-tables-of-A", "cartpole", 30, 2, False, "oc4", 204, {"MPCQP_SETUP_CAP": "16384"}, 6, False),
    ("quadrotor-N20-slab-no-tables", "quadrotor", 20, 2, False, "oc4", 204, {"MPCQP_SETUP_CAP": "16384", "MPCQP_NO_IX16": "1"}, 7, False),
]


def test_cases_enter_every_arm_of_scale_phase():
    assert {c[8] for c in CASES} == set(ARMS)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _case(name, N, batch, reduced):
    """-> (LocalSystem, fixed rows or None, the QP the handle iterates on, oracle result on it, its free variables / kept rows or None)"""
    mdl, ls, _ = models.make_workload(name, batch, N=N)
    if not reduced:
        return ls, None, ls, problems.oracle_solve(ls), None
    fixed = list(range(mdl.np))
    red, free, kept, _, _ = problems.reduce_qp(ls, fixed)
    return ls, fixed, red, problems.oracle_solve(red), (free, kept)


def _solve(monkeypatch, capfd, ls, inner, fixed, off, family, variant, extra, arm, staged):
    from optimal_control_problem_amd.batch_qp import BatchQP
    with monkeypatch.context() as mp:
        mp.delenv(OFF, raising=False)
        mp.setenv("MPCQP_VARIANT", family); mp.setenv("MPCQP_VERBOSE", "1")
        for k, v in extra.items():
            mp.setenv(k, v)
        if off:
            mp.setenv(OFF, "1")
        capfd.readouterr()
        qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai, fixed_rows=fixed)
        err = capfd.readouterr().err
        info, _ = describe(inner, (), batch=ls.batch, cus=_cus(), family=family)
    try:
        assert qp.plan_info()["variant"] == variant
        # which arm this handle's set-up kernel enters, from the library's own line, and which of the new paths (the host's view of the same selection)
        m = SHAPE.search(err)
        assert m, err
        got = (m.group(1) == "staged", m.group(2) == "staged", {"A and P": 3, "A": 1, "off": 0}[m.group(3)])
        assert got == ARMS[arm], (got, arm)
        assert (info["a_lds"] == 1, info["p_lds"] == 1, info["ix16"]) == ARMS[arm]
        assert info["su_path"] & 12 == (0 if off else (12 if staged else 4)), info
        qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve()
        return qp.get()
    finally:
        qp.close()


@pytest.mark.parametrize("cid,name,N,batch,reduced,family,variant,extra,arm,staged", CASES, ids=[c[0] for c in CASES])
def test_batched_phases_give_the_bits_of_the_paths_before(built, monkeypatch, capfd, cid, name, N, batch, reduced, family, variant, extra, arm, staged):
    ls, fixed, inner, ref, sub = _case(name, N, batch, reduced)
    on = _solve(monkeypatch, capfd, ls, inner, fixed, False, family, variant, extra, arm, staged)
    off = _solve(monkeypatch, capfd, ls, inner, fixed, True, family, variant, extra, arm, staged)
    for k in BITS:
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    if sub is not None:
        on = dict(on, x=on["x"][:, sub[0]], y=on["y"][:, sub[1]], z=on["z"][:, sub[1]])
    assert (on["status"] == ref["status"]).all(), (on["status"], ref["status"])
    assert (on["iters"] == ref["iters"]).all(), (on["iters"], ref["iters"])
    for k in ("x", "y", "z"):
        _close(on, ref, k)
