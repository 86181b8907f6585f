"""CPU: the kernel selection of the library (csrc/select.hpp select_kernel, run through tests/support/plan_interp.cpp plan_select with the knobs of
the environment) against tests/golden/selection_grid.json -- what the library of the commit before select_kernel existed reported for the same
patterns, batches, forced families and knobs on an MI355X (tools/selection_grid.py).  test_gpu_parity.py holds the library against the same file."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.support import problems

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "libplan_interp.so")
GRID = problems.selection_grid()
PLAN_KEYS = ["n", "m", "batch", "npad", "mpad", "n_blocks", "L_blocks", "lds_bytes", "workspace_bytes_per_qp", "ordering", "nnzP_triu", "nnzA", "T_blocks",
             "factor_ops", "ell_slots", "variant"]
OC_KEYS = ["chain_blocks", "has_hub", "chain_e", "chain_f", "lds_blocks", "positions_per_wave", "hub_blocks_in_registers", "launch_pairs_for_rho_updates",
           "slots_A", "slots_At", "slots_P", "chain_pairs"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def select(r, monkeypatch, forced=None):
    """-> (rc, plan_info dict, oc_info dict, set-up launch list, instance list, MPCQP_VERBOSE line without the resident workgroups)"""
    n, m, Pp, Pi, Ap, Ai, _ = problems.selection_pattern(r, inner=True)      # (a reduced row: the pattern mpcqp_create_reduced hands to the inner handle)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    L = C.CDLL(SO)
    L.plan_select_shape.restype = C.c_char_p
    out = np.zeros(48, np.int64)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (Pp, Pi, Ap, Ai))
    rc = L.plan_select(n, m, r["batch"], _p(Pp), _p(Pi), _p(Ap), _p(Ai), GRID["multiProcessorCount"], forced, _p(out))
    o = out.tolist()
    return rc, dict(zip(PLAN_KEYS, o[:16])), dict(zip(OC_KEYS, o[16:28])), o[28:40], o[40:48], L.plan_select_shape().decode()


@pytest.mark.parametrize("r", GRID["rows"], ids=problems.selection_row_id)
def test_selection_matches_the_recorded_library(built, monkeypatch, r):
    rc, plan, oc, setup, inst, text = select(r, monkeypatch)
    assert rc == r["rc"]
    if rc:
        return
    assert plan == r["plan_info"]
    assert oc == r["oc_info"]
    if r["setup_shape"] is None:
        assert text == "" and not setup[9]
    else:       # (the line ends with what only the device knows: ", <n> resident workgroups")
        assert r["setup_shape"].rsplit(",", 1)[0] == text and setup[9] == 1 and setup[0] == 4 and ("%d B of LDS" % setup[1]) in text


def test_grid_covers_every_family_order_and_experiment():
    """the condition the grid was drawn up under: every family code the library can report, both eight-wave instances, z and y in the slab
    and in LDS, every chain order, one / two / four chain pairs, each experiment switched on, every family forced both ways"""
    ok = [r for r in GRID["rows"] if r["rc"] == 0]
    assert {r["plan_info"]["variant"] for r in ok} == {0, 1, 2, 4, 8, 102, 104, 204, 208}
    assert {r["oc_info"]["positions_per_wave"] for r in ok if r["plan_info"]["variant"] == 208} >= {4, 7}
    assert {r["oc_info"]["chain_pairs"] for r in ok if r["plan_info"]["variant"] >= 200} == {1, 2, 4}
    assert {r["plan_info"]["ordering"] for r in ok} >= {0, 1, 2, 4}
    for fam in ("stream", "res1", "res2", "res4", "res8", "gres4", "gres2", "oc4", "oc8"):
        assert {r["rc"] for r in GRID["rows"] if r["env"].get("MPCQP_VARIANT") == fam} == {0, 5}, fam
    for knob in ("MPCQP_TILES", "MPCQP_VTILES", "MPCQP_DOUBLES"):
        assert any(knob in r["env"] for r in ok), knob


def test_stated_values(built, monkeypatch):
    """what the project states elsewhere about the rule, on 256 CUs (README / DESIGN.md section 3, test_gpu_parity.py, test_plan.py)"""
    def sel(workload, N, batch, env=None, forced=None):
        with monkeypatch.context() as mp:
            return select(dict(workload=workload, N=N, batch=batch, env=env or {}, reduced=False), mp, forced)
    rc, plan, oc, setup, inst, text = sel("quadrotor", 20, 8192)
    assert (rc, plan["variant"], plan["lds_bytes"], plan["ordering"], oc["chain_pairs"]) == (0, 204, 81672, 2, 1)
    assert setup[:5] == [4, 52488, setup[2], 1, 0]                                   # set-up: 52,488 B (three per CU), A staged
    rc, plan, oc, setup, inst, text = sel("quadrotor", 50, 8192)
    assert (plan["variant"], plan["lds_bytes"], inst[6], setup[1], setup[3]) == (208, 160336, 2, 78928, 0)      # BASELINE config 3 as mpcqp_create takes it (test_plan.py)
    rc, plan, oc, setup, inst, text = sel("cartpole", 100, 16384)
    assert (plan["variant"], plan["lds_bytes"], plan["ordering"], inst[6], oc["chain_pairs"], setup[1]) == (208, 99656, 4, 1, 4, 52424)
    rc, plan, oc, setup, inst, text = sel("quadrotor", 5, 8192)
    assert (plan["variant"], inst[4]) == (4, 3)                                      # 168-VGPR instance of the LDS-resident kernel
    rc, plan, oc, setup, inst, text = sel("quadrotor", 55, 4096)
    assert (plan["variant"], plan["lds_bytes"], inst[0], inst[1]) == (104, 36952, 1, 1)
    assert sel("quadrotor", 56, 8192)[1]["variant"] == 104                           # the tables exist, but the LDS of one CU does not hold it (test_plan.py)
    # mpcqp_create_tuned's way of asking for a family: by argument, whatever MPCQP_VARIANT says ("" = the rule)
    assert sel("quadrotor", 20, 64, forced=b"oc4")[1]["variant"] == 204
    assert sel("quadrotor", 20, 64, env={"MPCQP_VARIANT": "res4"}, forced=b"oc4")[1]["variant"] == 204
    assert sel("quadrotor", 20, 8192, env={"MPCQP_VARIANT": "res4"}, forced=b"")[1]["variant"] == 204
    assert sel("quadrotor", 30, 64, forced=b"oc4")[0] == 5 and sel("quadrotor", 57, 64, forced=b"oc8")[0] == 5
