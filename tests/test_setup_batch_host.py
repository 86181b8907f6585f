"""CPU: the A' -> A map of the set-up kernel's write-out (csrc/plan.hpp build_at_map, oc_setup_tables), read out of the array the kernel
reads it from, for the handles the library's own selection makes of the MPC patterns (tests/support/setup_batch_interp.cpp): every entry of A' finds the
entry of A with its source index, padding carries the sentinel, no two entries share a target, and shapes that do not stage A have no map."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "libsetup_batch_interp.so")
CUS = problems.selection_grid()["multiProcessorCount"]
INFO = ["split", "a_lds", "p_lds", "ix16", "batch", "at_map", "o_map", "nblk", "A_entries", "At_entries", "none", "su_path"]
ARRAYS = ["A_src", "At_src", "map"]
# id -> (workload, N, reduced, A staged by the rule on 256 CUs: pinned)
CASES = {
    "quadrotor-N20": ("quadrotor", 20, False, True),
    "quadrotor-N20-reduced": ("quadrotor", 20, True, True),
    "cartpole-N30": ("cartpole", 30, False, True),
    "double_integrator-N60": ("double_integrator", 60, False, True),
    "quadrotor-N50": ("quadrotor", 50, False, False),
    "cartpole-N100": ("cartpole", 100, False, False),
}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _system(name, N, reduced):
    mdl, ls, _ = models.make_workload(name, 2, N=N)
    return problems.reduce_qp(ls, list(range(mdl.np)))[0] if reduced else ls


def describe(ls, env=(), batch=8192, cus=CUS, family=None):
    """-> (info dict, arrays dict) of the handle the library makes of this pattern, with `env` set for the call"""
    L = C.CDLL(SO)
    L.setup_batch_describe.restype = C.c_long
    info = np.zeros(len(INFO), np.int64); buf = np.zeros(1 << 20, np.int32)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai))
    old = {k: os.environ.get(k) for k, _ in env}
    try:
        for k, v in env:
            os.environ[k] = v
        w = L.setup_batch_describe(ls.n, ls.m, batch, _p(Pp), _p(Pi), _p(Ap), _p(Ai), cus, family.encode() if family else None, _p(info), _p(buf), C.c_long(buf.size))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert w > 0, w
    arrays, o = {}, 0
    for name in ARRAYS:
        cnt = int(buf[o]); arrays[name] = buf[o + 1:o + 1 + cnt].copy(); o += 1 + cnt
    assert o == w
    return dict(zip(INFO, info.tolist())), arrays


@functools.lru_cache(maxsize=None)
def _case(cid):
    name, N, reduced, _ = CASES[cid]
    return describe(_system(name, N, reduced))


@pytest.mark.parametrize("cid", [c for c in CASES if CASES[c][3]])
def test_map_sends_every_entry_of_At_to_the_entry_of_A_with_its_source(built, cid):
    info, a = _case(cid)
    assert info["split"] == 1 and info["a_lds"] == 1 and info["batch"] == 1 and info["at_map"] == 1
    assert info["su_path"] & 4 and info["su_path"] & 8
    assert info["o_map"] > 0 and info["o_map"] % 2 == 0
    m, at_src, a_src, none = a["map"], a["At_src"], a["A_src"], info["none"]
    assert m.size == at_src.size == info["At_entries"] and a_src.size == info["A_entries"] < none
    real = at_src >= 0
    assert real.any() and (~real).any()
    # every A' entry with a source maps to an A entry with the same source
    assert (m[real] < a_src.size).all()
    assert np.array_equal(a_src[m[real]], at_src[real])
    # every padding entry carries the sentinel
    assert (m[~real] == none).all()
    # injective on the non-padding entries -- and onto A's: both layouts hold every non-zero once
    assert np.unique(m[real]).size == int(real.sum()) == int((a_src >= 0).sum())


@pytest.mark.parametrize("cid", [c for c in CASES if not CASES[c][3]])
def test_no_map_where_A_is_not_staged(built, cid):
    info, a = _case(cid)
    assert info["split"] == 1 and info["a_lds"] == 0
    assert info["at_map"] == 0 and info["o_map"] == 0 and a["map"].size == 0
    assert info["batch"] == 1 and info["su_path"] & 4 and not info["su_path"] & 8      # (the batched phases themselves do not need staged values)


def test_the_switch_clears_both_bits_and_the_map(built):
    ls = _system("quadrotor", 20, False)
    info, a = describe(ls, (("MPCQP_NO_SETUP_BATCH", "1"),))
    assert info["batch"] == 0 and info["at_map"] == 0 and info["o_map"] == 0 and a["map"].size == 0
    assert info["su_path"] & 12 == 0 and info["su_path"] & 3 == _case("quadrotor-N20")[0]["su_path"] & 3      # (the other paths' bits stay)
    # any other value than 1 does not switch it off (the convention of the set-up kernel's other switches)
    assert describe(ls, (("MPCQP_NO_SETUP_BATCH", "0"),))[0]["su_path"] & 12 == 12
