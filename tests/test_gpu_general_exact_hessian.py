"""GPU: the exact Hessian of the Lagrangian on the general NLP path (mpcqp_nlp_lagrangian; csrc/general_kernels.hpp general_curvature_kernel and
general_curvature_apply_kernel) against its NumPy statement (general_nlp.GeneralNLP.lagrangian_system), bitwise across batch sizes, positions and
launches, its refusals, graph capture, and the device SQP loop against the host loop over the CPU oracle on the recipe.

Tolerances: P, C and shift to 1e-12 max(1, |ref|) (general_problems.close: the same operations as the statement's complex-step columns, in another
order, with compiler contraction); the loops to 1e-6 (1 + max |x|) per iteration, the bar of tests/test_gpu_exact_hessian.py (the device QPs stop at
1e-3 like the oracle's, from another ADMM path).  The CPU side (tests/test_general_exact_hessian_host.py) pins the inputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from optimal_control_problem_amd import _lib
from tests.support import general_exact_hessian_cases as ge
from tests.support import general_problems as gp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def _bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def evaluators(built):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    evs = {}
    yield lambda name: evs[name] if name in evs else evs.setdefault(name, GeneralEvaluator(ge.model(name)))
    for ev in evs.values():
        ev.close()


def _launch(ev, c, mode, y=None, status=None, workspace=True, rows=None, tile=1):
    """eval + lagrangian on fresh device copies: (P after eval, P', C workspace (NaN where not written) or None, shift (0 where not written))"""
    pick = lambda a: np.tile(a if rows is None else a[rows], (tile,) + (1,) * (np.ndim(a) - 1))
    t = {k: _dev(pick(c[k])) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")}
    yv = _dev(pick(c["y"] if y is None else y))
    st = None if status is None else _dev(pick(status), torch.int32)
    B = t["x"].shape[0]
    out = ev.eval(t["p"], t["x"], t["lbx"], t["ubx"], t["lbg"], t["ubg"])
    P0 = out["P"].clone()
    Cw = torch.full((B, ev.nnzP), float("nan"), dtype=torch.float64, device="cuda") if workspace else None
    shift = torch.zeros((B, ev.n), dtype=torch.float64, device="cuda")
    ev.lagrangian(t["p"], t["x"], yv, out["P"], status=st, mode=mode, C=Cw, shift=shift)
    torch.cuda.synchronize()
    return P0.cpu().numpy(), out["P"].cpu().numpy(), None if Cw is None else Cw.cpu().numpy(), shift.cpu().numpy()


@pytest.mark.parametrize("name", ge.NAMES)
def test_kernels_match_the_statement(evaluators, name):
    ev = evaluators(name)
    c = ge.case(name); mdl = c["model"]
    assert ev.has_exact_hessian and (ev.n, ev.m, ev.nnzP) == (mdl.n, mdl.m, len(mdl.Pi)) and np.array_equal(ev.Pi, mdl.Pi)
    cur, rows, cols = ge.slots(mdl)
    Cd = mdl.constraint_curvature(c["p"], c["x"], c["y"])[:, rows, cols]
    for mode, key in ((0, 0), (1, "dominant")):
        P0, Pn, Cw, shift = _launch(ev, c, key)
        assert gp.close(P0, c["P"], ge.TOL) and not P0[:, ~mdl_plain_slots(name)].any()       # eval writes every slot, 0 in the added ones
        Pr, sr = mdl.lagrangian_system(c["p"], c["x"], c["y"], P0, None, mode)
        print(name, "mode", mode, "P", np.abs(Pn - Pr).max(), "shift", np.abs(shift - sr).max())
        assert gp.close(Pn, Pr, ge.TOL) and gp.close(shift, sr, ge.TOL)
        assert gp.close(Cw[:, cur], Cd[:, cur], ge.TOL) and np.isnan(Cw[:, ~cur]).all()
        if mode == 0:
            assert not shift.any()
            _, Pd, none, _ = _launch(ev, c, 0, workspace=False)
            assert none is None and _bits(Pd, Pn)                                            # the same bits with and without the workspace
        if name == "skip_coupled":
            assert _bits(Pn, P0) and not shift.any()                                         # no curvature: a no-op


def mdl_plain_slots(name):
    """[nnzP] bool: the slots of the flagged pattern that the unflagged model has too"""
    mdl, plain = ge.model(name), ge.model(name, False)
    _, rows, cols = ge.slots(mdl)
    return plain.hm[rows, cols]


@pytest.mark.parametrize("mode", [0, "dominant"])
def test_same_bits_across_batches_positions_and_launches(evaluators, mode):
    """B = 133 = 19 copies of the 7 instances: 798 curvature threads and 2128 apply threads, several blocks each, ending inside one"""
    ev = evaluators("pendulum")
    c = ge.case("pendulum")
    _, small, Cs, ss = _launch(ev, c, mode)
    _, big, Cb, sb = _launch(ev, c, mode, tile=19)
    _, again, Ca, sa = _launch(ev, c, mode, tile=19)
    assert big.shape[0] == 133
    cur = ge.slots(c["model"])[0]
    for b in range(ge.BATCH):
        _, one, Co, so = _launch(ev, c, mode, rows=[b])                                      # each instance alone in a batch-1 launch
        for k in range(b, 133, ge.BATCH):                                                    # ... and at 19 positions of the large batch
            assert _bits(big[k], one[0]) and _bits(sb[k], so[0]) and _bits(Cb[k, cur], Co[0, cur]), (mode, b, k)
    assert _bits(big[:7], small) and _bits(big, again) and _bits(sb, sa) and _bits(Cb[:, cur], Ca[:, cur])


@pytest.mark.parametrize("name", ("pendulum", "recipe"))
def test_failed_instances_and_zero_multipliers_keep_every_bit(evaluators, name):
    ev = evaluators(name)
    c = ge.case(name)
    bad = ~np.isin(c["status"], ge.OK)
    for mode in (0, "dominant"):
        for ws in ((True, False) if mode == 0 else (True,)):
            P0, Pn, Cw, shift = _launch(ev, c, mode, y=c["ynan"], status=c["status"], workspace=ws)
            assert _bits(Pn[bad], P0[bad]) and not shift[bad].any() and np.isfinite(Pn).all()
            if ws:
                assert np.isnan(Cw[bad]).all()                                               # neither read nor written
            _, Pa, _, sa = _launch(ev, c, mode, workspace=ws)
            assert _bits(Pn[~bad], Pa[~bad]) and _bits(shift[~bad], sa[~bad]) and not _bits(Pa[bad], P0[bad])
            P0, Pz, _, sz = _launch(ev, c, mode, y=np.zeros_like(c["y"]), workspace=ws)
            assert _bits(Pz, P0) and not sz.any()                                            # y = 0 is a no-op


# ------------------------------------------------------------------------------------------------ refusals
def _args(ev, B, **over):
    from optimal_control_problem_amd.general_eval import LagrangianArgs
    t = {k: torch.ones((B, w), dtype=torch.float64, device="cuda") for k, w in (("p", ev.np), ("x", ev.nvar), ("y", ev.m))}
    t["P"] = torch.full((B, ev.nnzP), 0.25, dtype=torch.float64, device="cuda")
    t["C"] = torch.full((B, ev.nnzP), float("nan"), dtype=torch.float64, device="cuda")
    a = LagrangianArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr() or None)
    a.mode = 0
    for k, v in over.items():
        setattr(a, k, v)
    return a, t


def test_argument_errors_leave_the_handle_usable(evaluators):
    from optimal_control_problem_amd.general_eval import _bind
    L = _bind(_lib.lib())
    B = 3
    ev = evaluators("pendulum")
    kept = []

    def valid():
        a, t = _args(ev, B, mode=1)
        assert L.mpcqp_nlp_lagrangian(ev._h, B, C.byref(a), None) == _lib.OK
        torch.cuda.synchronize()
        assert not (t["P"] == 0.25).all() and torch.isfinite(t["P"]).all()

    def refused(handle=ev._h, batch=B, **over):
        a, t = _args(ev, B, **over)
        kept.append(t)
        rc = L.mpcqp_nlp_lagrangian(handle, batch, C.byref(a), None)
        valid()                                                                           # after each refusal a valid call still works
        return rc

    assert L.mpcqp_nlp_has_exact_hessian(ev._h) == 1 and L.mpcqp_nlp_has_exact_hessian(None) == 0
    assert refused(handle=None) == _lib.ERR_ARG and refused(batch=0) == _lib.ERR_ARG and refused(batch=-2) == _lib.ERR_ARG
    assert L.mpcqp_nlp_lagrangian(ev._h, B, None, None) == _lib.ERR_ARG
    for missing in ("p", "x", "y", "P"):
        assert refused(**{missing: None}) == _lib.ERR_ARG, missing
    assert refused(mode=1, C=None) == _lib.ERR_ARG
    for mode in (2, -1, 3):
        assert refused(mode=mode) == _lib.ERR_ARG, mode
    torch.cuda.synchronize()
    for t in kept:                                                                        # nothing was launched
        assert (t["P"] == 0.25).all() and torch.isnan(t["C"]).all()
    with pytest.raises(ValueError):
        a, t = _args(ev, B)
        ev.lagrangian(t["p"], t["x"], t["y"][:, :-1], t["P"])
    with pytest.raises(ValueError):
        ev.lagrangian(t["p"], t["x"], t["y"], t["P"], mode="project")


def test_library_without_the_export(built):
    from optimal_control_problem_amd.general_eval import GeneralEvaluator, _bind
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver
    L = _bind(_lib.lib())
    plain = ge.model("pendulum", False)
    old = GeneralEvaluator(plain)
    try:
        assert not old.has_exact_hessian and old.has_line_search and L.mpcqp_nlp_has_exact_hessian(old._h) == 0
        B = 2
        a, t = _args(old, B)
        rc = L.mpcqp_nlp_lagrangian(old._h, B, C.byref(a), None)
        assert rc == _lib.ERR_LIMIT
        msg = L.mpcqp_strerror(rc).decode()
        assert "mpcqp_general_lagrangian" in msg and "exact_hessian=True" in msg
        torch.cuda.synchronize()
        assert (t["P"] == 0.25).all()
        f, g = old.merit(t["p"], t["x"], lbg=torch.zeros((B, old.ng), dtype=torch.float64, device="cuda"),
                         ubg=torch.zeros((B, old.ng), dtype=torch.float64, device="cuda"))  # the rest of the handle works
        torch.cuda.synchronize()
        assert not torch.isnan(f).any()
        with pytest.raises(ValueError, match="general evaluator"):                           # a flagged model on an unflagged library
            DeviceSQPOptimizationSolver(ge.model("pendulum"), {"max_iter": 1, "alpha": 1.0, "exact_hessian": True}, batch=B, evaluator=old)
        with pytest.raises(ValueError, match="without exact_hessian=True"):                  # ... and an unflagged model on it
            DeviceSQPOptimizationSolver(plain,{"max_iter": 1, "alpha": 1.0, "exact_hessian": "dominant"}, batch=B, evaluator=old)
    finally:
        old.close()


def test_a_captured_graph_replays_eval_and_lagrangian(evaluators):
    """nothing is allocated inside the calls and nothing synchronises: eval -> lagrangian on caller-owned buffers capture into a single-stream
    graph, and the replay gives the bits of the eager run"""
    from optimal_control_problem_amd.general_eval import LagrangianArgs
    ev = evaluators("pendulum")
    c = ge.case("pendulum")
    B = ge.BATCH
    _, eager, Ce, se = _launch(ev, c, "dominant", y=c["ynan"], status=c["status"])
    t = {k: _dev(c[k]) for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")}
    y = _dev(c["ynan"]); st = _dev(c["status"], torch.int32)
    out = ev.alloc(B)
    Cw = torch.full((B, ev.nnzP), float("nan"), dtype=torch.float64, device="cuda"); shift = torch.zeros((B, ev.n), dtype=torch.float64, device="cuda")
    a = LagrangianArgs()
    a.p, a.x, a.y, a.status, a.P, a.C, a.mode, a.shift = (t["p"].data_ptr(), t["x"].data_ptr(), y.data_ptr(), st.data_ptr(), out["P"].data_ptr(),
                                                            Cw.data_ptr(), 1, shift.data_ptr())
    L = _lib.lib()
    s = torch.cuda.Stream(); gr = torch.cuda.CUDAGraph()
    ptrs = [t[k].data_ptr() for k in ("p", "x", "lbx", "ubx", "lbg", "ubg")] + [out[k].data_ptr() for k in ("P", "q", "A", "l", "u")]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            _lib.check(L.mpcqp_nlp_eval(ev._h, B, *ptrs, s.cuda_stream))
            _lib.check(L.mpcqp_nlp_lagrangian(ev._h, B, C.byref(a), s.cuda_stream))
        out["P"].fill_(float("nan")); Cw.fill_(float("nan")); shift.zero_()                  # (whatever the capture did or did not run)
        gr.replay(); s.synchronize()
        again = out["P"].clone()
        gr.replay(); s.synchronize()                                                        # eval rewrites P: a second replay gives the same
    cur = ge.slots(c["model"])[0]
    assert _bits(out["P"].cpu().numpy(), eager) and _bits(again.cpu().numpy(), eager)
    assert _bits(shift.cpu().numpy(), se) and _bits(Cw.cpu().numpy()[:, cur], Ce[:, cur])


# ------------------------------------------------------------------------------------------------ the two loops on the recipe
@pytest.mark.parametrize("search", [False, True])
def test_device_loop_equals_host_loop(built, search):
    """iteration by iteration with "dominant" in both loops; the host loop solves its QPs on the CPU oracle at the loop's own 1e-3"""
    from optimal_control_problem_amd.general_eval import GeneralEvaluator
    from optimal_control_problem_amd.sqp import DeviceSQPOptimizationSolver, SQPOptimizationSolver
    from tests.support.oracle_backend import OracleCuCaQP
    mdl, arg, x0 = ge.recipe()
    B = x0.shape[0]
    opt = {"max_iter": 1, "alpha": 1.0, "exact_hessian": "dominant", "skip_failed_steps": True}
    if search:
        opt["line_search"] = True
    host = SQPOptimizationSolver(mdl, opt, batch=B, qp_solver=OracleCuCaQP(B))
    dev = DeviceSQPOptimizationSolver(mdl, opt, batch=B, evaluator=GeneralEvaluator(mdl))
    worst = 0.0
    try:
        assert dev.ev.has_exact_hessian and dev._nlp_mode == 1
        host.setInitialGuess(x0); dev.setInitialGuess(x0)
        for it in range(6):
            # the shift both loops put into this iteration's QP, from the same statement on each loop's own iterate and multipliers
            ref_shift = mdl.lagrangian_system(arg["p"], dev.x.cpu().numpy(), dev.lam.cpu().numpy(),
                                              mdl.local_system(arg["p"], dev.x.cpu().numpy(), arg["lbx"], arg["ubx"], arg["lbg"], arg["ubg"]).P, None, 1)[1]
            rh = host.getOptimalSolution(arg); rd = dev.getOptimalSolution(arg)
            assert gp.close(dev.shift.cpu().numpy(), ref_shift, ge.TOL), (search, it)
            scale = 1.0 + np.abs(rh["x"]).max()
            dist = np.abs(rd["x"] - rh["x"]).max()
            worst = max(worst, dist / scale)
            print(search, it, "max |x_dev - x_host|", dist, "shift max", float(dev.shift.max()))
            assert dist <= 1e-6 * scale, (search, it, dist)
            print("   shift dev - host", np.abs(dev.shift.cpu().numpy() - host.shift).max(), "lam dev - host", np.abs(dev.lam.cpu().numpy() - host.lam).max(),
                  "" if not search else "alpha dev %s host %s" % (dev.alpha_taken.cpu().numpy(), host.alpha_taken))
        print("search", search, "worst distance / (1 + max|x|) over 6 iterations", worst)
    finally:
        dev.close()


def test_example_runs(built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "general_exact_hessian.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.strip().split("\n") if "last step" in l]
    assert len(lines) == 2 and lines[0].startswith("hessian(f, w)") and lines[1].startswith("exact_hessian = 'dominant'")
    worst = [float(l.split("..")[1].split(",")[0]) for l in lines]                          # the largest last step of each leg
    print(r.stdout)
    assert worst[1] < 1e-6 < worst[0]
