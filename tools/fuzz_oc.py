#!/usr/bin/env python3
"""Randomised GPU-vs-oracle sweep of the on-chip mode (MPCQP_VARIANT=oc4) over stage-OCP patterns: random state / input sizes, horizons,
weights, nonlinear dynamics and iterates -- block tridiagonal + arrow patterns with single and twisted chains, phantom slots, hubs that
share their block with the last frame.  Sizes the instance does not take (ERR_LIMIT) are counted and skipped.  Each case: a cold solve
and a kept-workspace solve (new q, shifted bounds), against the oracle's.  usage: python tools/fuzz_oc.py [n_cases] [seed0] [oc4|oc8] [rf|rf25]
(oc8: the eight-wave instances for long chains -- horizons drawn so that the chain part is 21 ... 56 blocks; rf: MPCQP_RESUME_ROUNDS=0 and
adaptive_rho_tolerance = 1.5, so that an instance's second rho update already re-factorises in place in the iteration kernel -- the count of cold solves
with two or more updates is printed, a few per cent; rf25: also adaptive_rho_interval = 25 and rho = 1e-3, where a fifth of them have)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FAMILY = sys.argv[3] if len(sys.argv) > 3 else "oc4"
pairs = {}
os.environ["MPCQP_VARIANT"] = FAMILY
RF = len(sys.argv) > 4 and sys.argv[4] in ("rf", "rf25")
SETTINGS = dict(adaptive_rho_tolerance=1.5) if RF else {}
if RF and sys.argv[4] == "rf25":
    SETTINGS.update(adaptive_rho_interval=25, rho=1e-3)
if RF:
    os.environ["MPCQP_RESUME_ROUNDS"] = "0"
import numpy as np

from optimal_control_problem_amd import _lib, models
from optimal_control_problem_amd.batch_qp import BatchQP
from oracle import oracle as orc
from tests.support.problems import oracle_rho_updates, random_stage_ocp

ncase = int(sys.argv[1]) if len(sys.argv) > 1 else 30
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
tight = soft = bad = skipped = inplace = cold = 0
for c in range(ncase):
    ls, dims, rng = random_stage_ocp(seed0 + c, FAMILY); B = ls.batch
    try:
        qp = BatchQP(ls.n, ls.m, B, ls.Pp, ls.Pi, ls.Ap, ls.Ai, **SETTINGS)
    except _lib.MpcqpError as e:
        if e.code == _lib.ERR_LIMIT:
            skipped += 1; continue
        raise
    assert qp.plan_info()["variant"] == (208 if FAMILY == "oc8" else 204)
    pairs[qp.oc_info().get("chain_pairs", 1)] = pairs.get(qp.oc_info().get("chain_pairs", 1), 0) + 1
    qp.keep_workspace(True)
    if RF:
        inplace += int((oracle_rho_updates(ls, **SETTINGS) >= 2).sum()); cold += B
    pat = orc.Pattern(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai); st = orc.State(pat, B, orc.default_settings(**SETTINGS))
    q2 = ls.q * 1.2 + 0.05 * rng.normal(size=ls.q.shape); sh = 0.02 * rng.normal(size=ls.l.shape)
    for tag, run_g, run_o in (("cold", lambda: (qp.update(ls.P, ls.q, ls.A, ls.l, ls.u), qp.solve(), qp.get())[2], lambda: st.solve(ls.P, ls.q, ls.A, ls.l, ls.u)),
                              ("kept", lambda: (qp.update_vectors(q2, ls.l + sh, ls.u + sh), qp.solve(), qp.get())[2], lambda: st.solve_vectors(q2, ls.l + sh, ls.u + sh))):
        got, ref = run_g(), run_o()
        fin = np.isfinite(ref["x"])
        err = np.abs(got["x"][fin] - ref["x"][fin]).max() / (1 + np.abs(ref["x"][fin]).max()) if fin.any() else 0.0
        same = (got["status"] == ref["status"]).all() and np.array_equal(np.isfinite(got["x"]), fin)
        if same and (got["iters"] == ref["iters"]).all() and err <= 1e-6:
            tight += 1
        elif same and err <= 2e-2 and ref["iters"].max() >= 200:
            soft += 1; print("tolerance-level %s case %d %s iters %s/%s rel err %.2e" % (tag, c, dims, got["iters"], ref["iters"], err))
        else:
            bad += 1; print("MISMATCH %s case %d %s status %s/%s iters %s/%s rel err %.2e" % (tag, c, dims, got["status"], ref["status"], got["iters"], ref["iters"], err))
    qp.close()
print("patterns by twisted pairs of chains (1 = plain / twisted order, more = the dissected order): %s" % dict(sorted(pairs.items())))
if RF:
    print("cold solves with two or more rho updates (the second re-factorises in place): %d of %d" % (inplace, cold))
print("done: %d cases (%d skipped: outside the instance's limits), %d solves at the tight bar, %d tolerance-level, %d mismatches" % (ncase, skipped, tight, soft, bad))
sys.exit(1 if bad else 0)
