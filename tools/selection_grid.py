#!/usr/bin/env python3
"""Records what the library's kernel selection decides over a grid of patterns, batches, forced families and knobs:
plan_info(), oc_info(), the CU count and the set-up kernel's launch shape (the MPCQP_VERBOSE line) of one handle per row.

usage (GPU box): python tools/selection_grid.py [out.json]        (default: tests/golden/selection_grid.json)

tests/golden/selection_grid.json is this tool's output for the library of the commit BEFORE select_kernel existed; tests/test_select.py
holds the CPU function (csrc/select.hpp through tests/support/libplan_interp.so) against it row by row, and test_gpu_parity.py the library.
MPCQP_LIB=<other libmpcqp.so> records another build for a byte-for-byte comparison of the two files."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.support import problems  # noqa: E402

HORIZONS = {"double_integrator": [10, 20, 24, 30, 60, 100, 120],
            "cartpole": [10, 15, 20, 22, 24, 25, 30, 40, 50, 60, 65, 100, 150],
            "quadrotor": [5, 7, 10, 20, 30, 40, 50, 55, 56, 57]}
BATCHES = [64, 1024, 8192]
FAMILIES = ["stream", "res1", "res2", "res4", "res8", "gres4", "gres2", "oc4", "oc8"]


def row(workload, N, batch, env=None, reduced=False):
    return {"workload": workload, "N": N, "batch": batch, "env": dict(env or {}), "reduced": bool(reduced)}


def rows():
    """every threshold of the rule from both sides, then the hub-less patterns, every family forced where it takes the pattern and
    where it refuses it, and every selection knob alone where it changes what is reported"""
    out = [row(w, N, b) for w in ("double_integrator", "cartpole", "quadrotor") for N in HORIZONS[w] for b in BATCHES]
    out += [row("cartpole", 100, 16384), row("quadrotor", 55, 4096)]
    out += [row("quadrotor", 20, 8192, reduced=True), row("quadrotor", 50, 8192, reduced=True)]
    takes = {"gres2": ("double_integrator", 100), "oc8": ("quadrotor", 40)}
    refuses = {"oc4": ("quadrotor", 30), "oc8": ("quadrotor", 57), "stream": ("quadrotor", 200), "gres4": ("quadrotor", 300), "gres2": ("quadrotor", 200)}
    for fam in FAMILIES:
        w, N = takes.get(fam, ("quadrotor", 20))
        out.append(row(w, N, 64, {"MPCQP_VARIANT": fam}))
        w, N = refuses.get(fam, ("quadrotor", 57))
        out.append(row(w, N, 64, {"MPCQP_VARIANT": fam}))
    knobs = [("MPCQP_NO_TWIST", "1", "quadrotor", 20), ("MPCQP_NO_OC", "1", "quadrotor", 20), ("MPCQP_NO_RES2", "1", "double_integrator", 20),
             ("MPCQP_NO_OC8", "1", "quadrotor", 40), ("MPCQP_NO_DISSECT", "1", "cartpole", 100), ("MPCQP_NO_DISSECT", "1", "cartpole", 40),
             ("MPCQP_OC_MONO", "1", "quadrotor", 20), ("MPCQP_OC_MONO", "1", "quadrotor", 40), ("MPCQP_NO_PADTWIST", "1", "cartpole", 22),
             ("MPCQP_TILES", "1", "quadrotor", 20), ("MPCQP_VTILES", "1", "quadrotor", 20), ("MPCQP_DOUBLES", "4", "cartpole", 100),
             ("MPCQP_OC_PAD4", "1", "quadrotor", 20), ("MPCQP_NO_ZYG", "1", "quadrotor", 55), ("MPCQP_RESUME_ROUNDS", "3", "quadrotor", 20),
             ("MPCQP_LDS_MIN", "65536", "double_integrator", 20), ("MPCQP_NO_IX16", "1", "cartpole", 40), ("MPCQP_SETUP_CAP", "81920", "quadrotor", 20)]
    out += [row(w, N, 8192, {k: v}) for k, v, w, N in knobs]
    return out


class capture_stderr:
    """what the C library writes to file descriptor 2 while the block runs"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(); self.saved = os.dup(2); os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0); self.text = self.tmp.read().decode(); self.tmp.close()


def record(r):
    from optimal_control_problem_amd import _lib
    from optimal_control_problem_amd.batch_qp import BatchQP
    n, m, Pp, Pi, Ap, Ai, fixed = problems.selection_pattern(r)
    env = dict(r["env"], MPCQP_VERBOSE="1")
    os.environ.update(env)
    res = dict(r)
    try:
        with capture_stderr() as cap:
            try:
                qp = BatchQP(n, m, r["batch"], Pp, Pi, Ap, Ai, fixed_rows=fixed)
                res["rc"] = 0
                pi, oi = qp.plan_info(), qp.oc_info()
                qp.close()
            except _lib.MpcqpError as e:
                res["rc"] = e.code
    finally:
        for k in env:
            os.environ.pop(k, None)
    if res["rc"] == 0:
        pi.pop("tiles")
        res["plan_info"] = pi; res["oc_info"] = oi
        shape = [l for l in cap.text.splitlines() if l.startswith("mpcqp: set-up kernel shape:")]
        res["setup_shape"] = shape[0] if shape else None
    return res


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "selection_grid.json")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t0 = time.perf_counter()
    recs = [record(r) for r in rows()]
    codes = sorted({r["plan_info"]["variant"] for r in recs if r["rc"] == 0})
    with open(out, "w") as f:
        f.write(json.dumps({"multiProcessorCount": cus, "rows": recs}, indent=0, sort_keys=True) + "\n")
    print("%d rows (%d refused) in %.1f s, %d CUs, family codes %s -> %s" % (len(recs), sum(r["rc"] != 0 for r in recs), time.perf_counter() - t0, cus, codes, out))


if __name__ == "__main__":
    main()
