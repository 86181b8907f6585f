"""Solution polishing (OSQP's `polishing`; OsqpEigen::Settings::setPolish) on the quadrotor batch at the reference's tolerance: the same solve with and
without the polish kernel behind it, residuals recomputed on the host from the caller's data.  The reference leaves polishing off, and so does the
default here; BatchQP.set_polish() switches it on per handle.  Needs an MI355X."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from optimal_control_problem_amd import BatchQP, models  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
mdl, ls, meta = models.make_workload("quadrotor", batch)


def host_residuals(x, y, b):
    """max-norm primal and dual residual of instance b from the caller's CSC arrays"""
    cols = np.repeat(np.arange(ls.n), np.diff(ls.Ap)); pcols = np.repeat(np.arange(ls.n), np.diff(ls.Pp))
    ax = np.zeros(ls.m); np.add.at(ax, ls.Ai, ls.A[b] * x[cols])
    aty = np.zeros(ls.n); np.add.at(aty, cols, ls.A[b] * y[ls.Ai])
    up = ls.Pi <= pcols                                               # the upper triangle is what the engine reads
    px = np.zeros(ls.n); np.add.at(px, ls.Pi[up], ls.P[b][up] * x[pcols[up]])
    lo = up & (ls.Pi < pcols); np.add.at(px, pcols[lo], ls.P[b][lo] * x[ls.Pi[lo]])
    z = np.clip(ax, ls.l[b], ls.u[b])
    return np.abs(ax - z).max(), np.abs(px + ls.q[b] + aty).max()


sample = range(0, batch, max(1, batch // 32))
for polish in (False, True):
    qp = BatchQP(ls.n, ls.m, ls.batch, ls.Pp, ls.Pi, ls.Ap, ls.Ai)     # eps_abs = eps_rel = 1e-3 as the reference sets them
    if polish:
        qp.set_polish(True)                                            # delta = 1e-6, refine_iter = 3: OSQP's defaults
    for _ in range(2):
        qp.update(ls.P, ls.q, ls.A, ls.l, ls.u); qp.solve(); qp.sync()
    res = qp.get()
    r = np.array([host_residuals(res["x"][b], res["y"][b], b) for b in sample])
    line = "polishing %s: kernel %.2f ms" % ("on " if polish else "off", qp.last_kernel_ms())
    if polish:
        line += " + polish %.2f ms, polished %d of %d" % (qp.last_polish_ms(), (res["polish_status"] == 1).sum(), batch)
    print(line + "; host-recomputed residuals on %d instances: primal median %.2e max %.2e, dual median %.2e max %.2e"
          % (len(r), np.median(r[:, 0]), r[:, 0].max(), np.median(r[:, 1]), r[:, 1].max()))
    qp.close()
