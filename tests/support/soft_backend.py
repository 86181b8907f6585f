"""A CuCaQP-shaped object backed by tests/support/soft_ref.py -- TEST INFRASTRUCTURE ONLY.  Lets the host-side SQP driver (optimal_control_problem_amd.sqp)
be exercised with options["soft_rows"] on a machine without a GPU; never used by the product.  Without setSoftRows every row is hard."""
import numpy as np

from tests.support import soft_ref


class SoftRefCuCaQP:
    def __init__(self, batch=1):
        self.batch = batch
        self.kw = {}; self.ls = None; self.res = None
        self.soft = None

    def setDimension(self, n, m):
        self.n, self.m = n, m
        return n > 0 and m > 0

    def setVerbosity(self, v): pass
    def setWarmStart(self, w): pass
    def setAbsoluteTolerance(self, t): self.kw["eps_abs"] = t
    def setRelativeTolerance(self, t): self.kw["eps_rel"] = t
    def setMaxIteration(self, k): self.kw["max_iter"] = k
    def setSystem(self, ls): self.ls = ls; self.res = None

    def setSoftRows(self, w1, w2=None):
        self.soft = None if w1 is None else (np.asarray(w1, float), None if w2 is None else np.asarray(w2, float))
        return True

    def initSolver(self): return self.ls is not None

    def solve(self):
        w1, w2 = self.soft if self.soft is not None else (None, None)
        self.res = soft_ref.solve_batch(self.ls, w1, w2, self.kw)
        return True

    def getSolutionAsDM(self): return self.res["x"]
    def getInfo(self): return self.res
