// general_lagrangian.hpp -- the parts of mpcqp_nlp_lagrangian (include/mpcqp.h; general_nlp.GeneralNLP.lagrangian_system is its NumPy statement)
// that the gfx950 kernels (general_kernels.hpp: general_curvature_kernel, general_curvature_apply_kernel) and general_host_lagrangian (the g++
// build codegen.py generates for checks without a GPU) share as host/device functions: the accessor of the multipliers, the sink of a curvature
// pass and the walk over one column of P with the DOMINANT safeguard.  Both compile THIS text, so the two can differ by compiler contraction and
// libm only.  M is the generated functor of a model built with exact_hessian=True: its tables ccols, cptr, clist, cdiag are those of
// general_eval.compress_curvature.
#pragma once
#include "stage_models.hpp"
#include "../../include/mpcqp.h"

// the multipliers of the general rows: plain values, as theta enters the stage bodies
struct GnMulIn {
  const double *y;
  SM_HD double operator()(int i) const { return y[i]; }
};

// the dual part of output r of a curvature pass is entry (r, c) of C, c the one column of the pass's colour with row r: it goes to that entry's
// slot of the workspace, or -- mode 0 without a workspace -- is added to P there (read, add, write; a zero leaves the bits of P)
struct GnCurvOut {
  double *dst; const int *slot; bool add;
  SM_HD void operator()(int r, Dual v) const {
    const int s = slot[r];
    if (s < 0) return;
    if (!add) dst[s] = v.d;
    else if (v.d != 0.0) dst[s] = dst[s] + v.d;
  }
};

// column ccols[ci] of one instance: P[s] += C[s] over the column's curvature slots in ascending order, R = sum of |C| off the diagonal in the same
// order; with the safeguard d = max(0, R - C_cc) is added to the diagonal slot after its own C, and written to shift when that is asked for.
// C + diag(d) is then diagonally dominant with a non-negative diagonal, hence positive semidefinite.  A zero addend leaves the bits of P.
template <class M>
SM_HD void gn_lag_apply_column(int ci, const double *C, double *P, bool dominant, double *shift) {
  const int dg = M::cdiag[ci];
  double R = 0.0, cd = 0.0;
  for (int k = M::cptr[ci]; k < M::cptr[ci + 1]; k++) {
    const int s = M::clist[k];
    const double c = C[s];
    if (c != 0.0) P[s] = P[s] + c;
    if (s == dg) cd = c; else R += fabs(c);
  }
  if (dominant) {
    const double d = fmax(0.0, R - cd);
    if (d > 0.0) P[dg] = P[dg] + d;
    if (shift) shift[M::ccols[ci]] = d;
  }
}
