// kernel_table.hpp -- where mpcqp.hip finds the kernel instances that other translation units instantiate (k_*.hip); nullptr = no such instance
#pragma once
#define MPCQP_HIDDEN __attribute__((visibility("hidden")))
#include "select.hpp"      // OC_NG, OC_NH, OC8_INST: the shapes of the on-chip instances are part of the selection policy

// (the instances with and without the kept-workspace entry are separate translation units: _r1 / _r0)
// mpcqp_res_kernel<NW, MINW, false, REUSE>: factor in LDS
MPCQP_HIDDEN const void *mpcqp_kernel_res_lds_r0(int nw, int minw);
MPCQP_HIDDEN const void *mpcqp_kernel_res_lds_r1(int nw, int minw);
// mpcqp_res_kernel<NW, MINW, true, REUSE, ZYG>: factor streamed from the slab
MPCQP_HIDDEN const void *mpcqp_kernel_res_gb_r0(int nw, int minw, bool zyg);
MPCQP_HIDDEN const void *mpcqp_kernel_res_gb_r1(int nw, int minw, bool zyg);
// mpcqp_res_kernel<NW, 2, true, REUSE, false, NG, NH, TL>: the on-chip mode as one kernel (the tile experiment; MPCQP_OC_MONO=1 for A/B runs)
MPCQP_HIDDEN const void *mpcqp_kernel_oc_mono_r0(int nw, int ng, int nh, bool tiles);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_mono_r1(int nw, int ng, int nh, bool tiles);
// kernel_oc_split.hpp: the on-chip mode as set-up + iteration kernels
MPCQP_HIDDEN const void *mpcqp_kernel_oc_setup(int nw, bool hub, bool reuse);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_rescale(int nw, bool hub);            // kernel_oc_rescale.hpp: new matrices, kept D, E, c and rho (mpcqp_update_matrices)
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm(int nw, int ng, int nh);        // leaves for a re-factorisation
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_rf(int nw, int ng, int nh);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_p4(int rf);                      // four waves, two twisted pairs of chains (dissected order)
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_tl(int nw, int ng, int nh);     // sweeps on dense tiles of A (experiment, MPCQP_VTILES=1)     // re-factorises in place (the last launch of a solve)
// mpcqp_oc_admm_soft_kernel: the soft-row twins of the three iteration tables above (mpcqp_set_soft_rows; k_oc_admm_soft*.hip); the tile experiment has none
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_soft(int nw, int ng, int nh);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_soft_rf(int nw, int ng, int nh);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_soft_p4(int rf);

// kernel_polish.hpp (k_polish.hip): OSQP's polishing as a post-solve kernel, one wavefront per instance of a slice.  Per-instance pointers stand at the
// slice's first instance (the kernel indexes by blockIdx); `fac` is the polish factor's own scratch (Lf, Lb, T of one instance: fac_stride doubles)
struct DevPolish {
  const double *q; long sq;                 // the caller's (or the handle's owned) q
  double *x, *y, *z; const int *status; double *info;      // the handle's outputs: the ADMM result in, the accepted candidate out
  const double *ws, *cscale;                // per-QP slabs (scaled A, A', P, l, u, D, E) and c
  double *fac; long fac_stride;
  int *pstatus; double *pinfo;              // MPCQP_POLISH_* and {objective, primal residual, dual residual, active rows} of the candidate
  double delta; int refine;
  const int *skip;                          // mpcqp_set_skip: per instance of the slice, nonzero = leave it as it is (NULL = none)
};
MPCQP_HIDDEN size_t mpcqp_polish_lds(const DevPlan &pl);           // dynamic LDS of one workgroup, bytes
MPCQP_HIDDEN long mpcqp_polish_fac_doubles(const DevPlan &pl);     // scratch of one instance, doubles
MPCQP_HIDDEN int mpcqp_polish_prepare(const DevPlan &pl, int device);      // raises the kernel's dynamic-LDS limit where the handle needs it; MPCQP_ERR_LIMIT when it cannot fit
MPCQP_HIDDEN int mpcqp_polish_launch(const DevPlan &pl, const mpcqp_settings &st, const DevPolish &po, int count, hipStream_t s);
