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
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm(int nw, int ng, int nh);        // leaves for a re-factorisation
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_rf(int nw, int ng, int nh);
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_p4(int rf);                      // four waves, two twisted pairs of chains (dissected order)
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_tl(int nw, int ng, int nh);     // sweeps on dense tiles of A (experiment, MPCQP_VTILES=1)     // re-factorises in place (the last launch of a solve)
