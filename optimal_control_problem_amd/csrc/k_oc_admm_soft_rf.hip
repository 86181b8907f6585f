// k_oc_admm_soft_rf.hip -- the soft-row twins (mpcqp_set_soft_rows) of k_oc_admm_rf.hip's instances: mpcqp_oc_admm_soft_kernel<..., RF = 1> (kernel_oc_split.hpp),
// the last launch of a solve, which re-factorises in place
#include "kernels_all.hpp"
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_soft_rf(int nw, int ng, int nh) {
  constexpr int RF = 1;
  if (nw == 4 && ng == OC_NG) {
    if (nh == OC_NH) return (const void *)mpcqp_oc_admm_soft_kernel<4, OC_NG, OC_NH, RF>;
    if (nh == 0) return (const void *)mpcqp_oc_admm_soft_kernel<4, OC_NG, 0, RF>;
    return nullptr;
  }
  if (nw == 8) {
    if (ng == OC8_INST[0].ng && nh == OC8_INST[0].nh) return (const void *)mpcqp_oc_admm_soft_kernel<8, OC8_INST[0].ng, OC8_INST[0].nh, RF>;
    if (ng == OC8_INST[1].ng && nh == OC8_INST[1].nh) return (const void *)mpcqp_oc_admm_soft_kernel<8, OC8_INST[1].ng, OC8_INST[1].nh, RF>;
    if (ng == OC8_INST[0].ng && nh == 0) return (const void *)mpcqp_oc_admm_soft_kernel<8, OC8_INST[0].ng, 0, RF>;
    if (ng == OC8_INST[1].ng && nh == 0) return (const void *)mpcqp_oc_admm_soft_kernel<8, OC8_INST[1].ng, 0, RF>;
  }
  return nullptr;
}
