// k_oc_admm_soft_p4.hip -- the soft-row twins (mpcqp_set_soft_rows) of k_oc_admm_p4.hip's instances: four waves, two twisted pairs of chains
#include "kernels_all.hpp"
MPCQP_HIDDEN const void *mpcqp_kernel_oc_admm_soft_p4(int rf) {
  return rf ? (const void *)mpcqp_oc_admm_soft_kernel<4, OC_NG, OC_NH, 1, true> : (const void *)mpcqp_oc_admm_soft_kernel<4, OC_NG, OC_NH, 0, true>;
}
