// k_oc_rescale.hip -- instances of mpcqp_oc_rescale_kernel (kernel_oc_rescale.hpp): new matrices on a kept workspace (mpcqp_update_matrices).
// Four waves only: the set-up side of the two-kernel form runs four-wave workgroups whatever the iteration kernel's shape (select.hpp SetupShape).
#include "kernels_all.hpp"
#include "kernel_oc_rescale.hpp"
MPCQP_HIDDEN const void *mpcqp_kernel_oc_rescale(int nw, bool hub) {
  if (nw == 4) return hub ? (const void *)mpcqp_oc_rescale_kernel<4, true> : (const void *)mpcqp_oc_rescale_kernel<4, false>;
  return nullptr;
}
