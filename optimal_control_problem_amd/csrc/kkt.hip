// kkt.hip -- the one instantiation of the optimality-residual kernels (kkt_kernels.hpp) and what mpcqp_stage_kkt (stage_eval.hip) and
// mpcqp_nlp_kkt (general_eval.hip) share: the upload of a handle's pattern when the handle is created, the argument checks, the launch.  Generated libraries
// take no part in this: the kernel depends on the pattern alone.
#include <hip/hip_runtime.h>
#include <vector>

#include "../../include/mpcqp.h"
#include "common.hpp"
#include "kkt_kernels.hpp"

int mpcqp_kkt_upload(int n, int m, int col0, const std::vector<int> &Ap, const std::vector<int> &Ai, int **dpat) {
  const int nnzA = (int)Ai.size();
  // every address the kernel forms lies inside its array: the column pointers walk [0, nnzA], the row indices stay below m
  bool ok = (int)Ap.size() == n + 1 && Ap[0] == 0 && Ap[n] == nnzA && col0 >= 0 && col0 <= n;
  for (int j = 0; ok && j < n; j++) ok = Ap[j + 1] >= Ap[j];
  for (int e = 0; ok && e < nnzA; e++) ok = Ai[e] >= 0 && Ai[e] < m;
  if (!ok) return mpcqp_set_error(MPCQP_ERR_ARG, "the handle's pattern of A is inconsistent");
  std::vector<int> tab(Ap);
  tab.insert(tab.end(), Ai.begin(), Ai.end());
  int *p = nullptr;
  MPCQP_HIPCHK(hipMalloc(&p, tab.size() * sizeof(int)));
  if (hipMemcpy(p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the pattern of A failed");
  }
  *dpat = p;
  return MPCQP_OK;
}

int mpcqp_kkt_run(int device, int n, int m, int col0, int nnzA, const int *dpat, int batch, const mpcqp_kkt_args *a, void *stream) {
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->q || !a->A || !a->l || !a->u || !a->y || !a->res) return mpcqp_set_error(MPCQP_ERR_ARG, "q, A, l, u, y and res are required");
  if (!(a->tol_stat >= 0.0) || !(a->tol_feas >= 0.0) || !(a->tol_compl >= 0.0))
    return mpcqp_set_error(MPCQP_ERR_ARG, "the tolerances must not be negative or NaN");
  if (!dpat) return mpcqp_set_error(MPCQP_ERR_STATE, "the handle holds no pattern of A on the device");
  MPCQP_HIPCHK(hipSetDevice(device));
  const KktDims d{n, m, col0, nnzA, dpat, dpat + n + 1};
  MPCQP_HIPCHK(kkt_launch(batch, d, *a, (hipStream_t)stream));
  return MPCQP_OK;
}
