// k_polish.hip -- the polish kernel (kernel_polish.hpp) and its launcher: the one translation unit that holds its device code
#include <map>
#include <mutex>
#include "kernels_all.hpp"
#include "kernel_polish.hpp"

size_t mpcqp_polish_lds(const DevPlan &pl) { return ((size_t)3 * pl.npad + (size_t)5 * pl.mpad + 2 * BS * 17) * sizeof(double); }
long mpcqp_polish_fac_doubles(const DevPlan &pl) { return (2L * pl.nblk + std::max(pl.nT, 1)) * BLK; }

int mpcqp_polish_prepare(const DevPlan &pl, int device) {
  const long want = (long)mpcqp_polish_lds(pl);
  if (want > 160 * 1024) return mpcqp_set_error(MPCQP_ERR_LIMIT, "polishing: the vectors of one QP exceed a CU's LDS");
  if (want <= 48 * 1024) return MPCQP_OK;
  // (a property of the kernel function, shared by every handle that launches it: a running maximum per device, as for the solve kernels)
  static std::mutex mu; static std::map<int, long> limit;
  std::lock_guard<std::mutex> lock(mu);
  long &cur = limit[device];
  if (want <= cur) return MPCQP_OK;
  MPCQP_HIPCHK(hipFuncSetAttribute((const void *)mpcqp_polish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
  cur = want;
  return MPCQP_OK;
}

int mpcqp_polish_launch(const DevPlan &pl, const mpcqp_settings &st, const DevPolish &po, int count, hipStream_t s) {
  hipLaunchKernelGGL(mpcqp_polish_kernel, dim3(count), dim3(WAVE), mpcqp_polish_lds(pl), s, pl, st, po);
  MPCQP_HIPCHK(hipGetLastError());
  return MPCQP_OK;
}
