// common.hpp -- helpers shared by the translation units of libmpcqp.so (not part of the ABI)
#pragma once
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/mpcqp.h"

// records the message mpcqp_strerror() appends, returns `code` (defined in mpcqp.hip)
__attribute__((visibility("hidden"))) int mpcqp_set_error(int code, const std::string &msg);
// picks / validates the device like mpcqp_create: ordinal < 0 = current device; must be gfx950
__attribute__((visibility("hidden"))) int mpcqp_pick_device(int requested, int *device);

#define MPCQP_HIPCHK(expr)                                                                                              \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mpcqp_set_error(MPCQP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
// the damped update x += alpha * dw[np:] of both evaluators (stage_eval.hip: stage_step_kernel depends on the dimensions only); asynchronous on `st`
__attribute__((visibility("hidden"))) hipError_t mpcqp_launch_step(int batch, int nvar, int n, int np, double alpha, const double *dw, double *x,
                                                                    double *step_max, const int *status, hipStream_t st);
// the optimality residuals of both evaluators (kkt.hip: the kernel depends on the pattern of A only).  _upload: at handle creation, on the handle's
// device: checks that every index lies inside its array and puts Ap, then Ai, into one allocation *dpat (the handle frees it).  _run: checks batch
// and the argument block and launches on `stream` -- no allocation, no copy, no synchronisation.  Both return an MPCQP code
__attribute__((visibility("hidden"))) int mpcqp_kkt_upload(int n, int m, int col0, const std::vector<int> &Ap, const std::vector<int> &Ai, int **dpat);
__attribute__((visibility("hidden"))) int mpcqp_kkt_run(int device, int n, int m, int col0, int nnzA, const int *dpat, int batch, const mpcqp_kkt_args *a,
                                                         void *stream);
// makes work queued on `s` from here on wait for the handle's last solve if that ran on another stream (a caller that rewrites arrays the
// handle borrows -- mpcqp_stageqp_update's packed P and A -- calls this first); defined in mpcqp.hip
__attribute__((visibility("hidden"))) int mpcqp_order_after_last_solve(mpcqp_handle *h, hipStream_t s);
