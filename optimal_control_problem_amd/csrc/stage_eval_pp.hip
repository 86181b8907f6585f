// stage_eval_pp.hip -- the zoo's per-instance-parameter (PP) instances of the five stage kernels that call F (stage_kernels.hpp; mpcqp_stage_set_instance_params
// in include/mpcqp.h): quadrotor and cart-pole, each with one shared reference and with per-frame references.  The double integrator
// has no parameters and no instance here.  A translation unit of its own, so that these eighteen instances compile beside stage_eval.hip's.
#include <hip/hip_runtime.h>

#include "../../include/mpcqp.h"
#include "stage_kernels.hpp"

// (an invalid value is not reached: mpcqp_stage_set_instance_params refuses a model without parameters)
hipError_t mpcqp_launch_eval_pp(const StageDev &sd, int batch, const StageEvalArgs &a, hipStream_t st, StageTheta th) {
  return stage_visit_zoo<true>(sd.model, sd.pref, [&](auto t) { using T = decltype(t); return stage_launch_eval<typename T::M, T::PF>(sd, batch, a, st, th); });
}

hipError_t mpcqp_launch_merit_pp(const StageDev &sd, int batch, const StageMeritArgs &a, hipStream_t st, StageTheta th) {
  return stage_visit_zoo<true>(sd.model, sd.pref, [&](auto t) { using T = decltype(t); return stage_launch_merit<typename T::M, T::PF>(sd, batch, a, st, th); });
}

hipError_t mpcqp_launch_advance_pp(const StageDev &sd, int batch, const mpcqp_stage_advance_args &a, hipStream_t st, StageTheta th) {
  return stage_visit_zoo<true>(sd.model, sd.pref, [&](auto t) { using T = decltype(t); return stage_launch_advance<typename T::M, T::PF>(sd, batch, a, st, th); });
}

hipError_t mpcqp_launch_linesearch_pp(const StageDev &sd, int batch, const mpcqp_stage_linesearch_args &a, hipStream_t st, StageTheta th) {
  return stage_visit_zoo<true>(sd.model, sd.pref, [&](auto t) { using T = decltype(t); return stage_launch_linesearch<typename T::M, T::PF>(sd, batch, a, st, th); });
}

hipError_t mpcqp_launch_rollout_pp(const StageDev &sd, int batch, const mpcqp_stage_rollout_args &a, hipStream_t st, StageTheta th) {
  return stage_visit_zoo<true>(sd.model, sd.pref, [&](auto t) { using T = decltype(t); return stage_launch_rollout<typename T::M>(sd, batch, a, st, th); });
}
