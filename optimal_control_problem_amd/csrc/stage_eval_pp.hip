// stage_eval_pp.hip -- the zoo's per-instance-parameter (PP) instances of the four stage kernels that call F (stage_kernels.hpp; mpcqp_stage_set_instance_params
// in include/mpcqp.h): quadrotor and cart-pole, each with one shared reference and with per-frame references.  The double integrator
// has no parameters and no instance here.  A translation unit of its own, so that these sixteen instances compile beside stage_eval.hip's.
#include <hip/hip_runtime.h>

#include "../../include/mpcqp.h"
#include "stage_kernels.hpp"

hipError_t mpcqp_launch_eval_pp(const StageDev &sd, int batch, const double *p, const double *x, const double *lbx, const double *ubx, const double *lbg,
                                const double *ubg, double *P, double *q, double *A, double *l, double *u, hipStream_t st, StageTheta th) {
  switch (sd.model) {
    case SM_QUADROTOR: return sd.pref ? stage_launch_eval<SmQuadrotor, true>(sd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, st, th)
                                      : stage_launch_eval<SmQuadrotor, false>(sd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, st, th);
    case SM_CARTPOLE: return sd.pref ? stage_launch_eval<SmCartPole, true>(sd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, st, th)
                                     : stage_launch_eval<SmCartPole, false>(sd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, st, th);
  }
  return hipErrorInvalidValue;      // (not reached: mpcqp_stage_set_instance_params refuses a model without parameters)
}

hipError_t mpcqp_launch_merit_pp(const StageDev &sd, int batch, const double *p, const double *x, double *f, double *gmax, hipStream_t st, StageTheta th) {
  switch (sd.model) {
    case SM_QUADROTOR: return sd.pref ? stage_launch_merit<SmQuadrotor, true>(sd, batch, p, x, f, gmax, st, th) : stage_launch_merit<SmQuadrotor, false>(sd, batch, p, x, f, gmax, st, th);
    case SM_CARTPOLE: return sd.pref ? stage_launch_merit<SmCartPole, true>(sd, batch, p, x, f, gmax, st, th) : stage_launch_merit<SmCartPole, false>(sd, batch, p, x, f, gmax, st, th);
  }
  return hipErrorInvalidValue;
}

hipError_t mpcqp_launch_advance_pp(const StageDev &sd, int batch, const mpcqp_stage_advance_args &a, hipStream_t st, StageTheta th) {
  switch (sd.model) {
    case SM_QUADROTOR: return sd.pref ? stage_launch_advance<SmQuadrotor, true>(sd, batch, a, st, th) : stage_launch_advance<SmQuadrotor, false>(sd, batch, a, st, th);
    case SM_CARTPOLE: return sd.pref ? stage_launch_advance<SmCartPole, true>(sd, batch, a, st, th) : stage_launch_advance<SmCartPole, false>(sd, batch, a, st, th);
  }
  return hipErrorInvalidValue;
}

hipError_t mpcqp_launch_linesearch_pp(const StageDev &sd, int batch, const mpcqp_stage_linesearch_args &a, hipStream_t st, StageTheta th) {
  switch (sd.model) {
    case SM_QUADROTOR: return sd.pref ? stage_launch_linesearch<SmQuadrotor, true>(sd, batch, a, st, th) : stage_launch_linesearch<SmQuadrotor, false>(sd, batch, a, st, th);
    case SM_CARTPOLE: return sd.pref ? stage_launch_linesearch<SmCartPole, true>(sd, batch, a, st, th) : stage_launch_linesearch<SmCartPole, false>(sd, batch, a, st, th);
  }
  return hipErrorInvalidValue;
}
