// CPU harness for tests: the CSC structure builders of csrc/stage_models.hpp in tracking mode (per-frame references, p = [r_0; ...; r_{N-1}]),
// so that what mpcqp_stage_create_tracking hands to mpcqp_create is checked against models.py without a GPU.
#include <algorithm>
#include <vector>
#include "../../optimal_control_problem_amd/csrc/stage_models.hpp"

extern "C" {
// two-call protocol: sizes first (pointers null), then fill.  pref = 0 gives today's single-reference pattern through the same entry.
int sm_tracking_pattern(int nx, int nu, int N, int nh, int nk, int pref, int *nnzP, int *nnzA, int *Pp, int *Pi, int *Ap, int *Ai) {
  std::vector<int> a, b, c, d;
  sm_build_pattern(nx, nu, N, nh, nk, a, b, c, d, pref != 0);
  *nnzP = (int)b.size(); *nnzA = (int)d.size();
  if (Pp) { std::copy(a.begin(), a.end(), Pp); std::copy(b.begin(), b.end(), Pi); std::copy(c.begin(), c.end(), Ap); std::copy(d.begin(), d.end(), Ai); }
  return 0;
}
// mask: (2 nx + nu)^2 bytes, row-major, the Hessian's structure over [s; u; r]
int sm_tracking_cost_pattern(int nx, int nu, int N, const unsigned char *mask, int pref, int *nnzP, int *Pp, int *Pi) {
  std::vector<int> a, b;
  sm_build_cost_pattern(nx, nu, N, mask, a, b, pref != 0);
  *nnzP = (int)b.size();
  if (Pp) { std::copy(a.begin(), a.end(), Pp); std::copy(b.begin(), b.end(), Pi); }
  return 0;
}
}
