// Host access to the pattern builders of csrc/stage_models.hpp with a link cost, for tests/test_link_cost_host.py -- TEST INFRASTRUCTURE ONLY.
#include "../../optimal_control_problem_amd/csrc/stage_models.hpp"

extern "C" {
// cost_mask: (f + nx)^2 bytes or null (diagonal weights); lmask: (2 f)^2 bytes or null.  First call with Pi = Ai = null for the sizes.
void link_cost_pattern(int nx, int nu, int N, int nh, int nk, int pref, const unsigned char *cost_mask, const unsigned char *lmask,
                       int *Pp, int *Pi, int *Ap, int *Ai, int *nnz /* [2] */) {
  std::vector<int> a, b, c, d;
  sm_build_pattern(nx, nu, N, nh, nk, a, b, c, d, pref != 0, lmask);
  if (cost_mask) sm_build_cost_pattern(nx, nu, N, cost_mask, a, b, pref != 0, lmask);
  nnz[0] = (int)b.size(); nnz[1] = (int)d.size();
  if (!Pi || !Ai) return;
  for (size_t i = 0; i < a.size(); i++) Pp[i] = a[i];
  for (size_t i = 0; i < b.size(); i++) Pi[i] = b[i];
  for (size_t i = 0; i < c.size(); i++) Ap[i] = c[i];
  for (size_t i = 0; i < d.size(); i++) Ai[i] = d[i];
}
}
