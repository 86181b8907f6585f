// StageSQP.hpp with setLineSearch: 8 cart-pole instances (N = 30), 4 SQP iterations from x = 0, first candidate alpha = 1, 4 candidates.
// Prints the iterate and the last iteration's step lengths for tests/test_gpu_linesearch.py, which runs the Python device loop on the same
// problem.  Exit code 0 = ran, 3 = no GPU (refused loudly), 1 = error.
#include <cstdio>
#include <limits>

#include "StageSQP.hpp"

int main() {
  const int B = 8, N = 30;
  mpcqp_stage_desc d;
  if (mpcqp_stage_default(MPCQP_MODEL_CARTPOLE, N, &d) != MPCQP_OK) return 1;
  try {
    StageSQP sqp(d, B, 4, 1.0);
    sqp.setLineSearch(4, 0.5, 1e-4);
    const int f = sqp.nx() + sqp.nu();
    const double inf = std::numeric_limits<double>::infinity();
    StageSQP::Arg a;
    a.p.assign((size_t)B * sqp.np(), 0.0); a.lbg.assign((size_t)B * sqp.ng(), 0.0); a.ubg.assign((size_t)B * sqp.ng(), 0.0);
    a.lbx.resize((size_t)B * sqp.nvar()); a.ubx.resize((size_t)B * sqp.nvar());
    for (int b = 0; b < B; b++)
      for (int k = 0; k < N; k++) {
        double *lo = &a.lbx[((size_t)b * N + k) * f], *hi = &a.ubx[((size_t)b * N + k) * f];
        for (int i = 0; i < f; i++) { lo[i] = -inf; hi[i] = inf; }
        lo[0] = -2.4; hi[0] = 2.4; lo[4] = -20.0; hi[4] = 20.0;                              // track and force limits
        if (k == 0) { for (int i = 0; i < f; i++) lo[i] = hi[i] = 0.0; lo[1] = hi[1] = 0.25 + 0.125 * b; }   // pole angle of the pinned frame
      }
    StageSQP::Result r = sqp.getOptimalSolution(a);
    if ((int)sqp.alphaTaken().size() != B) return 1;
    for (int b = 0; b < B; b++) {
      std::printf("x %d", b);
      for (int i = 0; i < sqp.nvar(); i++) std::printf(" %.17g", r.x[(size_t)b * sqp.nvar() + i]);
      std::printf("\nalpha %d %.17g\n", b, sqp.alphaTaken()[b]);
    }
    std::printf("StageSQP line search ok\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "StageSQP: %s\n", e.what());
    return std::string(e.what()).find("gfx950") != std::string::npos || std::string(e.what()).find("no device") != std::string::npos ? 3 : 1;
  }
}
