// StageSQP.hpp with setInitialGuessMode on the bounds of tests/support/kkt_cases.py's recipe: cart-pole N = 20, 8 instances whose start angles grow by
// the factor 1.835 from 0.01 rad, full steps, 2 iterations per call, the start rolled out from the pinned first frame with its input held.  Two calls:
// the second continues from the stored iterate (the option is applied once to a fresh iterate).  Prints what the Python device loop reports --
// rollout_diverged, rollout_box_viol and x after each call -- for tests/test_gpu_rollout.py to compare.  Exit code 0 = ran, 3 = no GPU, 1 = error.
#include <cstdio>
#include <limits>
#include <string>

#include "StageSQP.hpp"

int main() {
  const int B = 8, N = 20;
  mpcqp_stage_desc d;
  if (mpcqp_stage_default(MPCQP_MODEL_CARTPOLE, N, &d) != MPCQP_OK) return 1;
  try {
    StageSQP sqp(d, B, 2, 1.0);
    sqp.setInitialGuessMode(StageSQP::GUESS_ROLLOUT);
    const int f = sqp.nx() + sqp.nu();
    const double inf = std::numeric_limits<double>::infinity();
    const double lo[5] = {-2.4, -inf, -inf, -inf, -20.0}, hi[5] = {2.4, inf, inf, inf, 20.0};
    StageSQP::Arg a;
    a.p.assign((size_t)B * sqp.np(), 0.0); a.lbg.assign((size_t)B * sqp.ng(), 0.0); a.ubg.assign((size_t)B * sqp.ng(), 0.0);
    a.lbx.resize((size_t)B * sqp.nvar()); a.ubx.resize((size_t)B * sqp.nvar());
    double angle = 0.01;
    for (int b = 0; b < B; b++) {
      for (int k = 0; k < N; k++)
        for (int c = 0; c < f; c++) {
          const size_t at = ((size_t)b * N + k) * f + c;
          a.lbx[at] = k == 0 ? (c == 1 ? angle : 0.0) : lo[c];
          a.ubx[at] = k == 0 ? (c == 1 ? angle : 0.0) : hi[c];
        }
      angle *= 1.835;
    }
    StageSQP::Result r1 = sqp.getOptimalSolution(a);
    std::printf("diverged"); for (int v : sqp.rolloutDiverged()) std::printf(" %d", v); std::printf("\n");
    std::printf("box_viol"); for (double v : sqp.rolloutBoxViolation()) std::printf(" %.17g", v); std::printf("\n");
    std::printf("x1"); for (double v : r1.x) std::printf(" %.17g", v); std::printf("\n");
    StageSQP::Result r2 = sqp.getOptimalSolution(a);
    std::printf("x2"); for (double v : r2.x) std::printf(" %.17g", v); std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "StageSQP: %s\n", e.what());
    return std::string(e.what()).find("gfx950") != std::string::npos || std::string(e.what()).find("no device") != std::string::npos ? 3 : 1;
  }
}
