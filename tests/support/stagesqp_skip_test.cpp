// StageSQP.hpp with setKktTolerance and setSkipConvergedQPs on the recipe of tests/support/kkt_cases.py: cart-pole N = 20, 8 instances whose start angles
// grow by the factor 1.835 from 0.01 rad, full steps from x = 0, at most 12 iterations, all three tolerances 2e-3; the frozen instances are left out of
// the QP launches (mpcqp_set_skip with the verdict array).  Prints what the Python device loop reports -- iterations_done, converged, converged_at, the
// last residuals and x -- for tests/test_gpu_skip.py to compare.  Second leg: the tolerance is switched off again (all three 0) and the loop called once
// more, next to a twin that never had setSkipConvergedQPs: with the stop off no verdict of the first call may skip a QP, so the two x are the same bits
// (x_off, x_off_plain).  Exit code 0 = ran, 3 = no GPU, 1 = error.
#include <cstdio>
#include <limits>
#include <string>

#include "StageSQP.hpp"

int main() {
  const int B = 8, N = 20;
  mpcqp_stage_desc d;
  if (mpcqp_stage_default(MPCQP_MODEL_CARTPOLE, N, &d) != MPCQP_OK) return 1;
  try {
    StageSQP sqp(d, B, 12, 1.0), plain(d, B, 12, 1.0);
    sqp.setKktTolerance(2e-3, 2e-3, 2e-3);
    sqp.setSkipConvergedQPs(true);
    plain.setKktTolerance(2e-3, 2e-3, 2e-3);
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
    StageSQP::Result r = sqp.getOptimalSolution(a);
    std::printf("iterations_done %d\n", sqp.iterationsDone());
    std::printf("converged"); for (int v : sqp.converged()) std::printf(" %d", v); std::printf("\n");
    std::printf("converged_at"); for (int v : sqp.convergedAt()) std::printf(" %d", v); std::printf("\n");
    std::printf("res"); for (double v : sqp.kktResiduals()) std::printf(" %.17g", v); std::printf("\n");
    std::printf("x"); for (double v : r.x) std::printf(" %.17g", v); std::printf("\n");
    StageSQP::Result rp = plain.getOptimalSolution(a);
    std::printf("x_plain"); for (double v : rp.x) std::printf(" %.17g", v); std::printf("\n");
    // the stop off again, the skip option still set: twelve more iterations of the whole batch on both
    sqp.setKktTolerance(0.0, 0.0, 0.0); plain.setKktTolerance(0.0, 0.0, 0.0);
    r = sqp.getOptimalSolution(a); rp = plain.getOptimalSolution(a);
    std::printf("iterations_off %d %d\n", sqp.iterationsDone(), plain.iterationsDone());
    std::printf("x_off"); for (double v : r.x) std::printf(" %.17g", v); std::printf("\n");
    std::printf("x_off_plain"); for (double v : rp.x) std::printf(" %.17g", v); std::printf("\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "StageSQP: %s\n", e.what());
    return std::string(e.what()).find("gfx950") != std::string::npos || std::string(e.what()).find("no device") != std::string::npos ? 3 : 1;
  }
}
