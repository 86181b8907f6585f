// StageSQP.hpp with setInstanceParams: the cart-pole recipe of tests/support/instance_params_cases.py -- N = 10, four instances from one start, pole length
// x {0.6, 1, 1.5, 2}, three SQP iterations from x = 0 with alpha = 0.5.  Prints the iterate for tests/test_gpu_instance_params.py, which runs the
// Python device loop on the same problem.  Exit code 0 = ran, 3 = no GPU (refused loudly), 1 = error.
#include <cstdio>
#include <limits>

#include "StageSQP.hpp"

int main() {
  const int B = 4, N = 10;
  const double scale[B] = {0.6, 1.0, 1.5, 2.0};
  mpcqp_stage_desc d;
  if (mpcqp_stage_default(MPCQP_MODEL_CARTPOLE, N, &d) != MPCQP_OK) return 1;
  try {
    StageSQP sqp(d, B, 3, 0.5);
    if (sqp.paramCount() != 4) return 1;
    std::vector<double> theta;
    for (int b = 0; b < B; b++) for (int i = 0; i < 4; i++) theta.push_back(i == 2 ? d.par[i] * scale[b] : d.par[i]);
    sqp.setInstanceParams(MPCQP_PARAMS_MODEL, theta);
    const int f = sqp.nx() + sqp.nu();
    const double inf = std::numeric_limits<double>::infinity();
    const double frame0[5] = {0.3, 0.4, 0.0, 0.0, 0.0};
    StageSQP::Arg a;
    a.p.assign((size_t)B * sqp.np(), 0.0); a.lbg.assign((size_t)B * sqp.ng(), 0.0); a.ubg.assign((size_t)B * sqp.ng(), 0.0);
    a.lbx.resize((size_t)B * sqp.nvar()); a.ubx.resize((size_t)B * sqp.nvar());
    for (int b = 0; b < B; b++)
      for (int k = 0; k < N; k++) {
        double *lo = &a.lbx[((size_t)b * N + k) * f], *hi = &a.ubx[((size_t)b * N + k) * f];
        for (int i = 0; i < f; i++) { lo[i] = -inf; hi[i] = inf; }
        lo[0] = -2.4; hi[0] = 2.4; lo[4] = -20.0; hi[4] = 20.0;                              // track and force limits
        if (k == 0) for (int i = 0; i < f; i++) lo[i] = hi[i] = frame0[i];
      }
    StageSQP::Result r = sqp.getOptimalSolution(a);
    for (int b = 0; b < B; b++) {
      std::printf("x %d", b);
      for (int i = 0; i < sqp.nvar(); i++) std::printf(" %.17g", r.x[(size_t)b * sqp.nvar() + i]);
      std::printf("\n");
    }
    std::printf("StageSQP instance params ok\n");
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "StageSQP: %s\n", e.what());
    return std::string(e.what()).find("gfx950") != std::string::npos || std::string(e.what()).find("no device") != std::string::npos ? 3 : 1;
  }
}
