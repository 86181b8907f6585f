// soft_interp.cpp -- TEST INFRASTRUCTURE ONLY: the host mapping of csrc/select.hpp with the `soft` flag, for tests/test_soft_rows_host.py (no GPU, no HIP).
// tests/support/plan_interp.cpp shows the mapping as every existing caller asks for it; this shows what a handle with soft rows set asks for.
#include <algorithm>
#include "../../optimal_control_problem_amd/csrc/select.hpp"
using namespace mpcqp;

// select_kernel on a pattern under the environment's knobs (forced_family as in plan_interp.cpp) -> 0 and kid[13 r .. 13 r + 12] =
// {kind, nw, minw, zyg, ng, nh, hub, pd, reuse, rf, tiles, soft, 1} for r = 0: kernel_id_of(s, false, false), 1: (s, false, true) -- what existing callers get --
// and r = 2, 3: the same two with soft = true; out[0] = takes_soft_rows(s), out[1] = the family code of mpcqp_plan_info, out[2] = two-kernel form.  Or the error code.
extern "C" int soft_select_kernels(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai, int cus, const char *forced_family, long *out, long *kid) {
  const Selection s = select_kernel(n, m, batch, Pp, Pi, Ap, Ai, cus, forced_family, Knobs::from_env());
  std::fill(kid, kid + 4 * 13, 0L);
  if (s.err) return s.err;
  auto put = [&](int role, const KernelId &k) {
    const long v[13] = {k.kind, k.nw, k.minw, k.zyg, k.ng, k.nh, k.hub, k.pd, k.reuse, k.rf, k.tiles, k.soft, 1};
    std::copy(v, v + 13, kid + 13 * role);
  };
  put(0, kernel_id_of(s, false, false)); put(1, kernel_id_of(s, false, true));
  put(2, kernel_id_of(s, false, false, true)); put(3, kernel_id_of(s, false, true, true));
  out[0] = takes_soft_rows(s) ? 1 : 0; out[1] = s.family(); out[2] = s.split ? 1 : 0;
  return 0;
}
