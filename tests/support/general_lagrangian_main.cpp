// general_lagrangian_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program around general_host_lagrangian of a generated host source
// (codegen.general_host_source of a model built with exact_hessian=True), for sanitizer runs: tests/test_general_exact_hessian_host.py compiles it with
// -fsanitize=address,undefined and -DGEN_SRC="<path of the generated source>" and runs it; it is never loaded into Python.  Every array has exactly
// the length the entry may touch (heap allocations, so that a step outside is seen), and the program checks itself what needs no reference: y = 0
// and a failed instance leave every bit of P, mode 0 gives the same bits with and without the workspace, NaN multipliers write no slot outside
// the curvature's structure.
#include <cstdio>
#include <cstring>
#include <vector>
#include GEN_SRC

static unsigned long long lcg = 88172645463325252ULL;
static double rnd() { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(lcg >> 11) / 9007199254740992.0 * 2.0 - 1.0; }

int main() {
  constexpr int n = GnUser::n, np = GnUser::np, nvar = GnUser::nvar, ng = GnUser::ng, nnzP = GnUser::nnzP;
  int bad = 0;
  for (int round = 0; round < 8; round++) {
    std::vector<double> p(np), x(nvar), y(n + ng), P0(nnzP), C(nnzP), shift(n);
    for (auto &v : p) v = 0.4 * rnd();
    for (auto &v : x) v = 0.5 * rnd();
    for (auto &v : y) v = 2.0 * rnd();
    for (auto &v : P0) v = rnd();
    std::vector<double> w(n), q(n), A(GnUser::nnzA), l(n + ng), u(n + ng), lbx(nvar, -1.0), ubx(nvar, 1.0), lbg(ng, 0.0), ubg(ng, 0.0);
    for (int i = 0; i < n; i++) w[i] = i < np ? p[i] : x[i - np];
    general_host_eval(w.data(), lbx.data(), ubx.data(), lbg.data(), ubg.data(), P0.data(), q.data(), A.data(), l.data(), u.data());
    auto run = [&](const std::vector<double> &yy, int mode, bool ws, const int *status, std::vector<double> &P, std::vector<double> &sh) {
      P = P0; sh.assign(n, 0.0);
      std::vector<double> Cw(nnzP, 7.0);
      mpcqp_nlp_lagrangian_args a;
      std::memset(&a, 0, sizeof a);
      a.p = np ? p.data() : nullptr; a.x = x.data(); a.y = yy.data(); a.status = status; a.P = P.data(); a.C = ws ? Cw.data() : nullptr;
      a.mode = mode; a.shift = sh.data();
      general_host_lagrangian(&a);
    };
    std::vector<double> Pa, Pb, Pd, sa, sb, sd;
    run(y, 0, true, nullptr, Pa, sa); run(y, 0, false, nullptr, Pb, sb); run(y, MPCQP_NLP_DOMINANT, true, nullptr, Pd, sd);
    if (std::memcmp(Pa.data(), Pb.data(), nnzP * sizeof(double))) { std::printf("round %d: mode 0 differs with and without the workspace\n", round); bad++; }
    for (int c = 0; c < n; c++) if (!(sd[c] >= 0.0) || sa[c] != 0.0) { std::printf("round %d: shift[%d]\n", round, c); bad++; }
    std::vector<double> zero(n + ng, 0.0), nan(n + ng, std::nan(""));
    const int failed = 3;
    for (int mode = 0; mode <= 1; mode++) {
      run(zero, mode, true, nullptr, Pa, sa);
      if (std::memcmp(Pa.data(), P0.data(), nnzP * sizeof(double))) { std::printf("round %d mode %d: y = 0 changed P\n", round, mode); bad++; }
      run(nan, mode, true, &failed, Pa, sa);
      if (std::memcmp(Pa.data(), P0.data(), nnzP * sizeof(double))) { std::printf("round %d mode %d: a failed instance changed P\n", round, mode); bad++; }
      run(nan, mode, mode == 1, nullptr, Pa, sa);                      // NaN multipliers under an ok status: must stay inside the arrays
    }
  }
  std::printf("%s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
