// convexify_host.cpp -- TEST INFRASTRUCTURE ONLY.  The g++ build of csrc/stage_convexify.hpp: the Jacobi / f(Lambda) core the device kernel runs, as one
// "lane group" of width 1.  As a shared library (tests/test_convexify_host.py) it is compared with numpy.linalg.eigh; with -DCONVEXIFY_HOST_MAIN it
// is a stand-alone program that runs the core over a set of matrices and checks V Lambda V' = A and V'V = I itself (for sanitizer runs).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../optimal_control_problem_amd/csrc/stage_convexify.hpp"

extern "C" {
// A [n * n] row-major symmetric -> lam [n] (the diagonal left by the sweeps, unsorted), V [n * n] (columns = eigenvectors), D [n * n] = f(A) - A,
// T [n * n] = the tile after the sweeps (its off-diagonal is what remains); returns the sweep count
int convexify_host_run(int n, const double *A, int mode, double eps, double *lam, double *V, double *D, double *T) {
  std::vector<double> a(A, A + (size_t)n * n);
  const int sweeps = sm_jacobi<1>(a.data(), V, n, 0, true);
  for (int i = 0; i < n; i++) lam[i] = a[(size_t)i * n + i];
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) D[(size_t)r * n + c] = sm_convexify_delta(a.data(), V, n, r, c, mode, eps);
  if (T) for (size_t i = 0; i < (size_t)n * n; i++) T[i] = a[i];
  return sweeps;
}
double convexify_host_lam_min(int n, const double *tile) { return sm_convexify_lam_min<1>(tile, n, 0); }
int convexify_host_sweep_cap() { return SM_JACOBI_SWEEP_CAP; }
}

#ifdef CONVEXIFY_HOST_MAIN
static unsigned long long state = 88172645463325252ull;
static double rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0; }

static int check(int n, std::vector<double> A, const char *what) {
  std::vector<double> lam(n), V((size_t)n * n), D((size_t)n * n), T((size_t)n * n);
  const int sweeps = convexify_host_run(n, A.data(), MPCQP_CONVEXIFY_MIRROR, 1e-6, lam.data(), V.data(), D.data(), T.data());
  double fro = 0.0, rec = 0.0, orth = 0.0;
  for (int i = 0; i < n * n; i++) fro += A[i] * A[i];
  fro = std::sqrt(fro);
  for (int r = 0; r < n; r++)
    for (int c = 0; c < n; c++) {
      double v = 0.0, o = 0.0;
      for (int j = 0; j < n; j++) { v += V[r * n + j] * lam[j] * V[c * n + j]; o += V[j * n + r] * V[j * n + c]; }
      rec = std::fmax(rec, std::fabs(v - A[r * n + c])); orth = std::fmax(orth, std::fabs(o - (r == c ? 1.0 : 0.0)));
    }
  const double bar = 1e-12 * std::fmax(1.0, fro);
  const bool ok = rec <= bar && orth <= 1e-12 && sweeps < SM_JACOBI_SWEEP_CAP;
  std::printf("%-14s n %2d  sweeps %2d  |V L V' - A| %.2e (bar %.2e)  |V'V - I| %.2e  %s\n", what, n, sweeps, rec, bar, orth, ok ? "ok" : "FAIL");
  return ok ? 0 : 1;
}

int main() {
  int bad = 0;
  const int orders[] = {1, 2, 9, 28, 40};
  for (int n : orders) {
    std::vector<double> A((size_t)n * n), Z((size_t)n * n, 0.0), R((size_t)n * n, 0.0), B((size_t)n * n, 0.0), I((size_t)n * n, 0.0);
    for (int r = 0; r < n; r++) for (int c = 0; c <= r; c++) A[r * n + c] = A[c * n + r] = rnd();
    bad += check(n, A, "random");
    bad += check(n, Z, "zero");
    for (int j = 0; j < (n + 1) / 2; j++) { std::vector<double> v(n); for (auto &x : v) x = rnd(); for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) R[r * n + c] += (j % 2 ? -1.0 : 1.0) * v[r] * v[c]; }
    bad += check(n, R, "rank-deficient");
    const int h = n / 2;
    for (int r = 0; r < n; r++) for (int c = 0; c <= r; c++) if ((r < h) == (c < h)) B[r * n + c] = B[c * n + r] = rnd();
    bad += check(n, B, "block-diagonal");
    for (int r = 0; r < n; r++) I[r * n + r] = r % 3 == 0 ? 2.0 : -1.0;
    if (n >= 2) { I[1] = I[n] = 0.0; }
    bad += check(n, I, "repeated");
    for (auto &x : A) x *= 1e8;
    bad += check(n, A, "large");
  }
  std::printf("%s\n", bad ? "FAILED" : "all ok");
  return bad ? 1 : 0;
}
#endif
