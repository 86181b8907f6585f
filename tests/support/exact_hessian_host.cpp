// exact_hessian_host.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone host program that drives the generated functors FG / HG of a model with
// exact_hessian = True through the g++ build of the same source (codegen.build_host_library, export user_host_curvature): one pass per column on dual
// numbers, -FG.d + HG.d, what a thread of stage_lagrangian_kernel does.  tests/test_exact_hessian_host.py compares its output with the NumPy statement
// (models.StageOCP.constraint_curvature); being a program with its own main it can also be built with a sanitizer.
//   exact_hessian_host <library.so> <input.txt>
// input:  "frames nx nu nh ntheta nsd", then per frame: dyn (0 / 1), theta [ntheta], s [nx], u [nu], lam [nx], mu [nh], d [nsd]
// output: per frame one line of f * f values, row-major, %.17g
#include <dlfcn.h>
#include <cstdio>
#include <vector>

typedef void (*curvature_fn)(const double *, const double *, const double *, const double *, const double *, const double *, int, double *);

static bool read(FILE *fh, std::vector<double> &v) {
  for (double &x : v) if (std::fscanf(fh, "%lf", &x) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s library.so input.txt\n", argv[0]); return 2; }
  void *lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!lib) { std::fprintf(stderr, "cannot load %s: %s\n", argv[1], dlerror()); return 2; }
  curvature_fn fn = (curvature_fn)dlsym(lib, "user_host_curvature");
  auto dims = (void (*)(int *, int *))dlsym(lib, "user_host_dims");
  if (!fn || !dims) { std::fprintf(stderr, "the library does not export user_host_curvature (exact_hessian = False?)\n"); return 3; }
  FILE *fh = std::fopen(argv[2], "r");
  if (!fh) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  int frames, nx, nu, nh, nth, nsd, lnx = 0, lnu = 0;
  if (std::fscanf(fh, "%d %d %d %d %d %d", &frames, &nx, &nu, &nh, &nth, &nsd) != 6) return 4;
  dims(&lnx, &lnu);
  if (lnx != nx || lnu != nu || frames < 0 || nh < 0 || nth < 0 || nsd < 0) { std::fprintf(stderr, "the input does not fit the library\n"); return 4; }
  const int f = nx + nu;
  std::vector<double> theta(nth), s(nx), u(nu), lam(nx), mu(nh), d(nsd), C((size_t)f * f);
  for (int i = 0; i < frames; i++) {
    int dyn;
    if (std::fscanf(fh, "%d", &dyn) != 1 || !read(fh, theta) || !read(fh, s) || !read(fh, u) || !read(fh, lam) || !read(fh, mu) || !read(fh, d)) return 4;
    fn(nth ? theta.data() : nullptr, s.data(), u.data(), lam.data(), mu.data(), nsd ? d.data() : nullptr, dyn, C.data());
    for (int e = 0; e < f * f; e++) std::printf("%.17g%c", C[e], e + 1 == f * f ? '\n' : ' ');
  }
  std::fclose(fh);
  dlclose(lib);
  return 0;
}
