// general_eval.hip -- local-system evaluation on device for a general (non-stage) NLP (include/mpcqp.h, mpcqp_nlp_*): the handle around
// a library optimal_control_problem_amd/codegen.py generated (emit_general) from the traced cost and constraints of any problem.
// Replaces the construction and the per-iteration call of localSystemFunction_ for problems the stage pattern does not cover
// (reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77,100-120) and the update / objective of :171-181.  The kernels live in
// general_kernels.hpp and are instantiated by the generated unit; this file loads it, checks its ABI version, uploads its tables once
// and forwards the calls.  Nothing is allocated inside eval / merit / step / linesearch / lagrangian, so a captured graph replays them.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mpcqp.h"
#include "common.hpp"
#include "general_kernels.hpp"

typedef int (*gn_eval_fn)(const GnDev *, int, const double *, const double *, const double *, const double *, const double *, const double *,
                          double *, double *, double *, double *, double *, void *);
typedef int (*gn_merit_fn)(int, const double *, const double *, const double *, const double *, double *, double *, void *);
typedef int (*gn_linesearch_fn)(int, const mpcqp_nlp_linesearch_args *, void *);
typedef int (*gn_lagrangian_fn)(int, const mpcqp_nlp_lagrangian_args *, void *);

struct mpcqp_nlp {
  GnDev gd;
  int device = 0;
  std::vector<int> Pp, Pi, Ap, Ai;
  int *dtab = nullptr;               // one device allocation: Ap, hslot, jslot
  int *dkkt = nullptr;               // Ap and Ai on the device for mpcqp_nlp_kkt
  void *lib = nullptr;
  gn_eval_fn eval = nullptr;
  gn_merit_fn merit = nullptr;
  gn_linesearch_fn linesearch = nullptr;   // optional: a library generated before mpcqp_nlp_linesearch (or without it) does not export it
  gn_lagrangian_fn lagrangian = nullptr;   // optional: only a library generated from a model with exact_hessian=True exports it
};

extern "C" {

int mpcqp_nlp_create(const char *library_path, int device, mpcqp_nlp **out) {
  if (!out) return mpcqp_set_error(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (!library_path) return mpcqp_set_error(MPCQP_ERR_ARG, "library path is null");
  void *lib = dlopen(library_path, RTLD_NOW | RTLD_LOCAL);
  if (!lib) return mpcqp_set_error(MPCQP_ERR_ARG, std::string("cannot load the evaluator library: ") + dlerror());
  auto abi = (int (*)())dlsym(lib, "mpcqp_general_abi");
  auto dims = (void (*)(int *))dlsym(lib, "mpcqp_general_dims");
  auto tables = (void (*)(int *, int *, int *, int *, int *, int *, int *, int *))dlsym(lib, "mpcqp_general_tables");
  auto ev = (gn_eval_fn)dlsym(lib, "mpcqp_general_eval");
  auto me = (gn_merit_fn)dlsym(lib, "mpcqp_general_merit");
  if (!abi || !dims || !tables || !ev || !me) { dlclose(lib); return mpcqp_set_error(MPCQP_ERR_ARG, "the library does not export mpcqp_general_abi/dims/tables/eval/merit"); }
  if (abi() != GENERAL_ABI_VERSION) { dlclose(lib); return mpcqp_set_error(MPCQP_ERR_ARG, "the library was generated for another version of the general kernels; regenerate it"); }
  int d[9] = {0};
  dims(d);
  const int nvar = d[0], np = d[1], ng = d[2], n = d[3], m = d[4], nnzP = d[5], nnzA = d[6], passes = d[7], hp = d[8];
  if (nvar <= 0 || np < 0 || ng < 0 || n != np + nvar || m != n + ng || nnzP < 0 || nnzA < n || hp < 1 || passes < hp || (ng == 0) != (passes == hp)) {
    dlclose(lib); return mpcqp_set_error(MPCQP_ERR_ARG, "the library reports inconsistent dimensions");
  }
  int dev = 0;
  if (int rc = mpcqp_pick_device(device, &dev)) { dlclose(lib); return rc; }
  mpcqp_nlp *s = new mpcqp_nlp();
  s->lib = lib; s->eval = ev; s->merit = me; s->device = dev;
  s->linesearch = (gn_linesearch_fn)dlsym(lib, "mpcqp_general_linesearch");
  s->lagrangian = (gn_lagrangian_fn)dlsym(lib, "mpcqp_general_lagrangian");
  const int jp = passes - hp;
  s->Pp.resize(n + 1); s->Pi.resize(nnzP); s->Ap.resize(n + 1); s->Ai.resize(nnzA);
  std::vector<int> tab((size_t)(n + 1) + (size_t)hp * n + (size_t)jp * ng);
  int *hslot = tab.data() + n + 1, *jslot = hslot + (size_t)hp * n;
  tables(s->Pp.data(), s->Pi.data(), s->Ap.data(), s->Ai.data(), nullptr, nullptr, hslot, jslot);
  std::copy(s->Ap.begin(), s->Ap.end(), tab.begin());
  // every slot the kernels will store through lies inside its array, and the identity entry is the first of its column
  bool ok = s->Pp[0] == 0 && s->Ap[0] == 0 && s->Pp[n] == nnzP && s->Ap[n] == nnzA;
  for (int j = 0; ok && j < n; j++) ok = s->Pp[j + 1] >= s->Pp[j] && s->Ap[j + 1] > s->Ap[j] && s->Ai[s->Ap[j]] == j;
  for (size_t i = 0; ok && i < (size_t)hp * n; i++) ok = hslot[i] >= -1 && hslot[i] < nnzP;
  for (size_t i = 0; ok && i < (size_t)jp * ng; i++) ok = jslot[i] >= -1 && jslot[i] < nnzA;
  if (!ok) { mpcqp_nlp_destroy(s); return mpcqp_set_error(MPCQP_ERR_ARG, "the library's tables are inconsistent"); }
  if (hipSetDevice(dev) != hipSuccess) { mpcqp_nlp_destroy(s); return mpcqp_set_error(MPCQP_ERR_HIP, "hipSetDevice failed"); }
  if (hipMalloc(&s->dtab, tab.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(s->dtab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    mpcqp_nlp_destroy(s); return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the evaluator's tables failed");
  }
  if (int rc = mpcqp_kkt_upload(n, m, np, s->Ap, s->Ai, &s->dkkt)) { mpcqp_nlp_destroy(s); return rc; }
  GnDev &gd = s->gd;
  gd.n = n; gd.np = np; gd.nvar = nvar; gd.ng = ng; gd.m = m; gd.nnzP = nnzP; gd.nnzA = nnzA; gd.hp = hp; gd.jp = jp;
  gd.Ap = s->dtab; gd.hslot = s->dtab + n + 1; gd.jslot = gd.hslot + (size_t)hp * n;
  *out = s;
  return MPCQP_OK;
}

void mpcqp_nlp_destroy(mpcqp_nlp *s) {
  if (!s) return;
  if (s->dtab) { (void)hipSetDevice(s->device); (void)hipFree(s->dtab); }
  if (s->dkkt) { (void)hipSetDevice(s->device); (void)hipFree(s->dkkt); }
  if (s->lib) dlclose(s->lib);
  delete s;
}

int mpcqp_nlp_dims(const mpcqp_nlp *s, int *o) {
  if (!s || !o) return mpcqp_set_error(MPCQP_ERR_ARG, "null argument");
  const GnDev &d = s->gd;
  o[0] = d.nvar; o[1] = d.np; o[2] = d.ng; o[3] = d.n; o[4] = d.m; o[5] = d.nnzP; o[6] = d.nnzA; o[7] = d.hp + d.jp;
  return MPCQP_OK;
}

int mpcqp_nlp_pattern(const mpcqp_nlp *s, int *Pp, int *Pi, int *Ap, int *Ai) {
  if (!s || !Pp || !Pi || !Ap || !Ai) return mpcqp_set_error(MPCQP_ERR_ARG, "null argument");
  std::copy(s->Pp.begin(), s->Pp.end(), Pp); std::copy(s->Pi.begin(), s->Pi.end(), Pi);
  std::copy(s->Ap.begin(), s->Ap.end(), Ap); std::copy(s->Ai.begin(), s->Ai.end(), Ai);
  return MPCQP_OK;
}

int mpcqp_nlp_eval(mpcqp_nlp *s, int batch, const double *p, const double *x, const double *lbx, const double *ubx,
                   const double *lbg, const double *ubg, double *P, double *q, double *A, double *l, double *u, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  const GnDev &d = s->gd;
  // (an array without elements has no address: p when np = 0, lbg / ubg when ng = 0, P when the Hessian is empty)
  if ((!p && d.np > 0) || !x || !lbx || !ubx || ((!lbg || !ubg) && d.ng > 0) || (!P && d.nnzP > 0) || !q || !A || !l || !u)
    return mpcqp_set_error(MPCQP_ERR_ARG, "null data pointer");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK((hipError_t)s->eval(&s->gd, batch, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u, stream));
  return MPCQP_OK;
}

int mpcqp_nlp_merit(mpcqp_nlp *s, int batch, const double *p, const double *x, const double *lbg, const double *ubg,
                    double *f, double *gmax, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  const GnDev &d = s->gd;
  if (batch <= 0 || (!p && d.np > 0) || !x || (gmax && (!lbg || !ubg) && d.ng > 0)) return mpcqp_set_error(MPCQP_ERR_ARG, "bad batch or null data pointer");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK((hipError_t)s->merit(batch, p, x, lbg, ubg, f, gmax, stream));
  return MPCQP_OK;
}

int mpcqp_nlp_step(mpcqp_nlp *s, int batch, double alpha, const double *dw, double *x, double *step_max, const int *status, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  if (batch <= 0 || !dw || !x) return mpcqp_set_error(MPCQP_ERR_ARG, "bad batch or null data pointer");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK(mpcqp_launch_step(batch, s->gd.nvar, s->gd.n, s->gd.np, alpha, dw, x, step_max, status, (hipStream_t)stream));
  return MPCQP_OK;
}

int mpcqp_nlp_has_linesearch(const mpcqp_nlp *s) { return s && s->linesearch ? 1 : 0; }

int mpcqp_nlp_linesearch(mpcqp_nlp *s, int batch, const mpcqp_nlp_linesearch_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  const GnDev &d = s->gd;
  if ((!a->p && d.np > 0) || !a->x || !a->lbx || !a->ubx || ((!a->lbg || !a->ubg) && d.ng > 0) || !a->q || !a->dw || !a->y)
    return mpcqp_set_error(MPCQP_ERR_ARG, "p, x, lbx, ubx, lbg, ubg, q, dw and y are required (p with np > 0, lbg and ubg with ng > 0)");
  if (a->candidates < 1 || a->candidates > MPCQP_LINESEARCH_MAX_CANDIDATES) return mpcqp_set_error(MPCQP_ERR_ARG, "candidates must be in 1..8");
  if (!(a->beta > 0.0 && a->beta < 1.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "beta must lie in (0, 1)");
  if (!(a->alpha0 > 0.0) || !std::isfinite(a->alpha0)) return mpcqp_set_error(MPCQP_ERR_ARG, "alpha0 must be positive");
  if (!(a->c1 >= 0.0 && a->c1 < 1.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "c1 must lie in [0, 1)");
  if (!(a->mu_min >= 0.0) || !(a->mu_factor >= 0.0) || !std::isfinite(a->mu_min) || !std::isfinite(a->mu_factor))
    return mpcqp_set_error(MPCQP_ERR_ARG, "mu_min and mu_factor must be finite and not negative");
  if (!s->linesearch)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_general_linesearch (generated before this entry, or without it); regenerate it");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK((hipError_t)s->linesearch(batch, a, stream));
  return MPCQP_OK;
}

int mpcqp_nlp_has_exact_hessian(const mpcqp_nlp *s) { return s && s->lagrangian ? 1 : 0; }

int mpcqp_nlp_lagrangian(mpcqp_nlp *s, int batch, const mpcqp_nlp_lagrangian_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if ((!a->p && s->gd.np > 0) || !a->x || !a->y || !a->P) return mpcqp_set_error(MPCQP_ERR_ARG, "p, x, y and P are required (p with np > 0)");
  if (a->mode != 0 && a->mode != MPCQP_NLP_DOMINANT) return mpcqp_set_error(MPCQP_ERR_ARG, "mode must be 0 or MPCQP_NLP_DOMINANT");
  if (a->mode == MPCQP_NLP_DOMINANT && !a->C) return mpcqp_set_error(MPCQP_ERR_ARG, "MPCQP_NLP_DOMINANT needs the workspace C");
  if (!s->lagrangian)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_general_lagrangian: generate it from a model with exact_hessian=True");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK((hipError_t)s->lagrangian(batch, a, stream));
  return MPCQP_OK;
}

// the optimality residuals at the system mpcqp_nlp_eval just wrote (kkt.hip; the library takes no part)
int mpcqp_nlp_kkt(mpcqp_nlp *s, int batch, const mpcqp_kkt_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "nlp handle is null");
  return mpcqp_kkt_run(s->device, s->gd.n, s->gd.m, s->gd.np, s->gd.nnzA, s->dkkt, batch, a, stream);
}

}  // extern "C"
