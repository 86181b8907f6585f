// stage_eval.hip -- local-system evaluation on device for the stage-OCP model zoo (include/mpcqp.h, "Local-system
// evaluation on device").  Replaces SQPOptimizationSolver::getLocalSystem
// (reference src/sqp_solver/SQPOptimizationSolver.cpp:100-120) for a batch of instances.
//
// Mapping: one thread per (instance b, QP column j).  A thread owns everything indexed by its column of w = [p; x]:
// the CSC column of P, the CSC column of A = [I; dg/dw] (its identity entry, the +1 of s_{k+1} in g_k, and column c of
// -dF(s_k, u_k), obtained by running F on dual numbers seeded in direction c), q[j], the identity row's bounds
// l[j], u[j], and -- for state columns -- the shifted bounds of dynamics row g_k[c].  Adjacent lanes own adjacent
// columns, so every store stream is contiguous across a wave; the value part of F is recomputed by the f lanes of a
// stage (cheaper than exchanging it).  HBM-bound: one pass, algorithmic bytes = inputs + outputs.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mpcqp.h"
#include "common.hpp"
#include "stage_kernels.hpp"
#include "stage_riccati.hpp"
#include "stage_riccati_active.hpp"
#include "stage_riccati_ipm.hpp"

// The launchers a generated library exports (model == MPCQP_MODEL_USER), one per operation: the handle's constants, the batch, the operation's
// argument block (convexify: then the handle's tables and scratch; lagrangian: then the curvature's slot table and the convexification's tables and
// scratch, null without a mode), the rows (StageRows) and the stream.  The library chooses the kernel instance from the rows (stage_with_rows).
// eval and merit are required; the others are optional: a library generated before the entry, or from a model without the flag, has none.
struct StageUserLib {
  int (*eval)(const StageDev *, int, const StageEvalArgs *, const StageRows *, void *) = nullptr;
  int (*merit)(const StageDev *, int, const StageMeritArgs *, const StageRows *, void *) = nullptr;
  int (*advance)(const StageDev *, int, const mpcqp_stage_advance_args *, const StageRows *, void *) = nullptr;
  int (*linesearch)(const StageDev *, int, const mpcqp_stage_linesearch_args *, const StageRows *, void *) = nullptr;
  int (*rollout)(const StageDev *, int, const mpcqp_stage_rollout_args *, const StageRows *, void *) = nullptr;
  int (*convexify)(const StageDev *, int, const mpcqp_stage_convexify_args *, const StageCvxBuf *, const StageRows *, void *) = nullptr;
  int (*lagrangian)(const StageDev *, int, const mpcqp_stage_lagrangian_args *, const int *, const StageCvxBuf *, const StageRows *, void *) = nullptr;
};
template <class Fn> static void stage_sym(void *lib, const char *name, Fn *&fn) { fn = (Fn *)dlsym(lib, name); }
static StageUserLib stage_user_lib(void *lib) {
  StageUserLib u;
  stage_sym(lib, "mpcqp_user_eval", u.eval); stage_sym(lib, "mpcqp_user_merit", u.merit);
  stage_sym(lib, "mpcqp_user_advance", u.advance); stage_sym(lib, "mpcqp_user_linesearch", u.linesearch);
  stage_sym(lib, "mpcqp_user_convexify", u.convexify); stage_sym(lib, "mpcqp_user_lagrangian", u.lagrangian);
  stage_sym(lib, "mpcqp_user_rollout", u.rollout);
  return u;
}

// the zoo's PP instances (quadrotor, cart-pole) live in stage_eval_pp.hip, a translation unit of their own that compiles beside this one
hipError_t mpcqp_launch_eval_pp(const StageDev &sd, int batch, const StageEvalArgs &a, hipStream_t st, StageTheta th);
hipError_t mpcqp_launch_merit_pp(const StageDev &sd, int batch, const StageMeritArgs &a, hipStream_t st, StageTheta th);
hipError_t mpcqp_launch_advance_pp(const StageDev &sd, int batch, const mpcqp_stage_advance_args &a, hipStream_t st, StageTheta th);
hipError_t mpcqp_launch_linesearch_pp(const StageDev &sd, int batch, const mpcqp_stage_linesearch_args &a, hipStream_t st, StageTheta th);
hipError_t mpcqp_launch_rollout_pp(const StageDev &sd, int batch, const mpcqp_stage_rollout_args &a, hipStream_t st, StageTheta th);

struct mpcqp_stage {
  mpcqp_stage_desc desc;
  StageDev sd;
  int device = 0;
  std::vector<int> Pp, Pi, Ap, Ai;
  int *dPp = nullptr, *dAp = nullptr;
  double *dQk = nullptr, *dRk = nullptr;
  double *dhlo = nullptr, *dhhi = nullptr;   // per-frame path bounds (mpcqp_stage_set_path_bounds)
  unsigned char *dmask = nullptr;     // Hessian structure of a generated general stage cost
  void *user_lib = nullptr;           // dlopen handle of a generated dynamics library (model == MPCQP_MODEL_USER)
  StageUserLib user;
  bool general_cost = false;          // the library carries its own stage cost: Q, R and mpcqp_stage_set_weights do not apply
  bool link_cost = false;             // the library carries a link cost between consecutive frames (mpcqp_user_link_cost): P couples frame k to k + 1
  int residual_rows = 0;              // the library's frame cost is a Gauss-Newton one (mpcqp_user_residual_cost): its residual rows nr; 0: none
  // per-instance parameters (mpcqp_stage_set_instance_params): set `which` is in force when th_batch[which] > 0
  int ntheta = 0;                     // entries of a row the model reads: 7 quadrotor, 4 cart-pole, 0 double integrator, mpcqp_user_ntheta of a library
  double *dth[2] = {nullptr, nullptr};
  int th_batch[2] = {0, 0}, th_cap[2] = {0, 0};
  const double *theta(int which) const { return th_batch[which] > 0 ? dth[which] : nullptr; }
  // stage data (mpcqp_stage_set_stage_data): rows [sd_batch * N * nsd] in dsd[sd_cur]; the other buffer takes the next shift (mpcqp_stage_shift_data)
  int nsd = 0;                        // values per frame the library's hfun / lcost / lterm read (mpcqp_user_nsd); 0: the zoo, a library without
  double *dsd[2] = {nullptr, nullptr};
  int sd_cur = 0, sd_batch = 0, sd_cap = 0;
  bool tdata = false;                 // the library's F, kfun and llink read the stage data too (mpcqp_user_transition_data)
  const double *sdata() const { return sd_batch > 0 ? dsd[sd_cur] : nullptr; }
  // convexification (mpcqp_stage_convexify): the slot tables of the frame term, built with the handle of a library that exports the launcher, and
  // the scratch of the launch ([cvx_cap * N * nx * nx] doubles, then [cvx_cap * N] flags), sized on first use like the stage-data buffers
  bool convexify = false;
  int *dslots = nullptr;
  double *dcvx = nullptr;
  int cvx_cap = 0;
  // the exact Lagrangian Hessian (mpcqp_stage_lagrangian): the slot table of the constraint curvature [N * f * f], built with the handle of a
  // library that exports the launchers
  bool exact = false;
  int *dlslots = nullptr;
  int *dkkt = nullptr;                // Ap and Ai on the device for mpcqp_stage_kkt
  int *dric = nullptr;                // the slot tables of mpcqp_stage_riccati, [N f f] of P then [(N - 1) nx f] of A, built by its first call
  // the direct solve (mpcqp_stage_riccati_solve): its own slot tables (StageDirTab, built by its first call; dir_off: where each one starts) and
  // the workspace of the launch, sized on first use like the convexification's
  int *ddir = nullptr;
  size_t dir_off[5] = {0, 0, 0, 0, 0};
  double *ddws = nullptr;
  int dir_cap = 0;
  // the workspace of mpcqp_stage_riccati_solve_active (stage_riccati_active.hpp: the one above plus val and the set words), grown the same way
  double *dactws = nullptr;
  int act_cap = 0;
  // the workspace of mpcqp_stage_riccati_solve_ipm (stage_riccati_ipm.hpp: the gains, the iterate, its step, val, slacks and multipliers)
  double *dipmws = nullptr;
  int ipm_cap = 0;
};

// a launch may not be larger than a stored parameter set
static int stage_theta_batch_ok(const mpcqp_stage *s, int which, int batch) {
  if (s->th_batch[which] > 0 && batch > s->th_batch[which])
    return mpcqp_set_error(MPCQP_ERR_ARG, which == MPCQP_PARAMS_MODEL ? "batch is larger than the stored per-instance model parameters (mpcqp_stage_set_instance_params)"
                                                                      : "batch is larger than the stored per-instance plant parameters (mpcqp_stage_set_instance_params)");
  return MPCQP_OK;
}

// The receding-horizon hand-over of the stage data (mpcqp_stage_shift_data), out of place: out[b, k, :] = in[b, k + 1, :] for k < N - 1, the last
// row d_new[b, :] or, without one, in[b, N - 1, :] again.  One thread per element, adjacent threads adjacent elements; one writer per element.
__global__ void __launch_bounds__(256) stage_shift_data_kernel(int batch, int N, int nsd, const double *__restrict__ in, const double *__restrict__ d_new,
                                                               double *__restrict__ out) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, per = (long)N * nsd;
  if (gid >= (long)batch * per) return;
  const long b = gid / per, r = gid - b * per;
  out[gid] = r < per - nsd ? in[gid + nsd] : d_new ? d_new[b * nsd + (r - (per - nsd))] : in[gid];
}

__global__ void __launch_bounds__(256) stage_step_kernel(int batch, int nvar, int n, int np, double alpha, const double *__restrict__ dw,
                                                         double *__restrict__ x, double *__restrict__ step_max, const int *__restrict__ status) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  double mx = 0.0;
  if (status) {
    const int s = status[b];
    if (s != MPCQP_SOLVED && s != MPCQP_SOLVED_INACCURATE && s != MPCQP_MAX_ITER_REACHED) { if (step_max && lane == 0) step_max[b] = 0.0; return; }
  }
  for (int i = lane; i < nvar; i += 64) {
    const double d = alpha * dw[(long)b * n + np + i];
    x[(long)b * nvar + i] += d; mx = fmax(mx, fabs(d));
  }
  for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (step_max && lane == 0) step_max[b] = mx;
}

// ------------------------------------------------------------------------------------------ host side
hipError_t mpcqp_launch_step(int batch, int nvar, int n, int np, double alpha, const double *dw, double *x, double *step_max, const int *status,
                             hipStream_t st) {
  stage_step_kernel<<<(unsigned)((batch + 3) / 4), 256, 0, st>>>(batch, nvar, n, np, alpha, dw, x, step_max, status);
  return hipGetLastError();
}

// The common tail of the six entry points that launch a model's kernel, after their own argument checks.  `rows` says which stored parameter sets
// the operation reads (the stage data: every one): a launch may not be larger than a stored set it reads or than the stored stage data.  Then the
// rows, and one of three launches: zoo(tag) launches the plain zoo instance of StageTag tag; zoo_pp(th) calls the PP twin in stage_eval_pp.hip;
// user(rows) calls the library's export and answers an MPCQP code (stage_hipchk for a bare launcher).
enum { STAGE_ROWS_THETA = 1, STAGE_ROWS_PLANT = 2 };
static int stage_hipchk(int e) { MPCQP_HIPCHK((hipError_t)e); return MPCQP_OK; }
template <class Zoo, class ZooPP, class User>
static int stage_launch(mpcqp_stage *s, int batch, int rows, Zoo zoo, ZooPP zoo_pp, User user) {
  if (rows & STAGE_ROWS_THETA) if (int rc = stage_theta_batch_ok(s, MPCQP_PARAMS_MODEL, batch)) return rc;
  if (rows & STAGE_ROWS_PLANT) if (int rc = stage_theta_batch_ok(s, MPCQP_PARAMS_PLANT, batch)) return rc;
  if (s->sd_batch > 0 && batch > s->sd_batch) return mpcqp_set_error(MPCQP_ERR_ARG, "batch is larger than the stored stage data (mpcqp_stage_set_stage_data)");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  const StageRows r{rows & STAGE_ROWS_THETA ? s->theta(MPCQP_PARAMS_MODEL) : nullptr, rows & STAGE_ROWS_PLANT ? s->theta(MPCQP_PARAMS_PLANT) : nullptr, s->sdata()};
  if (s->sd.model == MPCQP_MODEL_USER) return user(r);
  MPCQP_HIPCHK(r.theta || r.plant ? zoo_pp(StageTheta{r.theta, r.plant}) : stage_visit_zoo(s->sd.model, s->sd.pref != 0, zoo));
  return MPCQP_OK;
}
// (convexify and lagrangian: generated libraries only, the entry point has refused the zoo)
template <class User> static int stage_launch(mpcqp_stage *s, int batch, int rows, User user) {
  auto none = [](auto) { return hipErrorInvalidValue; };
  return stage_launch(s, batch, rows, none, none, user);
}

extern "C" {

int mpcqp_stage_default(int model, int horizon, mpcqp_stage_desc *d) {
  if (!d) return mpcqp_set_error(MPCQP_ERR_ARG, "desc is null");
  if (model < 0 || model >= SM_NMODELS) return mpcqp_set_error(MPCQP_ERR_ARG, "unknown model");
  *d = mpcqp_stage_desc();
  d->model = model; d->horizon = horizon; d->device = -1;
  switch (model) {
    case SM_DOUBLE_INTEGRATOR:
      d->dt = 0.05; d->Q[0] = 10.0; d->Q[1] = 1.0; d->R[0] = 0.1; break;
    case SM_QUADROTOR: {
      d->dt = 0.02;
      const double Qd[12] = {10, 10, 10, 1, 1, 1, 1, 1, 1, 0.1, 0.1, 0.1};
      for (int i = 0; i < 12; i++) d->Q[i] = Qd[i];
      for (int i = 0; i < 4; i++) d->R[i] = 0.1;
      const double pr[7] = {1.0, 9.81, 0.2, 0.05, 0.01, 0.01, 0.02};
      for (int i = 0; i < 7; i++) d->par[i] = pr[i];
      break;
    }
    case SM_CARTPOLE: {
      d->dt = 0.02;
      const double Qd[4] = {1.0, 10.0, 0.1, 0.1};
      for (int i = 0; i < 4; i++) d->Q[i] = Qd[i];
      d->R[0] = 0.01;
      const double pr[4] = {1.0, 0.1, 0.5, 9.81};
      for (int i = 0; i < 4; i++) d->par[i] = pr[i];
      break;
    }
  }
  return MPCQP_OK;
}

static int stage_create_common(const mpcqp_stage_desc *d, int nx, int nu, int nh, const double *h_lo, const double *h_hi, mpcqp_stage *s,
                               const unsigned char *cost_mask = nullptr, int nk = 0, const double *k_lo = nullptr, const double *k_hi = nullptr,
                               bool pref = false, const unsigned char *link_mask = nullptr) {
  int dev = 0;
  if (int rc = mpcqp_pick_device(d->device, &dev)) return rc;
  s->desc = *d; s->device = dev;
  StageDev &sd = s->sd;
  sd.model = d->model; sd.N = d->horizon; sd.dt = d->dt; sd.nx = nx; sd.nu = nu;
  sd.f = sd.nx + sd.nu; sd.pref = pref ? 1 : 0; sd.np = pref ? sd.N * sd.nx : sd.nx; sd.nvar = sd.N * sd.f; sd.n = sd.np + sd.nvar;
  sd.nh = nh; sd.nk = nk; sd.ngd = (sd.N - 1) * sd.nx; sd.ng = sd.ngd + sd.N * nh + (sd.N - 1) * nk; sd.m = sd.n + sd.ng;
  for (int i = 0; i < SM_MAXNK; i++) { sd.k_lo[i] = (k_lo && i < nk) ? k_lo[i] : -INFINITY; sd.k_hi[i] = (k_hi && i < nk) ? k_hi[i] : INFINITY; }
  for (int i = 0; i < SM_MAXNH; i++) { sd.h_lo[i] = (h_lo && i < nh) ? h_lo[i] : -INFINITY; sd.h_hi[i] = (h_hi && i < nh) ? h_hi[i] : INFINITY; }
  for (int i = 0; i < SM_MAXNX; i++) sd.Q[i] = d->Q[i];
  for (int i = 0; i < SM_MAXNU; i++) sd.R[i] = d->R[i];
  for (int i = 0; i < SM_NPAR; i++) sd.par[i] = d->par[i];
  sm_build_pattern(sd.nx, sd.nu, sd.N, sd.nh, sd.nk, s->Pp, s->Pi, s->Ap, s->Ai, pref, link_mask);
  if (cost_mask) sm_build_cost_pattern(sd.nx, sd.nu, sd.N, cost_mask, s->Pp, s->Pi, pref, link_mask);
  sd.nnzP = (int)s->Pi.size(); sd.nnzA = (int)s->Ai.size();
  if (hipSetDevice(dev) != hipSuccess) return mpcqp_set_error(MPCQP_ERR_HIP, "hipSetDevice failed");
  const size_t bytes = (size_t)(sd.n + 1) * sizeof(int);
  if (hipMalloc(&s->dPp, bytes) != hipSuccess || hipMalloc(&s->dAp, bytes) != hipSuccess)
    return mpcqp_set_error(MPCQP_ERR_HIP, "hipMalloc of the column pointers failed");
  if (hipMemcpy(s->dPp, s->Pp.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(s->dAp, s->Ap.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the column pointers failed");
  if (int rc = mpcqp_kkt_upload(sd.n, sd.m, sd.np, s->Ap, s->Ai, &s->dkkt)) return rc;
  sd.Pp = s->dPp; sd.Ap = s->dAp; sd.Qk = nullptr; sd.Rk = nullptr; sd.hmask = nullptr; sd.h_lok = nullptr; sd.h_hik = nullptr;
  if (cost_mask) {
    const size_t mb = (size_t)(sd.f + sd.nx) * (sd.f + sd.nx);
    if (hipMalloc(&s->dmask, mb) != hipSuccess || hipMemcpy(s->dmask, cost_mask, mb, hipMemcpyHostToDevice) != hipSuccess)
      return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the cost structure failed");
    sd.hmask = s->dmask;
  }
  return MPCQP_OK;
}

// Slot tables of mpcqp_stage_convexify (StageCvxBuf): element (r, c) of frame k's Hessian over [s; u; r] sits in column col(c), row row(r) of P --
// local index t < f is variable np + k f + t, t >= f the reference entry t - f (per-frame references: k nx + t - f); the slot is found in the
// pattern itself, so a link cost's extra rows in a frame column are stepped over.  The r-r block of a shared reference goes to ppslot.
static int stage_build_convexify_tables(mpcqp_stage *s, const unsigned char *mask) {
  const StageDev &sd = s->sd;
  const int f = sd.f, nx = sd.nx, nl = f + nx, N = sd.N;
  std::vector<int> tab((size_t)N * nl * nl + (size_t)nx * nx, -1);
  auto var = [&](int k, int t) { return t < f ? sd.np + k * f + t : (sd.pref ? k * nx : 0) + t - f; };
  auto find = [&](int row, int col) {
    for (int e = s->Pp[col]; e < s->Pp[col + 1]; e++) if (s->Pi[e] == row) return e;
    return -1;
  };
  for (int k = 0; k < N; k++)
    for (int r = 0; r < nl; r++)
      for (int c = 0; c < nl; c++) {
        if (!mask[r * nl + c] || (!sd.pref && r >= f && c >= f)) continue;
        tab[((size_t)k * nl + r) * nl + c] = find(var(k, r), var(k, c));
      }
  if (!sd.pref)
    for (int r = 0; r < nx; r++)
      for (int c = 0; c < nx; c++) if (mask[(f + r) * nl + f + c]) tab[(size_t)N * nl * nl + r * nx + c] = find(r, c);
  if (hipMalloc(&s->dslots, tab.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(s->dslots, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the convexification tables failed");
  s->convexify = true;
  return MPCQP_OK;
}

// Slot table of mpcqp_stage_lagrangian: element (r, c) of frame k's curvature C_k over [s; u] sits in column np + k f + c, row np + k f + r of P; -1
// outside the curvature's structure `mask` (f^2 bytes).  The slot is found in the pattern itself, as for the convexification tables.
static int stage_build_lagrangian_table(mpcqp_stage *s, const unsigned char *mask) {
  const StageDev &sd = s->sd;
  const int f = sd.f, N = sd.N;
  std::vector<int> tab((size_t)N * f * f, -1);
  for (int k = 0; k < N; k++)
    for (int r = 0; r < f; r++)
      for (int c = 0; c < f; c++) {
        if (!mask[r * f + c]) continue;
        const int col = sd.np + k * f + c, row = sd.np + k * f + r;
        for (int e = s->Pp[col]; e < s->Pp[col + 1]; e++) if (s->Pi[e] == row) tab[((size_t)k * f + r) * f + c] = e;
      }
  if (hipMalloc(&s->dlslots, tab.size() * sizeof(int)) != hipSuccess ||
      hipMemcpy(s->dlslots, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the curvature's slot table failed");
  s->exact = true;
  return MPCQP_OK;
}

static int stage_create_zoo(const mpcqp_stage_desc *d, bool pref, mpcqp_stage **out) {
  if (!out) return mpcqp_set_error(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (!d) return mpcqp_set_error(MPCQP_ERR_ARG, "desc is null");
  if (d->model < 0 || d->model >= SM_NMODELS) return mpcqp_set_error(MPCQP_ERR_ARG, "unknown model");
  if (d->horizon < 2 || !(d->dt > 0.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "horizon must be >= 2 and dt > 0");
  int nx, nu;
  sm_model_dims(d->model, &nx, &nu);
  mpcqp_stage *s = new mpcqp_stage();
  s->ntheta = d->model == SM_QUADROTOR ? SmQuadrotor::ntheta : d->model == SM_CARTPOLE ? SmCartPole::ntheta : 0;
  if (int rc = stage_create_common(d, nx, nu, 0, nullptr, nullptr, s, nullptr, 0, nullptr, nullptr, pref)) { mpcqp_stage_destroy(s); return rc; }
  *out = s;
  return MPCQP_OK;
}

// a generated library says with the optional export mpcqp_user_pref() whether it was traced for per-frame references; the entry point asks for one kind
static int stage_create_library(const mpcqp_stage_desc *d, const char *library_path, bool pref, mpcqp_stage **out) {
  if (!out) return mpcqp_set_error(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (!d || !library_path) return mpcqp_set_error(MPCQP_ERR_ARG, "null argument");
  if (d->horizon < 2 || !(d->dt > 0.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "horizon must be >= 2 and dt > 0");
  void *lib = dlopen(library_path, RTLD_NOW | RTLD_LOCAL);
  if (!lib) return mpcqp_set_error(MPCQP_ERR_ARG, std::string("cannot load the dynamics library: ") + dlerror());
  auto abi = (int (*)())dlsym(lib, "mpcqp_user_abi");
  auto dims = (void (*)(int *, int *))dlsym(lib, "mpcqp_user_dims");
  const StageUserLib user = stage_user_lib(lib);
  if (!abi || !dims || !user.eval || !user.merit) { dlclose(lib); return mpcqp_set_error(MPCQP_ERR_ARG, "the library does not export mpcqp_user_abi/dims/eval/merit"); }
  if (abi() != STAGE_ABI_VERSION) { dlclose(lib); return mpcqp_set_error(MPCQP_ERR_ARG, "the library was generated for another version of the stage kernels; regenerate it"); }
  auto pf = (int (*)())dlsym(lib, "mpcqp_user_pref");
  if ((pf && pf() != 0) != pref) {
    dlclose(lib);
    return mpcqp_set_error(MPCQP_ERR_ARG, pref ? "the library was generated for one shared reference; mpcqp_stage_create_user takes it"
                                               : "the library was generated for per-frame references; mpcqp_stage_create_tracking takes it");
  }
  int nx = 0, nu = 0, nh = 0;
  dims(&nx, &nu);
  auto nhf = (int (*)())dlsym(lib, "mpcqp_user_nh");
  auto hb = (void (*)(double *, double *))dlsym(lib, "mpcqp_user_path_bounds");
  if (nhf) nh = nhf();
  if (nx <= 0 || nx > SM_MAXNX || nu <= 0 || nu > SM_MAXNU || nh < 0 || nh > SM_MAXNH || (nh > 0 && !hb)) {
    dlclose(lib); return mpcqp_set_error(MPCQP_ERR_LIMIT, "nx must be in 1..16, nu in 1..8 and the path constraint in 0..16 rows");
  }
  double h_lo[SM_MAXNH], h_hi[SM_MAXNH];
  if (nh > 0) hb(h_lo, h_hi);
  int nk = 0;
  auto nkf = (int (*)())dlsym(lib, "mpcqp_user_nk");
  auto kb = (void (*)(double *, double *))dlsym(lib, "mpcqp_user_link_bounds");
  if (nkf) nk = nkf();
  if (nk < 0 || nk > SM_MAXNK || (nk > 0 && !kb)) { dlclose(lib); return mpcqp_set_error(MPCQP_ERR_LIMIT, "the link constraint may have 0..8 rows"); }
  double k_lo[SM_MAXNK], k_hi[SM_MAXNK];
  if (nk > 0) kb(k_lo, k_hi);
  mpcqp_stage *s = new mpcqp_stage();
  s->user_lib = lib; s->user = user;
  mpcqp_stage_desc dd = *d; dd.model = MPCQP_MODEL_USER;
  // optional exports of a library generated with parameters: their count and their defaults (which become sd.par: d->par stays ignored for a
  // generated library).  A library without them has no parameters.
  {
    auto ntf = (int (*)())dlsym(lib, "mpcqp_user_ntheta");
    auto t0f = (void (*)(double *))dlsym(lib, "mpcqp_user_theta0");
    const int nt = ntf ? ntf() : 0;
    if (nt < 0 || nt > SM_NPAR || (nt > 0 && !t0f)) {
      mpcqp_stage_destroy(s);
      return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library declares parameters but not 0..8 of them, or lacks mpcqp_user_theta0");
    }
    s->ntheta = nt;
    for (int i = 0; i < SM_NPAR; i++) dd.par[i] = 0.0;
    if (nt > 0) t0f(dd.par);
  }
  // optional export of a library generated with stage data: how many values per frame its hfun / lcost / lterm read.  A library without it has none.
  {
    auto nsf = (int (*)())dlsym(lib, "mpcqp_user_nsd");
    const int ns = nsf ? nsf() : 0;
    if (ns < 0 || ns > SM_MAXSD) {
      mpcqp_stage_destroy(s);
      return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library declares stage data but not 0..8 values per frame");
    }
    s->nsd = ns;
    // optional export of a library generated with transition_data: the rows reach F, kfun and llink as well.  A library without it reports 0.
    auto tdf = (int (*)())dlsym(lib, "mpcqp_user_transition_data");
    s->tdata = ns > 0 && tdf && tdf() != 0;
  }
  std::vector<unsigned char> mask((size_t)(2 * nx + nu) * (2 * nx + nu));
  auto cf = (int (*)(unsigned char *))dlsym(lib, "mpcqp_user_cost");
  s->general_cost = cf && cf(mask.data());
  // optional export of a library generated with a link cost (llink): the structure of its Hessian over [s; u; s_next; u_next], which joins the
  // pattern of P; the kernels of that library carry the same table.  A library without it -- every one generated before this entry -- has none.
  std::vector<unsigned char> lmask((size_t)4 * (nx + nu) * (nx + nu));
  auto lf = (int (*)(unsigned char *))dlsym(lib, "mpcqp_user_link_cost");
  s->link_cost = lf && lf(lmask.data());
  // optional export of a library generated with a Gauss-Newton frame cost (rcost): the number of its residual rows.  Nothing else differs for the
  // handle: the library's eval kernel writes 2 J'J into the pattern of the cost mask
  {
    auto rf = (int (*)())dlsym(lib, "mpcqp_user_residual_cost");
    s->residual_rows = s->general_cost && rf ? rf() : 0;
  }
  if (int rc = stage_create_common(&dd, nx, nu, nh, h_lo, h_hi, s, s->general_cost ? mask.data() : nullptr, nk, k_lo, k_hi, pref,
                                   s->link_cost ? lmask.data() : nullptr)) { mpcqp_stage_destroy(s); return rc; }
  // optional export of a library generated with convexify = True: the launcher of mpcqp_stage_convexify.  Its cost mask is closed under the
  // fill-in of the correction, so every element the kernel adds has a slot in the pattern just built; the tables say which.
  if (s->general_cost && user.convexify) {
    if (int rc = stage_build_convexify_tables(s, mask.data())) { mpcqp_stage_destroy(s); return rc; }
  }
  // optional exports of a library generated with exact_hessian = True: the structure of the constraint curvature over [s; u] -- part of the cost mask,
  // so every element has a slot in the pattern just built -- and the launcher of mpcqp_stage_lagrangian
  {
    auto ef = (int (*)(unsigned char *))dlsym(lib, "mpcqp_user_exact_hessian");
    std::vector<unsigned char> cmask((size_t)(nx + nu) * (nx + nu));
    if (s->general_cost && ef && ef(cmask.data()) && user.lagrangian) {
      if (int rc = stage_build_lagrangian_table(s, cmask.data())) { mpcqp_stage_destroy(s); return rc; }
    }
  }
  *out = s;
  return MPCQP_OK;
}

int mpcqp_stage_create(const mpcqp_stage_desc *d, mpcqp_stage **out) { return stage_create_zoo(d, false, out); }

int mpcqp_stage_create_user(const mpcqp_stage_desc *d, const char *library_path, mpcqp_stage **out) { return stage_create_library(d, library_path, false, out); }

int mpcqp_stage_create_tracking(const mpcqp_stage_desc *d, const char *library_path, mpcqp_stage **out) {
  return library_path ? stage_create_library(d, library_path, true, out) : stage_create_zoo(d, true, out);
}

void mpcqp_stage_destroy(mpcqp_stage *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->dPp) (void)hipFree(s->dPp);
  if (s->dAp) (void)hipFree(s->dAp);
  if (s->dQk) (void)hipFree(s->dQk);
  if (s->dRk) (void)hipFree(s->dRk);
  if (s->dmask) (void)hipFree(s->dmask);
  if (s->dhlo) (void)hipFree(s->dhlo);
  if (s->dhhi) (void)hipFree(s->dhhi);
  for (int w = 0; w < 2; w++) if (s->dth[w]) (void)hipFree(s->dth[w]);
  for (int w = 0; w < 2; w++) if (s->dsd[w]) (void)hipFree(s->dsd[w]);
  if (s->dslots) (void)hipFree(s->dslots);
  if (s->dcvx) (void)hipFree(s->dcvx);
  if (s->dlslots) (void)hipFree(s->dlslots);
  if (s->dkkt) (void)hipFree(s->dkkt);
  if (s->dric) (void)hipFree(s->dric);
  if (s->ddir) (void)hipFree(s->ddir);
  if (s->ddws) (void)hipFree(s->ddws);
  if (s->dactws) (void)hipFree(s->dactws);
  if (s->dipmws) (void)hipFree(s->dipmws);
  if (s->user_lib) dlclose(s->user_lib);
  delete s;
}

// two optional per-frame arrays on the device (da, db: the handle's buffers, allocated on first use; sa, sb: StageDev's pointers).  a, b null:
// back to the shared values, the buffers stay for the next call
static int stage_upload_pair(mpcqp_stage *s, const double *a, const double *b, size_t bytes_a, size_t bytes_b, double **da, double **db,
                             const double **sa, const double **sb) {
  MPCQP_HIPCHK(hipSetDevice(s->device));
  if (!a) { *sa = nullptr; *sb = nullptr; return MPCQP_OK; }
  if (!*da) MPCQP_HIPCHK(hipMalloc(da, bytes_a));
  if (!*db) MPCQP_HIPCHK(hipMalloc(db, bytes_b));
  MPCQP_HIPCHK(hipMemcpy(*da, a, bytes_a, hipMemcpyHostToDevice));
  MPCQP_HIPCHK(hipMemcpy(*db, b, bytes_b, hipMemcpyHostToDevice));
  *sa = *da; *sb = *db;
  return MPCQP_OK;
}

int mpcqp_stage_set_weights(mpcqp_stage *s, const double *Qk, const double *Rk) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if ((Qk == nullptr) != (Rk == nullptr)) return mpcqp_set_error(MPCQP_ERR_ARG, "give both weight arrays or neither");
  if (s->general_cost) return mpcqp_set_error(MPCQP_ERR_ARG, "this evaluator was generated with its own stage cost; diagonal weights do not apply");
  StageDev &sd = s->sd;
  return stage_upload_pair(s, Qk, Rk, (size_t)sd.N * sd.nx * sizeof(double), (size_t)sd.N * sd.nu * sizeof(double), &s->dQk, &s->dRk, &sd.Qk, &sd.Rk);
}

int mpcqp_stage_set_path_bounds(mpcqp_stage *s, const double *lo, const double *hi) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if ((lo == nullptr) != (hi == nullptr)) return mpcqp_set_error(MPCQP_ERR_ARG, "give both bound arrays or neither");
  StageDev &sd = s->sd;
  if (sd.nh == 0) return mpcqp_set_error(MPCQP_ERR_ARG, "this evaluator has no path constraint");
  const size_t bytes = (size_t)sd.N * sd.nh * sizeof(double);
  return stage_upload_pair(s, lo, hi, bytes, bytes, &s->dhlo, &s->dhhi, &sd.h_lok, &sd.h_hik);
}

int mpcqp_stage_param_count(const mpcqp_stage *s) { return s ? s->ntheta : 0; }

int mpcqp_stage_set_instance_params(mpcqp_stage *s, int which, int batch, const double *theta, int mem) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (s->ntheta == 0)
    return mpcqp_set_error(MPCQP_ERR_ARG, s->sd.model == MPCQP_MODEL_USER
                                              ? "this library was generated without parameters (ntheta = 0): its constants are part of the code; declare ntheta and theta on the model and regenerate"
                                              : "this model has no parameters (mpcqp_stage_param_count is 0)");
  if (which != MPCQP_PARAMS_MODEL && which != MPCQP_PARAMS_PLANT) return mpcqp_set_error(MPCQP_ERR_ARG, "which must be MPCQP_PARAMS_MODEL or MPCQP_PARAMS_PLANT");
  if (!theta) { s->th_batch[which] = 0; return MPCQP_OK; }      // back to the shared values; the buffer stays for the next call
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return mpcqp_set_error(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  const size_t bytes = (size_t)batch * SM_NPAR * sizeof(double);
  if (batch > s->th_cap[which]) {
    double *nb = nullptr;
    MPCQP_HIPCHK(hipMalloc(&nb, bytes));
    MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that reads the old rows may still be queued
    if (s->dth[which]) (void)hipFree(s->dth[which]);
    s->dth[which] = nb; s->th_cap[which] = batch; s->th_batch[which] = 0;
  }
  MPCQP_HIPCHK(hipMemcpy(s->dth[which], theta, bytes, mem == MPCQP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
  s->th_batch[which] = batch;
  return MPCQP_OK;
}

int mpcqp_stage_data_count(const mpcqp_stage *s) { return s ? s->nsd : 0; }
int mpcqp_stage_has_transition_data(const mpcqp_stage *s) { return s && s->tdata ? 1 : 0; }

int mpcqp_stage_set_stage_data(mpcqp_stage *s, int batch, const double *d, int mem) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (s->nsd == 0)
    return mpcqp_set_error(MPCQP_ERR_ARG, s->sd.model == MPCQP_MODEL_USER
                                              ? "this library was generated without stage data (nsd = 0): the numbers in its constraints and costs are part of the code; declare nsd and sdata on the model and regenerate"
                                              : "the built-in models take no stage data (mpcqp_stage_data_count is 0)");
  if (!d) { s->sd_batch = 0; return MPCQP_OK; }      // back to the defaults; the buffers stay for the next call
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return mpcqp_set_error(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  const size_t bytes = (size_t)batch * s->sd.N * s->nsd * sizeof(double);
  if (batch > s->sd_cap) {
    double *nb[2] = {nullptr, nullptr};
    MPCQP_HIPCHK(hipMalloc(&nb[0], bytes));
    if (hipMalloc(&nb[1], bytes) != hipSuccess) { (void)hipFree(nb[0]); return mpcqp_set_error(MPCQP_ERR_HIP, "hipMalloc of the stage data failed"); }
    MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that reads the old rows may still be queued
    for (int w = 0; w < 2; w++) { if (s->dsd[w]) (void)hipFree(s->dsd[w]); s->dsd[w] = nb[w]; }
    s->sd_cap = batch; s->sd_batch = 0; s->sd_cur = 0;
  }
  MPCQP_HIPCHK(hipMemcpy(s->dsd[s->sd_cur], d, bytes, mem == MPCQP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
  s->sd_batch = batch;
  return MPCQP_OK;
}

int mpcqp_stage_shift_data(mpcqp_stage *s, int batch, const double *d_new, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (s->nsd == 0) return mpcqp_set_error(MPCQP_ERR_ARG, "this handle takes no stage data (mpcqp_stage_data_count is 0)");
  if (s->sd_batch == 0) return mpcqp_set_error(MPCQP_ERR_STATE, "no stage data are stored (mpcqp_stage_set_stage_data): the defaults do not shift");
  if (batch != s->sd_batch) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be that of the stored stage data: every stored row shifts");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  const long tot = (long)batch * s->sd.N * s->nsd;
  stage_shift_data_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, (hipStream_t)stream>>>(batch, s->sd.N, s->nsd, s->dsd[s->sd_cur], d_new, s->dsd[1 - s->sd_cur]);
  MPCQP_HIPCHK(hipGetLastError());
  s->sd_cur = 1 - s->sd_cur;
  return MPCQP_OK;
}

int mpcqp_stage_dims(const mpcqp_stage *s, int *o) {
  if (!s || !o) return mpcqp_set_error(MPCQP_ERR_ARG, "null argument");
  const StageDev &d = s->sd;
  o[0] = d.nx; o[1] = d.nu; o[2] = d.np; o[3] = d.n; o[4] = d.m; o[5] = d.nnzP; o[6] = d.nnzA; o[7] = d.nvar;
  return MPCQP_OK;
}

int mpcqp_stage_has_cost(const mpcqp_stage *s) { return s && s->general_cost ? 1 : 0; }

int mpcqp_stage_has_link_cost(const mpcqp_stage *s) { return s && s->link_cost ? 1 : 0; }

int mpcqp_stage_has_residual_cost(const mpcqp_stage *s) { return s ? s->residual_rows : 0; }

int mpcqp_stage_pattern(const mpcqp_stage *s, int *Pp, int *Pi, int *Ap, int *Ai) {
  if (!s || !Pp || !Pi || !Ap || !Ai) return mpcqp_set_error(MPCQP_ERR_ARG, "null argument");
  std::copy(s->Pp.begin(), s->Pp.end(), Pp); std::copy(s->Pi.begin(), s->Pi.end(), Pi);
  std::copy(s->Ap.begin(), s->Ap.end(), Ap); std::copy(s->Ai.begin(), s->Ai.end(), Ai);
  return MPCQP_OK;
}

int mpcqp_stage_eval(mpcqp_stage *s, int batch, const double *p, const double *x, const double *lbx, const double *ubx,
                     const double *lbg, const double *ubg, double *P, double *q, double *A, double *l, double *u, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!p || !x || !lbx || !ubx || !lbg || !ubg || !P || !q || !A || !l || !u) return mpcqp_set_error(MPCQP_ERR_ARG, "null data pointer");
  const StageDev &sd = s->sd;
  const StageEvalArgs a{p, x, lbx, ubx, lbg, ubg, P, q, A, l, u};
  hipStream_t st = (hipStream_t)stream;
  return stage_launch(s, batch, STAGE_ROWS_THETA,
      [&](auto t) { using T = decltype(t); return stage_launch_eval<typename T::M, T::PF>(sd, batch, a, st); },
      [&](StageTheta th) { return mpcqp_launch_eval_pp(sd, batch, a, st, th); },
      [&](const StageRows &r) { return stage_hipchk(s->user.eval(&sd, batch, &a, &r, stream)); });
}

int mpcqp_stage_merit(mpcqp_stage *s, int batch, const double *p, const double *x, double *f, double *gmax, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch <= 0 || !p || !x) return mpcqp_set_error(MPCQP_ERR_ARG, "bad batch or null data pointer");
  const StageDev &sd = s->sd;
  const StageMeritArgs a{p, x, f, gmax};
  hipStream_t st = (hipStream_t)stream;
  return stage_launch(s, batch, STAGE_ROWS_THETA,
      [&](auto t) { using T = decltype(t); return stage_launch_merit<typename T::M, T::PF>(sd, batch, a, st); },
      [&](StageTheta th) { return mpcqp_launch_merit_pp(sd, batch, a, st, th); },
      [&](const StageRows &r) { return stage_hipchk(s->user.merit(&sd, batch, &a, &r, stream)); });
}

int mpcqp_stage_step(mpcqp_stage *s, int batch, double alpha, const double *dw, double *x, double *step_max, const int *status, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch <= 0 || !dw || !x) return mpcqp_set_error(MPCQP_ERR_ARG, "bad batch or null data pointer");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  MPCQP_HIPCHK(mpcqp_launch_step(batch, s->sd.nvar, s->sd.n, s->sd.np, alpha, dw, x, step_max, status, (hipStream_t)stream));
  return MPCQP_OK;
}

int mpcqp_stage_advance(mpcqp_stage *s, int batch, const mpcqp_stage_advance_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->x_in || !a->x_out || !a->lbx || !a->ubx) return mpcqp_set_error(MPCQP_ERR_ARG, "x_in, x_out, lbx and ubx are required");
  if (a->x_out == a->x_in) return mpcqp_set_error(MPCQP_ERR_ARG, "the shift is out of place: x_out must differ from x_in");
  if ((a->dw_in == nullptr) != (a->dw_out == nullptr) || (a->y_in == nullptr) != (a->y_out == nullptr))
    return mpcqp_set_error(MPCQP_ERR_ARG, "give both dw_in and dw_out (y_in and y_out) or neither");
  if ((a->dw_out && a->dw_out == a->dw_in) || (a->y_out && a->y_out == a->y_in))
    return mpcqp_set_error(MPCQP_ERR_ARG, "the shift is out of place: dw_out / y_out must differ from dw_in / y_in");
  if (s->sd.pref) {
    if (!a->p_in || !a->p_out) return mpcqp_set_error(MPCQP_ERR_ARG, "a tracking handle needs p_in and p_out");
    if (a->p_out == a->p_in) return mpcqp_set_error(MPCQP_ERR_ARG, "the shift is out of place: p_out must differ from p_in");
    if (a->p) return mpcqp_set_error(MPCQP_ERR_ARG, "p belongs to non-tracking handles; a tracking handle takes its references from p_in");
  } else {
    if (a->p_in || a->p_out || a->r_new) return mpcqp_set_error(MPCQP_ERR_ARG, "p_in, p_out and r_new belong to tracking handles");
    if (a->stage_cost && !a->p) return mpcqp_set_error(MPCQP_ERR_ARG, "stage_cost needs the reference p");
  }
  if (a->w && a->s_meas) return mpcqp_set_error(MPCQP_ERR_ARG, "a disturbance applies to the simulated plant only: give w or s_meas, not both");
  if (a->tail != MPCQP_TAIL_REPEAT && a->tail != MPCQP_TAIL_ROLLOUT) return mpcqp_set_error(MPCQP_ERR_ARG, "unknown tail");
  if (s->sd.model == MPCQP_MODEL_USER && !s->user.advance)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_user_advance (generated before this entry); regenerate it");
  const StageDev &sd = s->sd;
  hipStream_t st = (hipStream_t)stream;
  return stage_launch(s, batch, STAGE_ROWS_THETA | STAGE_ROWS_PLANT,
      [&](auto t) { using T = decltype(t); return stage_launch_advance<typename T::M, T::PF>(sd, batch, *a, st); },
      [&](StageTheta th) { return mpcqp_launch_advance_pp(sd, batch, *a, st, th); },
      [&](const StageRows &r) { return stage_hipchk(s->user.advance(&sd, batch, a, &r, stream)); });
}

int mpcqp_stage_linesearch(mpcqp_stage *s, int batch, const mpcqp_stage_linesearch_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch <= 0) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->p || !a->x || !a->lbx || !a->ubx || !a->q || !a->dw || !a->y) return mpcqp_set_error(MPCQP_ERR_ARG, "p, x, lbx, ubx, q, dw and y are required");
  if (a->candidates < 1 || a->candidates > MPCQP_LINESEARCH_MAX_CANDIDATES) return mpcqp_set_error(MPCQP_ERR_ARG, "candidates must be in 1..8");
  if (!(a->beta > 0.0 && a->beta < 1.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "beta must lie in (0, 1)");
  if (!(a->alpha0 > 0.0) || !std::isfinite(a->alpha0)) return mpcqp_set_error(MPCQP_ERR_ARG, "alpha0 must be positive");
  if (!(a->c1 >= 0.0 && a->c1 < 1.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "c1 must lie in [0, 1)");
  if (!(a->mu_min >= 0.0) || !(a->mu_factor >= 0.0) || !std::isfinite(a->mu_min) || !std::isfinite(a->mu_factor))
    return mpcqp_set_error(MPCQP_ERR_ARG, "mu_min and mu_factor must be finite and not negative");
  if (s->sd.model == MPCQP_MODEL_USER && !s->user.linesearch)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_user_linesearch (generated before this entry); regenerate it");
  const StageDev &sd = s->sd;
  hipStream_t st = (hipStream_t)stream;
  return stage_launch(s, batch, STAGE_ROWS_THETA,
      [&](auto t) { using T = decltype(t); return stage_launch_linesearch<typename T::M, T::PF>(sd, batch, *a, st); },
      [&](StageTheta th) { return mpcqp_launch_linesearch_pp(sd, batch, *a, st, th); },
      [&](const StageRows &r) { return stage_hipchk(s->user.linesearch(&sd, batch, a, &r, stream)); });
}

int mpcqp_stage_rollout(mpcqp_stage *s, int batch, const mpcqp_stage_rollout_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->x_in || !a->x_out) return mpcqp_set_error(MPCQP_ERR_ARG, "x_in and x_out are required");
  if ((a->lbx == nullptr) != (a->ubx == nullptr)) return mpcqp_set_error(MPCQP_ERR_ARG, "give both lbx and ubx or neither");
  if (a->inputs != MPCQP_ROLLOUT_INPUTS_ITERATE && a->inputs != MPCQP_ROLLOUT_INPUTS_HOLD)
    return mpcqp_set_error(MPCQP_ERR_ARG, "inputs must be MPCQP_ROLLOUT_INPUTS_ITERATE or MPCQP_ROLLOUT_INPUTS_HOLD");
  if (s->sd.model == MPCQP_MODEL_USER && !s->user.rollout)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_user_rollout (generated before this entry); regenerate it");
  const StageDev &sd = s->sd;
  hipStream_t st = (hipStream_t)stream;
  return stage_launch(s, batch, STAGE_ROWS_THETA,
      [&](auto t) { using T = decltype(t); return stage_launch_rollout<typename T::M>(sd, batch, *a, st); },
      [&](StageTheta th) { return mpcqp_launch_rollout_pp(sd, batch, *a, st, th); },
      [&](const StageRows &r) { return stage_hipchk(s->user.rollout(&sd, batch, a, &r, stream)); });
}

int mpcqp_stage_has_convexify(const mpcqp_stage *s) { return s && s->convexify ? 1 : 0; }

// the scratch of a convexification launch, grown on first use, and the handle's tables as the kernels take them
static int stage_convexify_buffers(mpcqp_stage *s, int batch, StageCvxBuf *w) {
  const StageDev &sd = s->sd;
  const size_t nx2 = (size_t)sd.nx * sd.nx;
  if (batch > s->cvx_cap) {
    double *nb = nullptr;
    MPCQP_HIPCHK(hipMalloc(&nb, (size_t)batch * sd.N * (nx2 * sizeof(double) + sizeof(int))));
    MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that uses the old scratch may still be queued
    if (s->dcvx) (void)hipFree(s->dcvx);
    s->dcvx = nb; s->cvx_cap = batch;
  }
  const int nl = sd.f + sd.nx;
  *w = StageCvxBuf{s->dslots, s->dslots + (size_t)sd.N * nl * nl, s->dcvx, (int *)(s->dcvx + (size_t)s->cvx_cap * sd.N * nx2)};
  return MPCQP_OK;
}

int mpcqp_stage_convexify(mpcqp_stage *s, int batch, const mpcqp_stage_convexify_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (a->mode != MPCQP_CONVEXIFY_PROJECT && a->mode != MPCQP_CONVEXIFY_MIRROR)
    return mpcqp_set_error(MPCQP_ERR_ARG, "mode must be MPCQP_CONVEXIFY_PROJECT or MPCQP_CONVEXIFY_MIRROR");
  if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return mpcqp_set_error(MPCQP_ERR_ARG, "eps must be positive and finite");
  if (!a->P || !a->x || (s->sd.np > 0 && !a->p)) return mpcqp_set_error(MPCQP_ERR_ARG, "p, x and P are required");
  if (s->sd.model != MPCQP_MODEL_USER)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the built-in models have diagonal weights: there is nothing to convexify (a generated model with lcost and convexify = True has)");
  if (!s->convexify)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_user_convexify: regenerate it from a model with a stage cost (lcost) and convexify = True");
  return stage_launch(s, batch, 0, [&](const StageRows &r) -> int {      // (lcost / lterm read no theta: the parameter rows are not looked at)
    StageCvxBuf w;
    if (int rc = stage_convexify_buffers(s, batch, &w)) return rc;
    return stage_hipchk(s->user.convexify(&s->sd, batch, a, &w, &r, stream));
  });
}

int mpcqp_stage_has_exact_hessian(const mpcqp_stage *s) { return s && s->exact ? 1 : 0; }

int mpcqp_stage_lagrangian(mpcqp_stage *s, int batch, const mpcqp_stage_lagrangian_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (a->mode != 0 && a->mode != MPCQP_CONVEXIFY_PROJECT && a->mode != MPCQP_CONVEXIFY_MIRROR)
    return mpcqp_set_error(MPCQP_ERR_ARG, "mode must be 0, MPCQP_CONVEXIFY_PROJECT or MPCQP_CONVEXIFY_MIRROR");
  if (a->mode != 0 && (!(a->eps > 0.0) || !std::isfinite(a->eps))) return mpcqp_set_error(MPCQP_ERR_ARG, "eps must be positive and finite");
  if (!a->P || !a->x || !a->y || (a->mode != 0 && s->sd.np > 0 && !a->p)) return mpcqp_set_error(MPCQP_ERR_ARG, "x, y and P (with a mode: p) are required");
  if (s->sd.model != MPCQP_MODEL_USER)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the built-in models have diagonal weights: their pattern has no slots for the constraint curvature (a generated model with lcost and exact_hessian = True has)");
  if (!s->exact)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "the library does not export mpcqp_user_lagrangian: regenerate it from a model with a stage cost (lcost) and exact_hessian = True");
  if (a->mode != 0 && !s->convexify)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "a mode needs the convexification: regenerate the library from a model that also sets convexify = True");
  return stage_launch(s, batch, STAGE_ROWS_THETA, [&](const StageRows &r) -> int {
    StageCvxBuf w;
    if (a->mode != 0) if (int rc = stage_convexify_buffers(s, batch, &w)) return rc;
    return stage_hipchk(s->user.lagrangian(&s->sd, batch, a, s->dlslots, a->mode != 0 ? &w : nullptr, &r, stream));
  });
}

// the optimality residuals at the system mpcqp_stage_eval just wrote (kkt.hip; no model code takes part, so a generated library needs no export)
int mpcqp_stage_kkt(mpcqp_stage *s, int batch, const mpcqp_kkt_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  return mpcqp_kkt_run(s->device, s->sd.n, s->sd.m, s->sd.np, s->sd.nnzA, s->dkkt, batch, a, stream);
}

// Slot tables of mpcqp_stage_riccati (StageRicTab): H_k[r][c] sits in column np + k f + c, row np + k f + r of P, -[A_k B_k][r][c] in column
// np + k f + c, row n + k nx + r of A; both are found in the pattern itself, -1 where it has no such entry.
static int stage_build_riccati_tables(mpcqp_stage *s) {
  const StageDev &sd = s->sd;
  const int f = sd.f, nx = sd.nx, N = sd.N;
  const size_t np_ = (size_t)N * f * f;
  std::vector<int> tab(np_ + (size_t)(N - 1) * nx * f, -1);
  auto find = [](const std::vector<int> &cp, const std::vector<int> &ri, int row, int col) {
    for (int e = cp[col]; e < cp[col + 1]; e++) if (ri[e] == row) return e;
    return -1;
  };
  for (int k = 0; k < N; k++)
    for (int r = 0; r < f; r++)
      for (int c = 0; c < f; c++) tab[((size_t)k * f + r) * f + c] = find(s->Pp, s->Pi, sd.np + k * f + r, sd.np + k * f + c);
  for (int k = 0; k < N - 1; k++)
    for (int r = 0; r < nx; r++)
      for (int c = 0; c < f; c++) tab[np_ + ((size_t)k * nx + r) * f + c] = find(s->Ap, s->Ai, sd.n + k * nx + r, sd.np + k * f + c);
  int *d = nullptr;
  if (hipMalloc(&d, tab.size() * sizeof(int)) != hipSuccess) return mpcqp_set_error(MPCQP_ERR_HIP, "hipMalloc of the Riccati slot tables failed");
  if (hipMemcpy(d, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the Riccati slot tables failed");
  }
  s->dric = d;
  return MPCQP_OK;
}

// the feedback gains along the plan (stage_riccati.hpp; no model code takes part, so a generated library needs no export)
int mpcqp_stage_riccati(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->P || !a->A || !a->K) return mpcqp_set_error(MPCQP_ERR_ARG, "P, A and K are required");
  if (!((a->x && a->lbx && a->ubx) || (!a->x && !a->lbx && !a->ubx))) return mpcqp_set_error(MPCQP_ERR_ARG, "the clamp needs x, lbx and ubx: give all three or none");
  if (!(a->clamp_tol >= 0.0) || !(a->reg >= 0.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "clamp_tol and reg must not be negative");
  if (s->link_cost)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "this handle has a link cost: its P couples neighbouring frames, and a Riccati sweep over the frame blocks alone would drop those terms");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (!s->dric) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    MPCQP_HIPCHK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return mpcqp_set_error(MPCQP_ERR_STATE, "the first mpcqp_stage_riccati of a handle builds its slot tables and may not run while the stream is capturing: call it once before the capture");
    if (int rc = stage_build_riccati_tables(s)) return rc;
  }
  const StageDev &sd = s->sd;
  const StageRicTab tab{s->dric, s->dric + (size_t)sd.N * sd.f * sd.f};
  const hipError_t e = sd.f <= 8 ? stage_launch_riccati<16, 8>(sd, batch, *a, tab, st)
                     : sd.f <= 16 ? stage_launch_riccati<16, 16>(sd, batch, *a, tab, st) : stage_launch_riccati<32, 24>(sd, batch, *a, tab, st);
  MPCQP_HIPCHK(e);
  return MPCQP_OK;
}

// Slot tables of mpcqp_stage_riccati_solve on top of the sweep's (StageDirTab): the path rows' and the link rows' entries of A per frame, and the
// parameter columns of P below the parameter rows; all found in the pattern itself.
static int stage_build_direct_tables(mpcqp_stage *s) {
  const StageDev &sd = s->sd;
  const int f = sd.f, nx = sd.nx, N = sd.N, nh = sd.nh, nk = sd.nk, np = sd.np;
  const int rowh = sd.n + (N - 1) * nx, rowk = rowh + N * nh;
  auto find = [&](int row, int col) {
    for (int e = s->Ap[col]; e < s->Ap[col + 1]; e++) if (s->Ai[e] == row) return e;
    return -1;
  };
  std::vector<int> hs((size_t)N * nh * f, -1), k0((size_t)(N - 1) * nk * f, -1), k1((size_t)(N - 1) * nk * f, -1), pcp(np + 1, 0), pcs, pcr;
  for (int k = 0; k < N; k++)
    for (int r = 0; r < nh; r++)
      for (int c = 0; c < f; c++) hs[((size_t)k * nh + r) * f + c] = find(rowh + k * nh + r, np + k * f + c);
  for (int k = 0; k < N - 1; k++)
    for (int r = 0; r < nk; r++)
      for (int c = 0; c < f; c++) {
        k0[((size_t)k * nk + r) * f + c] = find(rowk + k * nk + r, np + k * f + c);
        k1[((size_t)k * nk + r) * f + c] = find(rowk + k * nk + r, np + (k + 1) * f + c);
      }
  for (int j = 0; j < np; j++) {
    for (int e = s->Pp[j]; e < s->Pp[j + 1]; e++)
      if (s->Pi[e] >= np && s->Pi[e] < sd.n) { pcs.push_back(e); pcr.push_back(s->Pi[e] - np); }
    pcp[j + 1] = (int)pcs.size();
  }
  std::vector<int> tab;
  const std::vector<int> *parts[6] = {&hs, &k0, &k1, &pcp, &pcs, &pcr};
  for (int i = 0; i < 6; i++) { if (i >= 1) s->dir_off[i - 1] = tab.size(); tab.insert(tab.end(), parts[i]->begin(), parts[i]->end()); }
  tab.push_back(0);      // (never empty)
  int *d = nullptr;
  if (hipMalloc(&d, tab.size() * sizeof(int)) != hipSuccess) return mpcqp_set_error(MPCQP_ERR_HIP, "hipMalloc of the direct solve's slot tables failed");
  if (hipMemcpy(d, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return mpcqp_set_error(MPCQP_ERR_HIP, "upload of the direct solve's slot tables failed");
  }
  s->ddir = d;
  return MPCQP_OK;
}

// the direct solve of the stage QP (stage_riccati.hpp; no model code takes part, so a generated library needs no export)
int mpcqp_stage_riccati_solve(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->P || !a->q || !a->A || !a->l || !a->u) return mpcqp_set_error(MPCQP_ERR_ARG, "P, q, A, l and u are required");
  if (!a->w || !a->y || !a->direct) return mpcqp_set_error(MPCQP_ERR_ARG, "w, y and direct are required");
  if (!(a->feas_tol >= 0.0) || !(a->reg >= 0.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "feas_tol and reg must not be negative");
  if (s->link_cost)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "this handle has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame blocks alone would drop those terms");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  const StageDev &sd = s->sd;
  if (!s->dric || !s->ddir || batch > s->dir_cap) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    MPCQP_HIPCHK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return mpcqp_set_error(MPCQP_ERR_STATE, "the first mpcqp_stage_riccati_solve of a handle (and the first at a larger batch) builds its slot tables and its workspace and may not run while the stream is capturing: call it once before the capture");
    if (!s->dric) if (int rc = stage_build_riccati_tables(s)) return rc;
    if (!s->ddir) if (int rc = stage_build_direct_tables(s)) return rc;
    if (batch > s->dir_cap) {
      double *nb = nullptr;
      MPCQP_HIPCHK(hipMalloc(&nb, (size_t)batch * sd.N * ((size_t)sd.nu * (sd.nx + 1) + sd.f) * sizeof(double)));
      MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that uses the old workspace may still be queued
      if (s->ddws) (void)hipFree(s->ddws);
      s->ddws = nb; s->dir_cap = batch;
    }
  }
  const StageDirTab tab{s->dric, s->dric + (size_t)sd.N * sd.f * sd.f, s->ddir, s->ddir + s->dir_off[0], s->ddir + s->dir_off[1],
                        s->ddir + s->dir_off[2], s->ddir + s->dir_off[3], s->ddir + s->dir_off[4]};
  const hipError_t e = sd.f <= 8 ? stage_launch_direct<16, 8>(sd, batch, *a, tab, s->ddws, st)
                     : sd.f <= 16 ? stage_launch_direct<16, 16>(sd, batch, *a, tab, s->ddws, st) : stage_launch_direct<32, 24>(sd, batch, *a, tab, s->ddws, st);
  MPCQP_HIPCHK(e);
  return MPCQP_OK;
}

// the direct solve with held input bounds (stage_riccati_active.hpp): the tables of the entry above, a workspace of its own
int mpcqp_stage_riccati_solve_active(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_active_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->P || !a->q || !a->A || !a->l || !a->u) return mpcqp_set_error(MPCQP_ERR_ARG, "P, q, A, l and u are required");
  if (!a->w || !a->y || !a->direct) return mpcqp_set_error(MPCQP_ERR_ARG, "w, y and direct are required");
  if (!(a->feas_tol >= 0.0) || !(a->reg >= 0.0) || !(a->dual_tol >= 0.0)) return mpcqp_set_error(MPCQP_ERR_ARG, "feas_tol, reg and dual_tol must not be negative");
  if (a->rounds < 1 || a->rounds > MPCQP_ACTIVE_MAX_ROUNDS) return mpcqp_set_error(MPCQP_ERR_ARG, "rounds must be 1 .. 8");
  if (s->link_cost)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "this handle has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame blocks alone would drop those terms");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  const StageDev &sd = s->sd;
  if (!s->dric || !s->ddir || batch > s->act_cap) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    MPCQP_HIPCHK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return mpcqp_set_error(MPCQP_ERR_STATE, "the first mpcqp_stage_riccati_solve_active of a handle (and the first at a larger batch) builds its slot tables and its workspace and may not run while the stream is capturing: call it once before the capture");
    if (!s->dric) if (int rc = stage_build_riccati_tables(s)) return rc;
    if (!s->ddir) if (int rc = stage_build_direct_tables(s)) return rc;
    if (batch > s->act_cap) {
      double *nb = nullptr;
      MPCQP_HIPCHK(hipMalloc(&nb, (size_t)batch * stage_act_ws_doubles(sd) * sizeof(double)));
      MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that uses the old workspace may still be queued
      if (s->dactws) (void)hipFree(s->dactws);
      s->dactws = nb; s->act_cap = batch;
    }
  }
  const StageDirTab tab{s->dric, s->dric + (size_t)sd.N * sd.f * sd.f, s->ddir, s->ddir + s->dir_off[0], s->ddir + s->dir_off[1],
                        s->ddir + s->dir_off[2], s->ddir + s->dir_off[3], s->ddir + s->dir_off[4]};
  const hipError_t e = sd.f <= 8 ? stage_launch_direct_active<16, 8>(sd, batch, *a, tab, s->dactws, st)
                     : sd.f <= 16 ? stage_launch_direct_active<16, 16>(sd, batch, *a, tab, s->dactws, st)
                                  : stage_launch_direct_active<32, 24>(sd, batch, *a, tab, s->dactws, st);
  MPCQP_HIPCHK(e);
  return MPCQP_OK;
}

// the interior-point direct solve (stage_riccati_ipm.hpp): the tables of mpcqp_stage_riccati_solve, a workspace of its own
int mpcqp_stage_riccati_solve_ipm(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_ipm_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->P || !a->q || !a->A || !a->l || !a->u) return mpcqp_set_error(MPCQP_ERR_ARG, "P, q, A, l and u are required");
  if (!a->w || !a->y || !a->direct) return mpcqp_set_error(MPCQP_ERR_ARG, "w, y and direct are required");
  if (!(a->feas_tol >= 0.0) || !(a->reg >= 0.0) || !(a->comp_tol >= 0.0) || !(a->stat_tol >= 0.0))
    return mpcqp_set_error(MPCQP_ERR_ARG, "feas_tol, reg, comp_tol and stat_tol must not be negative");
  if (a->iters < 1 || a->iters > MPCQP_IPM_MAX_ITERS) return mpcqp_set_error(MPCQP_ERR_ARG, "iters must be 1 .. 50");
  if (s->link_cost)
    return mpcqp_set_error(MPCQP_ERR_LIMIT, "this handle has a link cost: its P couples neighbouring frames, and a Riccati recursion over the frame blocks alone would drop those terms");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  const StageDev &sd = s->sd;
  if (!s->dric || !s->ddir || batch > s->ipm_cap) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    MPCQP_HIPCHK(hipStreamIsCapturing(st, &cap));
    if (cap != hipStreamCaptureStatusNone)
      return mpcqp_set_error(MPCQP_ERR_STATE, "the first mpcqp_stage_riccati_solve_ipm of a handle (and the first at a larger batch) builds its slot tables and its workspace and may not run while the stream is capturing: call it once before the capture");
    if (!s->dric) if (int rc = stage_build_riccati_tables(s)) return rc;
    if (!s->ddir) if (int rc = stage_build_direct_tables(s)) return rc;
    if (batch > s->ipm_cap) {
      double *nb = nullptr;
      MPCQP_HIPCHK(hipMalloc(&nb, (size_t)batch * stage_ipm_ws_doubles(sd) * sizeof(double)));
      MPCQP_HIPCHK(hipDeviceSynchronize());       // a launch that uses the old workspace may still be queued
      if (s->dipmws) (void)hipFree(s->dipmws);
      s->dipmws = nb; s->ipm_cap = batch;
    }
  }
  const StageDirTab tab{s->dric, s->dric + (size_t)sd.N * sd.f * sd.f, s->ddir, s->ddir + s->dir_off[0], s->ddir + s->dir_off[1],
                        s->ddir + s->dir_off[2], s->ddir + s->dir_off[3], s->ddir + s->dir_off[4]};
  const hipError_t e = sd.f <= 8 ? stage_launch_direct_ipm<16, 8>(sd, batch, *a, tab, s->dipmws, st)
                     : sd.f <= 16 ? stage_launch_direct_ipm<16, 16>(sd, batch, *a, tab, s->dipmws, st)
                                  : stage_launch_direct_ipm<32, 24>(sd, batch, *a, tab, s->dipmws, st);
  MPCQP_HIPCHK(e);
  return MPCQP_OK;
}

int mpcqp_stage_feedback(mpcqp_stage *s, int batch, const mpcqp_stage_feedback_args *a, void *stream) {
  if (!s) return mpcqp_set_error(MPCQP_ERR_ARG, "stage handle is null");
  if (batch < 1) return mpcqp_set_error(MPCQP_ERR_ARG, "batch must be positive");
  if (!a) return mpcqp_set_error(MPCQP_ERR_ARG, "the argument block is null");
  if (!a->K || !a->s || !a->s_nom || !a->u_nom || !a->x_out) return mpcqp_set_error(MPCQP_ERR_ARG, "K, s, s_nom, u_nom and x_out are required");
  if ((a->lo == nullptr) != (a->hi == nullptr) || (a->lbx == nullptr) != (a->ubx == nullptr))
    return mpcqp_set_error(MPCQP_ERR_ARG, "give both lo and hi (lbx and ubx) or neither");
  const StageDev &sd = s->sd;
  if (a->k < 0 || a->k >= sd.N) return mpcqp_set_error(MPCQP_ERR_ARG, "k must be a frame of the horizon, 0 .. N - 1");
  MPCQP_HIPCHK(hipSetDevice(s->device));
  const long tot = (long)batch * sd.nu;
  stage_feedback_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, (hipStream_t)stream>>>(batch, sd.N, sd.nx, sd.nu, sd.nvar, *a);
  MPCQP_HIPCHK(hipGetLastError());
  return MPCQP_OK;
}

}  // extern "C"
