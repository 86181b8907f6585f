// stage_models.hpp -- the stage-OCP model zoo as scalar-generic functors (host + device).
//
// In the reference the dynamics are CasADi SX expressions that SQPOptimizationSolver differentiates symbolically
// (reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77, AutoDifferentiator.cpp:99-140).  Here every model is a
// template over the scalar type: instantiated with double it evaluates, with Dual it carries one directional
// derivative (forward mode), which is how the device kernels obtain one Jacobian column per thread.
// The expressions follow optimal_control_problem_amd/models.py operation by operation (same association order), so
// host and device values agree to rounding of sin/cos.
#pragma once
#include <cmath>
#include <type_traits>
#include <vector>

#if defined(__HIPCC__)
#define SM_HD __host__ __device__ __forceinline__
#else
#define SM_HD inline
#endif

struct Dual { double v, d; };
SM_HD Dual mk(double v) { return {v, 0.0}; }
SM_HD Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
SM_HD Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
SM_HD Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
SM_HD Dual operator/(Dual a, Dual b) { const double q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
SM_HD Dual operator+(Dual a, double b) { return {a.v + b, a.d}; }
SM_HD Dual operator+(double a, Dual b) { return {a + b.v, b.d}; }
SM_HD Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
SM_HD Dual operator-(double a, Dual b) { return {a - b.v, -b.d}; }
SM_HD Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
SM_HD Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
SM_HD Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
SM_HD Dual operator/(double a, Dual b) { const double q = a / b.v; return {q, -q * b.d / b.v}; }
SM_HD Dual sm_sin(Dual a) { return {sin(a.v), cos(a.v) * a.d}; }
SM_HD Dual sm_cos(Dual a) { return {cos(a.v), -sin(a.v) * a.d}; }
SM_HD Dual sm_tan(Dual a) { const double t = tan(a.v); return {t, (1.0 + t * t) * a.d}; }
SM_HD Dual sm_exp(Dual a) { const double e = exp(a.v); return {e, e * a.d}; }
SM_HD Dual sm_log(Dual a) { return {log(a.v), a.d / a.v}; }
SM_HD Dual sm_sqrt(Dual a) { const double r = sqrt(a.v); return {r, 0.5 * a.d / r}; }
SM_HD Dual sm_tanh(Dual a) { const double t = tanh(a.v); return {t, (1.0 - t * t) * a.d}; }
SM_HD Dual operator-(Dual a) { return {-a.v, -a.d}; }
SM_HD double sm_tan(double a) { return tan(a); }
SM_HD double sm_exp(double a) { return exp(a); }
SM_HD double sm_log(double a) { return log(a); }
SM_HD double sm_sqrt(double a) { return sqrt(a); }
SM_HD double sm_tanh(double a) { return tanh(a); }
SM_HD double sm_sin(double a) { return sin(a); }
SM_HD double sm_cos(double a) { return cos(a); }
SM_HD double sm_val(double a) { return a; }
SM_HD double sm_val(Dual a) { return a.v; }
SM_HD double sm_der(double) { return 0.0; }
SM_HD double sm_der(Dual a) { return a.d; }

// a functor with a cooperative F (Fc: the lanes of a stage share the value part's expensive pieces) says so with `coop`; generated functors have none
template <class M, class = void> struct sm_has_coop : std::false_type {};
template <class M> struct sm_has_coop<M, std::void_t<decltype(M::coop)>> : std::bool_constant<(M::coop != 0)> {};

enum { SM_DOUBLE_INTEGRATOR = 0, SM_QUADROTOR = 1, SM_CARTPOLE = 2, SM_NMODELS = 3 };
constexpr int SM_MAXNX = 16, SM_MAXNU = 8, SM_NPAR = 8, SM_MAXNH = 16, SM_MAXNK = 8;

// continuous dynamics + RK4 over dt (models.py StageOCP.F); models with a closed-form discrete map override F.  `cd(state, derivative)` is the
// continuous dynamics at fixed u (a callable, so that a model can pass a cooperative form of it: SmQuadrotor::Fc)
template <int nx, class T, class CD>
SM_HD void sm_rk4_with(double h, const T *s, T *out, CD &&cd) {
  T k[nx], acc[nx], st[nx];
  cd(s, k);
#pragma unroll
  for (int i = 0; i < nx; i++) { acc[i] = k[i]; st[i] = s[i] + (0.5 * h) * k[i]; }
  cd(st, k);
#pragma unroll
  for (int i = 0; i < nx; i++) { acc[i] = acc[i] + 2.0 * k[i]; st[i] = s[i] + (0.5 * h) * k[i]; }
  cd(st, k);
#pragma unroll
  for (int i = 0; i < nx; i++) { acc[i] = acc[i] + 2.0 * k[i]; st[i] = s[i] + h * k[i]; }
  cd(st, k);
#pragma unroll
  for (int i = 0; i < nx; i++) out[i] = s[i] + (h / 6.0) * (acc[i] + k[i]);
}
template <class M, class T>
SM_HD void sm_rk4(const double *par, double h, const T *s, const T *u, T *out) {
  sm_rk4_with<M::nx, T>(h, s, out, [&](const T *st, T *k) { M::cdyn(par, st, u, k); });
}

// nx = 2, nu = 1; exact zero-order-hold map (models.py DoubleIntegrator.F); no parameters
struct SmDoubleIntegrator {
  static constexpr int nx = 2, nu = 1, nh = 0, nk = 0, has_cost = 0, has_term = 0, ntheta = 0;
  template <class T> SM_HD static void H(const T *, const T *, T *) {}
  template <class T> SM_HD static void F(const double *, double h, const T *s, const T *u, T *out) {
    out[0] = s[0] + h * s[1] + ((0.5 * h) * h) * u[0];
    out[1] = s[1] + h * u[0];
  }
};

// 12-state quadrotor (models.py Quadrotor.cdyn); par = {mass, grav, arm, kappa, Jx, Jy, Jz}
struct SmQuadrotor {
  static constexpr int nx = 12, nu = 4, nh = 0, nk = 0, has_cost = 0, has_term = 0, ntheta = 7;
  static constexpr int coop = 1;      // has Fc: the lanes of a stage evaluate the trigonometry together (stage_kernels.hpp)
  template <class T> SM_HD static void H(const T *, const T *, T *) {}
  // t = {sin, cos} of roll, pitch, yaw
  template <class T> SM_HD static void trig(const T *s, T *t) { t[1] = sm_cos(s[3]); t[0] = sm_sin(s[3]); t[3] = sm_cos(s[4]); t[2] = sm_sin(s[4]); t[5] = sm_cos(s[5]); t[4] = sm_sin(s[5]); }
  template <class T> SM_HD static void cdyn(const double *par, const T *s, const T *u, T *ds) { T t[6]; trig(s, t); cdyn_t(par, s, u, t, ds); }
  template <class T> SM_HD static void cdyn_t(const double *par, const T *s, const T *u, const T *t, T *ds) {
    const double mass = par[0], grav = par[1], arm = par[2], kappa = par[3], Jx = par[4], Jy = par[5], Jz = par[6];
    const T cph = t[1], sph = t[0], cth = t[3], sth = t[2], cps = t[5], sps = t[4];
    const T tth = sth / cth;
    const T thrust = u[0] + u[1] + u[2] + u[3];
    const T a = thrust / mass;
    const T p_ = s[9], q_ = s[10], r_ = s[11];
    ds[0] = s[6]; ds[1] = s[7]; ds[2] = s[8];
    ds[3] = p_ + sph * tth * q_ + cph * tth * r_;
    ds[4] = cph * q_ - sph * r_;
    ds[5] = (sph * q_ + cph * r_) / cth;
    ds[6] = a * (cps * sth * cph + sps * sph);
    ds[7] = a * (sps * sth * cph - cps * sph);
    ds[8] = a * (cth * cph) - grav;
    const T tx = arm * (u[3] - u[1]), ty = arm * (u[2] - u[0]), tz = kappa * (u[0] - u[1] + u[2] - u[3]);
    ds[9] = (tx - (Jz - Jy) * q_ * r_) / Jx;
    ds[10] = (ty - (Jx - Jz) * p_ * r_) / Jy;
    ds[11] = (tz - (Jy - Jx) * p_ * q_) / Jz;
  }
  template <class T> SM_HD static void F(const double *par, double h, const T *s, const T *u, T *out) { sm_rk4<SmQuadrotor, T>(par, h, s, u, out); }
#if defined(__HIPCC__)
  // F on dual numbers for the f = 16 lanes of one stage together (stage_eval_kernel: lane r of the group carries direction r, the VALUE parts of s and
  // u are the same in all of them -- and so are those of every RK4 stage state).  The six sines and cosines of a cdyn call are what the evaluation
  // spends its time on (f64 sin / cos: ~70 instructions each, times 6, times 4 RK4 stages, in each of the 16 lanes): lane r < 3 evaluates angle r, the
  // values travel by shuffle, and every lane applies its own derivative part: one sin + one cos per call instead of three each.  Same values, same
  // operation order everywhere else: the result is bitwise F<Dual>'s.
  __device__ static void Fc(const double *par, double h, const Dual *s, const Dual *u, Dual *out, const int r) {
    const int base = (int)(threadIdx.x & 63) - r;
    sm_rk4_with<nx, Dual>(h, s, out, [&](const Dual *st, Dual *k) {
      const double a = r == 0 ? st[3].v : (r == 1 ? st[4].v : st[5].v);
      double sv, cv; sincos(a, &sv, &cv);
      Dual t[6];
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const double sq = __shfl(sv, base + q, 64), cq = __shfl(cv, base + q, 64);
        t[2 * q] = {sq, cq * st[3 + q].d}; t[2 * q + 1] = {cq, -sq * st[3 + q].d};
      }
      cdyn_t(par, st, u, t, k);
    });
  }
#endif
};

// cart-pole, s = [x, theta, xdot, thetadot], theta = 0 upright (models.py CartPole.cdyn); par = {mc, mp, length, grav}
struct SmCartPole {
  static constexpr int nx = 4, nu = 1, nh = 0, nk = 0, has_cost = 0, has_term = 0, ntheta = 4;
  template <class T> SM_HD static void H(const T *, const T *, T *) {}
  template <class T> SM_HD static void cdyn(const double *par, const T *s, const T *u, T *ds) {
    const double mc = par[0], mp = par[1], len = par[2], grav = par[3];
    const T sn = sm_sin(s[1]), cs = sm_cos(s[1]);
    const T thd = s[3];
    const double tot = mc + mp;
    const T tmp = (u[0] + (mp * len) * thd * thd * sn) / tot;
    const T thdd = (grav * sn - cs * tmp) / (len * (4.0 / 3.0 - mp * cs * cs / tot));
    const T xdd = tmp - (mp * len) * thdd * cs / tot;
    ds[0] = s[2]; ds[1] = s[3]; ds[2] = xdd; ds[3] = thdd;
  }
  template <class T> SM_HD static void F(const double *par, double h, const T *s, const T *u, T *out) { sm_rk4<SmCartPole, T>(par, h, s, u, out); }
};

// ---------------------------------------------------------------------------------------------- host-side structure
inline void sm_model_dims(int model, int *nx, int *nu) {
  switch (model) {
    case SM_DOUBLE_INTEGRATOR: *nx = SmDoubleIntegrator::nx; *nu = SmDoubleIntegrator::nu; break;
    case SM_QUADROTOR: *nx = SmQuadrotor::nx; *nu = SmQuadrotor::nu; break;
    case SM_CARTPOLE: *nx = SmCartPole::nx; *nu = SmCartPole::nu; break;
    default: *nx = *nu = 0;
  }
}

// CSC structure of the local system in the reference's formulation (w = [p; x], rows [p; x; g],
// reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77), rows ascending inside a column:
//   P column p_i: rows p_i, s_0[i] .. s_{N-1}[i];  column s_k[i]: rows p_i, s_k[i];  column u_k[i]: row u_k[i]
//   A column j: row j; for a state column of frame k >= 1 the +1 of s_k in g_{k-1}[c]; for k < N-1 the nx rows of g_k;
//   then the nh path-constraint rows of frame k (rows [p; x; g; h; r], h_k behind all dynamics rows), then the nk link-constraint
//   rows r_{k-1} and r_k this frame takes part in (r_k = K(frame_k, frame_{k+1}), k < N - 1, behind all path rows)
// pref (per-frame references, p = [r_0; ...; r_{N-1}], np = N nx): column p_k[i] has the rows p_k[i], s_k[i]; column s_k[i] the rows p_k[i], s_k[i];
// A is the same with the larger identity block
inline void sm_build_pattern(int nx, int nu, int N, int nh, int nk, std::vector<int> &Pp, std::vector<int> &Pi, std::vector<int> &Ap, std::vector<int> &Ai,
                             bool pref = false) {
  const int f = nx + nu, np = pref ? N * nx : nx, n = np + N * f;
  Pp.assign(1, 0); Ap.assign(1, 0); Pi.clear(); Ai.clear();
  for (int i = 0; i < np; i++) {
    Pi.push_back(i);
    if (pref) Pi.push_back(np + (i / nx) * f + i % nx);
    else for (int k = 0; k < N; k++) Pi.push_back(np + k * f + i);
    Pp.push_back((int)Pi.size());
    Ai.push_back(i); Ap.push_back((int)Ai.size());
  }
  for (int k = 0; k < N; k++)
    for (int c = 0; c < f; c++) {
      const int j = np + k * f + c;
      if (c < nx) Pi.push_back(pref ? k * nx + c : c);
      Pi.push_back(j);
      Pp.push_back((int)Pi.size());
      Ai.push_back(j);
      if (k >= 1 && c < nx) Ai.push_back(n + (k - 1) * nx + c);
      if (k < N - 1) for (int r = 0; r < nx; r++) Ai.push_back(n + k * nx + r);
      for (int r = 0; r < nh; r++) Ai.push_back(n + (N - 1) * nx + k * nh + r);
      if (k >= 1) for (int r = 0; r < nk; r++) Ai.push_back(n + (N - 1) * nx + N * nh + (k - 1) * nk + r);
      if (k < N - 1) for (int r = 0; r < nk; r++) Ai.push_back(n + (N - 1) * nx + N * nh + k * nk + r);
      Ap.push_back((int)Ai.size());
    }
}

// P structure for a general stage cost sum_k l(s_k, u_k, p) (generated libraries, codegen.py): mask is the Hessian's structure over
// the local variables [s; u; r] (row-major nl x nl, nl = f + nx, symmetric, diagonal set).  Both triangles, rows ascending:
//   column p_i: rows p_r with mask[f + r][f + i], then per frame k the rows frame_k[r] with mask[r][f + i]
//   column frame_k[c]: rows p_i with mask[f + i][c], then rows frame_k[r] with mask[r][c]
// pref (sum_k l(s_k, u_k, r_k), the mask still over [s; u; r]): column p_k[i]: rows p_k[r] with mask[f + r][f + i], then rows frame_k[r] with mask[r][f + i];
//   column frame_k[c]: rows p_k[i] with mask[f + i][c], then rows frame_k[r] with mask[r][c]
inline void sm_build_cost_pattern(int nx, int nu, int N, const unsigned char *mask, std::vector<int> &Pp, std::vector<int> &Pi, bool pref = false) {
  const int f = nx + nu, np = pref ? N * nx : nx, nl = f + nx;
  Pp.assign(1, 0); Pi.clear();
  if (pref) {
    for (int k = 0; k < N; k++)
      for (int i = 0; i < nx; i++) {
        for (int r = 0; r < nx; r++) if (mask[(f + r) * nl + f + i]) Pi.push_back(k * nx + r);
        for (int r = 0; r < f; r++) if (mask[r * nl + f + i]) Pi.push_back(np + k * f + r);
        Pp.push_back((int)Pi.size());
      }
    for (int k = 0; k < N; k++)
      for (int c = 0; c < f; c++) {
        for (int i = 0; i < nx; i++) if (mask[(f + i) * nl + c]) Pi.push_back(k * nx + i);
        for (int r = 0; r < f; r++) if (mask[r * nl + c]) Pi.push_back(np + k * f + r);
        Pp.push_back((int)Pi.size());
      }
    return;
  }
  for (int i = 0; i < np; i++) {
    for (int r = 0; r < np; r++) if (mask[(f + r) * nl + f + i]) Pi.push_back(r);
    for (int k = 0; k < N; k++)
      for (int r = 0; r < f; r++) if (mask[r * nl + f + i]) Pi.push_back(np + k * f + r);
    Pp.push_back((int)Pi.size());
  }
  for (int k = 0; k < N; k++)
    for (int c = 0; c < f; c++) {
      for (int i = 0; i < np; i++) if (mask[(f + i) * nl + c]) Pi.push_back(i);
      for (int r = 0; r < f; r++) if (mask[r * nl + c]) Pi.push_back(np + k * f + r);
      Pp.push_back((int)Pi.size());
    }
}
