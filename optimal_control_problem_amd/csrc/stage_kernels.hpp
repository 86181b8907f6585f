// stage_kernels.hpp -- device templates of the local-system evaluation (see stage_eval.hip for the design notes).
// Included by stage_eval.hip (the built-in zoo) and by the translation units optimal_control_problem_amd/codegen.py
// generates for user-defined dynamics (the native analogue of the reference's gen_code / load_lib flow,
// reference src/OptimalControlProblem.cpp:263-287,602-640).  STAGE_ABI_VERSION guards the StageDev layout shared between
// libmpcqp.so and a generated library.
#pragma once
#include <hip/hip_runtime.h>
#include "stage_models.hpp"
#include "stage_convexify.hpp"
#include "../../include/mpcqp.h"

#define STAGE_ABI_VERSION 8

struct StageDev {
  int model, N, nx, nu, f, np, n, m, ng, nvar, nnzP, nnzA;   // ng = all general rows: (N-1)*nx dynamics rows, then N*nh path rows, then (N-1)*nk link rows
  int nh, ngd, nk;
  int pref;   // per-frame references (mpcqp_stage_create_tracking): p = [r_0; ...; r_{N-1}], np = N nx, frame k's cost terms take r_k (the PF = true kernels)
  double h_lo[SM_MAXNH], h_hi[SM_MAXNH];   // path-constraint bounds, for the merit kernel's violation measure
  double k_lo[SM_MAXNK], k_hi[SM_MAXNK];   // link-constraint bounds (the same on every stage), likewise
  double dt;
  double Q[SM_MAXNX], R[SM_MAXNU], par[SM_NPAR];
  const int *Pp, *Ap;   // device copies of the column pointers
  const double *Qk, *Rk;   // optional per-frame diagonal weights [N * nx], [N * nu] (device; NULL = Q, R for every frame)
  const unsigned char *hmask;   // general stage cost (M::has_cost): Hessian structure over [s; u; r], (f + nx)^2 bytes (device)
  const double *h_lok, *h_hik;  // optional per-frame path-constraint bounds [N * nh] (device; NULL = h_lo, h_hi on every frame)
};

// PP (per-instance plant parameters, mpcqp_stage_set_instance_params): rows of SM_NPAR doubles, instance b's at [b * SM_NPAR], in the order of
// StageDev::par.  `model` is what the controller believes (eval, merit, linesearch, the rollout tail of advance), `plant` what the plant step of
// advance uses; a null set stands for the shared values sd.par.  The PP instances of the four kernels below take one StageTheta as an extra,
// last argument -- the template's trailing pack PP is empty or {StageTheta}, so the instances without it keep their signature and their code.
struct StageTheta { const double *model, *plant; };
// SD (stage data, mpcqp_stage_set_stage_data): rows of M::nsd doubles, frame k of instance b at [(b * N + k) * nsd] -- values the generated hfun,
// lcost and lterm read as d[i] (an obstacle's centre, a scheduled weight): data, not variables, no derivative is taken with respect to them.  A null
// pointer stands for the defaults M::sdata0 on every frame.  The SD instances take one StageData as the last argument, behind the StageTheta of
// a PP instance: the trailing pack is {}, {StageTheta}, {StageData} or {StageTheta, StageData}, and an instance without an element keeps its
// signature and its code.  Generated functors only: the zoo declares no nsd.
struct StageData { const double *d; };
constexpr int SM_MAXSD = 8;
template <class T, class... PP> inline constexpr bool stage_has = (std::is_same_v<T, PP> || ...);
// the pack's element of type T, or a null one
template <class T> __device__ __forceinline__ T stage_get() { return T{}; }
template <class T, class A, class... R> __device__ __forceinline__ T stage_get(A a, R... r) {
  if constexpr (std::is_same_v<T, A>) return a; else return stage_get<T>(r...);
}
template <class... PP> __device__ __forceinline__ StageTheta stage_theta(PP... pp) { return stage_get<StageTheta>(pp...); }
// how many entries of a parameter row the functor reads (M::ntheta; functors without the member read none)
template <class M, class = void> struct sm_ntheta : std::integral_constant<int, 0> {};
template <class M> struct sm_ntheta<M, std::void_t<decltype(M::ntheta)>> : std::integral_constant<int, M::ntheta> {};
// how many stage-data values per frame the functor reads (M::nsd; functors without the member read none and keep the signatures without d)
template <class M, class = void> struct sm_nsd : std::integral_constant<int, 0> {};
template <class M> struct sm_nsd<M, std::void_t<decltype(M::nsd)>> : std::integral_constant<int, M::nsd> {};
template <class M> inline constexpr int sm_nsd_regs = sm_nsd<M>::value > 0 ? sm_nsd<M>::value : 1;
// frame k's row of instance b into registers (a functor without stage data: nothing)
template <class M, class... PP> __device__ __forceinline__ void stage_load_data(double (&dv)[sm_nsd_regs<M>], int b, int N, int k, PP... pp) {
  if constexpr (sm_nsd<M>::value > 0) {
    constexpr int nsd = sm_nsd<M>::value;
    const double *dp = stage_get<StageData>(pp...).d;
    if (dp) dp += ((long)b * N + k) * nsd;
#pragma unroll
    for (int i = 0; i < nsd; i++) dv[i] = dp ? dp[i] : M::sdata0[i];
  }
}
// H, and the generated gradient of the frame cost (the last frame the terminal one's), of a functor with or without stage data
template <class M, class T> __device__ __forceinline__ void stage_path(const T *s, const T *u, const double *d, T *out) {
  if constexpr (sm_nsd<M>::value > 0) M::template H<T>(s, u, d, out); else M::template H<T>(s, u, out);
}
template <class M, class T> __device__ __forceinline__ void stage_cost_grad(bool last, const T *s, const T *u, const T *r, const double *d, T *out) {
  if constexpr (sm_nsd<M>::value > 0) { if (M::has_term && last) M::template LTG<T>(s, u, r, d, out); else M::template LG<T>(s, u, r, d, out); }
  else { if (M::has_term && last) M::template LTG<T>(s, u, r, out); else M::template LG<T>(s, u, r, out); }
}
// what stage_eval_kernel reads for the column that carries the seed: g[i].d = column c of the frame Hessian, g[c].v = the column's gradient entry.  A
// functor with a scalar cost: the generated gradient on dual numbers (the exact Hessian); one with a residual (sm_has_residual): the Gauss-Newton
// column 2 J' J_c and 2 J_c' r (sm_residual_column).  Each lane forms its own column: the mapping of threads to columns is that of the exact path
template <class M> __device__ __forceinline__ void stage_cost_column(bool last, const Dual *s, const Dual *u, const Dual *r, const double *d, Dual *out) {
  if constexpr (sm_has_residual<M>::value) sm_residual_column<M, (sm_nsd<M>::value > 0)>(last, s, u, r, d, out);
  else stage_cost_grad<M, Dual>(last, s, u, r, d, out);
}

// the QP returned a point (solved, solved inaccurately, or stopped at the iteration limit): its dw, y may be used
__device__ __forceinline__ bool stage_status_ok(int s) { return s == MPCQP_SOLVED || s == MPCQP_SOLVED_INACCURATE || s == MPCQP_MAX_ITER_REACHED; }
// the generated stage cost (M::has_cost); the last frame takes the terminal one where the model has it
template <class M, class T> __device__ __forceinline__ void stage_cost_value(bool last, const T *s, const T *u, const T *r, const double *d, T *out) {
  if constexpr (sm_nsd<M>::value > 0) { if (M::has_term && last) M::template LT<T>(s, u, r, d, out); else M::template L<T>(s, u, r, d, out); }
  else { if (M::has_term && last) M::template LT<T>(s, u, r, out); else M::template L<T>(s, u, r, out); }
}

// Transition data (models.StageOCP.transition_data): a generated functor that declares tdata = 1 takes the stage-data row of the
// transition's first frame -- row k for the step k -> k + 1 -- behind the inputs of F, K, LK, LKG and FG as well.  One trait decides for all five; the
// zoo and every functor generated without the flag declare nothing and keep their signatures and their code.
template <class M, class = void> struct sm_tdata : std::false_type {};
template <class M> struct sm_tdata<M, std::void_t<decltype(M::tdata)>> : std::bool_constant<M::tdata != 0> {};
template <class M, class T> __device__ __forceinline__ void stage_dyn(const double *par, double dt, const T *s, const T *u, const double *d, T *out) {
  if constexpr (sm_tdata<M>::value) M::template F<T>(par, dt, s, u, d, out); else M::template F<T>(par, dt, s, u, out);
}
template <class M, class T> __device__ __forceinline__ void stage_link(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out) {
  if constexpr (sm_tdata<M>::value) M::template K<T>(s, u, sn, un, d, out); else M::template K<T>(s, u, sn, un, out);
}
template <class M, class T> __device__ __forceinline__ void stage_link_cost(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out) {
  if constexpr (sm_tdata<M>::value) M::template LK<T>(s, u, sn, un, d, out); else M::template LK<T>(s, u, sn, un, out);
}
template <class M, class T> __device__ __forceinline__ void stage_link_cost_grad(const T *s, const T *u, const T *sn, const T *un, const double *d, T *out) {
  if constexpr (sm_tdata<M>::value) M::template LKG<T>(s, u, sn, un, d, out); else M::template LKG<T>(s, u, sn, un, out);
}
// the second row the eval kernel needs: row k - 1 for the pair (k - 1, k), compiled in only for a functor that has a link constraint or a link cost
template <class M> inline constexpr bool sm_tdata_pair = sm_tdata<M>::value && (M::nk > 0 || sm_has_link_cost<M>::value);

// PF (per-frame references, StageDev::pref): the parameter block holds one reference state per frame.  Parameter column j = k nx + i is thread j of
// its instance, as before; the cooperative mapping pads the N nx parameter slots up to a multiple of f, so that every frame's f lanes still start
// at a multiple of f (threads per instance ceil(N nx / f) f + N f).  Adjacent lanes still own adjacent columns: the store streams stay contiguous.
template <class M, bool PF = false, class... PP>
__global__ void __launch_bounds__(256) stage_eval_kernel(StageDev sd, int batch, const double *__restrict__ p, const double *__restrict__ x,
                                                         const double *__restrict__ lbx, const double *__restrict__ ubx,
                                                         const double *__restrict__ lbg, const double *__restrict__ ubg,
                                                         double *__restrict__ P, double *__restrict__ q, double *__restrict__ A,
                                                         double *__restrict__ l, double *__restrict__ u, PP... pp) {
  constexpr bool HASPP = stage_has<StageTheta, PP...>;
  constexpr int NT = sm_ntheta<M>::value > 0 ? sm_ntheta<M>::value : 1;
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu;
  // cooperative functors (sm_has_coop): the f lanes of a stage sit in one wave at a multiple of f -- the parameter columns get a group of f thread
  // slots of their own (nx of them used), every frame the next f; threads per instance f (N + 1) instead of n
  constexpr bool COOP = sm_has_coop<M>::value && (64 % f == 0) && nx <= f;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = sd.n, N = sd.N;
  const int npar = PF ? N * nx : nx;                                  // parameter columns
  const int ppad = PF ? (npar + f - 1) / f * f : f;                   // their thread slots under the cooperative mapping
  const int per = COOP ? ppad + f * N : n;
  if (gid >= (long)batch * per) return;
  const int b = (int)(gid / per), jt = (int)(gid - (long)b * per);
  // PP: a wave holds lanes of several instances (the cooperative quadrotor at N = 2: 48 thread slots per instance), so b and the parameter row are
  // per lane; the entries the functor reads are loaded once, here, and live in registers from then on
  double th[NT];
  const double *par = sd.par;
  if constexpr (HASPP) {
    const double *row = stage_theta(pp...).model + (long)b * SM_NPAR;
#pragma unroll
    for (int i = 0; i < NT; i++) th[i] = row[i];
    par = th;
  }
  if (COOP && jt < ppad && jt >= npar) return;       // (padding lanes of the parameter group)
  const int j = COOP ? (jt < ppad ? jt : jt - ppad + npar) : jt;
  const double *pb = p + (long)b * npar, *xb = x + (long)b * sd.nvar;
  double *Pc = P + (long)b * sd.nnzP + sd.Pp[j], *Ac = A + (long)b * sd.nnzA + sd.Ap[j];
  double *qb = q + (long)b * n, *lb = l + (long)b * sd.m, *ub = u + (long)b * sd.m;
  if constexpr (PF) {
    if (j < npar) {
      // column p_k[i]: only frame k takes r_k.  Diagonal cost: H = {d2f/dr_k[i]2, d2f/dr_k[i] ds_k[i]} = {2 Q_k,i, -2 Q_k,i}, grad = -2 Q_k,i (s_k[i] - r_k[i]);
      // general cost: one pass of frame k's gradient on dual numbers seeded on r_k[i], rows p_k first, then the frame's.  Rows l = u = p - p.
      const int k = j / nx, i = j - k * nx;
      const double *fr = xb + k * f, *rk = pb + k * nx;
      const double pi = rk[i];
      if constexpr (M::has_cost) {
        constexpr int nl = f + nx;
        const unsigned char *mk = sd.hmask + f + i;
        Dual s[nx], uu[nu], rr[nx], g[nl];
        double dv[sm_nsd_regs<M>];
        stage_load_data<M>(dv, b, N, k, pp...);
#pragma unroll
        for (int a = 0; a < nx; a++) { s[a] = {fr[a], 0.0}; rr[a] = {rk[a], a == i ? 1.0 : 0.0}; }
#pragma unroll
        for (int a = 0; a < nu; a++) uu[a] = {fr[nx + a], 0.0};
        stage_cost_column<M>(k == N - 1, s, uu, rr, dv, g);
        int e = 0;
        double gv = 0.0;
#pragma unroll
        for (int r = 0; r < nx; r++) { if (mk[(f + r) * nl]) Pc[e++] = g[f + r].d; gv = r == i ? g[f + r].v : gv; }
#pragma unroll
        for (int r = 0; r < f; r++) if (mk[r * nl]) Pc[e++] = g[r].d;
        qb[j] = gv;
      } else {
        const double Qi = sd.Qk ? sd.Qk[j] : sd.Q[i];
        Pc[0] = 2.0 * Qi; Pc[1] = -2.0 * Qi;
        qb[j] = -2.0 * Qi * (fr[i] - pi);
      }
      Ac[0] = 1.0;
      lb[j] = pi - pi; ub[j] = pi - pi;
      return;
    }
  } else if (j < nx) {
    const double pi = pb[j];
    if constexpr (M::has_cost) {
      // general stage cost: column p_i of the Hessian = sum over the frames of d(grad l_k)/dr_i (dual numbers through the
      // generated gradient); the rows p_r accumulate over k, the rows of frame k are written as they come
      constexpr int nl = f + nx;
      const unsigned char *mk = sd.hmask + f + j;
      int e = 0;
#pragma unroll
      for (int r = 0; r < nx; r++) e += mk[(f + r) * nl] ? 1 : 0;
      double acc[nx], qa = 0.0;
#pragma unroll
      for (int r = 0; r < nx; r++) acc[r] = 0.0;
      Dual s[nx], uu[nu], rr[nx], g[nl];
      double dv[sm_nsd_regs<M>];
#pragma unroll
      for (int i = 0; i < nx; i++) rr[i] = {pb[i], i == j ? 1.0 : 0.0};
      for (int k = 0; k < N; k++) {
        const double *fr = xb + k * f;
        stage_load_data<M>(dv, b, N, k, pp...);
#pragma unroll
        for (int i = 0; i < nx; i++) s[i] = {fr[i], 0.0};
#pragma unroll
        for (int i = 0; i < nu; i++) uu[i] = {fr[nx + i], 0.0};
        stage_cost_column<M>(k == N - 1, s, uu, rr, dv, g);
        double gv = 0.0;
#pragma unroll
        for (int r = 0; r < nx; r++) { acc[r] += g[f + r].d; gv = r == j ? g[f + r].v : gv; }
        qa += gv;
#pragma unroll
        for (int r = 0; r < f; r++) if (mk[r * nl]) Pc[e++] = g[r].d;
      }
      e = 0;
#pragma unroll
      for (int r = 0; r < nx; r++) if (mk[(f + r) * nl]) Pc[e++] = acc[r];
      qb[j] = qa;
    } else if (sd.Qk) {   // per-frame weights: d2f/dp_i2 = 2 sum_k Q_k,i
      // column p_i: H = d2f/dp_i2 = 2 N Q_i, d2f/dp_i ds_k[i] = -2 Q_i; grad = -2 Q_i sum_k (s_k[i] - p_i); rows l = u = p - p
      double e = 0.0, qs = 0.0;
      for (int k = 0; k < N; k++) { const double Qi = sd.Qk[k * nx + j]; qs += Qi; Pc[1 + k] = -2.0 * Qi; e += (xb[k * f + j] - pi) * Qi; }
      Pc[0] = 2.0 * qs;
      qb[j] = -2.0 * e;
    } else {
      double e = 0.0;
      const double Qi = sd.Q[j];
      Pc[0] = 2.0 * N * Qi;
      for (int k = 0; k < N; k++) { Pc[1 + k] = -2.0 * Qi; e += (xb[k * f + j] - pi) * Qi; }
      qb[j] = -2.0 * e;
    }
    Ac[0] = 1.0;
    lb[j] = pi - pi; ub[j] = pi - pi;
    return;
  }
  const int jj = j - npar, k = jj / f, c = jj - k * f;
  const double *fr = xb + k * f;
  if constexpr (PF) pb += k * nx;               // frame k's reference r_k stands where p stood
  const double xv = fr[c];
  // SD: the f lanes of a frame read the same row, once, into registers: hfun and the frame cost below take it from there
  double dv[sm_nsd_regs<M>];
  stage_load_data<M>(dv, b, N, k, pp...);
  // transition data: F, K and LKG of the pair (k, k + 1) take dv; K and LKG of the pair (k - 1, k) take row k - 1, a second load skipped at k = 0
  [[maybe_unused]] double dvp[sm_nsd_regs<M>];
  if constexpr (sm_tdata_pair<M>) { if (k >= 1) stage_load_data<M>(dvp, b, N, k - 1, pp...); }
  Dual s[nx], uu[nu];
#pragma unroll
  for (int i = 0; i < nx; i++) s[i] = {fr[i], i == c ? 1.0 : 0.0};
#pragma unroll
  for (int i = 0; i < nu; i++) uu[i] = {fr[nx + i], nx + i == c ? 1.0 : 0.0};
  if constexpr (sm_has_link_cost<M>::value) {
    // Link cost sum_{k<N-1} llink(frame_k, frame_{k+1}) (generated functors: LK, LKG, lmask).  Column frame_k[c] takes part in pair k-1 as the second
    // frame and in pair k as the first: up to two more passes of the generated gradient LKG on dual numbers, the seed on this column.  Rows in
    // the pattern's order (sm_frame_column_rows): the p rows, then frame k-1's rows M^{k-1}[r][f + c], then frame k's -- the frame term first, then
    // M^{k-1}[f + r][f + c], then M^k[r][c], a fixed order -- then frame k+1's rows M^k[f + r][c].  One writer per entry, as everywhere here.
    constexpr int f2 = 2 * f;
    const bool first = k >= 1, second = k < N - 1;      // this column is the second frame of a pair / the first frame of one
    // the rows of this column as bit sets (sm_link_bits: four loads), empty where the pair does not exist
    const unsigned bprev = first ? sm_link_bits<M>::tab.prev[c] : 0u, bown1 = first ? sm_link_bits<M>::tab.own1[c] : 0u;
    const unsigned bown0 = second ? sm_link_bits<M>::tab.own0[c] : 0u, bnext = second ? sm_link_bits<M>::tab.next[c] : 0u;
    unsigned bbase;                // the rows of frame k the frame term has in this column
    int e = 0;
    double hb[f], ha[f], gv;       // frame k's rows of the frame term's column and of pair k-1's; q[j]
    if constexpr (M::has_cost) {
      constexpr int nl = f + nx;
      const unsigned char *mk = sd.hmask + c;
      Dual rr[nx], g[nl];
#pragma unroll
      for (int i = 0; i < nx; i++) rr[i] = {pb[i], 0.0};
      stage_cost_column<M>(k == N - 1, s, uu, rr, dv, g);
#pragma unroll
      for (int i = 0; i < nx; i++) if (mk[(f + i) * nl]) Pc[e++] = g[f + i].d;
      gv = 0.0; bbase = 0u;
#pragma unroll
      for (int r = 0; r < f; r++) { hb[r] = g[r].d; gv = r == c ? g[r].v : gv; bbase |= (mk[r * nl] ? 1u : 0u) << r; }
    } else {
      double w;
      if (c < nx) {
        w = sd.Qk ? sd.Qk[k * nx + c] : sd.Q[c];
        Pc[e++] = -2.0 * w;
        gv = 2.0 * (xv - pb[c]) * w;
      } else {
        w = sd.Rk ? sd.Rk[k * nu + c - nx] : sd.R[c - nx];
        gv = 2.0 * xv * w;
      }
#pragma unroll
      for (int r = 0; r < f; r++) hb[r] = r == c ? 2.0 * w : 0.0;
      bbase = 1u << c;
    }
    Dual os[nx], ou[nu], g2[f2];
#pragma unroll
    for (int r = 0; r < f; r++) ha[r] = 0.0;
    if (first) {
      const double *pf = fr - f;
#pragma unroll
      for (int i = 0; i < nx; i++) os[i] = {pf[i], 0.0};
#pragma unroll
      for (int i = 0; i < nu; i++) ou[i] = {pf[nx + i], 0.0};
      stage_link_cost_grad<M, Dual>(os, ou, s, uu, dvp, g2);
      double ga = 0.0;
#pragma unroll
      for (int r = 0; r < f; r++) if ((bprev >> r) & 1u) Pc[e++] = g2[r].d;
#pragma unroll
      for (int r = 0; r < f; r++) { ha[r] = g2[f + r].d; ga = r == c ? g2[f + r].v : ga; }
      gv += ga;
    }
    if (second) {
      const double *nf = fr + f;
#pragma unroll
      for (int i = 0; i < nx; i++) os[i] = {nf[i], 0.0};
#pragma unroll
      for (int i = 0; i < nu; i++) ou[i] = {nf[nx + i], 0.0};
      stage_link_cost_grad<M, Dual>(s, uu, os, ou, dv, g2);
      double gb = 0.0;
#pragma unroll
      for (int r = 0; r < f; r++) gb = r == c ? g2[r].v : gb;
      gv += gb;
    }
#pragma unroll
    for (int r = 0; r < f; r++) {
      const bool hasb = (bbase >> r) & 1u, hasa = (bown1 >> r) & 1u, has2 = (bown0 >> r) & 1u;
      if (hasb || hasa || has2) {
        double v = hasb ? hb[r] : 0.0;
        if (hasa) v += ha[r];
        if (has2) v += g2[r].d;
        Pc[e++] = v;
      }
    }
    if (second) {
#pragma unroll
      for (int r = 0; r < f; r++) if ((bnext >> r) & 1u) Pc[e++] = g2[f + r].d;
    }
    qb[j] = gv;
  } else if constexpr (M::has_cost) {
    // column frame_k[c] of the Hessian of l_k: the dual parts of the generated gradient, rows p first, then the frame's
    constexpr int nl = f + nx;
    const unsigned char *mk = sd.hmask + c;
    Dual rr[nx], g[nl];
#pragma unroll
    for (int i = 0; i < nx; i++) rr[i] = {pb[i], 0.0};
    stage_cost_column<M>(k == N - 1, s, uu, rr, dv, g);
    int e = 0;
    double gv = 0.0;
#pragma unroll
    for (int i = 0; i < nx; i++) if (mk[(f + i) * nl]) Pc[e++] = g[f + i].d;
#pragma unroll
    for (int r = 0; r < f; r++) { if (mk[r * nl]) Pc[e++] = g[r].d; gv = r == c ? g[r].v : gv; }
    qb[j] = gv;
  } else if (c < nx) {
    const double Qc = sd.Qk ? sd.Qk[k * nx + c] : sd.Q[c];
    Pc[0] = -2.0 * Qc; Pc[1] = 2.0 * Qc;
    qb[j] = 2.0 * (xv - pb[c]) * Qc;
  } else {
    const double Rc = sd.Rk ? sd.Rk[k * nu + c - nx] : sd.R[c - nx];
    Pc[0] = 2.0 * Rc;
    qb[j] = 2.0 * xv * Rc;
  }
  lb[j] = lbx[(long)b * sd.nvar + jj] - xv; ub[j] = ubx[(long)b * sd.nvar + jj] - xv;
  int a = 0;
  Ac[a++] = 1.0;
  if (k >= 1 && c < nx) Ac[a++] = 1.0;
  if (k < N - 1) {
    Dual out[nx];
    if constexpr (COOP) M::Fc(par, sd.dt, s, uu, out, c); else stage_dyn<M, Dual>(par, sd.dt, s, uu, dv, out);
#pragma unroll
    for (int r = 0; r < nx; r++) Ac[a + r] = -out[r].d;
    a += nx;
    if (c < nx) {
      double Fc = 0.0;
#pragma unroll
      for (int r = 0; r < nx; r++) Fc = r == c ? out[r].v : Fc;
      const double g = fr[f + c] - Fc;
      const int row = n + k * nx + c; const long gi = (long)b * sd.ng + k * nx + c;
      lb[row] = lbg[gi] - g; ub[row] = ubg[gi] - g;
    }
  }
  if constexpr (M::nh > 0) {
    // path constraint rows of this frame: column c of +dh/d[s; u]; lane c < nh also owns the shifted bounds of row h_k[c]
    constexpr int nh = M::nh;
    Dual hv[nh];
    stage_path<M, Dual>(s, uu, dv, hv);
#pragma unroll
    for (int r = 0; r < nh; r++) Ac[a + r] = hv[r].d;
    a += nh;
    for (int r0 = c; r0 < nh; r0 += f) {      // nh may exceed the frame size: lane c takes rows c, c + f, ...
      double hc = 0.0;
#pragma unroll
      for (int r = 0; r < nh; r++) hc = r == r0 ? hv[r].v : hc;
      const int row = n + sd.ngd + k * nh + r0; const long gi = (long)b * sd.ng + sd.ngd + k * nh + r0;
      lb[row] = lbg[gi] - hc; ub[row] = ubg[gi] - hc;
    }
  }
  if constexpr (M::nk > 0) {
    // link constraint r_k = K(frame_k, frame_{k+1}) (rate limits u_{k+1} - u_k and the like): this column takes part in r_{k-1} as
    // the second frame and in r_k as the first; lane c < nk of frame k < N - 1 also owns the shifted bounds of row r_k[c]
    constexpr int nk = M::nk;
    const int g0 = sd.ngd + N * sd.nh;
    Dual os[nx], ou[nu], kv[nk];
    if (k >= 1) {
      const double *pf = fr - f;
#pragma unroll
      for (int i = 0; i < nx; i++) os[i] = {pf[i], 0.0};
#pragma unroll
      for (int i = 0; i < nu; i++) ou[i] = {pf[nx + i], 0.0};
      stage_link<M, Dual>(os, ou, s, uu, dvp, kv);
#pragma unroll
      for (int r = 0; r < nk; r++) Ac[a + r] = kv[r].d;
      a += nk;
    }
    if (k < N - 1) {
      const double *nf = fr + f;
#pragma unroll
      for (int i = 0; i < nx; i++) os[i] = {nf[i], 0.0};
#pragma unroll
      for (int i = 0; i < nu; i++) ou[i] = {nf[nx + i], 0.0};
      stage_link<M, Dual>(s, uu, os, ou, dv, kv);
#pragma unroll
      for (int r = 0; r < nk; r++) Ac[a + r] = kv[r].d;
      for (int r0 = c; r0 < nk; r0 += f) {
        double kc = 0.0;
#pragma unroll
        for (int r = 0; r < nk; r++) kc = r == r0 ? kv[r].v : kc;
        const int row = n + g0 + k * nk + r0; const long gi = (long)b * sd.ng + g0 + k * nk + r0;
        lb[row] = lbg[gi] - kc; ub[row] = ubg[gi] - kc;
      }
    }
  }
}

// one wave per instance: lanes stride over the frames, butterfly reduction (fixed order => deterministic)
template <class M, bool PF = false, class... PP>
__global__ void __launch_bounds__(256) stage_merit_kernel(StageDev sd, int batch, const double *__restrict__ p, const double *__restrict__ x,
                                                          double *__restrict__ fout, double *__restrict__ gout, PP... pp) {
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu;
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  // PP: b is the same on every lane of the wave, which the compiler cannot see through threadIdx.x >> 6; said so, the row's address is
  // scalar, its entries arrive by scalar loads and F sees a uniform pointer, as it does with sd.par
  const double *par = sd.par;
  if constexpr (stage_has<StageTheta, PP...>) par = stage_theta(pp...).model + (long)__builtin_amdgcn_readfirstlane(b) * SM_NPAR;
  const double *pb0 = p + (long)b * (PF ? sd.N * nx : nx), *xb = x + (long)b * sd.nvar;
  double cost = 0.0, gmax = 0.0;
  for (int k = lane; k < sd.N; k += 64) {
    const double *fr = xb + k * f, *pb = PF ? pb0 + k * nx : pb0;      // (PF: frame k's reference r_k)
    double s[nx], uu[nu];
#pragma unroll
    for (int i = 0; i < nx; i++) s[i] = fr[i];
#pragma unroll
    for (int i = 0; i < nu; i++) uu[i] = fr[nx + i];
    double dv[sm_nsd_regs<M>];      // SD: lane k reads row k
    stage_load_data<M>(dv, b, sd.N, k, pp...);
    if constexpr (M::has_cost) {
      double rr[nx], lv[1];
#pragma unroll
      for (int i = 0; i < nx; i++) rr[i] = pb[i];
      stage_cost_value<M, double>(k == sd.N - 1, s, uu, rr, dv, lv);
      cost += lv[0];
    } else {
#pragma unroll
      for (int i = 0; i < nx; i++) { const double e = s[i] - pb[i]; cost += e * e * (sd.Qk ? sd.Qk[k * nx + i] : sd.Q[i]); }
#pragma unroll
      for (int i = 0; i < nu; i++) cost += uu[i] * uu[i] * (sd.Rk ? sd.Rk[k * nu + i] : sd.R[i]);
    }
    if constexpr (sm_has_link_cost<M>::value) {
      // the link cost of stage k = llink(frame_k, frame_{k+1}), behind the frame's own term
      if (k < sd.N - 1) {
        double ns[nx], nun[nu], lk[1];
#pragma unroll
        for (int i = 0; i < nx; i++) ns[i] = fr[f + i];
#pragma unroll
        for (int i = 0; i < nu; i++) nun[i] = fr[f + nx + i];
        stage_link_cost<M, double>(s, uu, ns, nun, dv, lk);
        cost += lk[0];
      }
    }
    if (k < sd.N - 1) {
      double out[nx];
      stage_dyn<M, double>(par, sd.dt, s, uu, dv, out);
#pragma unroll
      for (int i = 0; i < nx; i++) gmax = fmax(gmax, fabs(fr[f + i] - out[i]));
    }
    if constexpr (M::nh > 0) {
      double hv[M::nh];
      stage_path<M, double>(s, uu, dv, hv);
#pragma unroll
      for (int i = 0; i < M::nh; i++) {
        const double lo = sd.h_lok ? sd.h_lok[k * M::nh + i] : sd.h_lo[i], hi = sd.h_hik ? sd.h_hik[k * M::nh + i] : sd.h_hi[i];
        gmax = fmax(gmax, fmax(lo - hv[i], hv[i] - hi));
      }
    }
    if constexpr (M::nk > 0) {
      if (k < sd.N - 1) {
        double ns[nx], nun[nu], kv[M::nk];
#pragma unroll
        for (int i = 0; i < nx; i++) ns[i] = fr[f + i];
#pragma unroll
        for (int i = 0; i < nu; i++) nun[i] = fr[f + nx + i];
        stage_link<M, double>(s, uu, ns, nun, dv, kv);
#pragma unroll
        for (int i = 0; i < M::nk; i++) gmax = fmax(gmax, fmax(sd.k_lo[i] - kv[i], kv[i] - sd.k_hi[i]));
      }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) { cost += __shfl_xor(cost, o, 64); gmax = fmax(gmax, __shfl_xor(gmax, o, 64)); }
  if (lane == 0) { if (fout) fout[b] = cost; if (gout) gout[b] = gmax; }
}

// out[base + i] = in[base + i + width] over `count` blocks of `width` entries, the last block zero; all zero for an instance that is not ok
__device__ __forceinline__ void stage_shift_block(double *__restrict__ out, const double *__restrict__ in, int base, int width, int count, bool ok, int lane) {
  const int tot = width * count, keep = tot - width;
  for (int i = lane; i < tot; i += 64) {
    double v = 0.0;
    if (ok && i < keep) v = in[base + i + width];
    out[base + i] = v;
  }
}

// Receding-horizon hand-over between two ticks (mpcqp_stage_advance).  One wave per instance like the merit kernel, lanes striding over the
// elements of every array: pure data movement but for two runs of F<double> -- the plant step F(s_0, u_0) on lane 0 and the rollout tail
// F(s_{N-1}, u_{N-1}) on lane 1, one pass of the wave for both -- and the k = 0 cost term on lane 0 (the frame term only: a link cost,
// sm_has_link_cost, is not part of that log).  Their nx results go by wave shuffle to the
// lanes c < nx that store them, so every store stream is contiguous.  No LDS, no atomics, one writer per output element.
template <class M, bool PF = false, class... PP>
__global__ void __launch_bounds__(256) stage_advance_kernel(StageDev sd, int batch, mpcqp_stage_advance_args a, PP... pp) {
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu;
  static_assert(f <= 64, "a frame is stored by one pass of the wave");
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  const int N = sd.N, nvar = sd.nvar, np = sd.np, n = sd.n, last = (N - 1) * f;
  const double *xi = a.x_in + (long)b * nvar;
  double *xo = a.x_out + (long)b * nvar;
  bool ok = true;
  if (a.status) ok = stage_status_ok(a.status[b]);
  const bool rollout = a.tail == MPCQP_TAIL_ROLLOUT;
  double Fo[nx];
#pragma unroll
  for (int i = 0; i < nx; i++) Fo[i] = 0.0;
  if (lane < 2) {
    const double *fr = xi + (lane == 0 ? 0 : last);
    double s[nx], uu[nu];
#pragma unroll
    for (int i = 0; i < nx; i++) s[i] = fr[i];
#pragma unroll
    for (int i = 0; i < nu; i++) uu[i] = fr[nx + i];
    // transition data: the plant step takes row 0, the rollout tail row N - 1 -- the rows stored before the shift (mpcqp_stage_shift_data comes after)
    [[maybe_unused]] double dt_[sm_nsd_regs<M>];
    if constexpr (sm_tdata<M>::value) stage_load_data<M>(dt_, b, N, lane == 0 ? 0 : N - 1, pp...);
    if constexpr (stage_has<StageTheta, PP...>) {
      // PP: the plant step (lane 0) takes the plant row, or the model row when no plant set is stored; the rollout tail (lane 1) the model
      // row; a set that is not stored stands for sd.par.  Values, not addresses, are selected: sd.par stays in its scalar registers
      constexpr int NT = sm_ntheta<M>::value > 0 ? sm_ntheta<M>::value : 1;
      const StageTheta t = stage_theta(pp...);
      const double *row = lane == 0 && t.plant ? t.plant : t.model;
      double th[NT];
#pragma unroll
      for (int i = 0; i < NT; i++) th[i] = row ? row[(long)b * SM_NPAR + i] : sd.par[i];
      if (lane == 0 ? a.s_meas == nullptr : rollout) stage_dyn<M, double>(th, sd.dt, s, uu, dt_, Fo);
    } else {
      if (lane == 0 ? a.s_meas == nullptr : rollout) stage_dyn<M, double>(sd.par, sd.dt, s, uu, dt_, Fo);
    }
    if (lane == 0 && a.stage_cost) {
      // the k = 0 term of stage_merit_kernel's objective, in its order of operations
      const double *pb = PF ? a.p_in + (long)b * np : a.p + (long)b * nx;
      double cost = 0.0;
      if constexpr (M::has_cost) {
        double rr[nx], lv[1];
#pragma unroll
        for (int i = 0; i < nx; i++) rr[i] = pb[i];
        double dv[sm_nsd_regs<M>];      // SD: the k = 0 term takes d_0, the row before any shift
        stage_load_data<M>(dv, b, N, 0, pp...);
        stage_cost_value<M, double>(false, s, uu, rr, dv, lv);
        cost += lv[0];
      } else {
#pragma unroll
        for (int i = 0; i < nx; i++) { const double e = s[i] - pb[i]; cost += e * e * (sd.Qk ? sd.Qk[i] : sd.Q[i]); }
#pragma unroll
        for (int i = 0; i < nu; i++) cost += uu[i] * uu[i] * (sd.Rk ? sd.Rk[i] : sd.R[i]);
      }
      a.stage_cost[b] = cost;
    }
  }
  double v0 = 0.0, vt = 0.0;      // lane c < nx: element c of F(X_0) and of F(X_{N-1})
#pragma unroll
  for (int i = 0; i < nx; i++) {
    const double t0 = __shfl(Fo[i], 0, 64), t1 = __shfl(Fo[i], 1, 64);
    if (lane == i) { v0 = t0; vt = t1; }
  }
  if (lane < f) {
    const int c = lane;
    double v;
    if (c < nx) {
      if (a.s_meas) v = a.s_meas[(long)b * nx + c];
      else { v = v0; if (a.w) v += a.w[(long)b * nx + c]; }
    } else {
      v = ok ? xi[f + c] : xi[c];
    }
    xo[c] = v; a.lbx[(long)b * nvar + c] = v; a.ubx[(long)b * nvar + c] = v;
    if (a.applied) a.applied[(long)b * f + c] = xi[c];
    double t = xi[last + c];
    if (rollout && c < nx) t = vt;
    xo[last + c] = t;
  }
  for (int i = f + lane; i < last; i += 64) xo[i] = xi[i + f];
  if constexpr (PF) {
    const double *pi = a.p_in + (long)b * np;
    double *po = a.p_out + (long)b * np;
    for (int i = lane; i < np; i += 64) po[i] = i < np - nx ? pi[i + nx] : a.r_new ? a.r_new[(long)b * nx + i - (np - nx)] : pi[i];
  }
  if (a.dw_out) {
    const double *di = a.dw_in + (long)b * n;
    double *dout = a.dw_out + (long)b * n;
    if constexpr (PF) stage_shift_block(dout, di, 0, nx, N, ok, lane);
    else if (lane < nx) dout[lane] = ok ? di[lane] : 0.0;
    stage_shift_block(dout, di, np, f, N, ok, lane);
  }
  if (a.y_out) {
    const double *yi = a.y_in + (long)b * sd.m;
    double *yo = a.y_out + (long)b * sd.m;
    if constexpr (PF) stage_shift_block(yo, yi, 0, nx, N, ok, lane);
    else if (lane < nx) yo[lane] = ok ? yi[lane] : 0.0;
    stage_shift_block(yo, yi, np, f, N, ok, lane);
    stage_shift_block(yo, yi, n, nx, N - 1, ok, lane);
    stage_shift_block(yo, yi, n + sd.ngd, sd.nh, N, ok, lane);
    stage_shift_block(yo, yi, n + sd.ngd + N * sd.nh, sd.nk, N - 1, ok, lane);
  }
}

// A dynamically feasible trajectory (mpcqp_stage_rollout): X_0 and the inputs projected onto the box, the states by the chain s_{k+1} = F(s_k, u_k).
// The chain of N - 1 dependent runs of F<double> is serial, so the parallelism is across instances: one thread per instance, 64-thread workgroups
// (a batch of 8192 is 128 workgroups).  A thread reads frame k's input before it writes frame k and touches its own instance only, so the launch
// may run in place; the state lives in registers between the frames.  No PF twin: F reads no reference.  No LDS, no atomics, one writer per element.
__device__ __forceinline__ double stage_clip(double v, const double *lo, const double *hi, long i) {
  if (lo) { const double l = lo[i], h = hi[i]; v = v < l ? l : v; v = v > h ? h : v; }
  return v;
}
__device__ __forceinline__ double stage_box_viol(double acc, double v, const double *lo, const double *hi, long i) {
  return lo ? fmax(acc, fmax(lo[i] - v, v - hi[i])) : acc;
}
template <class M, class... PP>
__global__ void __launch_bounds__(64) stage_rollout_kernel(StageDev sd, int batch, mpcqp_stage_rollout_args a, PP... pp) {
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  if (a.frozen && a.frozen[b] != 0) return;
  const int N = sd.N;
  const long base = (long)b * sd.nvar;
  const double *xi = a.x_in + base;
  double *xo = a.x_out + base;
  const double *lo = a.lbx ? a.lbx + base : nullptr, *hi = a.lbx ? a.ubx + base : nullptr;
  const bool hold = a.inputs == MPCQP_ROLLOUT_INPUTS_HOLD;
  constexpr int NT = sm_ntheta<M>::value > 0 ? sm_ntheta<M>::value : 1;
  double th[NT];
  {
    const double *row = stage_theta(pp...).model;      // (null without a PP element: the shared values, which stay in scalar registers)
#pragma unroll
    for (int i = 0; i < NT; i++) th[i] = row ? row[(long)b * SM_NPAR + i] : sd.par[i];
  }
  double s[nx], uu[nu], u0[nu], sn[nx];
  double viol = 0.0;
  bool fin = true;
#pragma unroll
  for (int i = 0; i < nx; i++) { s[i] = stage_clip(xi[i], lo, hi, i); fin = fin && isfinite(s[i]); }
#pragma unroll
  for (int i = 0; i < nu; i++) { uu[i] = u0[i] = stage_clip(xi[nx + i], lo, hi, nx + i); }
#pragma unroll
  for (int i = 0; i < nx; i++) { xo[i] = s[i]; viol = stage_box_viol(viol, s[i], lo, hi, i); }
#pragma unroll
  for (int i = 0; i < nu; i++) { xo[nx + i] = uu[i]; viol = stage_box_viol(viol, uu[i], lo, hi, nx + i); }
  int div = -1;
  for (int k = 0; k < N - 1; k++) {
    if (div < 0) {
      bool ok = fin;
#pragma unroll
      for (int i = 0; i < nu; i++) ok = ok && isfinite(uu[i]);
      // transition data: step k takes row k of the instance -- nsd loads per step, N nsd doubles apart between lanes
      [[maybe_unused]] double dv[sm_nsd_regs<M>];
      if constexpr (sm_tdata<M>::value) stage_load_data<M>(dv, b, N, k, pp...);
      stage_dyn<M, double>(th, sd.dt, s, uu, dv, sn);
#pragma unroll
      for (int i = 0; i < nx; i++) ok = ok && isfinite(sn[i]);
      if (ok) {
#pragma unroll
        for (int i = 0; i < nx; i++) s[i] = sn[i];
      } else {
        div = k;
      }
    }
    const long o = (long)(k + 1) * f;
#pragma unroll
    for (int i = 0; i < nu; i++) uu[i] = stage_clip(hold ? u0[i] : xi[o + nx + i], lo, hi, o + nx + i);
#pragma unroll
    for (int i = 0; i < nx; i++) { xo[o + i] = s[i]; viol = stage_box_viol(viol, s[i], lo, hi, o + i); }
#pragma unroll
    for (int i = 0; i < nu; i++) { xo[o + nx + i] = uu[i]; viol = stage_box_viol(viol, uu[i], lo, hi, o + nx + i); }
  }
  if (a.diverged) a.diverged[b] = div;
  if (a.box_viol) a.box_viol[b] = viol;
}

// per-candidate accumulators of the line search: the candidate is known at run time only, the registers are addressed statically (an unrolled
// select written as a compile-time recursion: a loop over j, even one that is unrolled later, is turned back into a dynamically indexed array
// by the optimiser, and that array goes to scratch)
template <int NC, int J = 0> __device__ __forceinline__ void stage_ls_add(double (&acc)[NC], int c, double v) {
  if constexpr (J < NC) { acc[J] = J == c ? acc[J] + v : acc[J]; stage_ls_add<NC, J + 1>(acc, c, v); }
}
template <int NC, int J = 0> __device__ __forceinline__ void stage_ls_max(double (&acc)[NC], int c, double v) {
  if constexpr (J < NC) { acc[J] = J == c ? fmax(acc[J], v) : acc[J]; stage_ls_max<NC, J + 1>(acc, c, v); }
}
template <int NC, int J = NC - 1> __device__ __forceinline__ double stage_ls_get(const double (&acc)[NC], int c) {
  if constexpr (J == 0) return acc[0];
  else return J == c ? acc[J] : stage_ls_get<NC, J - 1>(acc, c);
}

// Per-instance l1-merit backtracking line search (mpcqp_stage_linesearch; models.StageOCP.line_search is its host statement).  One wave per
// instance like the merit kernel.  Work items are (candidate, frame) pairs over (K + 1) N, strided over the 64 lanes; candidate 0 is the base point
// x, candidate j >= 1 the point x + alpha0 beta^(j-1) dx.  An item adds frame k's cost, l1 violation and max-norm violation at its candidate to the
// lane's per-candidate partial sums; the box terms, q' dx and max |y| stride over their arrays; one butterfly in fixed order reduces everything
// (two runs give the same bits) and leaves the totals on every lane, so the decision is taken redundantly by all of them.  x is written after that,
// by stage_step_kernel's expression: every read of x precedes it in program order of the same wave.  No LDS, no atomics, one writer per output.
template <class M, bool PF = false, class... PP>
__global__ void __launch_bounds__(256) stage_linesearch_kernel(StageDev sd, int batch, mpcqp_stage_linesearch_args a, PP... pp) {
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu, NC = MPCQP_LINESEARCH_MAX_CANDIDATES + 1;
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  const double *par = sd.par;      // PP: the instance's row through a wave-uniform b, as in stage_merit_kernel
  if constexpr (stage_has<StageTheta, PP...>) par = stage_theta(pp...).model + (long)__builtin_amdgcn_readfirstlane(b) * SM_NPAR;
  const int N = sd.N, nvar = sd.nvar, np = sd.np;
  bool ok = true;
  if (a.status) ok = stage_status_ok(a.status[b]);
  const int K = ok ? a.candidates : 0;          // an instance whose QP returned no point evaluates the base point only: its dw, y are not read
  double *xb = a.x + (long)b * nvar;
  const double *pb0 = a.p + (long)b * np, *dxb = a.dw + (long)b * sd.n + np;
  double al[NC];                                // al[0] = 0: the base point
  al[0] = 0.0; al[1] = a.alpha0;
#pragma unroll
  for (int j = 2; j < NC; j++) al[j] = al[j - 1] * a.beta;
  double cost[NC], vio[NC], gmx[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) { cost[j] = 0.0; vio[j] = 0.0; gmx[j] = 0.0; }
  for (int t = lane; t < (K + 1) * N; t += 64) {
    const int c = t / N, k = t - c * N;
    const double ac = stage_ls_get(al, c);
    const double *fr = xb + k * f, *dfr = dxb + k * f, *pb = PF ? pb0 + k * nx : pb0;
    double s[nx], uu[nu];
#pragma unroll
    for (int i = 0; i < nx; i++) { s[i] = fr[i]; if (c > 0) s[i] += ac * dfr[i]; }
#pragma unroll
    for (int i = 0; i < nu; i++) { uu[i] = fr[nx + i]; if (c > 0) uu[i] += ac * dfr[nx + i]; }
    double lc = 0.0, lv = 0.0, lg = 0.0;
    double dv[sm_nsd_regs<M>];      // SD: frame k's row (an item is one frame at one candidate)
    stage_load_data<M>(dv, b, N, k, pp...);
    // the objective and the max-norm violation exactly as stage_merit_kernel forms them, the l1 violation next to the latter
    if constexpr (M::has_cost) {
      double rr[nx], lval[1];
#pragma unroll
      for (int i = 0; i < nx; i++) rr[i] = pb[i];
      stage_cost_value<M, double>(k == N - 1, s, uu, rr, dv, lval);
      lc += lval[0];
    } else {
#pragma unroll
      for (int i = 0; i < nx; i++) { const double e = s[i] - pb[i]; lc += e * e * (sd.Qk ? sd.Qk[k * nx + i] : sd.Q[i]); }
#pragma unroll
      for (int i = 0; i < nu; i++) lc += uu[i] * uu[i] * (sd.Rk ? sd.Rk[k * nu + i] : sd.R[i]);
    }
    if constexpr (sm_has_link_cost<M>::value) {
      // the link cost of stage k at this candidate, as stage_merit_kernel adds it
      if (k < N - 1) {
        double ns[nx], nun[nu], lk[1];
#pragma unroll
        for (int i = 0; i < nx; i++) { ns[i] = fr[f + i]; if (c > 0) ns[i] += ac * dfr[f + i]; }
#pragma unroll
        for (int i = 0; i < nu; i++) { nun[i] = fr[f + nx + i]; if (c > 0) nun[i] += ac * dfr[f + nx + i]; }
        stage_link_cost<M, double>(s, uu, ns, nun, dv, lk);
        lc += lk[0];
      }
    }
    if (k < N - 1) {
      double out[nx];
      stage_dyn<M, double>(par, sd.dt, s, uu, dv, out);
#pragma unroll
      for (int i = 0; i < nx; i++) {
        double sn = fr[f + i];
        if (c > 0) sn += ac * dfr[f + i];
        const double d = fabs(sn - out[i]);
        lv += d; lg = fmax(lg, d);
      }
    }
    if constexpr (M::nh > 0) {
      double hv[M::nh];
      stage_path<M, double>(s, uu, dv, hv);
#pragma unroll
      for (int i = 0; i < M::nh; i++) {
        const double lo = sd.h_lok ? sd.h_lok[k * M::nh + i] : sd.h_lo[i], hi = sd.h_hik ? sd.h_hik[k * M::nh + i] : sd.h_hi[i];
        lv += fmax(lo - hv[i], 0.0) + fmax(hv[i] - hi, 0.0);
        lg = fmax(lg, fmax(lo - hv[i], hv[i] - hi));
      }
    }
    if constexpr (M::nk > 0) {
      if (k < N - 1) {
        double ns[nx], nun[nu], kv[M::nk];
#pragma unroll
        for (int i = 0; i < nx; i++) { ns[i] = fr[f + i]; if (c > 0) ns[i] += ac * dfr[f + i]; }
#pragma unroll
        for (int i = 0; i < nu; i++) { nun[i] = fr[f + nx + i]; if (c > 0) nun[i] += ac * dfr[f + nx + i]; }
        stage_link<M, double>(s, uu, ns, nun, dv, kv);
#pragma unroll
        for (int i = 0; i < M::nk; i++) {
          lv += fmax(sd.k_lo[i] - kv[i], 0.0) + fmax(kv[i] - sd.k_hi[i], 0.0);
          lg = fmax(lg, fmax(sd.k_lo[i] - kv[i], kv[i] - sd.k_hi[i]));
        }
      }
    }
    stage_ls_add(cost, c, lc); stage_ls_add(vio, c, lv); stage_ls_max(gmx, c, lg);
  }
  // box terms of every candidate, q' dx, max |y| over the box and general rows
  double qd = 0.0, ymax = 0.0;
  {
    const double *lb = a.lbx + (long)b * nvar, *ub = a.ubx + (long)b * nvar, *qb = a.q + (long)b * sd.n + np;
    for (int i = lane; i < nvar; i += 64) {
      const double xv = xb[i], lo = lb[i], hi = ub[i];
      vio[0] += fmax(lo - xv, 0.0) + fmax(xv - hi, 0.0);
      if (ok) {
        const double dv = dxb[i];
        qd += qb[i] * dv;
#pragma unroll
        for (int j = 1; j < NC; j++)
          if (j <= K) { const double xc = xv + al[j] * dv; vio[j] += fmax(lo - xc, 0.0) + fmax(xc - hi, 0.0); }
      }
    }
    if (ok) {
      const double *yb = a.y + (long)b * sd.m;
      for (int i = np + lane; i < sd.m; i += 64) ymax = fmax(ymax, fabs(yb[i]));
    }
  }
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int j = 0; j < NC; j++) {
      cost[j] += __shfl_xor(cost[j], o, 64); vio[j] += __shfl_xor(vio[j], o, 64); gmx[j] = fmax(gmx[j], __shfl_xor(gmx[j], o, 64));
    }
    qd += __shfl_xor(qd, o, 64); ymax = fmax(ymax, __shfl_xor(ymax, o, 64));
  }
  // the decision, the same on every lane
  double mu = a.mu_min;
  if (a.mu) mu = fmax(mu, a.mu[b]);
  if (ok) mu = fmax(mu, a.mu_factor * ymax);
  double phi[NC];
#pragma unroll
  for (int j = 0; j < NC; j++) phi[j] = cost[j] + mu * vio[j];
  double D = qd - mu * vio[0];
  D = D < 0.0 ? D : 0.0;
  int sel = 0, acc = -2;                        // sel: the candidate taken (0 = stay), acc: what `accepted` reports
  if (ok) {
    bool found = false;
#pragma unroll
    for (int j = 1; j < NC; j++)
      if (j <= K && !found && isfinite(phi[j]) && phi[j] <= phi[0] + a.c1 * al[j] * D) { found = true; sel = j; acc = j - 1; }
    if (!found && isfinite(stage_ls_get(phi, K))) { sel = K; acc = -1; }
  }
  const double alpha = stage_ls_get(al, sel);
  double mx = 0.0;
  if (sel > 0) {
    for (int i = lane; i < nvar; i += 64) {
      const double d = alpha * dxb[i];
      xb[i] += d; mx = fmax(mx, fabs(d));
    }
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) {
    if (a.mu && ok) a.mu[b] = mu;
    if (a.alpha_out) a.alpha_out[b] = alpha;
    if (a.accepted) a.accepted[b] = acc;
    if (a.step_max) a.step_max[b] = mx;
    if (a.f_out) a.f_out[b] = stage_ls_get(cost, sel);
    if (a.gmax_out) a.gmax_out[b] = stage_ls_get(gmx, sel);
    if (a.phi) { a.phi[2 * (long)b] = phi[0]; a.phi[2 * (long)b + 1] = stage_ls_get(phi, sel); }
  }
}

// Convexification of the frame term of a general stage cost (mpcqp_stage_convexify; models.StageOCP.convexify_system is its host statement; the
// eigen-solve is stage_convexify.hpp).  One group of W lanes per (instance, frame), W the smallest of 16 / 32 / 64 that holds nl = 2 nx + nu; a block
// holds as many groups as 48 KB of static LDS and 256 threads allow, always whole waves.  Per group: the tile A (the frame's Hessian, then its
// eigenvalues on the diagonal) and the eigenvectors V, nl x nl doubles each, in LDS -- they are indexed at run time, as registers they would be scratch.
template <class M> struct stage_cvx {
  static constexpr int nl = 2 * M::nx + M::nu;
  static constexpr int W = nl <= 16 ? 16 : nl <= 32 ? 32 : 64;
  static constexpr int tile = 2 * nl * nl;                          // doubles per group
  static constexpr int fit = (48 * 1024) / (tile * 8), per_wave = 64 / W;
  static constexpr int waves = fit / per_wave >= 4 ? 4 : fit / per_wave >= 1 ? fit / per_wave : 1;
  static constexpr int G = waves * per_wave;                        // groups per block
  static_assert(G * tile * 8 <= 64 * 1024, "the tiles of a block fit its static LDS");
};
// what the handle lends a convexify launch (device memory): slots [N * nl * nl], the slot of P that takes element (r, c) of frame k's correction, -1 =
// none (outside the pattern, or the r-r block of a shared reference); ppslot [nx * nx], the slot of the shared p-p entry (r, c), -1 = none (all of
// them for per-frame references, whose r-r entries are frame slots); rr [batch * N * nx * nx], the r-r parts of the touched frames' corrections
// on their way to the second pass; flags [batch * N], 1 = the frame was touched
struct StageCvxBuf { const int *slots, *ppslot; double *rr; int *flags; };

// The exact Lagrangian Hessian (mpcqp_stage_lagrangian; models.StageOCP.constraint_curvature and lagrangian_system are its host statement; DESIGN
// 6.18).  Generated functors with M::has_exact carry FG and HG, the gradients over [s; u] of lam' F and mu' H with the multipliers as plain doubles.
// StageExact is the pack element that switches the curvature on in stage_convexify_kernel (off by default: an instance without it keeps its
// signature and its code): y [batch * m] the multiplier estimate, rows [p; x; dynamics; path; link]; status [batch] or null.
struct StageExact { const double *y; const int *status; };
template <class M, class = void> struct sm_has_exact : std::false_type {};
template <class M> struct sm_has_exact<M, std::void_t<decltype(M::has_exact)>> : std::bool_constant<M::has_exact != 0> {};
// column c of C_k = -sum_i lam_i d2F_i + sum_i mu_i d2h_i over [s_k; u_k]: the dual parts of FG (k < N-1) and HG on the frame seeded on c, formed as
// -FG.d + HG.d in that order.  yb: the instance's row of y; par: the parameters F takes; dv: the frame's stage data
template <class M> __device__ __forceinline__ void stage_curvature_column(const StageDev &sd, int k, const Dual *s, const Dual *uu, const double *yb,
                                                                          const double *par, const double *dv, double (&cv)[M::nx + M::nu]) {
  constexpr int nx = M::nx, f = M::nx + M::nu;
#pragma unroll
  for (int r = 0; r < f; r++) cv[r] = 0.0;
  if (k < sd.N - 1) {
    const double *yd = yb + sd.n + k * nx;
    double lam[nx];
#pragma unroll
    for (int i = 0; i < nx; i++) lam[i] = yd[i];
    Dual g[f];
    if constexpr (sm_tdata<M>::value) M::template FG<Dual>(par, sd.dt, s, uu, lam, dv, g); else M::template FG<Dual>(par, sd.dt, s, uu, lam, g);
#pragma unroll
    for (int r = 0; r < f; r++) cv[r] = -g[r].d;
  }
  if constexpr (M::nh > 0) {
    constexpr int nh = M::nh;
    const double *yh = yb + sd.n + sd.ngd + k * nh;
    double mu[nh];
#pragma unroll
    for (int i = 0; i < nh; i++) mu[i] = yh[i];
    Dual g[f];
    if constexpr (sm_nsd<M>::value > 0) M::template HG<Dual>(s, uu, mu, dv, g); else M::template HG<Dual>(s, uu, mu, g);
#pragma unroll
    for (int r = 0; r < f; r++) cv[r] += g[r].d;
  }
}

// One thread per (instance, frame, column c of [s; u]): the column of C_k is added to its slots of P through the table the handle built from the
// pattern (slots [N * f * f], entry (k, r, c), -1 = outside the curvature's structure).  Each entry has one writer -- read, add, write; no atomics --
// so the result is bitwise repeatable and does not depend on the batch or the instance's position.  Adjacent lanes own adjacent columns: the store
// streams are those of stage_eval_kernel.  An instance whose status is given and is not one with a point is neither read nor written.
template <class M, class... PP>
__global__ void __launch_bounds__(256) stage_lagrangian_kernel(StageDev sd, int batch, const double *__restrict__ x, StageExact ex,
                                                               const int *__restrict__ slots, double *__restrict__ P, PP... pp) {
  constexpr int NT = sm_ntheta<M>::value > 0 ? sm_ntheta<M>::value : 1;
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = sd.N, per = N * f;
  if (gid >= (long)batch * per) return;
  const int b = (int)(gid / per), jj = (int)(gid - (long)b * per), k = jj / f, c = jj - k * f;
  if (ex.status && !stage_status_ok(ex.status[b])) return;
  double th[NT];
  const double *par = sd.par;
  if constexpr (stage_has<StageTheta, PP...>) {
    const double *row = stage_theta(pp...).model + (long)b * SM_NPAR;
#pragma unroll
    for (int i = 0; i < NT; i++) th[i] = row[i];
    par = th;
  }
  const double *fr = x + (long)b * sd.nvar + k * f;
  double dv[sm_nsd_regs<M>];
  stage_load_data<M>(dv, b, N, k, pp...);
  Dual s[nx], uu[nu];
#pragma unroll
  for (int i = 0; i < nx; i++) s[i] = {fr[i], i == c ? 1.0 : 0.0};
#pragma unroll
  for (int i = 0; i < nu; i++) uu[i] = {fr[nx + i], nx + i == c ? 1.0 : 0.0};
  double cv[f];
  stage_curvature_column<M>(sd, k, s, uu, ex.y + (long)b * sd.m, par, dv, cv);
  const int *sl = slots + (long)k * f * f + c;
  double *Pb = P + (long)b * sd.nnzP;
#pragma unroll
  for (int r = 0; r < f; r++) {
    const int slot = sl[r * f];
    if (slot >= 0) Pb[slot] += cv[r];
  }
}

// PP may hold a StageExact (mpcqp_stage_lagrangian with a mode): the tile is then H_k^L = H_k + C_k, C_k zero-padded over r -- the lanes < f add
// stage_curvature_column's values, the expression stage_lagrangian_kernel added to P before this launch -- F takes the StageTheta of the pack, and an
// instance whose status has no point is skipped (no read, no write but its flags = 0)
template <class M, bool PF = false, class... PP>
__global__ void __launch_bounds__(stage_cvx<M>::G * stage_cvx<M>::W) stage_convexify_kernel(StageDev sd, int batch, mpcqp_stage_convexify_args a,
                                                                                            StageCvxBuf w, PP... pp) {
  using C = stage_cvx<M>;
  constexpr bool EX = stage_has<StageExact, PP...>;
  constexpr int nx = M::nx, nu = M::nu, f = nx + nu, nl = C::nl, W = C::W, G = C::G;
  __shared__ double lds[G][2][nl * nl];
  const int grp = threadIdx.x / W, lane = threadIdx.x - grp * W;
  const int N = sd.N;
  const long item = (long)blockIdx.x * G + grp;                     // (instance, frame); a group past the end walks the barriers without work
  bool live = item < (long)batch * N;
  const int b = live ? (int)(item / N) : 0, k = live ? (int)(item - (long)b * N) : 0;
  [[maybe_unused]] const bool inside = live;
  if constexpr (EX) {
    const StageExact ex = stage_get<StageExact>(pp...);
    if (live && ex.status && !stage_status_ok(ex.status[b])) live = false;
  }
  double *A = lds[grp][0], *V = lds[grp][1];
  if (live && lane < nl) {
    // column `lane` of H_k: one pass of the generated gradient on dual numbers seeded on input `lane` of [s; u; r_k] -- the call, and so the
    // bits, of stage_eval_kernel's columns
    const double *fr = a.x + (long)b * sd.nvar + k * f, *rk = a.p + (long)b * sd.np + (PF ? k * nx : 0);
    Dual s[nx], uu[nu], rr[nx], g[nl];
    double dv[sm_nsd_regs<M>];
    stage_load_data<M>(dv, b, N, k, pp...);
#pragma unroll
    for (int i = 0; i < nx; i++) { s[i] = {fr[i], i == lane ? 1.0 : 0.0}; rr[i] = {rk[i], f + i == lane ? 1.0 : 0.0}; }
#pragma unroll
    for (int i = 0; i < nu; i++) uu[i] = {fr[nx + i], nx + i == lane ? 1.0 : 0.0};
    stage_cost_grad<M, Dual>(k == N - 1, s, uu, rr, dv, g);
    if constexpr (EX) {
      constexpr int NT = sm_ntheta<M>::value > 0 ? sm_ntheta<M>::value : 1;
      double cv[f], th[NT];
      const double *par = sd.par;
      if constexpr (stage_has<StageTheta, PP...>) {
        const double *row = stage_theta(pp...).model + (long)b * SM_NPAR;
#pragma unroll
        for (int i = 0; i < NT; i++) th[i] = row[i];
        par = th;
      }
#pragma unroll
      for (int r = 0; r < f; r++) cv[r] = 0.0;
      if (lane < f) stage_curvature_column<M>(sd, k, s, uu, stage_get<StageExact>(pp...).y + (long)b * sd.m, par, dv, cv);
#pragma unroll
      for (int r = 0; r < nl; r++) A[r * nl + lane] = r < f ? g[r].d + cv[r] : g[r].d;
    } else {
#pragma unroll
      for (int r = 0; r < nl; r++) A[r * nl + lane] = g[r].d;
    }
  }
  sm_jacobi<W>(A, V, nl, lane, live);
  const double lmin = sm_convexify_lam_min<W>(A, nl, lane);
  const bool touched = live && lmin < a.eps;
  if (touched) {
    // the correction, entry by entry: one lane per entry, one entry per slot -- read, add, write
    double *Pb = a.P + (long)b * sd.nnzP;
    const int *sl = w.slots + (long)k * nl * nl;
    for (int e = lane; e < nl * nl; e += W) {
      const int r = e / nl, c = e - r * nl, slot = sl[e];
      const bool shared_rr = !PF && r >= f && c >= f;
      if (slot >= 0 || shared_rr) {
        const double d = sm_convexify_delta(A, V, nl, r, c, a.mode, a.eps);
        if (slot >= 0) Pb[slot] += d;
        else w.rr[item * (nx * nx) + (r - f) * nx + (c - f)] = d;
      }
    }
  }
  if (live && lane == 0) {
    w.flags[item] = touched ? 1 : 0;
    if (a.lam_min) a.lam_min[item] = lmin;
  }
  if constexpr (EX) {
    if (inside && !live && lane == 0) w.flags[item] = 0;      // a skipped instance: the second pass finds no touched frame
  }
}

// the second pass: thread (b, e) adds to the shared p-p entry e of instance b the sum of the touched frames' corrections, k ascending, from 0.0 --
// the order of the statement -- and writes nothing where no frame was touched; thread (b, 0) counts the touched frames.  (A template only so that
// the kernel exists in the libraries that launch it.)
template <class M>
__global__ void __launch_bounds__(256) stage_convexify_sum_kernel(int batch, int N, int nnzP, StageCvxBuf w, double *__restrict__ P, int *__restrict__ touched) {
  constexpr int nx2 = M::nx * M::nx;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)batch * nx2) return;
  const int b = (int)(gid / nx2), e = (int)(gid - (long)b * nx2);
  const int *fl = w.flags + (long)b * N;
  if (e == 0 && touched) {
    int cnt = 0;
    for (int k = 0; k < N; k++) cnt += fl[k];
    touched[b] = cnt;
  }
  const int slot = w.ppslot[e];
  if (slot < 0) return;
  double acc = 0.0;
  bool any = false;
  for (int k = 0; k < N; k++)
    if (fl[k]) { acc += w.rr[((long)b * N + k) * nx2 + e]; any = true; }
  if (any) P[(long)b * nnzP + slot] += acc;
}

// The rows a launch reads beside its arguments (device pointers; null = the shared values sd.par, the defaults M::sdata0): the per-instance
// parameters of the controller's model and of the plant (only advance passes a plant row) and the stage data.  The one form in which the rows cross
// from libmpcqp.so into a generated library: every launcher of the boundary is (const StageDev *, batch, its argument block, ..., const StageRows *, stream).
struct StageRows { const double *theta, *plant, *sdata; };
// the argument blocks of the two operations whose public entry points take loose pointers (mpcqp_stage_eval, mpcqp_stage_merit)
struct StageEvalArgs { const double *p, *x, *lbx, *ubx, *lbg, *ubg; double *P, *q, *A, *l, *u; };
struct StageMeritArgs { const double *p, *x; double *f, *gmax; };
// fn(pack...) with the trailing pack of the kernel instance that takes these rows: a functor with stage data always ends in a StageData; a functor
// with parameters gets a StageTheta in front when a parameter row is set (THETA: the operation has instances that read theta -- convexify has none).
// A functor without the member compiles no instance with that element.
template <class M, bool THETA, class Fn> inline hipError_t stage_with_rows(const StageRows &r, Fn fn) {
  auto data = [&](auto... th) {
    if constexpr (sm_nsd<M>::value > 0) return fn(th..., StageData{r.sdata}); else return fn(th...);
  };
  if constexpr (THETA && sm_ntheta<M>::value > 0) if (r.theta || r.plant) return data(StageTheta{r.theta, r.plant});
  return data();
}

// launchers shared by the zoo dispatch and generated libraries
// (PP: empty, or a StageTheta and / or a StageData behind the stream -- the per-instance-parameter and the stage-data instances)
template <class M, bool PF = false, class... PP>
inline hipError_t stage_launch_eval(const StageDev &sd, int batch, const StageEvalArgs &a, hipStream_t st, PP... pp) {
  constexpr int f = M::nx + M::nu;
  const int ppad = PF ? (sd.N * M::nx + f - 1) / f * f : f;
  const long threads = (long)batch * ((sm_has_coop<M>::value && (64 % f == 0) && M::nx <= f) ? ppad + f * sd.N : sd.n);
  stage_eval_kernel<M, PF, PP...><<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(sd, batch, a.p, a.x, a.lbx, a.ubx, a.lbg, a.ubg, a.P, a.q, a.A, a.l, a.u, pp...);
  return hipGetLastError();
}
template <class M, bool PF = false, class... PP>
inline hipError_t stage_launch_merit(const StageDev &sd, int batch, const StageMeritArgs &a, hipStream_t st, PP... pp) {
  stage_merit_kernel<M, PF, PP...><<<(unsigned)((batch + 3) / 4), 256, 0, st>>>(sd, batch, a.p, a.x, a.f, a.gmax, pp...);
  return hipGetLastError();
}
template <class M, bool PF = false, class... PP>
inline hipError_t stage_launch_advance(const StageDev &sd, int batch, const mpcqp_stage_advance_args &a, hipStream_t st, PP... pp) {
  stage_advance_kernel<M, PF, PP...><<<(unsigned)((batch + 3) / 4), 256, 0, st>>>(sd, batch, a, pp...);
  return hipGetLastError();
}
// (one thread per instance in 64-thread workgroups; the same instance serves both kinds of reference)
template <class M, class... PP>
inline hipError_t stage_launch_rollout(const StageDev &sd, int batch, const mpcqp_stage_rollout_args &a, hipStream_t st, PP... pp) {
  stage_rollout_kernel<M, PP...><<<(unsigned)((batch + 63) / 64), 64, 0, st>>>(sd, batch, a, pp...);
  return hipGetLastError();
}
template <class M, bool PF = false, class... PP>
inline hipError_t stage_launch_linesearch(const StageDev &sd, int batch, const mpcqp_stage_linesearch_args &a, hipStream_t st, PP... pp) {
  stage_linesearch_kernel<M, PF, PP...><<<(unsigned)((batch + 3) / 4), 256, 0, st>>>(sd, batch, a, pp...);
  return hipGetLastError();
}
template <class M, bool PF = false, class... PP>
inline hipError_t stage_launch_convexify(const StageDev &sd, int batch, const mpcqp_stage_convexify_args &a, const StageCvxBuf &w, hipStream_t st, PP... pp) {
  if constexpr (M::has_cost != 0) {
    using C = stage_cvx<M>;
    const long items = (long)batch * sd.N, entries = (long)batch * M::nx * M::nx;
    stage_convexify_kernel<M, PF, PP...><<<(unsigned)((items + C::G - 1) / C::G), C::G * C::W, 0, st>>>(sd, batch, a, w, pp...);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    stage_convexify_sum_kernel<M><<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(batch, sd.N, sd.nnzP, w, a.P, a.touched);
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

// mpcqp_stage_lagrangian: the add kernel, then -- with a mode -- the convexify kernel with the StageExact element and its sum kernel on the updated P,
// so that a frame the convexification does not touch holds the bits mode = 0 gives.  slots: the curvature's table; w: the convexification's (mode != 0)
// (CVX: the library also carries the convexification -- without it only the add kernel is instantiated and a mode is an invalid value)
template <class M, bool CVX, bool PF = false, class... PP>
inline hipError_t stage_launch_lagrangian(const StageDev &sd, int batch, const mpcqp_stage_lagrangian_args &a, const int *slots, const StageCvxBuf *w,
                                          hipStream_t st, PP... pp) {
  if constexpr (sm_has_exact<M>::value) {
    const StageExact ex{a.y, a.status};
    const long threads = (long)batch * sd.N * (M::nx + M::nu);
    stage_lagrangian_kernel<M, PP...><<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(sd, batch, a.x, ex, slots, a.P, pp...);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.mode == 0) return hipSuccess;
    if constexpr (CVX) {
      if (!w) return hipErrorInvalidValue;
      using C = stage_cvx<M>;
      const mpcqp_stage_convexify_args ca{a.mode, a.eps, a.p, a.x, a.P, a.touched, a.lam_min};
      const long items = (long)batch * sd.N, entries = (long)batch * M::nx * M::nx;
      stage_convexify_kernel<M, PF, PP..., StageExact><<<(unsigned)((items + C::G - 1) / C::G), C::G * C::W, 0, st>>>(sd, batch, ca, *w, pp..., ex);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
      stage_convexify_sum_kernel<M><<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(batch, sd.N, sd.nnzP, *w, a.P, a.touched);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  } else {
    return hipErrorInvalidValue;
  }
}

// The model zoo, listed once: fn(StageTag<M, PF>{}) for the functor of `model` and the kind of reference.  A new zoo functor is one more case
// here.  PARAMS: only the functors that read parameters (the PP instances exist for those alone); any other model is an invalid value.
template <class M_, bool PF_> struct StageTag { using M = M_; static constexpr bool PF = PF_; };
template <class M, bool PARAMS, class Fn> inline hipError_t stage_visit_model(bool pref, Fn &fn) {
  if constexpr (PARAMS && sm_ntheta<M>::value == 0) return hipErrorInvalidValue;
  else return pref ? fn(StageTag<M, true>{}) : fn(StageTag<M, false>{});
}
template <bool PARAMS = false, class Fn> inline hipError_t stage_visit_zoo(int model, bool pref, Fn fn) {
  switch (model) {
    case SM_DOUBLE_INTEGRATOR: return stage_visit_model<SmDoubleIntegrator, PARAMS>(pref, fn);
    case SM_QUADROTOR: return stage_visit_model<SmQuadrotor, PARAMS>(pref, fn);
    case SM_CARTPOLE: return stage_visit_model<SmCartPole, PARAMS>(pref, fn);
  }
  return hipErrorInvalidValue;
}
