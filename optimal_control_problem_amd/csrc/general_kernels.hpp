// general_kernels.hpp -- device templates of the local-system evaluation for a general (non-stage) NLP: cost and constraints are
// arbitrary traced expressions over the whole vector w = [p; x], as the reference accepts them
// (reference src/sqp_solver/SQPOptimizationSolver.cpp:47-77 builds hessian(f, w) and jacobian([p; x; g], w) with their true sparsity,
// :100-120 evaluates them once per SQP iteration, :171-181 takes the step and the objective).
// Included only by the translation units optimal_control_problem_amd/codegen.py generates (emit_general): the functor M carries three
// scalar-generic bodies F (cost), G (reverse-derived gradient, n outputs) and C (constraints, ng outputs).  A body takes its inputs
// from an accessor `in(k)` and hands every output to a sink `out(r, value)` when it is produced, so a thread holds no array whose
// length grows with the problem.
//
// Compression by colouring (general_eval.py): the columns of the Hessian are partitioned into colours such that no two columns of a
// colour share a structurally non-zero row; one pass seeds the dual part 1.0 on every input of its colour, and the dual part of
// output row r IS entry (r, the one column of that colour with row r).  hslot[pass * n + r] is that entry's CSC value slot or -1:
// direct recovery, one writer per output element, no atomics and no sums across threads.  The same for the Jacobian with jslot.
//
// Mapping: one thread per (instance b, pass), pass fastest -- the lanes of an instance read the same w[k] (a broadcast load) and run
// the same straight-line code; the seed is data, not control flow.  Hessian passes, Jacobian passes and the identity rows sit in
// separate block ranges of one launch, so a wave runs one body.  GENERAL_ABI_VERSION guards the GnDev layout shared between
// libmpcqp.so and a generated library.
#pragma once
#include <hip/hip_runtime.h>
#include "stage_models.hpp"
#include "general_linesearch.hpp"
#include "general_lagrangian.hpp"

#define GENERAL_ABI_VERSION 1

struct GnDev {
  int n, np, nvar, ng, m, nnzP, nnzA;
  int hp, jp;                 // Hessian passes (>= 1: pass 0 writes q), Jacobian passes (0 when ng == 0)
  const int *Ap;              // device: column pointers of A [n + 1] (the identity entry is the first of its column)
  const int *hslot, *jslot;   // device: [hp * n], [jp * ng]
};

// ---- accessors: the inputs are formed where they are used
template <class M, const int *COLOUR> struct GnSeededIn {
  const double *p, *x; int pass;
  __device__ __forceinline__ Dual operator()(int k) const { return Dual{k < M::np ? p[k] : x[k - M::np], COLOUR[k] == pass ? 1.0 : 0.0}; }
};
template <class M> struct GnValueIn {
  const double *p, *x;
  __device__ __forceinline__ double operator()(int k) const { return k < M::np ? p[k] : x[k - M::np]; }
};

// the point a lane of the line search evaluates: x itself on the base lane, else x + alpha dx.  The base lane must not touch dx at all (a failed
// QP leaves NaN there, and x + 0 * NaN is NaN), and a load under a condition would turn every input into a branch: so `d` is dx on a candidate
// lane and x on the base lane -- one unconditional load from memory the lane may read -- and the value is chosen after the arithmetic
template <class M> struct GnCandidateIn {
  const double *p, *x, *d; double alpha; bool base;
  __device__ __forceinline__ double operator()(int k) const {
    if (k < M::np) return p[k];
    const double xv = x[k - M::np], c = gn_ls_point(xv, alpha, d[k - M::np]);
    return base ? xv : c;
  }
};

// ---- sinks: an output goes to its slot, or nowhere
struct GnHessOut {
  double *P, *q; const int *slot; bool first;
  __device__ __forceinline__ void operator()(int r, Dual v) const {
    const int s = slot[r];
    if (s >= 0) P[s] = v.d;
    if (first) q[r] = v.v;
  }
};
struct GnJacOut {
  double *A, *l, *u; const double *lbg, *ubg; const int *slot; bool first;      // l, u: at the first general row
  __device__ __forceinline__ void operator()(int r, Dual v) const {
    const int s = slot[r];
    if (s >= 0) A[s] = v.d;
    if (first) { l[r] = lbg[r] - v.v; u[r] = ubg[r] - v.v; }                    // an infinite bound stays infinite
  }
};
struct GnCostOut {
  double *f;
  __device__ __forceinline__ void operator()(int, double v) const { *f = v; }
};
struct GnViolationOut {
  const double *lbg, *ubg; double *gmax;
  __device__ __forceinline__ void operator()(int r, double v) const { *gmax = fmax(*gmax, fmax(lbg[r] - v, v - ubg[r])); }
};
// the l1 violation of the line search next to the max-norm violation, the latter exactly as GnViolationOut keeps it
struct GnMeritOut {
  const double *lbg, *ubg; double *v, *gmax;
  __device__ __forceinline__ void operator()(int r, double g) const {
    *gmax = fmax(*gmax, fmax(lbg[r] - g, g - ubg[r]));
    *v += gn_ls_outside(lbg[r], g, ubg[r]);
  }
};

template <class M>
__global__ void __launch_bounds__(256) general_eval_kernel(GnDev gd, int batch, unsigned hblocks, unsigned jblocks,
                                                           const double *__restrict__ p, const double *__restrict__ x,
                                                           const double *__restrict__ lbx, const double *__restrict__ ubx,
                                                           const double *__restrict__ lbg, const double *__restrict__ ubg,
                                                           double *__restrict__ P, double *__restrict__ q, double *__restrict__ A,
                                                           double *__restrict__ l, double *__restrict__ u) {
  constexpr int n = M::n, np = M::np, nvar = M::nvar, ng = M::ng;
  if (blockIdx.x < hblocks) {
    // Hessian passes: G on duals seeded by colour; pass 0 also stores the gradient
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)batch * gd.hp) return;
    const int b = (int)(gid / gd.hp), pass = (int)(gid - (long)b * gd.hp);
    const GnSeededIn<M, M::hcol> in{p + (long)b * np, x + (long)b * nvar, pass};
    const GnHessOut out{P + (long)b * gd.nnzP, q + (long)b * n, gd.hslot + (long)pass * n, pass == 0};
    M::template G<Dual>(in, out);
    return;
  }
  if (blockIdx.x < hblocks + jblocks) {
    // Jacobian passes: C on duals seeded by colour; pass 0 also stores the shifted bounds of the general rows
    if constexpr (ng > 0) {
      const long gid = (long)(blockIdx.x - hblocks) * blockDim.x + threadIdx.x;
      if (gid >= (long)batch * gd.jp) return;
      const int b = (int)(gid / gd.jp), pass = (int)(gid - (long)b * gd.jp);
      const GnSeededIn<M, M::jcol> in{p + (long)b * np, x + (long)b * nvar, pass};
      const GnJacOut out{A + (long)b * gd.nnzA, l + (long)b * gd.m + n, u + (long)b * gd.m + n, lbg + (long)b * ng, ubg + (long)b * ng,
                         gd.jslot + (long)pass * ng, pass == 0};
      M::template C<Dual>(in, out);
    }
    return;
  }
  // identity rows: A[j, j] = 1 and l, u = [p; lbx] - w, [p; ubx] - w, once per instance and column
  const long gid = (long)(blockIdx.x - hblocks - jblocks) * blockDim.x + threadIdx.x;
  if (gid >= (long)batch * n) return;
  const int b = (int)(gid / n), j = (int)(gid - (long)b * n);
  A[(long)b * gd.nnzA + gd.Ap[j]] = 1.0;
  double lo, hi, w;
  if (j < np) { w = p[(long)b * np + j]; lo = w; hi = w; }
  else { const long i = (long)b * nvar + (j - np); w = x[i]; lo = lbx[i]; hi = ubx[i]; }
  l[(long)b * gd.m + j] = lo - w; u[(long)b * gd.m + j] = hi - w;
}

// f and the max-norm violation of lbg <= g <= ubg, one thread per instance, plain doubles
template <class M>
__global__ void __launch_bounds__(256) general_merit_kernel(int batch, const double *__restrict__ p, const double *__restrict__ x,
                                                            const double *__restrict__ lbg, const double *__restrict__ ubg,
                                                            double *__restrict__ fout, double *__restrict__ gout) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const GnValueIn<M> in{p + b * M::np, x + b * M::nvar};
  if (fout) { double f = 0.0; M::template F<double>(in, GnCostOut{&f}); fout[b] = f; }
  if (gout) {
    double gmax = 0.0;
    if constexpr (M::ng > 0) M::template C<double>(in, GnViolationOut{lbg + b * M::ng, ubg + b * M::ng, &gmax});
    gout[b] = gmax;
  }
}

// Per-instance l1-merit backtracking line search (mpcqp_nlp_linesearch; general_nlp.GeneralNLP.line_search is its NumPy statement, the rule itself
// is general_linesearch.hpp).  A group of W lanes serves one instance, W = gn_ls_group_width(candidates) handed in as a value: lane 0 evaluates the
// base point x, lane j >= 1 the candidate x + alpha0 beta^(j-1) dx, lanes beyond the candidates idle; an instance whose QP returned no point runs
// lane 0 only and never reads its dw or y.  A lane runs F and C once each at its own point (GnCandidateIn forms it where it is used) and sums the
// box terms of that point; the lanes of a group read the same addresses, a broadcast load as in general_eval_kernel.  q' dx and max |y| stride over
// the group and are reduced by one xor butterfly in fixed order; the merits travel by shuffles, every lane takes the same decision.  x is written
// after that, strided over the group, by gn_ls_point: every read of x precedes the write in program order of the same wave, and the selected
// lane's f and gmax ARE mpcqp_nlp_merit at the x written.  No LDS, no atomics, one writer per output, no array in a thread.
template <class M>
__global__ void __launch_bounds__(256) general_linesearch_kernel(int batch, int W, mpcqp_nlp_linesearch_args a) {
  constexpr int n = M::n, np = M::np, nvar = M::nvar, ng = M::ng;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long b = gid / W;
  const int lane = (int)(gid - b * W);
  if (b >= batch) return;                       // (whole groups leave: the shuffles below stay inside a group)
  bool ok = true;
  if (a.status) ok = gn_ls_status_ok(a.status[b]);
  const int K = ok ? a.candidates : 0;
  double *xb = a.x + b * nvar;
  const double *dxb = a.dw + b * n + np;
  const bool base = lane == 0;
  const double alpha = base ? 0.0 : gn_ls_alpha(a.alpha0, a.beta, lane - 1);
  double cost = 0.0, vio = 0.0, gmx = 0.0;
  if (lane <= K) {
    const GnCandidateIn<M> in{a.p + b * np, xb, base ? xb : dxb, alpha, base};
    M::template F<double>(in, GnCostOut{&cost});
    if constexpr (ng > 0) M::template C<double>(in, GnMeritOut{a.lbg + b * ng, a.ubg + b * ng, &vio, &gmx});
    const double *lb = a.lbx + b * nvar, *ub = a.ubx + b * nvar;
    // (kept as a loop: unrolled over a constant nvar, its four loads per entry are all drawn to the top and the inputs of F and C stay alive for it)
#pragma unroll 4
    for (int i = 0; i < nvar; i++) vio += gn_ls_outside(lb[i], in(np + i), ub[i]);
  }
  double qd = 0.0, ymax = 0.0;
  if (ok) {
    const double *qb = a.q + b * n + np, *yb = a.y + b * (n + ng);
    for (int i = lane; i < nvar; i += W) qd += qb[i] * dxb[i];
    for (int i = np + lane; i < n + ng; i += W) ymax = fmax(ymax, fabs(yb[i]));
  }
  for (int o = W >> 1; o >= 1; o >>= 1) { qd += __shfl_xor(qd, o, W); ymax = fmax(ymax, __shfl_xor(ymax, o, W)); }
  // the decision, the same on every lane of the group
  const double mu = gn_ls_penalty(a.mu != nullptr, a.mu ? a.mu[b] : 0.0, a.mu_min, a.mu_factor, ok, ymax);
  const double phi = gn_ls_merit(cost, mu, vio);
  const double D = gn_ls_slope(qd, mu, __shfl(vio, 0, W));
  int acc;
  const int sel = gn_ls_decide(K, a.candidates, a.alpha0, a.beta, a.c1, D, [&](int j) { return __shfl(phi, j, W); }, &acc);
  const double alpha_sel = sel > 0 ? gn_ls_alpha(a.alpha0, a.beta, sel - 1) : 0.0;
  const double f_sel = __shfl(cost, sel, W), g_sel = __shfl(gmx, sel, W), phi_0 = __shfl(phi, 0, W), phi_sel = __shfl(phi, sel, W);
  double mx = 0.0;
  if (sel > 0) {
    for (int i = lane; i < nvar; i += W) {
      const double dv = dxb[i], d = alpha_sel * dv;
      xb[i] = gn_ls_point(xb[i], alpha_sel, dv); mx = fmax(mx, fabs(d));
    }
  }
  for (int o = W >> 1; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, W));
  if (base) {
    if (a.mu && ok) a.mu[b] = mu;
    if (a.alpha_out) a.alpha_out[b] = alpha_sel;
    if (a.accepted) a.accepted[b] = acc;
    if (a.step_max) a.step_max[b] = mx;
    if (a.f_out) a.f_out[b] = f_sel;
    if (a.gmax_out) a.gmax_out[b] = g_sel;
    if (a.phi) { a.phi[2 * b] = phi_0; a.phi[2 * b + 1] = phi_sel; }
  }
}

// The exact Hessian of the Lagrangian (mpcqp_nlp_lagrangian; general_nlp.GeneralNLP.lagrangian_system is its NumPy statement, the shared parts are
// general_lagrangian.hpp).  For a functor generated from a model with exact_hessian=True: CG is the reverse-derived gradient over w of the
// contracted scalar sum_i mul(i) g_i(w), the multipliers plain values; ccol colours the columns of the curvature's structure and
// cslot[pass * n + r] names the slot of entry (r, c) in P's CSC, as hcol / hslot do for the cost.  One thread per (instance, curvature pass), pass
// fastest as in general_eval_kernel: the dual part of output r goes to its slot of the workspace C, or, without a workspace (mode 0 only), is
// added to P there.  One writer per entry, no atomics, no LDS, no array in a thread.  An instance whose QP returned no point is neither read
// nor written: its y is NaN.
template <class M>
__global__ void __launch_bounds__(256) general_curvature_kernel(int batch, mpcqp_nlp_lagrangian_args a) {
  constexpr int n = M::n, np = M::np, nvar = M::nvar, ng = M::ng, cp = M::cp;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)batch * cp) return;
  const int b = (int)(gid / cp), pass = (int)(gid - (long)b * cp);
  if (a.status && !gn_ls_status_ok(a.status[b])) return;
  const GnSeededIn<M, M::ccol> in{a.p + (long)b * np, a.x + (long)b * nvar, pass};
  const GnMulIn mul{a.y + (long)b * (n + ng) + n};
  const GnCurvOut out{(a.C ? a.C : a.P) + (long)b * M::nnzP, M::cslot + pass * n, a.C == nullptr};
  M::template CG<Dual>(in, mul, out);
}

// P += C from the workspace, and the DOMINANT safeguard: one thread per (instance, column with curvature), the column walked by
// gn_lag_apply_column in ascending slot order -- every slot of P has one reader and writer, the result does not depend on the batch
template <class M>
__global__ void __launch_bounds__(256) general_curvature_apply_kernel(int batch, mpcqp_nlp_lagrangian_args a) {
  constexpr int ncc = M::ncc;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)batch * ncc) return;
  const int b = (int)(gid / ncc), ci = (int)(gid - (long)b * ncc);
  if (a.status && !gn_ls_status_ok(a.status[b])) return;
  gn_lag_apply_column<M>(ci, a.C + (long)b * M::nnzP, a.P + (long)b * M::nnzP, a.mode == MPCQP_NLP_DOMINANT,
                         a.shift ? a.shift + (long)b * M::n : nullptr);
}

template <class M>
inline hipError_t general_launch_eval(const GnDev &gd, int batch, const double *p, const double *x, const double *lbx, const double *ubx,
                                      const double *lbg, const double *ubg, double *P, double *q, double *A, double *l, double *u, hipStream_t st) {
  const unsigned hb = (unsigned)(((long)batch * gd.hp + 255) / 256), jb = (unsigned)(((long)batch * gd.jp + 255) / 256);
  const unsigned ib = (unsigned)(((long)batch * gd.n + 255) / 256);
  general_eval_kernel<M><<<hb + jb + ib, 256, 0, st>>>(gd, batch, hb, jb, p, x, lbx, ubx, lbg, ubg, P, q, A, l, u);
  return hipGetLastError();
}
template <class M>
inline hipError_t general_launch_merit(int batch, const double *p, const double *x, const double *lbg, const double *ubg, double *f, double *gmax,
                                       hipStream_t st) {
  general_merit_kernel<M><<<(unsigned)((batch + 255) / 256), 256, 0, st>>>(batch, p, x, lbg, ubg, f, gmax);
  return hipGetLastError();
}
// (no allocation, no synchronisation: a captured graph replays the launch)
template <class M>
inline hipError_t general_launch_linesearch(int batch, const mpcqp_nlp_linesearch_args &a, hipStream_t st) {
  const int W = gn_ls_group_width(a.candidates);
  general_linesearch_kernel<M><<<(unsigned)(((long)batch * W + 255) / 256), 256, 0, st>>>(batch, W, a);
  return hipGetLastError();
}
// (cp = 0 -- linear constraints or none: nothing to add, nothing is launched)
template <class M>
inline hipError_t general_launch_lagrangian(int batch, const mpcqp_nlp_lagrangian_args &a, hipStream_t st) {
  if constexpr (M::cp > 0) {
    general_curvature_kernel<M><<<(unsigned)(((long)batch * M::cp + 255) / 256), 256, 0, st>>>(batch, a);
    if (a.C) general_curvature_apply_kernel<M><<<(unsigned)(((long)batch * M::ncc + 255) / 256), 256, 0, st>>>(batch, a);
  }
  return hipGetLastError();
}
