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
