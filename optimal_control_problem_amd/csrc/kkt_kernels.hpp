// kkt_kernels.hpp -- first-order optimality residuals of the NLP per instance (include/mpcqp.h, mpcqp_stage_kkt / mpcqp_nlp_kkt; DESIGN 6.25;
// optimal_control_problem_amd/kkt.py kkt_residuals is the NumPy statement).  The reference's loop has no convergence test
// (src/sqp_solver/SQPOptimizationSolver.cpp:127-216); this measure is what the opt-in options["kkt_tol"] stops on.
//
// One kernel template over the group width G (16, 32, 64 lanes per instance, 256 / G instances per block).  Pass 1: a lane owns the columns
// lane, lane + G, ... of A and sums A_kj y_k in storage order -- products and sums rounded one by one (contraction off), so the NumPy statement
// reproduces t_j bit for bit -- the entries of neighbouring columns are neighbours in the value array, so the lanes of a group read whole cache
// lines; y[Ai[k]] comes through the cache (8 m bytes per instance: 4.5 KB at quadrotor N = 20, 7.2 KB at cart-pole N = 100).  Columns below col0
// are read for NaNs only.  Pass 2: the lanes stride over the rows for feas and compl.  The four maxima and the NaN flag cross the lanes by one xor butterfly of fixed order inside the
// group; lane 0 writes.  No LDS, no atomics, no array in a thread, one writer per output: bitwise repeatable, independent of batch and position.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mpcqp.h"

struct KktDims {
  int n, m, col0, nnzA;
  const int *Ap, *Ai;       // device: column pointers [n + 1], row indices [nnzA], every index in [0, m)
};

// the lanes of one instance: 16, 32 or 64, from the longer of its two loops
inline int kkt_group_width(int n, int m, int col0) {
  const int w = n - col0 > m ? n - col0 : m;
  return w <= 16 ? 16 : w <= 32 ? 32 : 64;
}

template <int G>
__global__ void __launch_bounds__(256) kkt_kernel(int batch, KktDims d, mpcqp_kkt_args a) {
#pragma clang fp contract(off)
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long b = gid / G;
  const int lane = (int)(gid - b * G);
  if (b >= batch) return;                       // (whole groups leave: the shuffles below stay inside a group)
  if (a.frozen && a.frozen[b] != 0) return;     // neither read nor written
  const double *__restrict__ qb = a.q + b * d.n, *__restrict__ Ab = a.A + b * d.nnzA;
  const double *__restrict__ lb = a.l + b * d.m, *__restrict__ ub = a.u + b * d.m, *__restrict__ yb = a.y + b * d.m;
  double stat = 0.0, scale = 0.0, feas = 0.0, cmpl = 0.0;
  int bad = 0;
  for (int j = lane; j < d.n; j += G) {
    const int e1 = d.Ap[j + 1];
    double t = 0.0;
    for (int e = d.Ap[j]; e < e1; e++) {
      const double av = Ab[e];
      bad |= av != av;
      t = t + av * yb[d.Ai[e]];
    }
    const double qj = qb[j], r = qj + t;
    bad |= (qj != qj) | (r != r);
    if (j >= d.col0) { stat = fmax(stat, fabs(r)); scale = fmax(scale, fmax(fabs(qj), fabs(t))); }
  }
  for (int i = lane; i < d.m; i += G) {
    const double li = lb[i], ui = ub[i], yi = yb[i];
    bad |= (li != li) | (ui != ui) | (yi != yi);
    feas = fmax(feas, fmax(fmax(li, -ui), 0.0));
    cmpl = fmax(cmpl, fmax(fmin(fmax(yi, 0.0), fmax(ui, 0.0)), fmin(fmax(-yi, 0.0), fmax(-li, 0.0))));
  }
#pragma unroll
  for (int o = G >> 1; o >= 1; o >>= 1) {
    stat = fmax(stat, __shfl_xor(stat, o, G)); scale = fmax(scale, __shfl_xor(scale, o, G));
    feas = fmax(feas, __shfl_xor(feas, o, G)); cmpl = fmax(cmpl, __shfl_xor(cmpl, o, G));
    bad |= __shfl_xor(bad, o, G);
  }
  if (lane != 0) return;
  // (+ 0.0: a maximum of signed zeros becomes +0, whichever the fmax returned)
  const double nan = __builtin_nan("");
  double *res = a.res + 4 * b;
  res[0] = bad ? nan : stat; res[1] = bad ? nan : feas + 0.0; res[2] = bad ? nan : cmpl + 0.0; res[3] = bad ? nan : scale;
  if (a.converged)
    a.converged[b] = !bad && stat <= a.tol_stat * fmax(1.0, scale) && feas <= a.tol_feas && cmpl <= a.tol_compl ? 1 : 0;
}

// (no allocation, no synchronisation: a captured graph replays the launch)
inline hipError_t kkt_launch(int batch, const KktDims &d, const mpcqp_kkt_args &a, hipStream_t st) {
  const int G = kkt_group_width(d.n, d.m, d.col0);
  const unsigned blocks = (unsigned)(((long)batch * G + 255) / 256);
  if (G == 16) kkt_kernel<16><<<blocks, 256, 0, st>>>(batch, d, a);
  else if (G == 32) kkt_kernel<32><<<blocks, 256, 0, st>>>(batch, d, a);
  else kkt_kernel<64><<<blocks, 256, 0, st>>>(batch, d, a);
  return hipGetLastError();
}
