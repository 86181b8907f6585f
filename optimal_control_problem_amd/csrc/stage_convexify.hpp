// stage_convexify.hpp -- the eigen-solve behind mpcqp_stage_convexify: cyclic Jacobi on one symmetric tile and the spectral
// correction f(H) - H, written as plain functions over a lane-strided loop.  On the device the W lanes of one group call them together on a
// tile in LDS (stage_kernels.hpp, stage_convexify_kernel); compiled by g++ the same text is one "group" of width 1 walking every index itself
// (tests/support/convexify_host.cpp), so the host build checks the very code the kernel runs.  No HIP header is needed to read this file.
#pragma once
#include <cmath>
#include "stage_models.hpp"
#include "../../include/mpcqp.h"

constexpr int SM_JACOBI_SWEEP_CAP = 30;         // at least twice the most sweeps seen on the test inputs (DESIGN 6.16 has the count)
constexpr double SM_JACOBI_RTOL2 = 1e-30;       // stop when off(A)^2 <= RTOL2 ||A_0||_F^2: off(A) <= 1e-15 ||A_0||_F

// The group primitives.  Device: every thread of the block reaches every sm_group_sync and sm_block_any (they are block barriers: a group is a
// part of one wave, a block holds several), the sums and minima run over the W lanes of the group.  Host: one lane, nothing to do.
#if defined(__HIP_DEVICE_COMPILE__)
SM_HD void sm_group_sync() { __syncthreads(); }
SM_HD bool sm_block_any(bool v) { return __syncthreads_or(v ? 1 : 0) != 0; }
template <int W> SM_HD double sm_group_sum(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}
template <int W> SM_HD double sm_group_min(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, W));
  return v;
}
#else
SM_HD void sm_group_sync() {}
SM_HD bool sm_block_any(bool v) { return v; }
template <int W> SM_HD double sm_group_sum(double v) { return v; }
template <int W> SM_HD double sm_group_min(double v) { return v; }
#endif

// Cyclic Jacobi, rows first (p, q) = (0, 1), (0, 2) .. (n-2, n-1), on the symmetric n x n tile A (row-major, both triangles kept); on return the
// diagonal of A holds the eigenvalues and the columns of V the eigenvectors, A_0 = V diag V'.  Returns the sweeps this group ran.
//   * a pivot that is exactly 0.0 is skipped: the rotation would be the identity, and entries that are structurally zero -- the blocks between
//     two connected components of the sparsity graph -- are never touched, so they stay exactly zero in A and in V
//   * lane i owns row i of a rotation: it rotates (A[i][p], A[i][q]) and mirrors the result into row p and row q, and rotates row i of V; lane 0
//     sets the four pivot entries.  No two lanes write one entry, no lane reads what another writes between two barriers
//   * the trip counts are the same for every thread of the block: n and the cap are constants, the sweep loop ends on a vote of the block; a
//     group that has converged, or has no work (live = false), goes through the barriers without arithmetic, so what a group computes does not
//     depend on its neighbours in the block
template <int W>
SM_HD int sm_jacobi(double *A, double *V, const int n, const int lane, const bool live) {
  for (int i = lane; i < n; i += W)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  sm_group_sync();      // the tile was written by the lanes of the group
  double fro = 0.0;
  bool done = !live;
  if (live) {
    for (int i = lane; i < n; i += W)
      for (int j = 0; j < n; j++) fro += A[i * n + j] * A[i * n + j];
    fro = sm_group_sum<W>(fro);
  }
  int sweeps = 0;
  for (int sw = 0; sw < SM_JACOBI_SWEEP_CAP; sw++) {
    if (!done) {
      double off = 0.0;
      for (int i = lane; i < n; i += W)
        for (int j = 0; j < n; j++) off += i == j ? 0.0 : A[i * n + j] * A[i * n + j];
      off = sm_group_sum<W>(off);
      done = off <= SM_JACOBI_RTOL2 * fro;
    }
    if (!sm_block_any(!done)) break;
    if (!done) sweeps++;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double app = 0.0, aqq = 0.0, apq = 0.0;
        if (!done) { app = A[p * n + p]; aqq = A[q * n + q]; apq = A[p * n + q]; }
        sm_group_sync();      // every lane holds the pivots before lane 0 replaces them
        if (!done && apq != 0.0) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          for (int i = lane; i < n; i += W) {
            if (i != p && i != q) {
              const double aip = A[i * n + p], aiq = A[i * n + q];
              const double nip = c * aip - s * aiq, niq = s * aip + c * aiq;
              A[i * n + p] = nip; A[p * n + i] = nip;
              A[i * n + q] = niq; A[q * n + i] = niq;
            }
            const double vip = V[i * n + p], viq = V[i * n + q];
            V[i * n + p] = c * vip - s * viq; V[i * n + q] = s * vip + c * viq;
          }
          if (lane == 0) { A[p * n + p] = app - t * apq; A[q * n + q] = aqq + t * apq; A[p * n + q] = 0.0; A[q * n + p] = 0.0; }
        }
        sm_group_sync();
      }
  }
  return sweeps;
}

// f of MPCQP_CONVEXIFY_PROJECT: max(lam, eps); of MPCQP_CONVEXIFY_MIRROR: max(|lam|, eps).  Both leave lam >= eps where it is.
SM_HD double sm_convexify_f(double lam, int mode, double eps) {
  const double a = mode == MPCQP_CONVEXIFY_MIRROR ? fabs(lam) : lam;
  return a > eps ? a : eps;
}

// the smallest eigenvalue on the diagonal sm_jacobi left, the same on every lane of the group
template <int W>
SM_HD double sm_convexify_lam_min(const double *A, const int n, const int lane) {
  double m = INFINITY;
  for (int i = lane; i < n; i += W) m = fmin(m, A[i * n + i]);
  return sm_group_min<W>(m);
}

// entry (r, c) of D = f(H) - H = sum over the eigenvalues lam_j < eps of (f(lam_j) - lam_j) v_j v_j': only the eigenvalues that move take part, so
// nothing is cancelled against H.  w (v_r v_c) with the product first: D[r][c] and D[c][r] are the same bits.
SM_HD double sm_convexify_delta(const double *A, const double *V, const int n, const int r, const int c, const int mode, const double eps) {
  double acc = 0.0;
  for (int j = 0; j < n; j++) {
    const double lam = A[j * n + j];
    if (lam < eps) acc += (sm_convexify_f(lam, mode, eps) - lam) * (V[r * n + j] * V[c * n + j]);
  }
  return acc;
}
