// kernel_oc_rescale.hpp -- the kept-workspace entry for NEW MATRICES of the two-kernel on-chip mode (mpcqp_update_matrices; OSQP's osqp_update_data_mat,
// what the reference's private CuCaQP::updateHessianMatrix / updateLinearConstraintsMatrix map to, reference src/sqp_solver/CuCaQP.cpp:106-116,129-140):
// D, E, c of the handle's last full set-up and every instance's current rho stay; the new P, q, A, l, u are scaled with them and the KKT matrix is
// factorised again.  No Ruiz pass, no staging of the unscaled values, no Ruiz state: every structure is read once from the caller's CSC arrays through
// the plan's source indices and written once, scaled, to the slab.
// It takes the place of mpcqp_oc_setup_kernel in the first launch of a solve (DevIO.reuse == 2) and runs in that kernel's launch shape -- four-wave
// workgroups with the set-up's own LDS layout (select.hpp SetupShape, oc_lds<NW, true>) --, so the slab it leaves is the slab the iteration kernel and
// the resume-mode launches of the set-up kernel expect: scaled ELL values, l, u, the scaled q in the Lb region, the factor, DevIO.status / iters / info[3].
// Included by k_oc_rescale.hip alone, behind kernels_all.hpp (not a stand-alone header).
#pragma once

template <int NW, bool HUB>
__global__ void __launch_bounds__(NW * WAVE, 2) mpcqp_oc_rescale_kernel(const DevPlan pl, const DevRes rs, const mpcqp_settings st, const DevIO io, const DevOc oc) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int NT = NW * WAVE;
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane(io.order ? io.order[blockIdx.x] : (int)blockIdx.x);
  if (b < 0) return;      // (mpcqp_set_skip: the dispatch list ends in -1 entries; the whole workgroup leaves, nothing of any instance is touched)
  int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if constexpr (NW == 4) wid = oc_wave_role4(lds, wid, lane, io.no_remap);
  const int tid = wid * WAVE + lane;
  const OcLds<NW> L = oc_lds<NW, true>(lds, pl, rs, oc);
  RCtx cx;
  cx.pl = &pl; cx.rs = &rs; cx.st = &st; cx.wid = wid; cx.lane = lane;
  cx.fts[0] = cx.fts[1] = cx.fts[2] = cx.fts[3] = 0;
  double *ws = io.ws + (long)b * pl.ws_stride; cx.ws = ws;
  cx.BL = ws + pl.o_Lf; cx.TMP = lds;
  cx.X = L.X; cx.Q = L.Q; cx.R = L.R; cx.Z = L.Z; cx.Y = L.Y; cx.W = L.W; cx.RB = L.RB; cx.RED = L.RED;
  double *valA = ws + pl.o_ellA, *valAt = ws + pl.o_ellAt, *valP = ws + pl.o_ellP;
  double *lb = ws + pl.o_l, *ub = ws + pl.o_u, *Qs = ws + pl.o_Lb;
  const double *Dg = ws + pl.o_D, *Eg = ws + pl.o_E;      // (read only: the scaling is the last full set-up's)
  const double *inP = io.P + (long)b * io.sP, *inA = io.A + (long)b * io.sA, *inq = io.q + (long)b * io.sq;
  const double *inl = io.l + (long)b * io.sl, *inu = io.u + (long)b * io.su;
  const int n = pl.n, m = pl.m, npad = pl.npad, mpad = pl.mpad;
  cx.unscale = st.scaling && !st.scaled_termination;
  oc_tables_to_lds<NW>(pl, oc, cx, L, tid);
  const double c = uni(io.cscale[b]); cx.c = c; cx.cinv = uni(1.0 / c);
  // D in R, E in W: where the set-up kernel's scaling phase has them (the factorisation overwrites both afterwards)
  for (int t = tid; t < npad; t += NT) { if (pl.perm[t] < 0) Qs[t] = 0.0; cx.R[t] = Dg[t]; }      // (q in place in the slab: padding positions here, the variables' below)
  for (int i = tid; i < mpad; i += NT) cx.W[i] = Eg[i];
  bsync<NW>();
  for (int j = tid; j < n; j += NT) { const int t = pl.pos[j]; Qs[t] = inq[j] * (c * cx.R[t]); }
  for (int i = tid; i < mpad; i += NT) {
    const double ei = cx.W[i];
    lb[i] = i < m ? ei * fmax(inl[i], -Q_INFTY) : 0.0;
    ub[i] = i < m ? ei * fmin(inu[i], Q_INFTY) : 0.0;
  }
  // A <- E A D by rows, A' the same numbers by variable, P <- c D P D: one pass each, gathered from the caller's arrays (ell_map_chunk<true>: up to eight
  // source indices, then the eight values they point at, in flight per lane; whole 512 B slots stored).  The products are formed as the set-up kernel forms them.
  for (int ch = wid; ch < pl.A.nchunks; ch += NW) {
    const int i = ch * WAVE + lane; const double ei = i < mpad ? cx.W[i] : 0.0;
    ell_map_chunk<true>(valA, pl.A.src, inA, pl.A.idx, valA, cx.coA[ch], cx.coA[ch + 1], lane, [&](double v, int j) { return v * (ei * cx.R[j]); });
  }
  for (int ch = wid; ch < pl.At.nchunks; ch += NW) {
    const int t = ch * WAVE + lane; const double dj = t < npad ? cx.R[t] : 0.0;
    ell_map_chunk<true>(valAt, pl.At.src, inA, pl.At.idx, valAt, cx.coAt[ch], cx.coAt[ch + 1], lane, [&](double v, int i) { return v * (dj * cx.W[i]); });
  }
  for (int ch = wid; ch < pl.P.nchunks; ch += NW) {
    const int t = ch * WAVE + lane; const double dj = t < npad ? cx.R[t] : 0.0;
    ell_map_chunk<true>(valP, pl.P.src, inP, pl.P.idx, valP, cx.coP[ch], cx.coP[ch + 1], lane, [&](double v, int k) { return v * (c * dj * cx.R[k]); });
  }
  bsync<NW>();
  // the instance's final rho of the previous solve (OSQP keeps rho over osqp_update_data_mat); a value no solve can have left falls back to the settings'
  double rho = io.info[4L * b + 3];
  if (!(rho >= Q_RHO_MIN && rho <= Q_RHO_MAX)) rho = fmin(fmax(st.rho, Q_RHO_MIN), Q_RHO_MAX);
  cx.rho = uni(rho);
  // always a new factor, whatever the previous problem's verdict was: the matrices are new
  const bool ok = factorize_res<NW, (HUB ? 2 : 1), false, true>(cx, &oc, L.octab, lds);
  if (tid == 0) {
    io.status[b] = ok ? MPCQP_UNSOLVED : MPCQP_NON_CVX; io.iters[b] = 0;
    io.info[4L * b + 3] = cx.rho;
  }
}
