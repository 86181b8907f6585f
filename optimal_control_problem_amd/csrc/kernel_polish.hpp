// kernel_polish.hpp -- mpcqp_polish_kernel: OSQP's solution polishing as a post-solve kernel, one QP per wavefront
// Part of the translation unit k_polish.hip only (included there behind kernels_all.hpp; not a stand-alone header).
//
// What osqp_solve does behind the ADMM loop when settings.polishing is set (OSQP's polish(): guess the active constraints from the iterate,
// solve the equality-constrained QP on them through one regularised KKT system, refine, keep the result if it is better).  The reference
// leaves polishing off (OsqpEigen's default, never touched in src/sqp_solver/CuCaQP.cpp:163-181), so this kernel only runs on a handle that
// asked for it (mpcqp_set_polish).  It reads what every kernel family leaves in the per-QP slab -- the scaled ELL values of A, A', P, the
// scaled bounds and D, E -- and the final iterate from the handle's output buffers; the factor of the polish system goes into scratch of its
// own (DevPolish.fac), so the slab's Lf / Lb / T -- where a kept workspace parks the ADMM factor -- are not touched.
//
// The KKT system [P + delta I, A_a'; A_a, -delta I] is solved in the engine's condensed form: with w = 1 / delta on the active rows (0 elsewhere)
//     M_pol = P + delta I + A' diag(w) A            (the assembly and block Cholesky of factorize(), kernels_common.hpp, with w in place of rho)
//     dx = M_pol^-1 (r_x + A_a'(w o r_y)),   dy_a = w o (A_a dx - r_y)
// and refined against the unregularised matrix [P, A_a'; A_a, 0].
// delta regularises the CALLER's problem: on the scaled data of the slab (x = D xs, P_s = c D P D, A_s = E A D, y_s = c y / E) the same system reads
//     c D M_pol D = P_s + c delta D^2 + A_s' diag(c / (delta E^2)) A_s,
// so the diagonal term is c delta D_t^2 and the row weight c / (delta E_i^2), and the active rows are tested on the unscaled iterate.  Where the guessed
// active set is consistent both metrics give the same point; where it is not (more active rows than variables: the regularised solve is then a weighted
// least-squares fit) the candidate would otherwise depend on the equilibration -- this way it is the one a dense solve on the caller's data gives.
#pragma once

// factorize() of kernels_common.hpp with the row weights taken from a vector (W, mpad long, 0 on the rows that do not enter) and the factor
// and T tiles at the addresses given, and c delta D^2 on the diagonal in place of sigma: assembly on the matrix cores, left-looking block Cholesky with
// explicit 16 x 16 inverses.  R receives the singleton diagonal.  Returns false on a non-positive pivot.
__device__ bool polish_factorize(const DevPlan &pl, const double *ws, double *Lf, double *Lb, double *T, const double *W, double *R, const double cdelta,
                                 double *S0, double *S1) {
  const int lane = threadIdx.x;
  const double *Dg = ws + pl.o_D;
  const double *valA = ws + pl.o_ellA, *valAt = ws + pl.o_ellAt, *valP = ws + pl.o_ellP;
  {
    const DevEll &E = pl.At;
    for (int c = 0; c < E.nchunks; c++) {
      double acc = 0.0;
      for (int s = E.chunk_off[c]; s < E.chunk_off[c + 1]; s++) {
        const unsigned e = (unsigned)s * WAVE + lane;
        const double v = valAt[e];
        if (E.flag[e]) acc += W[E.idx[e]] * v * v;
      }
      const int t = c * WAVE + lane;
      if (t < pl.npad) R[t] = pl.perm[t] >= 0 ? cdelta * Dg[t] * Dg[t] + acc : 1.0;      // (c delta D_t^2: delta I of the caller's problem)
    }
  }
  for (long k = lane; k < (long)pl.nT * BLK; k += WAVE) T[k] = 0.0;
  wsync();
  {
    const DevEll &E = pl.A;
    for (int c = 0; c < E.nchunks; c++) {
      const int i = c * WAVE + lane;
      const double sr = i < pl.mpad ? sqrt(W[i]) : 0.0;
      for (int s = E.chunk_off[c]; s < E.chunk_off[c + 1]; s++) {
        const unsigned e = (unsigned)s * WAVE + lane;
        const int tp = pl.tpos[e];
        if (tp >= 0) T[tp] = valA[e] * sr;
      }
    }
  }
  wsync();
  const int row0 = lane >> 4, col = lane & 15;
  for (int b = 0; b < pl.nblk; b++) {
    d4 acc = {0, 0, 0, 0};
    for (int g = pl.asm_ptr[b]; g < pl.asm_ptr[b + 1]; g++) acc = mfma_abt(T + (long)pl.asm_a[g] * BLK, T + (long)pl.asm_b[g] * BLK, acc);
    const int J = pl.blk_diag[b];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int pi = pl.asm_pidx[(long)b * BLK + g * WAVE + lane];
      if (pi >= 0) acc[g] += valP[pi];
      const int row = row0 + 4 * g;
      if (J >= 0 && row == col) acc[g] += R[J * BS + row];
      Lf[(long)b * BLK + row * BS + col] = acc[g];
    }
  }
  wsync();
  for (int f = 0; f < pl.nfac; f++) {
    const int4 op = pl.fac[f];
    double *dst = Lf + (long)op.y * BLK;
    if (op.x == FAC_SUB) {
      d4 prod = {0, 0, 0, 0};
      prod = mfma_abt(Lf + (long)op.z * BLK, Lf + (long)op.w * BLK, prod);
#pragma unroll
      for (int g = 0; g < 4; g++) dst[(row0 + 4 * g) * BS + col] -= prod[g];
    } else if (op.x == FAC_POTRF) {
      if (!potrf_inv(dst, Lb + (long)pl.bwd_of[op.y] * BLK, S0, S1)) return false;
    } else {
      d4 prod = {0, 0, 0, 0};
      prod = mfma_abt(dst, Lf + (long)op.z * BLK, prod);
      double *dbt = Lb + (long)pl.bwd_of[op.y] * BLK;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        dst[(row0 + 4 * g) * BS + col] = prod[g];
        dbt[col * BS + row0 + 4 * g] = prod[g];
      }
    }
    wsync();
  }
  return true;
}

// One workgroup (one wavefront) per instance of the slice; DevPolish's per-instance pointers stand at the slice's first instance.
// LDS: X, Q, R [npad]; Y, W, B, RY, V [mpad]; the two 16 x 17 Cholesky tiles.
__global__ void __launch_bounds__(WAVE) mpcqp_polish_kernel(const DevPlan pl, const mpcqp_settings st, const DevPolish po) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = pl.n, m = pl.m, npad = pl.npad, mpad = pl.mpad;
  if (po.skip && po.skip[b] != 0) return;      // (mpcqp_set_skip: polish_status / polish_info of a skipped instance keep their bits)
  if (po.status[b] != MPCQP_SOLVED) {      // (as osqp_solve: only a solved problem is polished)
    if (lane == 0) {
      po.pstatus[b] = MPCQP_POLISH_NOT_PERFORMED;
      po.pinfo[4L * b] = NAN; po.pinfo[4L * b + 1] = NAN; po.pinfo[4L * b + 2] = NAN; po.pinfo[4L * b + 3] = 0.0;
    }
    return;
  }
  double *X = lds, *Q = X + npad, *R = Q + npad;
  double *Y = R + npad, *W = Y + mpad, *B = W + mpad, *RY = B + mpad, *V = RY + mpad;
  double *S0 = V + mpad, *S1 = S0 + BS * 17;
  const double *ws = po.ws + (long)b * pl.ws_stride;
  const double *valA = ws + pl.o_ellA, *valAt = ws + pl.o_ellAt, *valP = ws + pl.o_ellP;
  const double *lb = ws + pl.o_l, *ub = ws + pl.o_u, *Dg = ws + pl.o_D, *Eg = ws + pl.o_E;
  double *Lf = po.fac + (long)b * po.fac_stride, *Lb = Lf + (long)pl.nblk * BLK, *T = Lb + (long)pl.nblk * BLK;
  const double *inq = po.q + (long)b * po.sq;
  const double *yin = po.y + (long)b * m, *zin = po.z + (long)b * m;
  const int unscale = st.scaling && !st.scaled_termination;
  const double c = uni(po.cscale[b]), cinv = uni(1.0 / c);
  const double delta = po.delta, winv = 1.0 / delta;

  // ---- 1. q in the scaled space of the slab; 2. / 3. active rows (tested on the unscaled iterate), their scaled bound and their weight c / (delta E^2)
  for (int t = lane; t < npad; t += WAVE) { X[t] = 0.0; Q[t] = 0.0; }
  wsync();
  for (int j = lane; j < n; j += WAVE) { const int t = pl.pos[j]; Q[t] = c * Dg[t] * inq[j]; }
  int nact = 0;
  for (int i = lane; i < mpad; i += WAVE) {
    double w = 0.0, bi = 0.0;
    if (i < m) {
      const double einv = 1.0 / Eg[i], yi = yin[i], zi = zin[i], lo = lb[i], up = ub[i], wi = c * winv * einv * einv;
      if (zi - einv * lo < -yi) { w = wi; bi = lo; }
      else if (einv * up - zi < yi) { w = wi; bi = up; }
      nact += w != 0.0;
    }
    W[i] = w; B[i] = bi; Y[i] = 0.0;
  }
  nact = (int)wave_sum((double)nact);
  wsync();

  if (!polish_factorize(pl, ws, Lf, Lb, T, W, R, c * delta, S0, S1)) {
    if (lane == 0) {
      po.pstatus[b] = MPCQP_POLISH_LINSYS_ERROR;
      po.pinfo[4L * b] = NAN; po.pinfo[4L * b + 1] = NAN; po.pinfo[4L * b + 2] = NAN; po.pinfo[4L * b + 3] = (double)nact;
    }
    return;
  }

  // ---- 4. one solve from (x, y_a) = 0 and `refine` refinements against the unregularised KKT matrix
  for (int it = 0; it <= po.refine; it++) {
    // r_y = b_a - A_a x;  v = y_a - w o r_y
    ell_rows(pl.A, valA, X, [&](int i, double ax) {
      if (i < mpad) { const double w = W[i], ry = w != 0.0 ? B[i] - ax : 0.0; RY[i] = ry; V[i] = Y[i] - w * ry; }
    });
    // rhs = r_x + A_a'(w o r_y) = -(P x + q) - A'v
    ell_rows(pl.P, valP, X, [&](int t, double px) { if (t < npad) R[t] = -(px + Q[t]); });
    wsync();
    ell_rows(pl.At, valAt, V, [&](int t, double atv) { if (t < npad) R[t] -= atv; });
    wsync();
    run_stream<4>(Lf, pl.fwd_ops, pl.nblk, R);
    run_stream<4>(Lb, pl.bwd_ops, pl.nblk, R);
    // y_a += w o (A_a dx - r_y);  x += dx
    ell_rows(pl.A, valA, R, [&](int i, double adx) { if (i < mpad) Y[i] += W[i] * (adx - RY[i]); });
    for (int t = lane; t < npad; t += WAVE) X[t] += R[t];
    wsync();
  }

  // ---- 5. the candidate: z = clip(A x) and the residuals / objective as update_info() states them
  double pr = 0.0;
  ell_rows(pl.A, valA, X, [&](int i, double ax) {
    if (i < mpad) {
      double zc = 0.0;
      if (i < m) {
        zc = fmin(fmax(ax, lb[i]), ub[i]);
        const double einv = unscale ? 1.0 / Eg[i] : 1.0;
        pr = fmax(pr, fabs(einv * (ax - zc)));
      }
      V[i] = zc;
    }
  });
  ell_rows(pl.P, valP, X, [&](int t, double px) { if (t < npad) R[t] = px; });
  wsync();
  double dr = 0.0, obj = 0.0;
  ell_rows(pl.At, valAt, Y, [&](int t, double aty) {
    if (t < npad) {
      const double dinv = unscale ? 1.0 / Dg[t] : 1.0, px = R[t], qv = Q[t];
      dr = fmax(dr, fabs(dinv * (qv + px + aty)));
      obj += X[t] * (0.5 * px + qv);
    }
  });
  // (a NaN anywhere must reject the candidate: fmax would drop it, so it is carried apart)
  int bad = 0;
  for (int t = lane; t < npad; t += WAVE) bad |= !(fabs(X[t]) < Q_INFTY);
  const double pri_pol = wave_max(pr), dua_pol = unscale ? cinv * wave_max(dr) : wave_max(dr);
  obj = wave_sum(obj);
  if (st.scaling) obj *= cinv;
  bad = __any(bad);

  // ---- 6. OSQP's acceptance rule; 7. write back
  const double pri = po.info[4L * b + 1], dua = po.info[4L * b + 2];
  const bool better = (pri_pol < pri && dua_pol < dua) || (pri_pol < pri && dua < 1e-10) || (dua_pol < dua && pri < 1e-10);
  const bool accept = better && !bad;
  if (accept) {
    double *xo = po.x + (long)b * n, *yo = po.y + (long)b * m, *zo = po.z + (long)b * m;
    for (int j = lane; j < n; j += WAVE) { const int t = pl.pos[j]; xo[j] = Dg[t] * X[t]; }
    for (int i = lane; i < m; i += WAVE) { yo[i] = cinv * Eg[i] * Y[i]; zo[i] = (1.0 / Eg[i]) * V[i]; }
  }
  if (lane == 0) {
    po.pstatus[b] = accept ? MPCQP_POLISH_SUCCESS : MPCQP_POLISH_FAILED;
    po.pinfo[4L * b] = obj; po.pinfo[4L * b + 1] = pri_pol; po.pinfo[4L * b + 2] = dua_pol; po.pinfo[4L * b + 3] = (double)nact;
    if (accept) { po.info[4L * b] = obj; po.info[4L * b + 1] = pri_pol; po.info[4L * b + 2] = dua_pol; }
  }
}
