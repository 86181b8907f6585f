// stage_riccati_ipm.hpp -- the interior-point direct solve of the stage QP behind mpcqp_stage_riccati_solve_ipm (include/mpcqp.h has the rule;
// DESIGN 6.32): iteration 0 is stage_direct_kernel's arithmetic, then up to `iters` primal-dual interior-point iterations over the box rows of the
// free variables, states included.  A barrier term sits on the diagonal of H_k and in q_k and nowhere else, so every iteration is the backward and
// the forward pass of that kernel on modified data; the adjoint pass runs only where an iterate is a candidate.  All iterations run in one launch.
// The passes are copies of stage_riccati.hpp's (not shared device functions: the existing instances keep their code as it is).
#pragma once
#include <hip/hip_runtime.h>
#include "stage_riccati.hpp"

// The size classes, lane groups, tiles and groups per block are stage_dir's.  The workspace holds, per instance, [K_k | kappa_k] as
// stage_direct_kernel's does, then seven arrays of N f doubles: the iterate w, the step dw of the iteration, val of the adjoint pass, and the
// slacks and multipliers t_L, t_U, lambda_L, lambda_U.  Element (k, c) of each is written and, outside the adjoint pass, read by the lane that
// owns column c alone.
inline size_t stage_ipm_ws_doubles(const StageDev &sd) { return (size_t)sd.N * ((size_t)sd.nu * (sd.nx + 1) + 7 * (size_t)sd.f); }

// the butterflies of a lane group; every lane ends with the same bits (the operations commute)
template <int W> __device__ inline double stage_ipm_sum(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, W);
  return v;
}
template <int W> __device__ inline double stage_ipm_max(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) { const double t = __shfl_xor(v, o, W); v = t > v ? t : v; }
  return v;
}
template <int W> __device__ inline double stage_ipm_min(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) { const double t = __shfl_xor(v, o, W); v = t < v ? t : v; }
  return v;
}

// The loop over the iterations is block-uniform: a group whose instance is done (or that never had one) walks every barrier and every shuffle of
// the remaining iterations with its arithmetic and stores masked off, and the block leaves the loop only on a block-wide vote that no group is
// open.  Whether the adjoint pass runs is a block-wide vote too.  One writer per element, no atomics.
// (The second launch bound asks for two waves per SIMD in the <16, 8> class, as stage_direct_active_kernel<16, 8> has.  Here it costs scratch: the
// iteration's state is 60 vector registers more than the class has at that occupancy, 244 bytes per lane.  Measured on the cart-pole workload,
// N = 100 x 16384: 51.9 ms with the bound against 86.3 ms without it (one wave per SIMD, no scratch) -- the second wave hides more than the
// scratch traffic costs, so the bound stays and the spill is recorded in profiles/direct_ipm_kernel_resources.txt.)
template <int W, int FM>
__global__ void __launch_bounds__((stage_dir<W, FM>::G * W), (FM == 8 ? 2 : 1)) stage_direct_ipm_kernel(StageDev sd, int batch, mpcqp_stage_riccati_solve_ipm_args a, StageDirTab tab, double *ws) {
  using C = stage_dir<W, FM>;
  __shared__ double lds[C::G * C::tile];
  const int lane = threadIdx.x % W, g = threadIdx.x / W;
  const long b = (long)blockIdx.x * C::G + g;
  const int nx = sd.nx, nu = sd.nu, f = sd.f, N = sd.N, np = sd.np, n = sd.n, nh = sd.nh, nk = sd.nk, ldv = nx | 1, ldf = f | 1;
  double *V = lds + g * C::tile, *Q = V + nx * ldv, *AB = Q + f * ldf, *T = AB + nx * ldf, *vec = T + nx * ldf;
  double *vv = vec, *gg = vec + FM, *bh = vec + 2 * FM;
  auto X = [&](int k) { return vec + (3 + (k + 3) % 3) * FM; };
  const bool live = b < batch && (!a.frozen || a.frozen[b] == 0);
  const long bb = live ? b : 0;      // (a group without an instance forms no address past the arrays)
  const double *Pb = a.P + bb * sd.nnzP, *Ab = a.A + bb * sd.nnzA, *qb = a.q + bb * n, *lb = a.l + bb * sd.m, *ub = a.u + bb * sd.m;
  const size_t per = (size_t)N * ((size_t)nu * (nx + 1) + 7 * (size_t)f);
  const long Nf = (long)N * f;
  double *KK = ws + bb * per, *Wk = KK + (long)N * nu * (nx + 1), *DW = Wk + Nf, *YV = DW + Nf, *TL = YV + Nf, *TU = TL + Nf, *LL = TU + Nf, *LU = LL + Nf;
  const int rowh = n + (N - 1) * nx, rowk = rowh + N * nh;

  bool el = true;
  unsigned pm = 0;
  if (live) {
    for (int j = lane; j < np; j += W) el = el && lb[j] == 0.0 && ub[j] == 0.0;
    for (int j = lane; j < nx; j += W) el = el && lb[np + j] == ub[np + j];
    for (int j = f + lane; j < N * f; j += W) { const double lo = lb[np + j], hi = ub[np + j]; el = el && lo == lo && hi == hi && !(lo == hi); }
    for (int j = lane; j < (N - 1) * nx; j += W) el = el && lb[n + j] == ub[n + j];
    for (int i = 0; i < nu; i++) {
      const double lo = lb[np + nx + i], hi = ub[np + nx + i];
      el = el && lo == lo && hi == hi;
      if (lo == hi) pm |= 1u << i;
    }
  }
  el = stage_dir_all<W>(el);
  // the barriered sides of column `lane` of frame k: an identity row of a free variable, each finite side on its own
  auto barred = [&](int k) { return k > 0 || (lane >= nx && !((pm >> (lane - nx)) & 1u)); };
  double cnt = 0.0;
  if (live && el && lane < f)
    for (int k = 0; k < N; k++)
      if (barred(k)) { const long j = np + (long)k * f + lane; cnt += (lb[j] > -HUGE_VAL ? 1.0 : 0.0) + (ub[j] < HUGE_VAL ? 1.0 : 0.0); }
  cnt = stage_ipm_sum<W>(cnt);      // (whole numbers: exact in any order)

  double sm = 0.0;      // sigma mu of the iteration at work
  double hq[C::fmax], ha[C::nxmax], qv = 0.0, bv = 0.0, hb = 0.0;
  auto fetch_a = [&](int k) {
    const int *as = tab.aslot + (long)k * nx * f;
    int ea[C::nxmax];
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ea[r] = r < nx && k < N - 1 ? as[r * f + lane] : -1;
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ha[r] = ea[r] >= 0 ? -Ab[ea[r]] : 0.0;
  };
  // barr: the barrier terms of the column join the fetch -- hb goes onto the diagonal of H_k, qv carries the shifted q_k
  auto fetch = [&](int k, bool barr) {
    const int *ps = tab.pslot + (long)k * f * f;
    int eq[C::fmax];
#pragma unroll
    for (int r = 0; r < C::fmax; r++) eq[r] = r < f ? ps[r * f + lane] : -1;
    fetch_a(k);
#pragma unroll
    for (int r = 0; r < C::fmax; r++) hq[r] = eq[r] >= 0 ? Pb[eq[r]] : 0.0;
    qv = qb[np + k * f + lane];
    bv = lane < nx && k < N - 1 ? lb[n + k * nx + lane] : 0.0;
    hb = 0.0;
    if (barr && barred(k)) {
      const long j = np + (long)k * f + lane, o = (long)k * f + lane;
      const double lo = lb[j], hi = ub[j];
      double hL = 0.0, qL = 0.0, hU = 0.0, qU = 0.0;
      if (lo > -HUGE_VAL) { const double t = TL[o], lm = LL[o], r = lm / t; hL = r; qL = -((sm / t + lm) + r * lo); }
      if (hi < HUGE_VAL) { const double t = TU[o], lm = LU[o], r = lm / t; hU = r; qU = (sm / t + lm) - r * hi; }
      hb = hL + hU;
      qv = qv + (qL + qU);
    }
  };
  // the directions of the slacks and multipliers of element o = (k, lane) from the step dwv at the point wv (the rule of the header)
  struct Dir { double tl, tu, ll, lu, dtl, dtu, dll, dlu; bool mL, mU; };
  auto dirs = [&](int k, double wv, double dwv) {
    Dir d{1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false, false};
    if (!barred(k)) return d;
    const long j = np + (long)k * f + lane, o = (long)k * f + lane;
    const double lo = lb[j], hi = ub[j];
    d.mL = lo > -HUGE_VAL; d.mU = hi < HUGE_VAL;
    if (d.mL) { d.tl = TL[o]; d.ll = LL[o]; d.dtl = dwv + ((wv - lo) - d.tl); d.dll = (sm / d.tl - d.ll) - (d.ll / d.tl) * d.dtl; }
    if (d.mU) { d.tu = TU[o]; d.lu = LU[o]; d.dtu = ((hi - wv) - d.tu) - dwv; d.dlu = (sm / d.tu - d.lu) - (d.lu / d.tu) * d.dtu; }
    return d;
  };

  bool open = live && el;      // group-uniform: the instance still needs an iteration
  bool recentre = false;
  int verdict = 0, fin = 0;
  double mu = 0.0, alpha = 1.0, r_pv = 0.0, r_comp = 0.0, r_stat = __builtin_nan("");
  for (int it = 0; it <= a.iters; it++) {
    const bool barr = it > 0;
    sm = (recentre ? 1.0 : alpha >= MPCQP_IPM_ALPHA_SHORT ? MPCQP_IPM_SIGMA : MPCQP_IPM_SIGMA_SHORT) * mu;
    sm = sm > MPCQP_IPM_TARGET * a.comp_tol ? sm : MPCQP_IPM_TARGET * a.comp_tol;      // mu is not driven below what the stop test asks for
    // ---- backwards: K_k and kappa_k to the workspace
    bool failed = false;
    if (open && lane < f) fetch(N - 1, barr);
    for (int k = N - 1; k >= 0; k--) {
      const bool run = open && !failed, last = k == N - 1;
      double *x0 = X(0), *x1 = X(1);
      if (run && lane < f) {
#pragma unroll
        for (int rr = 0; rr < C::fmax; rr++) if (rr < f) Q[rr * ldf + lane] = hq[rr];
        if (barr) Q[lane * ldf + lane] = Q[lane * ldf + lane] + hb;
        if (!last) {
#pragma unroll
          for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) AB[rr * ldf + lane] = ha[rr];
          if (lane < nx) bh[lane] = bv;
        }
        gg[lane] = qv;
      }
      const double qk = qv;
      sm_group_sync();
      if (run && lane < f && k > 0) fetch(k - 1, barr);
      if (!last) {
        if (run && lane < f)
          for (int rr = 0; rr < nx; rr++) {
            double acc = 0.0;
#pragma unroll 4
            for (int j = 0; j < nx; j++) acc += V[rr * ldv + j] * AB[j * ldf + lane];
            T[rr * ldf + lane] = acc;
          }
        if (run && lane < nx) {
          double acc = 0.0;
          for (int i = 0; i < nx; i++) acc += V[lane * ldv + i] * bh[i];
          x0[lane] = acc + vv[lane];
        }
        sm_group_sync();
        if (run && lane < f) {
          for (int rr = 0; rr <= lane; rr++) {
            double acc = 0.0;
#pragma unroll 4
            for (int j = 0; j < nx; j++) acc += AB[j * ldf + rr] * T[j * ldf + lane];
            const double qq = Q[rr * ldf + lane] + acc;
            Q[rr * ldf + lane] = qq; Q[lane * ldf + rr] = qq;
          }
          double acc = 0.0;
          for (int j = 0; j < nx; j++) acc += AB[j * ldf + lane] * x0[j];
          gg[lane] = qk + acc;
        }
        sm_group_sync();
      }
      // the pins of frame 0 and reg: lane c rewrites its column of the input rows (and its own entry of g)
      const unsigned cm = k == 0 ? pm : 0u;
      if (run && lane < f) {
        if (lane < nx) {
          for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) Q[(nx + i) * ldf + lane] = 0.0;
        } else {
          const int ic = lane - nx;
          const bool cc = (cm >> ic) & 1u;
          if (cc) gg[lane] = -lb[np + lane];
          else if (cm) {
            double acc = 0.0;
            for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) acc += Q[(nx + i) * ldf + lane] * lb[np + nx + i];
            gg[lane] += acc;
          }
          for (int i = 0; i < nu; i++) if (cc || ((cm >> i) & 1u)) Q[(nx + i) * ldf + lane] = i == ic ? 1.0 : 0.0;
          if (!cc) Q[lane * ldf + lane] += a.reg;
        }
      }
      sm_group_sync();
      double dmax = 1.0;
      if (run)
        for (int i = 0; i < nu; i++) { const double v = fabs(Q[(nx + i) * ldf + nx + i]); dmax = v > dmax ? v : dmax; }
      const double thr = MPCQP_RICCATI_PIVOT * dmax;
      bool bad = false;
      for (int jj = 0; jj < nu; jj++) {
        if (run && !bad) {
          const double *Mj = Q + (nx + jj) * ldf;
          double acc = 0.0;
          for (int t = 0; t < jj; t++) { const double v = Q[(nx + t) * ldf + nx + jj]; acc += v * v; }
          const double d = Mj[nx + jj] - acc;
          if (!(d > thr)) bad = true;
          else {
            const double ujj = sqrt(d);
            if (lane == nx + jj) {
              AB[jj] = ujj;
              double s = 0.0;
              for (int t = 0; t < jj; t++) s += Q[(nx + t) * ldf + nx + jj] * gg[nx + t];
              gg[lane] = (gg[lane] - s) / ujj;
            }
            if (lane < nx || (lane > nx + jj && lane < f)) {
              double s = 0.0;
              for (int t = 0; t < jj; t++) s += Q[(nx + t) * ldf + nx + jj] * Q[(nx + t) * ldf + lane];
              Q[(nx + jj) * ldf + lane] = (Mj[lane] - s) / ujj;
            }
          }
        }
        sm_group_sync();
      }
      if (run && bad) failed = true;
      const bool ok = run && !bad;
      if (ok && lane < nx) {
        for (int i = nu - 1; i >= 0; i--) {
          double s = 0.0;
          for (int t = i + 1; t < nu; t++) s += Q[(nx + i) * ldf + nx + t] * T[t * nx + lane];
          const double zz = (Q[(nx + i) * ldf + lane] - s) / AB[i];
          T[i * nx + lane] = zz;
          KK[((long)k * nu + i) * (nx + 1) + lane] = -zz;
        }
        if (k > 0) {
          for (int rr = 0; rr <= lane; rr++) {
            double acc = 0.0;
            for (int i = 0; i < nu; i++) acc += Q[(nx + i) * ldf + rr] * Q[(nx + i) * ldf + lane];
            const double v = Q[rr * ldf + lane] - acc;
            V[rr * ldv + lane] = v; V[lane * ldv + rr] = v;
          }
          double acc = 0.0;
          for (int i = 0; i < nu; i++) acc += Q[(nx + i) * ldf + lane] * gg[nx + i];
          vv[lane] = gg[lane] - acc;
        }
      }
      if (ok && lane == nx)
        for (int i = nu - 1; i >= 0; i--) {
          double s = 0.0;
          for (int t = i + 1; t < nu; t++) s += Q[(nx + i) * ldf + nx + t] * x1[t];
          const double zz = (gg[nx + i] - s) / AB[i];
          x1[i] = zz;
          KK[((long)k * nu + i) * (nx + 1) + nx] = -zz;
        }
      sm_group_sync();
    }

    // ---- forwards.  Iteration 0: the point w0 to the workspace, its box rows tested.  Later: the step dw = w+ - w to the workspace and the
    // ---- running minimum of the ratios -v / dv over the slacks and multipliers whose direction is negative
    const bool run = open && !failed;
    bool inb = true;
    double amin = HUGE_VAL, pvl = 0.0;
    if (run && lane < nx) X(0)[lane] = lb[np + lane];
    if (run && lane < f) fetch_a(0);
    for (int k = 0; k < N; k++) {
      double *dc = X(k), *dn = X(k + 1);
      if (run && lane < f && k < N - 1) {
#pragma unroll
        for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) AB[rr * ldf + lane] = ha[rr];
      }
      sm_group_sync();
      if (run && lane < f && k + 1 < N - 1) fetch_a(k + 1);
      if (run && lane >= nx && lane < f) {
        const int i = lane - nx;
        const double *Kr = KK + ((long)k * nu + i) * (nx + 1);
        double acc = 0.0;
        for (int j = 0; j < nx; j++) acc += Kr[j] * dc[j];
        double uv = acc + Kr[nx];
        if (k == 0 && ((pm >> i) & 1u)) uv = lb[np + lane];
        dc[lane] = uv;
      }
      sm_group_sync();
      if (run && lane < f) {
        const double dv = dc[lane];
        const long o = (long)k * f + lane;
        if (it == 0) {
          Wk[o] = dv;
          if (barred(k)) {
            const double lo = lb[np + o], hi = ub[np + o];
            inb = inb && lo - a.feas_tol <= dv && dv <= hi + a.feas_tol;
            const double va = lo > -HUGE_VAL ? lo - dv : 0.0, vb = hi < HUGE_VAL ? dv - hi : 0.0;
            pvl = va > pvl ? va : pvl; pvl = vb > pvl ? vb : pvl;
          }
        } else {
          const double wv = Wk[o], dwv = dv - wv;
          DW[o] = dwv;
          const Dir d = dirs(k, wv, dwv);
          if (d.mL) {
            if (d.dtl < 0.0) { const double r = -d.tl / d.dtl; amin = r < amin ? r : amin; }
            if (d.dll < 0.0) { const double r = -d.ll / d.dll; amin = r < amin ? r : amin; }
          }
          if (d.mU) {
            if (d.dtu < 0.0) { const double r = -d.tu / d.dtu; amin = r < amin ? r : amin; }
            if (d.dlu < 0.0) { const double r = -d.lu / d.dlu; amin = r < amin ? r : amin; }
          }
        }
        if (lane < nx && k < N - 1) {
          double acc = 0.0;
          for (int c = 0; c < f; c++) acc += AB[lane * ldf + c] * dc[c];
          dn[lane] = acc + lb[n + k * nx + lane];
        }
      }
      sm_group_sync();
    }
    amin = stage_ipm_min<W>(amin) * MPCQP_IPM_FRAC;
    const double alpha_n = amin < 1.0 ? amin : 1.0;
    const bool lost = it > 0 && !(alpha_n > 0.0 && alpha_n <= 1.0);
    bool boxok = stage_dir_all<W>(inb);

    // ---- the state.  Iteration 0, box violated: the start.  Later: the update by alpha; mu, max lambda t, the violation and the box test at the
    // ---- new point.  Every element by the lane of its column, no barrier.
    const bool upd = run && !lost && (it > 0 || !boxok);
    double s_l = 0.0, c_l = 0.0;
    if (upd) {
      double s = 0.0, cmx = 0.0;
      bool in2 = true;
      if (it > 0) pvl = 0.0;
      if (lane < f)
        for (int k = 0; k < N; k++) {
          if (!barred(k) && it == 0) continue;
          const long o = (long)k * f + lane;
          const double lo = lb[np + o], hi = ub[np + o];
          double pa = 0.0, pb = 0.0;
          if (it == 0) {
            const double dv = Wk[o];
            if (lo > -HUGE_VAL) { const double sl = dv - lo, t = sl > MPCQP_IPM_T0 ? sl : MPCQP_IPM_T0, lm = MPCQP_IPM_MU0 / t; TL[o] = t; LL[o] = lm; pa = lm * t; }
            if (hi < HUGE_VAL) { const double su = hi - dv, t = su > MPCQP_IPM_T0 ? su : MPCQP_IPM_T0, lm = MPCQP_IPM_MU0 / t; TU[o] = t; LU[o] = lm; pb = lm * t; }
          } else {
            const double wv = Wk[o], dwv = DW[o];
            const Dir d = dirs(k, wv, dwv);
            const double wn = wv + alpha_n * dwv;
            Wk[o] = wn;
            if (d.mL) { const double t = d.tl + alpha_n * d.dtl, lm = d.ll + alpha_n * d.dll; TL[o] = t; LL[o] = lm; pa = lm * t; const double va = lo - wn; pvl = va > pvl ? va : pvl; }
            if (d.mU) { const double t = d.tu + alpha_n * d.dtu, lm = d.lu + alpha_n * d.dlu; TU[o] = t; LU[o] = lm; pb = lm * t; const double vb = wn - hi; pvl = vb > pvl ? vb : pvl; }
            if (barred(k)) in2 = in2 && lo - a.feas_tol <= wn && wn <= hi + a.feas_tol;
          }
          s = s + pa; s = s + pb;
          cmx = pa > cmx ? pa : cmx; cmx = pb > cmx ? pb : cmx;
        }
      inb = in2;
      s_l = s; c_l = cmx;
    }
    const double s_g = stage_ipm_sum<W>(s_l), comp = stage_ipm_max<W>(c_l), p_g = stage_ipm_max<W>(pvl);
    const bool i_g = stage_dir_all<W>(inb);
    if (upd) {
      mu = s_g / cnt;
      if (it > 0) { alpha = alpha_n; boxok = i_g; r_comp = comp; r_stat = __builtin_nan(""); }
    }
    if (run && (it == 0 || upd)) r_pv = p_g;

    // ---- a candidate: the adjoint recursion backwards at the iterate, val to the workspace; what is left on the free input columns; the path
    // ---- and the link rows at the iterate
    const bool cand = run && !lost && boxok && (it == 0 || (comp <= a.comp_tol && mu <= a.comp_tol));
    bool rows = true;
    double stat = 0.0;
    if (__syncthreads_or(cand ? 1 : 0)) {
      if (cand && lane < f) fetch(N - 1, false);
      for (int k = N - 1; k >= 0; k--) {
        double *dc = X(k), *dn = X(k + 1), *lk = (k & 1) ? vv : gg, *lm = (k & 1) ? gg : vv;
        if (cand && lane < f) dc[lane] = Wk[(long)k * f + lane];
        sm_group_sync();
        if (cand && lane < f) {
          double e = 0.0;
#pragma unroll
          for (int rr = 0; rr < C::fmax; rr++) if (rr < f) e += hq[rr] * dc[rr];
          e += qv;
          double t = 0.0;
          if (k < N - 1) {
#pragma unroll
            for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) t += ha[rr] * lk[rr];
          }
          double val = t - e;
          const bool br = barred(k);
          if (it > 0 && br) {
            const long o = (long)k * f + lane;
            const double yid = (ub[np + o] < HUGE_VAL ? LU[o] : 0.0) - (lb[np + o] > -HUGE_VAL ? LL[o] : 0.0);
            val = val - yid;
          }
          if (k >= 1 && lane < nx) lm[lane] = val;
          YV[(long)k * f + lane] = val;
          if (br && lane >= nx) { const double v = fabs(val - a.reg * dc[lane]); stat = v > stat ? v : stat; }      // (reg sits on the free inputs' diagonal)
          if (k > 0) fetch(k - 1, false);
        }
        if (cand) {
          for (int rr = lane; rr < nh; rr += W) {
            const double zv = stage_dir_row(Ab, tab.hslot + ((long)k * nh + rr) * f, dc, f, 0.0);
            const long i = rowh + (long)k * nh + rr;
            rows = rows && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
          }
          if (k < N - 1)
            for (int rr = lane; rr < nk; rr += W) {
              const long o = ((long)k * nk + rr) * f, i = rowk + (long)k * nk + rr;
              const double zv = stage_dir_row(Ab, tab.k1slot + o, dn, f, stage_dir_row(Ab, tab.k0slot + o, dc, f, 0.0));
              rows = rows && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
            }
        }
      }
      stat = stage_ipm_max<W>(stat);
      rows = stage_dir_all<W>(rows);
    }

    // ---- the verdict of the iteration (group-uniform)
    if (open) {
      bool again = false;
      if (failed) { verdict = it == 0 ? -2 : 0; open = false; }
      else if (lost) open = false;
      else if (cand) {
        r_stat = stat;
        if (!rows) open = false;
        else if (it == 0 || stat <= a.stat_tol) { verdict = 1; open = false; }
        else again = true;
      }
      if (open && it == a.iters) open = false;
      fin = it;
      recentre = again;
    }
    if (__syncthreads_and(open ? 0 : 1)) break;
  }

  // ---- write-out: w, y, z of an accepted instance from the workspace (no barrier: every read is behind one)
  const bool wr = live && el && verdict == 1;
  if (wr) {
    for (int k = 0; k < N; k++) {
      const double *dc = Wk + (long)k * f, *dn = dc + f;
      if (lane < f) {
        const long o = (long)k * f + lane, j = np + o;
        const double dv = dc[lane], val = YV[o];
        a.w[b * n + j] = dv;
        if (a.z) a.z[b * sd.m + j] = dv;
        double yj = val;      // frame 0's pinned rows close their own columns
        if (barred(k)) yj = fin == 0 ? 0.0 : (ub[j] < HUGE_VAL ? LU[o] : 0.0) - (lb[j] > -HUGE_VAL ? LL[o] : 0.0);
        a.y[b * sd.m + j] = yj;
        if (k >= 1 && lane < nx) {
          const long i = n + (long)(k - 1) * nx + lane;
          a.y[b * sd.m + i] = val;
          if (a.z) a.z[b * sd.m + i] = lb[i];
        }
      }
      for (int rr = lane; rr < nh; rr += W) {
        const long i = rowh + (long)k * nh + rr;
        a.y[b * sd.m + i] = 0.0;
        if (a.z) a.z[b * sd.m + i] = stage_dir_row(Ab, tab.hslot + ((long)k * nh + rr) * f, dc, f, 0.0);
      }
      if (k < N - 1)
        for (int rr = lane; rr < nk; rr += W) {
          const long o = ((long)k * nk + rr) * f, i = rowk + (long)k * nk + rr;
          a.y[b * sd.m + i] = 0.0;
          if (a.z) a.z[b * sd.m + i] = stage_dir_row(Ab, tab.k1slot + o, dn, f, stage_dir_row(Ab, tab.k0slot + o, dc, f, 0.0));
        }
    }
    for (int j = lane; j < np; j += W) {
      double acc = 0.0;
      for (int e = tab.pcp[j]; e < tab.pcp[j + 1]; e++) acc += Pb[tab.pcs[e]] * Wk[tab.pcr[e]];
      a.y[b * sd.m + j] = -(acc + qb[j]);
      a.w[b * n + j] = 0.0;
      if (a.z) a.z[b * sd.m + j] = 0.0;
    }
  }
  // an ineligible or failed instance writes its verdict alone
  if (live && el && verdict != -2 && lane == 0) {
    if (a.iters_used) a.iters_used[b] = fin;
    if (a.res) { a.res[b * 3] = r_pv; a.res[b * 3 + 1] = r_comp; a.res[b * 3 + 2] = r_stat; }
  }
  if (live && lane == 0) a.direct[b] = !el ? -1 : verdict;
}

template <int W, int FM>
inline hipError_t stage_launch_direct_ipm(const StageDev &sd, int batch, const mpcqp_stage_riccati_solve_ipm_args &a, const StageDirTab &tab, double *ws, hipStream_t st) {
  using C = stage_dir<W, FM>;
  stage_direct_ipm_kernel<W, FM><<<(unsigned)((batch + C::G - 1) / C::G), C::G * W, 0, st>>>(sd, batch, a, tab, ws);
  return hipGetLastError();
}
