// stage_riccati.hpp -- the backward Riccati sweep behind mpcqp_stage_riccati and the feedback law of mpcqp_stage_feedback (include/mpcqp.h has the
// rule).  Not templated on the model: the sizes come from StageDev, the data from the local system mpcqp_stage_eval wrote, so the
// kernels live in libmpcqp.so only and serve zoo, generated and tracking handles alike.
#pragma once
#include <hip/hip_runtime.h>
#include "stage_kernels.hpp"

// One group of W lanes per instance in one of three size classes <W, FM>, FM the largest f the class holds: <16, 8> (f <= 8: the double
// integrator, the cart-pole), <16, 16> (f <= 16: the quadrotor) and <32, 24>; nx <= FM - 1, at most SM_MAXNX.  A block holds as many groups as
// 48 KB of static LDS and 256 threads allow, always whole waves.  Per group, in LDS because they are indexed at run time (as registers they would
// be scratch):
//   V [nx x nx] the value matrix of the frame above, Q [f x f], AB [nx x f] = [A_k B_k], T [nx x f] = V AB (later the back substitution's z).
// Rows are padded to an odd number of doubles (ld = n | 1): the mirrored stores walk a column, and an odd stride spreads them over the banks.  A
// W = 16 tile is 16 doubles modulo 32 long, so the two groups of a 32-lane half read opposite halves of the 64-bank row.
template <int W, int FM> struct stage_ric {
  static constexpr int fmax = FM, nxmax = FM - 1 < SM_MAXNX ? FM - 1 : SM_MAXNX;
  static constexpr int need = nxmax * (nxmax | 1) + fmax * (fmax | 1) + 2 * nxmax * (fmax | 1);      // doubles per group at the largest sizes
  static constexpr int tile = W == 16 ? ((need + 15) / 32) * 32 + 16 : need;
  static constexpr int fit = (48 * 1024) / (tile * 8), per_wave = 64 / W;
  static constexpr int waves = fit / per_wave >= 4 ? 4 : fit / per_wave >= 1 ? fit / per_wave : 1;
  static constexpr int G = waves * per_wave;                          // groups per block
  static_assert(FM <= W && FM <= SM_MAXNX + SM_MAXNU, "a lane per column of the frame");
  static_assert(tile >= need, "a group's tiles fit its share");
  static_assert(G * tile * 8 <= 48 * 1024, "the tiles of a block fit 48 KB of static LDS");
};

// what the handle lends a launch (device memory): pslot [N f f], the slot of P that holds H_k[r][c]; aslot [(N-1) nx f], the slot of A that holds
// -[A_k B_k][r][c]; -1 marks a structural zero
struct StageRicTab { const int *pslot, *aslot; };

// Every group of the block reaches every barrier: N, nx and nu are the same for the whole block, and a group without work -- past the batch, frozen,
// or below a failed frame -- walks the loop with its arithmetic and stores masked off.  Lane c owns column c of every tile it writes (and, for
// the mirrored entries, row c below the diagonal), so no element has two writers.
template <int W, int FM>
__global__ void __launch_bounds__((stage_ric<W, FM>::G * W)) stage_riccati_kernel(StageDev sd, int batch, mpcqp_stage_riccati_args a, StageRicTab tab) {
  using C = stage_ric<W, FM>;
  __shared__ double lds[C::G * C::tile];
  const int lane = threadIdx.x % W, g = threadIdx.x / W;
  const long b = (long)blockIdx.x * C::G + g;
  const int nx = sd.nx, nu = sd.nu, f = sd.f, N = sd.N, ldv = nx | 1, ldf = f | 1;
  double *V = lds + g * C::tile, *Q = V + nx * ldv, *AB = Q + f * ldf, *T = AB + nx * ldf;
  const bool live = b < batch && (!a.frozen || a.frozen[b] == 0);
  const double *Pb = a.P + b * sd.nnzP, *Ab = a.A + b * sd.nnzA;
  double *Kb = a.K + b * N * nu * nx, *Vb = a.V ? a.V + b * N * nx * nx : nullptr;
  // Frame k's column of H_k and of [A_k B_k] waits in registers (statically indexed: the loops run to the class's sizes under a guard) while
  // frame k + 1 is worked on: the loads through the slot tables are issued a frame ahead, right behind the barrier that publishes the tiles, so
  // their latency is hidden behind a frame of LDS work and not paid in front of every frame.
  double hq[C::fmax], ha[C::nxmax];
  auto fetch = [&](int k) {
    const int *ps = tab.pslot + (long)k * f * f, *as = tab.aslot + (long)k * nx * f;
    int eq[C::fmax], ea[C::nxmax];
#pragma unroll
    for (int r = 0; r < C::fmax; r++) eq[r] = r < f ? ps[r * f + lane] : -1;
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ea[r] = r < nx && k < N - 1 ? as[r * f + lane] : -1;
#pragma unroll
    for (int r = 0; r < C::fmax; r++) hq[r] = eq[r] >= 0 ? Pb[eq[r]] : 0.0;
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ha[r] = ea[r] >= 0 ? -Ab[ea[r]] : 0.0;
  };
  const bool loads = live && lane < f;
  if (loads) fetch(N - 1);
  int failed = -1;
  for (int k = N - 1; k >= 0; k--) {
    const bool run = live && failed < 0, last = k == N - 1;
    if (run && lane < f) {
#pragma unroll
      for (int r = 0; r < C::fmax; r++) if (r < f) Q[r * ldf + lane] = hq[r];
      if (!last) {
#pragma unroll
        for (int r = 0; r < C::nxmax; r++) if (r < nx) AB[r * ldf + lane] = ha[r];
      }
    }
    sm_group_sync();
    if (run && lane < f && k > 0) fetch(k - 1);
    if (!last) {
      if (run && lane < f)
        for (int r = 0; r < nx; r++) {
          double acc = 0.0;
#pragma unroll 4
          for (int j = 0; j < nx; j++) acc += V[r * ldv + j] * AB[j * ldf + lane];
          T[r * ldf + lane] = acc;
        }
      sm_group_sync();
      if (run && lane < f)
        for (int r = 0; r <= lane; r++) {
          double acc = 0.0;
#pragma unroll 4
          for (int j = 0; j < nx; j++) acc += AB[j * ldf + r] * T[j * ldf + lane];
          const double q = Q[r * ldf + lane] + acc;
          Q[r * ldf + lane] = q; Q[lane * ldf + r] = q;
        }
      sm_group_sync();
    }
    // clamp and reg: lane c rewrites its column of the input rows
    unsigned cm = 0;
    if (run && a.x) {
      const long o = b * sd.nvar + (long)k * f + nx;
      for (int i = 0; i < nu; i++) {
        const double xv = a.x[o + i];
        if (xv - a.lbx[o + i] <= a.clamp_tol || a.ubx[o + i] - xv <= a.clamp_tol) cm |= 1u << i;
      }
    }
    if (run && lane < f) {
      if (lane < nx) {
        for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) Q[(nx + i) * ldf + lane] = 0.0;
      } else {
        const int ic = lane - nx;
        const bool cc = (cm >> ic) & 1u;
        for (int i = 0; i < nu; i++) if (cc || ((cm >> i) & 1u)) Q[(nx + i) * ldf + lane] = i == ic ? 1.0 : 0.0;
        if (!cc) Q[lane * ldf + lane] += a.reg;
      }
    }
    sm_group_sync();
    // Q_uu = U'U by rows with the forward solve of Q_us riding along: M = the input rows of Q, lane c owns column c; the diagonal of U goes to
    // AB[0 .. nu-1] (free until the next frame's load), so row jj's pivot entry stays readable while the row is being scaled
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
          if (lane == nx + jj) AB[jj] = ujj;
          if (lane < nx || (lane > nx + jj && lane < f)) {
            double s = 0.0;
            for (int t = 0; t < jj; t++) s += Q[(nx + t) * ldf + nx + jj] * Q[(nx + t) * ldf + lane];
            Q[(nx + jj) * ldf + lane] = (Mj[lane] - s) / ujj;
          }
        }
      }
      sm_group_sync();
    }
    if (run && bad) failed = k;
    const bool ok = live && failed < 0;
    if (ok && lane < nx) {
      for (int i = nu - 1; i >= 0; i--) {
        double s = 0.0;
        for (int t = i + 1; t < nu; t++) s += Q[(nx + i) * ldf + nx + t] * T[t * nx + lane];
        const double z = (Q[(nx + i) * ldf + lane] - s) / AB[i];
        T[i * nx + lane] = z;      // (nu nx <= nx ldf doubles: inside T)
        Kb[((long)k * nu + i) * nx + lane] = -z;
      }
      for (int r = 0; r <= lane; r++) {
        double acc = 0.0;
        for (int i = 0; i < nu; i++) acc += Q[(nx + i) * ldf + r] * Q[(nx + i) * ldf + lane];
        const double v = Q[r * ldf + lane] - acc;
        V[r * ldv + lane] = v; V[lane * ldv + r] = v;
      }
    }
    sm_group_sync();
    if (live && lane < nx) {
      if (Vb) for (int r = 0; r < nx; r++) Vb[((long)k * nx + r) * nx + lane] = ok ? V[r * ldv + lane] : 0.0;
      if (!ok) for (int i = 0; i < nu; i++) Kb[((long)k * nu + i) * nx + lane] = 0.0;
    }
  }
  if (live && a.failed && lane == 0) a.failed[b] = failed;
}

// u = clip(u_nom + K_k (s - s_nom)): one thread per (instance, input).  The products and sums are rounded one by one, in the statement's order, so
// the result is bitwise models.StageOCP.feedback's.  A thread reads entries 0 .. nx-1 of its rows and its own input entry and writes entry nx + i.
__global__ void __launch_bounds__(256) stage_feedback_kernel(int batch, int N, int nx, int nu, int nvar, mpcqp_stage_feedback_args a) {
#pragma clang fp contract(off)
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)batch * nu) return;
  const long b = gid / nu;
  const int i = (int)(gid - b * nu);
  const double *Kr = a.K + ((b * N + a.k) * nu + i) * nx, *s = a.s + b * a.s_stride, *sn = a.s_nom + b * a.s_nom_stride;
  double acc = 0.0;
  for (int j = 0; j < nx; j++) {
    const double e = s[j] - sn[j];
    const double pr = Kr[j] * e;
    acc = acc + pr;
  }
  const double un = a.u_nom[b * a.u_nom_stride + i];
  double u = un + acc;
  if (a.lo) { const double l = a.lo[b * a.lo_stride + i], h = a.hi[b * a.hi_stride + i]; u = u < l ? l : u; u = u > h ? h : u; }
  const long o = b * nvar + nx + i;
  a.x_out[o] = u;
  if (a.lbx) { a.lbx[o] = u; a.ubx[o] = u; }
  if (a.du) a.du[gid] = u - un;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The direct solve of the stage QP behind mpcqp_stage_riccati_solve (include/mpcqp.h has the rule): the sweep above with its affine
// terms, then the step forwards, the multipliers backwards and the test against every inequality row, by the same group in the same kernel.
// The size classes and the tiles are those of stage_ric; behind T a group holds six vectors of FM doubles:
//   v the value gradient of the frame above (adjoint pass: lambda of the odd frames), g = [g_s; g_u -> y0] (adjoint pass: lambda of the even
//   frames), b_k, and three that rotate -- backwards x0 = V b + v and x1 = the back substitution of kappa; forwards and in the adjoint pass
//   d_{k-1}, d_k, d_{k+1}, so that a row over two frames is read while the next frame is being written.
// The classes keep their groups per block (static_assert), so stage_eval.riccati_groups_per_block holds for both kernels.
template <int W, int FM> struct stage_dir {
  using R = stage_ric<W, FM>;
  static constexpr int fmax = FM, nxmax = R::nxmax, nvec = 6;
  static constexpr int need = R::need + nvec * fmax;
  static constexpr int tile = W == 16 ? ((need + 15) / 32) * 32 + 16 : need;
  static constexpr int fit = (48 * 1024) / (tile * 8), per_wave = 64 / W;
  static constexpr int waves = fit / per_wave >= 4 ? 4 : fit / per_wave >= 1 ? fit / per_wave : 1;
  static constexpr int G = waves * per_wave;
  static_assert(G == R::G, "the direct solve keeps the sweep's groups per block");
  static_assert(tile >= need, "a group's tiles fit its share");
  static_assert(G * tile * 8 <= 48 * 1024, "the tiles of a block fit 48 KB of static LDS");
};

// what the handle lends a launch on top of StageRicTab: hslot [N nh f], k0slot and k1slot [(N-1) nk f], the slots of A that hold the path rows'
// and the link rows' entries over frame k (and, for k1slot, over frame k + 1), -1 a structural zero; the parameter columns of P below the
// parameter rows as a compressed list: column j's entries are pcp[j] .. pcp[j+1]-1, entry e sits in slot pcs[e] of P and row np + pcr[e]
struct StageDirTab { const int *pslot, *aslot, *hslot, *k0slot, *k1slot, *pcp, *pcs, *pcr; };

// acc + the entries of one row of A over one frame, in ascending column order (a structural zero is skipped)
__device__ inline double stage_dir_row(const double *Ab, const int *slot, const double *d, int f, double acc) {
  for (int c = 0; c < f; c++) { const int e = slot[c]; if (e >= 0) acc += Ab[e] * d[c]; }
  return acc;
}
template <int W> __device__ inline bool stage_dir_all(bool v) {
  int e = v ? 1 : 0;
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) e &= __shfl_xor(e, o, W);
  return e != 0;
}

// ws: per instance N nu (nx + 1) doubles [K_k | kappa_k], (k, i, j) row-major, then N f doubles, the step d_k.  Written and read by the instance's
// own group only, with block barriers in between.  Every group reaches every barrier of the three passes: an instance that is past the batch,
// frozen, ineligible or failed walks them with its arithmetic and stores masked off.
template <int W, int FM>
__global__ void __launch_bounds__((stage_dir<W, FM>::G * W)) stage_direct_kernel(StageDev sd, int batch, mpcqp_stage_riccati_solve_args a, StageDirTab tab, double *ws) {
  using C = stage_dir<W, FM>;
  __shared__ double lds[C::G * C::tile];
  const int lane = threadIdx.x % W, g = threadIdx.x / W;
  const long b = (long)blockIdx.x * C::G + g;
  const int nx = sd.nx, nu = sd.nu, f = sd.f, N = sd.N, np = sd.np, n = sd.n, nh = sd.nh, nk = sd.nk, ldv = nx | 1, ldf = f | 1;
  double *V = lds + g * C::tile, *Q = V + nx * ldv, *AB = Q + f * ldf, *T = AB + nx * ldf, *vec = T + nx * ldf;
  double *vv = vec, *gg = vec + FM, *bh = vec + 2 * FM;
  auto X = [&](int k) { return vec + (3 + (k + 3) % 3) * FM; };
  const bool live = b < batch && (!a.frozen || a.frozen[b] == 0);
  const double *Pb = a.P + b * sd.nnzP, *Ab = a.A + b * sd.nnzA, *qb = a.q + b * n, *lb = a.l + b * sd.m, *ub = a.u + b * sd.m;
  double *KK = ws + b * ((long)N * (nu * (nx + 1) + f)), *D = KK + (long)N * nu * (nx + 1);
  const int rowh = n + (N - 1) * nx, rowk = rowh + N * nh;       // the first path row, the first link row

  // eligibility, read from l and u alone; pm: the pinned inputs of frame 0
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

  double hq[C::fmax], ha[C::nxmax], qv = 0.0, bv = 0.0;
  auto fetch_a = [&](int k) {
    const int *as = tab.aslot + (long)k * nx * f;
    int ea[C::nxmax];
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ea[r] = r < nx && k < N - 1 ? as[r * f + lane] : -1;
#pragma unroll
    for (int r = 0; r < C::nxmax; r++) ha[r] = ea[r] >= 0 ? -Ab[ea[r]] : 0.0;
  };
  auto fetch = [&](int k) {
    const int *ps = tab.pslot + (long)k * f * f;
    int eq[C::fmax];
#pragma unroll
    for (int r = 0; r < C::fmax; r++) eq[r] = r < f ? ps[r * f + lane] : -1;
    fetch_a(k);
#pragma unroll
    for (int r = 0; r < C::fmax; r++) hq[r] = eq[r] >= 0 ? Pb[eq[r]] : 0.0;
    qv = qb[np + k * f + lane];
    bv = lane < nx && k < N - 1 ? lb[n + k * nx + lane] : 0.0;
  };

  // ---- backwards: K_k and kappa_k to the workspace
  bool failed = false;
  if (live && el && lane < f) fetch(N - 1);
  for (int k = N - 1; k >= 0; k--) {
    const bool run = live && el && !failed, last = k == N - 1;
    double *x0 = X(0), *x1 = X(1);
    if (run && lane < f) {
#pragma unroll
      for (int r = 0; r < C::fmax; r++) if (r < f) Q[r * ldf + lane] = hq[r];
      if (!last) {
#pragma unroll
        for (int r = 0; r < C::nxmax; r++) if (r < nx) AB[r * ldf + lane] = ha[r];
        if (lane < nx) bh[lane] = bv;
      }
      gg[lane] = qv;
    }
    const double qk = qv;
    sm_group_sync();
    if (run && lane < f && k > 0) fetch(k - 1);
    if (!last) {
      if (run && lane < f)
        for (int r = 0; r < nx; r++) {
          double acc = 0.0;
#pragma unroll 4
          for (int j = 0; j < nx; j++) acc += V[r * ldv + j] * AB[j * ldf + lane];
          T[r * ldf + lane] = acc;
        }
      if (run && lane < nx) {
        double acc = 0.0;
        for (int i = 0; i < nx; i++) acc += V[lane * ldv + i] * bh[i];
        x0[lane] = acc + vv[lane];
      }
      sm_group_sync();
      if (run && lane < f) {
        for (int r = 0; r <= lane; r++) {
          double acc = 0.0;
#pragma unroll 4
          for (int j = 0; j < nx; j++) acc += AB[j * ldf + r] * T[j * ldf + lane];
          const double q = Q[r * ldf + lane] + acc;
          Q[r * ldf + lane] = q; Q[lane * ldf + r] = q;
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
        const double z = (Q[(nx + i) * ldf + lane] - s) / AB[i];
        T[i * nx + lane] = z;
        KK[((long)k * nu + i) * (nx + 1) + lane] = -z;
      }
      if (k > 0) {
        for (int r = 0; r <= lane; r++) {
          double acc = 0.0;
          for (int i = 0; i < nu; i++) acc += Q[(nx + i) * ldf + r] * Q[(nx + i) * ldf + lane];
          const double v = Q[r * ldf + lane] - acc;
          V[r * ldv + lane] = v; V[lane * ldv + r] = v;
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
        const double z = (gg[nx + i] - s) / AB[i];
        x1[i] = z;
        KK[((long)k * nu + i) * (nx + 1) + nx] = -z;
      }
    sm_group_sync();
  }

  // ---- forwards: the step d_k to the workspace, every inequality row tested as soon as its frames are known
  const bool run = live && el && !failed;
  bool inb = true;
  if (run && lane < nx) X(0)[lane] = lb[np + lane];
  if (run && lane < f) fetch_a(0);
  for (int k = 0; k < N; k++) {
    double *dc = X(k), *dn = X(k + 1), *dp = X(k - 1);
    if (run && lane < f && k < N - 1) {
#pragma unroll
      for (int r = 0; r < C::nxmax; r++) if (r < nx) AB[r * ldf + lane] = ha[r];
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
      D[(long)k * f + lane] = dv;
      if (k > 0 || (lane >= nx && !((pm >> (lane - nx)) & 1u))) {
        const long j = np + (long)k * f + lane;
        inb = inb && lb[j] - a.feas_tol <= dv && dv <= ub[j] + a.feas_tol;
      }
      if (lane < nx && k < N - 1) {
        double acc = 0.0;
        for (int c = 0; c < f; c++) acc += AB[lane * ldf + c] * dc[c];
        dn[lane] = acc + lb[n + k * nx + lane];
      }
    }
    if (run) {
      for (int r = lane; r < nh; r += W) {
        const double zv = stage_dir_row(Ab, tab.hslot + ((long)k * nh + r) * f, dc, f, 0.0);
        const long i = rowh + (long)k * nh + r;
        inb = inb && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
      }
      if (k >= 1)
        for (int r = lane; r < nk; r += W) {
          const long o = ((long)(k - 1) * nk + r) * f;
          const double zv = stage_dir_row(Ab, tab.k1slot + o, dc, f, stage_dir_row(Ab, tab.k0slot + o, dp, f, 0.0));
          const long i = rowk + (long)(k - 1) * nk + r;
          inb = inb && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
        }
    }
    sm_group_sync();
  }
  const bool wr = stage_dir_all<W>(inb) && run;

  // ---- the adjoint recursion backwards; an accepted instance writes w, y, z as the frames pass
  if (run && lane < f) fetch(N - 1);
  for (int k = N - 1; k >= 0; k--) {
    double *dc = X(k), *dn = X(k + 1), *lk = (k & 1) ? vv : gg, *lm = (k & 1) ? gg : vv;
    if (run && lane < f) dc[lane] = D[(long)k * f + lane];
    sm_group_sync();
    if (run && lane < f) {
      double e = 0.0;
#pragma unroll
      for (int r = 0; r < C::fmax; r++) if (r < f) e += hq[r] * dc[r];
      e += qv;
      double t = 0.0;
      if (k < N - 1) {
#pragma unroll
        for (int r = 0; r < C::nxmax; r++) if (r < nx) t += ha[r] * lk[r];
      }
      const double val = t - e;
      if (k >= 1 && lane < nx) lm[lane] = val;
      if (wr) {
        const long j = np + (long)k * f + lane;
        a.w[b * n + j] = dc[lane];
        if (a.z) a.z[b * sd.m + j] = dc[lane];
        if (k >= 1) {
          a.y[b * sd.m + j] = 0.0;
          if (lane < nx) {
            const long i = n + (long)(k - 1) * nx + lane;
            a.y[b * sd.m + i] = val;
            if (a.z) a.z[b * sd.m + i] = lb[i];
          }
        } else
          a.y[b * sd.m + j] = lane < nx || ((pm >> (lane - nx)) & 1u) ? val : 0.0;
      }
      if (k > 0) fetch(k - 1);
    }
    if (wr) {
      for (int r = lane; r < nh; r += W) {
        const long i = rowh + (long)k * nh + r;
        a.y[b * sd.m + i] = 0.0;
        if (a.z) a.z[b * sd.m + i] = stage_dir_row(Ab, tab.hslot + ((long)k * nh + r) * f, dc, f, 0.0);
      }
      if (k < N - 1)
        for (int r = lane; r < nk; r += W) {
          const long o = ((long)k * nk + r) * f, i = rowk + (long)k * nk + r;
          a.y[b * sd.m + i] = 0.0;
          if (a.z) a.z[b * sd.m + i] = stage_dir_row(Ab, tab.k1slot + o, dn, f, stage_dir_row(Ab, tab.k0slot + o, dc, f, 0.0));
        }
    }
  }
  // the parameter rows close their own columns: -(P w + q)_j over the frame rows of column j (dp = 0)
  if (wr)
    for (int j = lane; j < np; j += W) {
      double acc = 0.0;
      for (int e = tab.pcp[j]; e < tab.pcp[j + 1]; e++) acc += Pb[tab.pcs[e]] * D[tab.pcr[e]];
      a.y[b * sd.m + j] = -(acc + qb[j]);
      a.w[b * n + j] = 0.0;
      if (a.z) a.z[b * sd.m + j] = 0.0;
    }
  if (live && lane == 0) a.direct[b] = !el ? -1 : failed ? -2 : wr ? 1 : 0;
}

template <int W, int FM>
inline hipError_t stage_launch_direct(const StageDev &sd, int batch, const mpcqp_stage_riccati_solve_args &a, const StageDirTab &tab, double *ws, hipStream_t st) {
  using C = stage_dir<W, FM>;
  stage_direct_kernel<W, FM><<<(unsigned)((batch + C::G - 1) / C::G), C::G * W, 0, st>>>(sd, batch, a, tab, ws);
  return hipGetLastError();
}

template <int W, int FM>
inline hipError_t stage_launch_riccati(const StageDev &sd, int batch, const mpcqp_stage_riccati_args &a, const StageRicTab &tab, hipStream_t st) {
  using C = stage_ric<W, FM>;
  stage_riccati_kernel<W, FM><<<(unsigned)((batch + C::G - 1) / C::G), C::G * W, 0, st>>>(sd, batch, a, tab);
  return hipGetLastError();
}
