// stage_riccati_active.hpp -- the direct solve of the stage QP with held input bounds behind mpcqp_stage_riccati_solve_active (include/mpcqp.h has
// the rule): round 0 is stage_direct_kernel's arithmetic, then up to `rounds` primal-dual active-set rounds over the input box rows,
// every round the three passes of that kernel with the held inputs of every frame treated as frame 0's pins are.  All rounds run in one launch.
// The passes are copies of stage_riccati.hpp's (not shared device functions: the existing instances keep their code as it is).
#pragma once
#include <hip/hip_runtime.h>
#include "stage_riccati.hpp"

// The size classes, lane groups, tiles and groups per block are stage_dir's.  The workspace holds, per instance, what stage_direct_kernel's does
// ([K_k | kappa_k], d_k) plus N f doubles for the adjoint pass's val (an instance is accepted only after that pass, so w, y, z are written by a
// pass of their own) and two arrays of N words, the set of the round at work and the one being formed: bit i = input i held at its lower bound,
// bit 8 + i = at its upper bound (SM_MAXNU = 8).
static_assert(SM_MAXNU <= 8, "a frame's held inputs fit two bytes of a word");
inline size_t stage_act_ws_doubles(const StageDev &sd) { return (size_t)sd.N * ((size_t)sd.nu * (sd.nx + 1) + 2 * (size_t)sd.f + 1); }

template <int W> __device__ inline unsigned stage_act_or(unsigned v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v |= __shfl_xor(v, o, W);
  return v;
}

// The loop over the rounds is block-uniform: a group whose instance is done (or that never had one) walks every barrier and every shuffle of the
// remaining rounds with its arithmetic and stores masked off, and the block leaves the loop only on a block-wide vote that no group is open.
// The set words are written by lane 0 of the instance's own group and read by that group behind a block barrier; every other element has the
// one writer it has in stage_direct_kernel.
// (The second launch bound asks for two waves per SIMD in the <16, 8> class, as stage_direct_kernel<16, 8> has: without it the round loop's state
// costs 261 vector registers and the class drops to one; with it 245, still no scratch.)
template <int W, int FM>
__global__ void __launch_bounds__((stage_dir<W, FM>::G * W), (FM == 8 ? 2 : 1)) stage_direct_active_kernel(StageDev sd, int batch, mpcqp_stage_riccati_solve_active_args a, StageDirTab tab, double *ws) {
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
  const size_t per = (size_t)N * ((size_t)nu * (nx + 1) + 2 * (size_t)f + 1);
  double *KK = ws + bb * per, *D = KK + (long)N * nu * (nx + 1), *YV = D + (long)N * f;
  unsigned *S0 = reinterpret_cast<unsigned *>(YV + (long)N * f), *S1 = S0 + N;
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
  // the value a held (or pinned) input i of frame k takes: its u where bit 8 + i of the set word is up, else its l
  auto cv = [&](unsigned sm, int k, int i) { const long j = np + (long)k * f + nx + i; return (sm >> (8 + i)) & 1u ? ub[j] : lb[j]; };

  bool open = live && el;      // group-uniform: the instance still needs a round
  int verdict = 0, fin = 0, cur = 0;
  for (int r = 0; r <= a.rounds; r++) {
    const unsigned *Sc = cur ? S1 : S0;
    unsigned *Sn = cur ? S0 : S1;
    // ---- backwards: K_k and kappa_k to the workspace
    bool failed = false;
    if (open && lane < f) fetch(N - 1);
    for (int k = N - 1; k >= 0; k--) {
      const bool run = open && !failed, last = k == N - 1;
      double *x0 = X(0), *x1 = X(1);
      if (run && lane < f) {
#pragma unroll
        for (int rr = 0; rr < C::fmax; rr++) if (rr < f) Q[rr * ldf + lane] = hq[rr];
        if (!last) {
#pragma unroll
          for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) AB[rr * ldf + lane] = ha[rr];
          if (lane < nx) bh[lane] = bv;
        }
        gg[lane] = qv;
      }
      const double qk = qv;
      sm_group_sync();
      if (run && lane < f && k > 0) fetch(k - 1);
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
      // the held inputs of the frame (frame 0: its pins as well) and reg: lane c rewrites its column of the input rows and its own entry of g
      const unsigned sm = r > 0 && run ? Sc[k] : 0u;
      const unsigned cm = (k == 0 ? pm : 0u) | ((sm | (sm >> 8)) & 0xffu);
      if (run && lane < f) {
        if (lane < nx) {
          if (cm) {
            if (k > 0) {
              double acc = 0.0;
              for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) acc += Q[(nx + i) * ldf + lane] * cv(sm, k, i);
              gg[lane] += acc;
            }
            for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) Q[(nx + i) * ldf + lane] = 0.0;
          }
        } else {
          const int ic = lane - nx;
          const bool cc = (cm >> ic) & 1u;
          if (cc) gg[lane] = -cv(sm, k, ic);
          else if (cm) {
            double acc = 0.0;
            for (int i = 0; i < nu; i++) if ((cm >> i) & 1u) acc += Q[(nx + i) * ldf + lane] * cv(sm, k, i);
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

    // ---- forwards: the step d_k to the workspace; the rows no set repairs, the free inputs' box rows, and the next round's set
    const bool run = open && !failed;
    bool inb = true, hard = true;
    if (run && lane < nx) X(0)[lane] = lb[np + lane];
    if (run && lane < f) fetch_a(0);
    for (int k = 0; k < N; k++) {
      double *dc = X(k), *dn = X(k + 1), *dp = X(k - 1);
      if (run && lane < f && k < N - 1) {
#pragma unroll
        for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) AB[rr * ldf + lane] = ha[rr];
      }
      sm_group_sync();
      if (run && lane < f && k + 1 < N - 1) fetch_a(k + 1);
      const unsigned sm = r > 0 && run ? Sc[k] : 0u;
      const unsigned hm = (k == 0 ? pm : 0u) | ((sm | (sm >> 8)) & 0xffu);
      if (run && lane >= nx && lane < f) {
        const int i = lane - nx;
        const double *Kr = KK + ((long)k * nu + i) * (nx + 1);
        double acc = 0.0;
        for (int j = 0; j < nx; j++) acc += Kr[j] * dc[j];
        double uv = acc + Kr[nx];
        if ((hm >> i) & 1u) uv = cv(sm, k, i);
        dc[lane] = uv;
      }
      sm_group_sync();
      unsigned nb = 0;
      if (run && lane < f) {
        const double dv = dc[lane];
        D[(long)k * f + lane] = dv;
        const long j = np + (long)k * f + lane;
        if (lane < nx) {
          if (k > 0) hard = hard && lb[j] - a.feas_tol <= dv && dv <= ub[j] + a.feas_tol;
        } else if (!((hm >> (lane - nx)) & 1u)) {
          const int i = lane - nx;
          const double lo = lb[j], hi = ub[j];
          const bool vlo = dv < lo - a.feas_tol, vhi = !vlo && dv > hi + a.feas_tol;
          inb = inb && lo - a.feas_tol <= dv && dv <= hi + a.feas_tol;
          if (vlo) nb = 1u << i;
          else if (vhi) nb = 0x100u << i;
          else if (r == 0 && a.act_in) {
            const int gs = a.act_in[(b * N + k) * nu + i];
            if (gs < 0 && fabs(lo) < HUGE_VAL) nb = 1u << i;
            else if (gs > 0 && fabs(hi) < HUGE_VAL) nb = 0x100u << i;
          }
        }
        if (lane < nx && k < N - 1) {
          double acc = 0.0;
          for (int c = 0; c < f; c++) acc += AB[lane * ldf + c] * dc[c];
          dn[lane] = acc + lb[n + k * nx + lane];
        }
      }
      if (run) {
        for (int rr = lane; rr < nh; rr += W) {
          const double zv = stage_dir_row(Ab, tab.hslot + ((long)k * nh + rr) * f, dc, f, 0.0);
          const long i = rowh + (long)k * nh + rr;
          hard = hard && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
        }
        if (k >= 1)
          for (int rr = lane; rr < nk; rr += W) {
            const long o = ((long)(k - 1) * nk + rr) * f;
            const double zv = stage_dir_row(Ab, tab.k1slot + o, dc, f, stage_dir_row(Ab, tab.k0slot + o, dp, f, 0.0));
            const long i = rowk + (long)(k - 1) * nk + rr;
            hard = hard && lb[i] - a.feas_tol <= zv && zv <= ub[i] + a.feas_tol;
          }
      }
      const unsigned nm = stage_act_or<W>(nb);
      if (run && lane == 0) Sn[k] = sm | nm;
      sm_group_sync();
    }
    const bool hopeless = !stage_dir_all<W>(hard), primal = stage_dir_all<W>(inb);

    // ---- the adjoint recursion backwards: val to the workspace, the multiplier signs of the held rows, the releases
    const bool adj = run && !hopeless;
    bool dual = true;
    if (adj && lane < f) fetch(N - 1);
    for (int k = N - 1; k >= 0; k--) {
      double *dc = X(k), *lk = (k & 1) ? vv : gg, *lm = (k & 1) ? gg : vv;
      if (adj && lane < f) dc[lane] = D[(long)k * f + lane];
      sm_group_sync();
      const unsigned sm = r > 0 && adj ? Sc[k] : 0u;
      unsigned rb = 0;
      if (adj && lane < f) {
        double e = 0.0;
#pragma unroll
        for (int rr = 0; rr < C::fmax; rr++) if (rr < f) e += hq[rr] * dc[rr];
        e += qv;
        double t = 0.0;
        if (k < N - 1) {
#pragma unroll
          for (int rr = 0; rr < C::nxmax; rr++) if (rr < nx) t += ha[rr] * lk[rr];
        }
        const double val = t - e;
        if (k >= 1 && lane < nx) lm[lane] = val;
        YV[(long)k * f + lane] = val;
        if (lane >= nx) {
          const int i = lane - nx;
          if (((sm >> (8 + i)) & 1u) && !(val >= -a.dual_tol)) rb = 0x101u << i;
          if (((sm >> i) & 1u) && !(val <= a.dual_tol)) rb = 0x101u << i;
        }
        if (k > 0) fetch(k - 1);
      }
      dual = dual && rb == 0;
      const unsigned rm = stage_act_or<W>(rb);
      if (adj && lane == 0 && rm) Sn[k] &= ~rm;
    }
    dual = stage_dir_all<W>(dual);

    // ---- the verdict of the round (group-uniform)
    if (open) {
      if (failed) { verdict = r == 0 ? -2 : 0; open = false; fin = r; }
      else if (hopeless) { open = false; fin = r; }
      else if (primal && dual) { verdict = 1; open = false; fin = r; }
      else if (r == a.rounds) { open = false; fin = r; }
      else cur ^= 1;
    }
    if (__syncthreads_and(!open)) break;
  }

  // ---- write-out: w, y, z of an accepted instance from the workspace of its last round (no barrier: every read is behind one)
  const unsigned *Sf = cur ? S1 : S0;
  const bool wr = live && el && verdict == 1;
  if (wr) {
    for (int k = 0; k < N; k++) {
      const unsigned sm = fin > 0 ? Sf[k] : 0u;
      const unsigned hm = (k == 0 ? pm : 0u) | ((sm | (sm >> 8)) & 0xffu);
      const double *dc = D + (long)k * f, *dn = dc + f;
      if (lane < f) {
        const double dv = dc[lane], val = YV[(long)k * f + lane];
        const long j = np + (long)k * f + lane;
        const bool held = lane >= nx && ((hm >> (lane - nx)) & 1u);
        a.w[b * n + j] = dv;
        if (a.z) a.z[b * sd.m + j] = dv;
        if (k >= 1) {
          a.y[b * sd.m + j] = held ? val : 0.0;
          if (lane < nx) {
            const long i = n + (long)(k - 1) * nx + lane;
            a.y[b * sd.m + i] = val;
            if (a.z) a.z[b * sd.m + i] = lb[i];
          }
        } else
          a.y[b * sd.m + j] = lane < nx || held ? val : 0.0;
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
      for (int e = tab.pcp[j]; e < tab.pcp[j + 1]; e++) acc += Pb[tab.pcs[e]] * D[tab.pcr[e]];
      a.y[b * sd.m + j] = -(acc + qb[j]);
      a.w[b * n + j] = 0.0;
      if (a.z) a.z[b * sd.m + j] = 0.0;
    }
  }
  // the last set formed (the set of the last round the instance ran), the pins of frame 0 left out; an ineligible or failed instance writes neither
  if (live && el && verdict != -2) {
    if (a.act_out && lane >= nx && lane < f) {
      const int i = lane - nx;
      for (int k = 0; k < N; k++) {
        if (k == 0 && ((pm >> i) & 1u)) continue;
        const unsigned sm = fin > 0 ? Sf[k] : 0u;
        a.act_out[(b * N + k) * nu + i] = (sm >> (8 + i)) & 1u ? 1 : (sm >> i) & 1u ? -1 : 0;
      }
    }
    if (a.rounds_used && lane == 0) a.rounds_used[b] = fin;
  }
  if (live && lane == 0) a.direct[b] = !el ? -1 : verdict;
}

template <int W, int FM>
inline hipError_t stage_launch_direct_active(const StageDev &sd, int batch, const mpcqp_stage_riccati_solve_active_args &a, const StageDirTab &tab, double *ws, hipStream_t st) {
  using C = stage_dir<W, FM>;
  stage_direct_active_kernel<W, FM><<<(unsigned)((batch + C::G - 1) / C::G), C::G * W, 0, st>>>(sd, batch, a, tab, ws);
  return hipGetLastError();
}
