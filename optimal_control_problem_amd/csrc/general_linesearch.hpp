// general_linesearch.hpp -- the rule of the per-instance l1-merit backtracking line search of the general NLP path (include/mpcqp.h,
// mpcqp_nlp_linesearch; general_nlp.GeneralNLP.line_search is its NumPy statement), as host/device functions: penalty, merit, slope, acceptance
// test, fallback, and the expression of a candidate point.  general_linesearch_kernel (general_kernels.hpp) and general_host_linesearch (the g++
// build codegen.py generates for checks without a GPU) both compile THIS text, so the two can differ by compiler contraction and libm only.
#pragma once
#include "stage_models.hpp"
#include "../../include/mpcqp.h"

// the statuses after which the QP returned a point: the set mpcqp_launch_step uses
SM_HD bool gn_ls_status_ok(int s) { return s == MPCQP_SOLVED || s == MPCQP_SOLVED_INACCURATE || s == MPCQP_MAX_ITER_REACHED; }
// lanes (or loop turns) the search needs: the base point and `candidates` trial points; the group width is the smallest of 2, 4, 8, 16 that holds them
SM_HD int gn_ls_group_width(int candidates) { return candidates + 1 <= 2 ? 2 : candidates + 1 <= 4 ? 4 : candidates + 1 <= 8 ? 8 : 16; }
// alpha_j = alpha0 beta^j by repeated multiplication, as the statement forms alphas[j] = alphas[j - 1] * beta
SM_HD double gn_ls_alpha(double alpha0, double beta, int j) {
  double a = alpha0;
  for (int i = 0; i < j; i++) a *= beta;
  return a;
}
// x + alpha d, the value mpcqp_launch_step writes: hipcc contracts stage_step_kernel's `x += alpha * d` into one fused multiply-add, so the
// rounding is spelled out here -- the candidate a lane evaluates, the x it writes and the x mpcqp_nlp_step(alpha) writes are the same bits
SM_HD double gn_ls_point(double x, double alpha, double d) { return __builtin_fma(alpha, d, x); }
// one term of the l1 violation: how far v lies outside [lo, hi]; an infinite bound contributes 0
SM_HD double gn_ls_outside(double lo, double v, double hi) { return fmax(lo - v, 0.0) + fmax(v - hi, 0.0); }
// mu_b = max(mu[b] if given, mu_min, mu_factor max |y_i|); an instance whose QP returned no point does not look at its multipliers
SM_HD double gn_ls_penalty(bool has_mu, double mu_in, double mu_min, double mu_factor, bool ok, double ymax) {
  double mu = mu_min;
  if (has_mu) mu = fmax(mu, mu_in);
  if (ok) mu = fmax(mu, mu_factor * ymax);
  return mu;
}
SM_HD double gn_ls_merit(double f, double mu, double v) { return f + mu * v; }
// D = min(0, q' dx - mu_b v(x))
SM_HD double gn_ls_slope(double qd, double mu, double v0) {
  const double D = qd - mu * v0;
  return D < 0.0 ? D : 0.0;
}
SM_HD bool gn_ls_accepts(double phi_j, double phi_0, double c1, double alpha_j, double D) {
  return __builtin_isfinite(phi_j) && phi_j <= phi_0 + c1 * alpha_j * D;
}
// The decision.  phi(j): the merit at the base point (j = 0) and at candidate j - 1 (j = 1 .. K); K = 0 for an instance that is not ok.  Every
// turn of the loop up to `candidates` calls phi, whatever was found before: on the device phi is a shuffle, which every lane of a wave has to reach.
// Returns the point taken (0 = stay, j = candidate j - 1); *accepted = j - 1, -1 (the last candidate, not accepted but finite) or -2 (stay).
template <class Phi>
SM_HD int gn_ls_decide(int K, int candidates, double alpha0, double beta, double c1, double D, const Phi &phi, int *accepted) {
  const double phi0 = phi(0);
  int sel = 0, acc = -2;
  double a = alpha0, last = phi0;
  bool found = false;
  for (int j = 1; j <= candidates; j++) {
    const double pj = phi(j);
    if (j <= K) {
      if (!found && gn_ls_accepts(pj, phi0, c1, a, D)) { found = true; sel = j; acc = j - 1; }
      last = pj;
    }
    a *= beta;
  }
  if (K > 0 && !found && __builtin_isfinite(last)) { sel = K; acc = -1; }
  *accepted = acc;
  return sel;
}
