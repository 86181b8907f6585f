// StageSQP.hpp -- C++ form of the device-resident SQP loop over the C ABI (include/mpcqp.h): the reference's
// SQPOptimizationSolver::getOptimalSolution (reference src/sqp_solver/SQPOptimizationSolver.cpp:127-216) for a batch of
// instances of a stage OCP, with every step on the GPU:
//     mpcqp_stage_eval (getLocalSystem, :100-120) -> mpcqp_update(device) + mpcqp_solve (setSystem/initSolver/solve, :155-157)
//     -> mpcqp_stage_step (result.x += alpha * solution[pSize:], :171-177) -> mpcqp_stage_merit (objective, :180-181).
// Same quirks as the reference: a fixed number of iterations (step_num), no line search, the iterate persists across calls
// and starts at zero, arg.x0 is ignored.  Opt-in extension: setTolerance(t) adds a convergence stop that the reference has
// only under `verbose` (:183-197) -- the loop ends after the first iteration in which every instance moved by less than t
// (max-norm of alpha * dx, mpcqp_stage_step's step_max).  Opt-in as well: setLineSearch(candidates, beta, c1) replaces the one alpha of :171-177
// by a step length per instance from an l1-merit backtracking search that starts at alpha (mpcqp_stage_linesearch, one kernel in place of
// the step; the penalty persists across iterations and calls); alphaTaken() reports the last iteration's step lengths.  Opt-in as well:
// setKktTolerance(stat, feas, compl) adds the per-instance stop on the NLP's optimality residuals (mpcqp_stage_kkt): in every iteration but
// the first of a call, between the evaluation and the QP, the residuals are taken with the multipliers of the previous QP; an instance that meets the
// tolerances is frozen for the rest of the call (its x is not stepped), and the loop ends before the QP once every instance is; converged(),
// convergedAt() and kktResiduals() report on the last call.  Opt-in as well: setInitialGuessMode(GUESS_ROLLOUT / GUESS_RESHOOT) makes a fresh iterate
// dynamically feasible before the first evaluation (mpcqp_stage_rollout).  Header-only; needs the HIP runtime for the device buffers (hipMalloc / hipMemcpy).
#pragma once
#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "mpcqp.h"

class StageSQP {
 public:
  struct Arg { std::vector<double> lbx, ubx, lbg, ubg, p; };      // instance-major, as the DMDict of the reference carries them
  struct Result { std::vector<double> x, f; };

  // desc: model / horizon / dt / weights (mpcqp_stage_default fills the zoo's values); library_path: a generated dynamics
  // library (codegen.py) or nullptr for the built-in model named by desc.model
  StageSQP(const mpcqp_stage_desc &desc, int batch, int stepNum, double alpha, const char *library_path = nullptr)
      : batch_(batch), stepNum_(stepNum), alpha_(alpha) {
    check(library_path ? mpcqp_stage_create_user(&desc, library_path, &ocp_) : mpcqp_stage_create(&desc, &ocp_), "mpcqp_stage_create");
    check(mpcqp_stage_dims(ocp_, dims_), "mpcqp_stage_dims");
    std::vector<int> Pp(n() + 1), Pi(nnzP()), Ap(n() + 1), Ai(nnzA());
    check(mpcqp_stage_pattern(ocp_, Pp.data(), Pi.data(), Ap.data(), Ai.data()), "mpcqp_stage_pattern");
    mpcqp_settings st; mpcqp_default_settings(&st);               // eps 1e-3 / 1e-3, max_iter 10000 (reference :81-85)
    st.device = desc.device;
    check(mpcqp_create(n(), m(), batch_, Pp.data(), Pi.data(), Ap.data(), Ai.data(), &st, &qp_), "mpcqp_create");
    const size_t B = batch_;
    x_ = dalloc(B * nvar()); hip(hipMemset(x_, 0, B * nvar() * sizeof(double)));   // result_.x persists, zero-initialised (:88-91)
    dP_ = dalloc(B * nnzP()); dq_ = dalloc(B * n()); dA_ = dalloc(B * nnzA()); dl_ = dalloc(B * m()); du_ = dalloc(B * m());
    dw_ = dalloc(B * n()); f_ = dalloc(B); g_ = dalloc(B);
    p_ = dalloc(B * np()); lbx_ = dalloc(B * nvar()); ubx_ = dalloc(B * nvar()); lbg_ = dalloc(B * ng()); ubg_ = dalloc(B * ng());
  }
  ~StageSQP() {
    for (double *p : bufs_) (void)hipFree(p);
    if (status_) (void)hipFree(status_);
    if (conv_) (void)hipFree(conv_);
    if (masked_) (void)hipFree(masked_);
    if (rollDiv_) (void)hipFree(rollDiv_);
    if (qp_) mpcqp_destroy(qp_);
    if (ocp_) mpcqp_stage_destroy(ocp_);
  }
  StageSQP(const StageSQP &) = delete;
  StageSQP &operator=(const StageSQP &) = delete;

  int nx() const { return dims_[0]; } int nu() const { return dims_[1]; } int np() const { return dims_[2]; }
  int n() const { return dims_[3]; } int m() const { return dims_[4]; } int nnzP() const { return dims_[5]; }
  int nnzA() const { return dims_[6]; } int nvar() const { return dims_[7]; } int ng() const { return m() - n(); }
  bool generalCost() const { return mpcqp_stage_has_cost(ocp_) == 1; }   // the generated library carries its own stage cost

  // per-frame diagonal weights (terminal costs): Qk [horizon * nx], Rk [horizon * nu]
  void setWeights(const std::vector<double> &Qk, const std::vector<double> &Rk) {
    need(Qk.size(), (size_t)(nvar() / (nx() + nu())) * nx(), "Qk"); need(Rk.size(), (size_t)(nvar() / (nx() + nu())) * nu(), "Rk");
    check(mpcqp_stage_set_weights(ocp_, Qk.data(), Rk.data()), "mpcqp_stage_set_weights");
  }

  // per-frame bounds of the path constraint [horizon * nh] for the violation measure (terminal constraints: loose but on the last frame)
  void setPathBounds(const std::vector<double> &lo, const std::vector<double> &hi) {
    check(mpcqp_stage_set_path_bounds(ocp_, lo.data(), hi.data()), "mpcqp_stage_set_path_bounds");
  }

  // per-instance plant parameters (mpcqp_stage_set_instance_params): values [batch * paramCount()], row b = instance b's parameters in the model's
  // order; which = MPCQP_PARAMS_MODEL (every evaluation of the loop) or MPCQP_PARAMS_PLANT (the plant step of mpcqp_stage_advance, for callers that
  // run the hand-over on stage()); an empty vector returns that set to the shared values
  int paramCount() const { return mpcqp_stage_param_count(ocp_); }
  void setInstanceParams(int which, const std::vector<double> &values) {
    if (values.empty()) { check(mpcqp_stage_set_instance_params(ocp_, which, 0, nullptr, MPCQP_MEM_HOST), "mpcqp_stage_set_instance_params"); return; }
    const int k = paramCount();
    need(values.size(), (size_t)batch_ * (k > 0 ? k : 1), "values");
    std::vector<double> rows((size_t)batch_ * MPCQP_STAGE_NPAR, 0.0);
    for (int b = 0; b < batch_; b++) for (int i = 0; i < k; i++) rows[(size_t)b * MPCQP_STAGE_NPAR + i] = values[(size_t)b * k + i];
    check(mpcqp_stage_set_instance_params(ocp_, which, batch_, rows.data(), MPCQP_MEM_HOST), "mpcqp_stage_set_instance_params");
  }
  mpcqp_stage *stage() const { return ocp_; }

  void setInitialGuess(const std::vector<double> &x) {            // extension: the reference always starts from zero
    need(x.size(), (size_t)batch_ * nvar(), "x");
    hip(hipMemcpy(x_, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice));
    if (mu_) hip(hipMemset(mu_, 0, (size_t)batch_ * sizeof(double)));
    fresh_ = true;
  }
  // option initial_guess (default GUESS_NONE: the stored iterate as it is): a fresh iterate -- after construction or setInitialGuess -- is made
  // dynamically feasible by one mpcqp_stage_rollout in place, in the first getOptimalSolution, with that call's lbx / ubx:
  // GUESS_ROLLOUT holds u_0, GUESS_RESHOOT keeps the iterate's own inputs.  Later calls continue from the stored iterate.
  enum { GUESS_NONE = 0, GUESS_ROLLOUT = 1, GUESS_RESHOOT = 2 };
  void setInitialGuessMode(int mode) {
    if (mode != GUESS_NONE && mode != GUESS_ROLLOUT && mode != GUESS_RESHOOT) throw std::invalid_argument("mode must be GUESS_NONE, GUESS_ROLLOUT or GUESS_RESHOOT");
    guessMode_ = mode;
    if (mode != GUESS_NONE && !rollViol_) { rollViol_ = dalloc(batch_); hip(hipMalloc(&rollDiv_, (size_t)batch_ * sizeof(int))); }
  }
  const std::vector<int> &rolloutDiverged() const { return rolloutDiverged_; }         // per instance: the first failed step, -1 if none (empty: no rollout ran)
  const std::vector<double> &rolloutBoxViolation() const { return rolloutBoxViol_; }  // per instance: max violation of lbx / ubx by the rolled-out states

  // option polish_qp (default off, as the reference leaves OSQP's `polishing` off, :80-85): every QP of the loop is polished (mpcqp_set_polish)
  void setPolishQP(bool on) { check(mpcqp_set_polish(qp_, on ? 1 : 0, 0.0, -1), "mpcqp_set_polish"); }
  // option keep_scaling (default off): the first QP of the solver's life runs the full set-up, every later one keeps its scaling D, E, c and the
  // instances' rho and only re-factorises (mpcqp_update_matrices = OSQP's osqp_update_data_mat); a handle that answers MPCQP_ERR_LIMIT goes on with full set-ups
  void setKeepScaling(bool on) { keepScaling_ = on; if (on) check(mpcqp_keep_workspace(qp_, 1), "mpcqp_keep_workspace"); }
  void setTolerance(double tol) { tol_ = tol; }                   // 0 (default) = the reference's fixed iteration count
  // option line_search (default off: candidates = 0): per-instance step length, first candidate alpha, then alpha beta, alpha beta^2, ...
  // (1 <= candidates <= 8, 0 < beta < 1, 0 <= c1 < 1; the penalty's mu_min = 1 and mu_factor = 1.1 as in the Python loops)
  void setLineSearch(int candidates, double beta = 0.5, double c1 = 1e-4) {
    if (candidates < 0 || candidates > MPCQP_LINESEARCH_MAX_CANDIDATES) throw std::invalid_argument("candidates must be in 0..8");
    lsCandidates_ = candidates; lsBeta_ = beta; lsC1_ = c1;
    if (candidates > 0 && !mu_) {
      const size_t B = batch_;
      needDuals();
      mu_ = dalloc(B); alphaOut_ = dalloc(B);
      hip(hipMemset(mu_, 0, B * sizeof(double)));
    }
  }
  // option kkt_tol (default off: all three 0): the per-instance stop on stat <= tol_stat max(1, scale), feas <= tol_feas, compl <= tol_compl
  void setKktTolerance(double stat, double feas, double compl_) {
    if (!(stat >= 0.0) || !(feas >= 0.0) || !(compl_ >= 0.0)) throw std::invalid_argument("the tolerances must not be negative or NaN");
    kktTol_[0] = stat; kktTol_[1] = feas; kktTol_[2] = compl_;
    kkt_ = stat > 0.0 || feas > 0.0 || compl_ > 0.0;
    if (kkt_ && !kktRes_) {
      const size_t B = batch_;
      needDuals();
      kktRes_ = dalloc(B * 4);
      hip(hipMalloc(&conv_, B * sizeof(int))); hip(hipMalloc(&masked_, B * sizeof(int)));
    }
  }
  // option skip_converged_qps (default off; with the KKT stop): from iteration 1 on the verdict array is the QP handle's skip array (mpcqp_set_skip), so
  // a frozen instance's QP is neither set up nor iterated; x, converged() and convergedAt() are bit for bit those of the loop without it
  // While the stop is switched off again (setKktTolerance(0, 0, 0)) the option stays set and does nothing: every iteration solves the whole batch.
  void setSkipConvergedQPs(bool on) {
    if (on && !kkt_) throw std::invalid_argument("setSkipConvergedQPs skips the QPs of the instances the KKT stop has frozen: call setKktTolerance first");
    skipConverged_ = on;
    if (!on) check(mpcqp_set_skip(qp_, nullptr, MPCQP_MEM_DEVICE), "mpcqp_set_skip");
  }
  const std::vector<int> &converged() const { return converged_; }          // per instance, 0 / 1, of the last call
  const std::vector<int> &convergedAt() const { return convergedAt_; }      // the iteration index of the check that froze the instance, -1 if never
  std::vector<double> kktResiduals() const {                                // [batch * 4] = stat, feas, compl, scale of the last check (empty: none ran)
    std::vector<double> r;
    if (kktRes_ && checked_) { r.resize((size_t)batch_ * 4); hip(hipMemcpy(r.data(), kktRes_, r.size() * sizeof(double), hipMemcpyDeviceToHost)); }
    return r;
  }
  const std::vector<double> &alphaTaken() const { return alphaTaken_; }      // per instance, last iteration (empty without the line search)
  int iterationsDone() const { return iterationsDone_; }

  Result getOptimalSolution(const Arg &arg) {
    const size_t B = batch_;
    need(arg.lbx.size(), B * nvar(), "lbx"); need(arg.ubx.size(), B * nvar(), "ubx");
    need(arg.lbg.size(), B * ng(), "lbg"); need(arg.ubg.size(), B * ng(), "ubg"); need(arg.p.size(), B * np(), "p");
    up(lbx_, arg.lbx); up(ubx_, arg.ubx); up(lbg_, arg.lbg); up(ubg_, arg.ubg); up(p_, arg.p);
    if (kkt_) { hip(hipMemset(conv_, 0, B * sizeof(int))); converged_.assign(B, 0); convergedAt_.assign(B, -1); checked_ = false; }
    iterationsDone_ = 0;
    if (guessMode_ != GUESS_NONE && fresh_) {
      mpcqp_stage_rollout_args r = {};
      r.x_in = x_; r.x_out = x_; r.lbx = lbx_; r.ubx = ubx_; r.diverged = rollDiv_; r.box_viol = rollViol_;
      r.inputs = guessMode_ == GUESS_ROLLOUT ? MPCQP_ROLLOUT_INPUTS_HOLD : MPCQP_ROLLOUT_INPUTS_ITERATE;
      check(mpcqp_stage_rollout(ocp_, batch_, &r, nullptr), "mpcqp_stage_rollout");
      rolloutDiverged_.resize(B); rolloutBoxViol_.resize(B);
      hip(hipMemcpy(rolloutDiverged_.data(), rollDiv_, B * sizeof(int), hipMemcpyDeviceToHost));
      hip(hipMemcpy(rolloutBoxViol_.data(), rollViol_, B * sizeof(double), hipMemcpyDeviceToHost));
    }
    fresh_ = false;
    for (int i = 0; i < stepNum_; i++) {
      check(mpcqp_stage_eval(ocp_, batch_, p_, x_, lbx_, ubx_, lbg_, ubg_, dP_, dq_, dA_, dl_, du_, nullptr), "mpcqp_stage_eval");
      if (kkt_ && i >= 1) {                                         // the verdicts of the earlier checks are the frozen mask of this one
        mpcqp_kkt_args k = {};
        k.q = dq_; k.A = dA_; k.l = dl_; k.u = du_; k.y = y_; k.res = kktRes_; k.converged = conv_; k.frozen = conv_;
        k.tol_stat = kktTol_[0]; k.tol_feas = kktTol_[1]; k.tol_compl = kktTol_[2];
        check(mpcqp_stage_kkt(ocp_, batch_, &k, nullptr), "mpcqp_stage_kkt");
        hip(hipMemcpy(converged_.data(), conv_, B * sizeof(int), hipMemcpyDeviceToHost));      // one vector back to the host per iteration
        checked_ = true;
        bool all = true;
        for (size_t b = 0; b < B; b++) { if (converged_[b] && convergedAt_[b] < 0) convergedAt_[b] = i; all = all && converged_[b] != 0; }
        if (all) break;
      }
      int rc = MPCQP_ERR_LIMIT;
      if (keepScaling_ && scaled_) {
        rc = mpcqp_update_matrices(qp_, dP_, nnzP(), dq_, n(), dA_, nnzA(), dl_, m(), du_, m(), MPCQP_MEM_DEVICE);
        if (rc == MPCQP_ERR_LIMIT) keepScaling_ = false;            // for good: this handle's kernel family has no such entry
        else check(rc, "mpcqp_update_matrices");
      }
      if (rc == MPCQP_ERR_LIMIT) {
        check(mpcqp_update(qp_, dP_, nnzP(), dq_, n(), dA_, nnzA(), dl_, m(), du_, m(), MPCQP_MEM_DEVICE), "mpcqp_update");
        scaled_ = true;
      }
      // (iteration 0, and every iteration once the KKT stop has been switched off again: the whole batch -- the verdicts of an earlier call must not linger on the handle)
      if (skipConverged_) check(mpcqp_set_skip(qp_, kkt_ && i >= 1 ? conv_ : nullptr, MPCQP_MEM_DEVICE), "mpcqp_set_skip");
      check(mpcqp_solve(qp_, nullptr), "mpcqp_solve");
      if (lsCandidates_ > 0) {
        check(mpcqp_get(qp_, dw_, y_, nullptr, status_, nullptr, nullptr, MPCQP_MEM_DEVICE), "mpcqp_get");
        if (kkt_) {                                                 // a frozen instance reads as one whose QP returned no point
          hostStatus_.resize(B);
          hip(hipMemcpy(hostStatus_.data(), status_, B * sizeof(int), hipMemcpyDeviceToHost));
          for (size_t b = 0; b < B; b++) if (converged_[b]) hostStatus_[b] = 0;
          hip(hipMemcpy(masked_, hostStatus_.data(), B * sizeof(int), hipMemcpyHostToDevice));
        }
        mpcqp_stage_linesearch_args ls = {};
        ls.p = p_; ls.x = x_; ls.lbx = lbx_; ls.ubx = ubx_; ls.q = dq_; ls.dw = dw_; ls.y = y_; ls.status = kkt_ ? masked_ : status_; ls.mu = mu_;
        ls.alpha_out = alphaOut_; ls.step_max = tol_ > 0.0 ? g_ : nullptr;
        ls.alpha0 = alpha_; ls.beta = lsBeta_; ls.c1 = lsC1_; ls.mu_min = 1.0; ls.mu_factor = 1.1; ls.candidates = lsCandidates_;
        check(mpcqp_stage_linesearch(ocp_, batch_, &ls, nullptr), "mpcqp_stage_linesearch");
      } else {
        check(mpcqp_get(qp_, dw_, kkt_ ? y_ : nullptr, nullptr, nullptr, nullptr, nullptr, MPCQP_MEM_DEVICE), "mpcqp_get");
        if (kkt_) {                                                 // every live instance steps as the reference does; a frozen one keeps its x
          hostStatus_.resize(B);
          for (size_t b = 0; b < B; b++) hostStatus_[b] = converged_[b] ? 0 : MPCQP_SOLVED;
          hip(hipMemcpy(masked_, hostStatus_.data(), B * sizeof(int), hipMemcpyHostToDevice));
        }
        check(mpcqp_stage_step(ocp_, batch_, alpha_, dw_, x_, tol_ > 0.0 ? g_ : nullptr, kkt_ ? masked_ : nullptr, nullptr), "mpcqp_stage_step");
      }
      iterationsDone_ = i + 1;
      if (tol_ > 0.0) {                                           // one vector of step norms back to the host per iteration
        stepMax_.resize(B);
        hip(hipMemcpy(stepMax_.data(), g_, B * sizeof(double), hipMemcpyDeviceToHost));
        // (instances whose QP failed report a NaN step: they neither stop the loop nor keep it going; a batch without a finite step goes on)
        double worst = 0.0; bool any = false;
        for (double v : stepMax_) if (v == v) { any = true; if (v > worst) worst = v; }
        if (any && worst < tol_) break;
      }
    }
    check(mpcqp_stage_merit(ocp_, batch_, p_, x_, f_, g_, nullptr), "mpcqp_stage_merit");
    if (lsCandidates_ > 0 && stepNum_ > 0) {
      alphaTaken_.resize(B);
      hip(hipMemcpy(alphaTaken_.data(), alphaOut_, B * sizeof(double), hipMemcpyDeviceToHost));
    }
    Result r; r.x.resize(B * nvar()); r.f.resize(B); violation_.resize(B);
    hip(hipMemcpy(r.x.data(), x_, r.x.size() * sizeof(double), hipMemcpyDeviceToHost));
    hip(hipMemcpy(r.f.data(), f_, B * sizeof(double), hipMemcpyDeviceToHost));
    hip(hipMemcpy(violation_.data(), g_, B * sizeof(double), hipMemcpyDeviceToHost));
    return r;
  }
  const std::vector<double> &constraintViolation() const { return violation_; }    // max-norm per instance after the last call

 private:
  static void hip(hipError_t e) { if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e)); }
  static void check(int rc, const char *what) { if (rc != MPCQP_OK) throw std::runtime_error(std::string(what) + ": " + mpcqp_strerror(rc)); }
  static void need(size_t got, size_t want, const char *name) {
    if (got != want) throw std::invalid_argument(std::string(name) + " 的维度不对: expected " + std::to_string(want) + ", got " + std::to_string(got));
  }
  // the multipliers and statuses of the QP on the device (the line search and the optimality residuals read them)
  void needDuals() {
    if (y_) return;
    y_ = dalloc((size_t)batch_ * m());
    hip(hipMalloc(&status_, (size_t)batch_ * sizeof(int)));
  }
  double *dalloc(size_t count) { double *p = nullptr; hip(hipMalloc(&p, (count ? count : 1) * sizeof(double))); bufs_.push_back(p); return p; }
  void up(double *dst, const std::vector<double> &src) { if (!src.empty()) hip(hipMemcpy(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice)); }

  int batch_, stepNum_; double alpha_; double tol_ = 0.0; int iterationsDone_ = 0;
  bool keepScaling_ = false, scaled_ = false;                     // (scaled_: a full set-up has run on the handle)
  std::vector<double> stepMax_;
  int lsCandidates_ = 0; double lsBeta_ = 0.5, lsC1_ = 1e-4;      // line search: 0 candidates = off
  double *y_ = nullptr, *mu_ = nullptr, *alphaOut_ = nullptr; int *status_ = nullptr;
  std::vector<double> alphaTaken_;
  bool skipConverged_ = false;
  int guessMode_ = GUESS_NONE; bool fresh_ = true;               // initial_guess: applied once to a fresh iterate
  double *rollViol_ = nullptr; int *rollDiv_ = nullptr;
  std::vector<int> rolloutDiverged_; std::vector<double> rolloutBoxViol_;
  bool kkt_ = false, checked_ = false; double kktTol_[3] = {0.0, 0.0, 0.0};   // optimality residuals: all tolerances 0 = off
  double *kktRes_ = nullptr; int *conv_ = nullptr, *masked_ = nullptr;
  std::vector<int> converged_, convergedAt_, hostStatus_;
  int dims_[8] = {0};
  mpcqp_stage *ocp_ = nullptr; mpcqp_handle *qp_ = nullptr;
  double *x_ = nullptr, *dP_ = nullptr, *dq_ = nullptr, *dA_ = nullptr, *dl_ = nullptr, *du_ = nullptr, *dw_ = nullptr, *f_ = nullptr, *g_ = nullptr;
  double *p_ = nullptr, *lbx_ = nullptr, *ubx_ = nullptr, *lbg_ = nullptr, *ubg_ = nullptr;
  std::vector<double *> bufs_;
  std::vector<double> violation_;
};
