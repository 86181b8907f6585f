// mpcqp.hip -- MI355X (gfx950) batched OSQP-style ADMM: device kernels + the C ABI of include/mpcqp.h.
//
// Replaces, for a batch of QPs sharing one sparsity, what the reference does per QP on the host through
// CuCaQP::setSystem -> initSolver -> solve -> getSolution (reference src/sqp_solver/CuCaQP.cpp:271-288,
// 183-224), i.e. OSQP's osqp_setup + osqp_solve (external to the reference, see oracle/osqp_oracle.h).
//
// One launch does the whole sequence for every QP of the batch (grid = batch, one workgroup per QP).  Kernel families
// (select_kernel, select.hpp, picks one per sparsity and batch size from measured rules):
//   * mpcqp_res_kernel<NW, MINW, GB, REUSE, ZYG, NG, NH, TL> -- NW wavefronts per QP (1, 2, 4 or 8), W-fused block LDL' of
//     M = P + sigma I + A' diag(rho) A in 16x16 blocks, solve driven by a host-built schedule of arithmetic-progression
//     segments (plan.hpp).  GB = false: the factor lives in LDS (small / mid-size problems, and any batch that fits one
//     resident round); GB = true: the factor stays in the per-QP HBM slab and LDS holds only vectors, temp tiles and the
//     schedule, so that 3-4 workgroups share a CU (two or four waves; long horizons that no on-chip instance takes; HBM-roofline-bound).
//     MINW selects the register budget (128 / 168 / 256 VGPRs), REUSE the kept-workspace entry (mpcqp_update_vectors),
//     ZYG keeps z and y in the slab too (long horizons).
//     NG / NH > 0: the on-chip mode of the global-block kernel (kernel_onchip.hpp) -- after each factorisation the factor is
//     brought on chip (chain blocks in LDS, inverse diagonal blocks and some hub blocks in registers; four waves at two workgroups per CU,
//     eight waves at one) and the triangular solves run on the matrix cores, register to register along each chain.
//   * mpcqp_oc_setup_kernel + mpcqp_oc_admm_kernel (kernel_oc_split.hpp) -- the on-chip mode as two kernels, set-up and iteration: the
//     default form of the on-chip mode, and with it of the 12-state quadrotor, N = 20.
//   * mpcqp_admm_kernel<PD> -- the first-generation streaming kernel, one QP per wavefront, block Cholesky streamed from
//     the slab; fallback when even the vectors exceed LDS, and a cross-check in the variant tests.
// Common to all: ADMM iterates in LDS; scaled A in two ELL orientations and scaled P in the slab, streamed with coalesced
// 512 B wave loads; the linear solve is a stream of 16x16 block mat-vecs (4 lanes per row, quad DPP reduction); the
// factorisation's block products are dense 16x16x16 GEMMs on the matrix cores (v_mfma_f64_16x16x4_f64); box projection,
// dual update and residual norms fused into the ELL sweeps; termination, infeasibility certificates and adaptive-rho
// re-factorisation in-kernel; workgroup-uniform state in scalar registers (uni()).
// Numerics are fp64 throughout and follow oracle/osqp_oracle.c step by step (same scaling rule, rho rule,
// termination / infeasibility tests and deterministic adaptive-rho schedule).
#include <map>
#include <mutex>
#include "kernels_all.hpp"
#include "kernels_util.hpp"
#include "reduced.hpp"

static_assert(SEL_ERR_ARG == MPCQP_ERR_ARG && SEL_ERR_LIMIT == MPCQP_ERR_LIMIT, "select.hpp reports its refusals in the codes of include/mpcqp.h");

// ------------------------------------------------------------------------------------------ host side
static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) { g_last_error = msg; return code; }
int mpcqp_set_error(int code, const std::string &msg) { return fail(code, msg); }
int mpcqp_pick_device(int requested, int *device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MPCQP_ERR_NO_GPU, "hipGetDeviceCount found no device");
  int dev = requested;
  if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
  if (dev >= ndev) return fail(MPCQP_ERR_ARG, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(MPCQP_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(MPCQP_ERR_NO_GPU, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  *device = dev;
  return MPCQP_OK;
}
#define HIPCHK(expr)                                                                              \
  do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(MPCQP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

struct mpcqp_handle {
  int n = 0, m = 0, batch = 0, device = 0;
  hipEvent_t ev_guard = nullptr;              // mpcqp_order_after_last_solve
  mpcqp_settings st;
  Knobs knobs;                                // the MPCQP_* switches as they stood when the handle was created
  Selection sel;                              // what select_kernel decided: family, instance, plans, LDS (sel.waves = -1: a reduced handle, `inner` runs)
  DevPlan dp; DevRes dres; DevOc doc; DevIO io;
  DevRes dres_setup; DevOc doc_setup;         // two-kernel on-chip form: the set-up kernel's copies of the arguments, with its own launch shape (sel.setup)
  int *qctr = nullptr; int qslots = 0;        // ... ticket counters of the resident iteration workgroups (16 per solve in flight), and how many workgroups the GPU holds at once
  std::vector<void *> dev_allocs;
  double *ws = nullptr;
  double *dP = nullptr, *dq = nullptr, *dA = nullptr, *dl = nullptr, *du = nullptr;  // owned copies (host-memory updates)
  double *dx0 = nullptr, *dy0 = nullptr, *drho0 = nullptr;
  bool keep = false, have_factor = false, reuse_next = false;
  bool rescale_next = false, rescale_done = false;   // mpcqp_update_matrices: solves scale the data with the kept D, E, c and re-factorise; one has run since the call
  int *order[2] = {nullptr, nullptr}; int order_cur = -1; bool lpt = true; hipEvent_t ev_order = nullptr;   // dispatch hint, double-buffered
  static constexpr int NPIPE = 8;
  hipStream_t pipe[NPIPE] = {};               // mpcqp_solve_host: compute streams, one per slice in flight
  hipStream_t pipe_copy = nullptr;            // ... and the one stream all host-to-device copies queue on, in slice order
  std::vector<hipEvent_t> pipe_ev;            // slice k's inputs have landed
  double *ox = nullptr, *oy = nullptr, *oz = nullptr, *oinfo = nullptr, *ocs = nullptr; int *ostatus = nullptr, *oiters = nullptr;
  long long *odbg = nullptr;
  bool have_data = false, solved = false;
  hipStream_t last_stream = nullptr;
  hipEvent_t ev_mid = nullptr;                // two-kernel on-chip mode: between the set-up and the iteration kernel (mpcqp_last_phase_ms)
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev0r = nullptr;   // (ev0r: reduced handles, ordering of the presolve behind a solve on another stream)
  // reduced form (mpcqp_create_reduced): this handle keeps the caller's dimensions, `inner` solves the QP without the eliminated variables
  mpcqp_handle *inner = nullptr; RedMaps red; DevRed dred; double *rx0 = nullptr, *ry0 = nullptr;
  // polishing (mpcqp_set_polish): off by default; the polish factor's scratch and the per-QP outcome are allocated when it is first switched on
  bool polish = false, polish_timed = false; double pol_delta = 1e-6; int pol_refine = 3;
  double *pfac = nullptr; long pfac_stride = 0; int *opstatus = nullptr; double *opinfo = nullptr;
  hipEvent_t evp0 = nullptr, evp1 = nullptr;
  // a subset of the batch (mpcqp_set_skip): the array the following solves read (borrowed, or dskip), the dispatch list the compaction kernel writes
  // ahead of every such solve (allocated when an array is first set: nothing is allocated inside a solve), whether the last solve wrote one, and what
  // the skipped instances' slabs may lack: skip_full = a full set-up ran under a skip array (their scaling and factor), skip_mat = an
  // mpcqp_update_matrices solve did (their factor)
  const int *skip = nullptr; int *dskip = nullptr, *skip_list = nullptr; bool skip_listed = false, skip_full = false, skip_mat = false;
  // soft rows (mpcqp_set_soft_rows): the argument of the soft twins of the iteration kernel -- the weights as they stand (borrowed, or the handle's copies dsw1 /
  // dsw2 of host arrays) and the per-instance buffer of scaled weights, allocated by the first set call; soft = the following solves launch the twins
  bool soft = false; DevSoft dsoft = {nullptr, nullptr, 0, 0, nullptr, 0}; double *dsw1 = nullptr, *dsw2 = nullptr;
};
// what a solve under the handle's skip array (or without one) leaves for the kept-workspace entries; mode = DevIO.reuse of the solve
static void note_skip_state(mpcqp_handle *h, int mode) {
  const bool sk = h->skip != nullptr;
  if (mode == 0) { h->skip_full = sk; h->skip_mat = false; }
  else if (mode == 2) h->skip_mat = sk;
  h->skip_listed = sk;
}

int mpcqp_order_after_last_solve(mpcqp_handle *h, hipStream_t s) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->solved || h->last_stream == s) return MPCQP_OK;
  if (!h->ev_guard) HIPCHK(hipEventCreateWithFlags(&h->ev_guard, hipEventDisableTiming));
  HIPCHK(hipEventRecord(h->ev_guard, h->last_stream));
  HIPCHK(hipStreamWaitEvent(s, h->ev_guard, 0));
  return MPCQP_OK;
}

template <class T>
static int upload(mpcqp_handle *h, const std::vector<T> &v, const T **out) {
  void *d = nullptr;
  size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  HIPCHK(hipMalloc(&d, bytes));
  h->dev_allocs.push_back(d);
  if (!v.empty()) HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = (const T *)d;
  return MPCQP_OK;
}
static int upload_ell(mpcqp_handle *h, const Ell &e, DevEll *d) {
  d->nchunks = e.nchunks; d->entries = e.entries();
  int rc;
  if ((rc = upload(h, e.chunk_off, &d->chunk_off))) return rc;
  if ((rc = upload(h, e.idx, &d->idx))) return rc;
  if ((rc = upload(h, e.src, &d->src))) return rc;
  if ((rc = upload(h, e.flag, &d->flag))) return rc;
  return MPCQP_OK;
}
template <class T>
static int dalloc(mpcqp_handle *h, T **p, size_t count) {
  void *d = nullptr;
  HIPCHK(hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
  h->dev_allocs.push_back(d);
  *p = (T *)d;
  return MPCQP_OK;
}

// the kernel instance a handle runs (instantiated in the k_*.hip units, kernel_table.hpp): which one is select.hpp's decision (kernel_id_of and its
// siblings); here a KernelId only becomes a table pointer -- nullptr where no such instance is compiled
static const void *kernel_of(const KernelId &k) {
  switch (k.kind) {
    case K_STREAM: return k.pd == 8 ? (const void *)mpcqp_admm_kernel<8> : k.pd == 4 ? (const void *)mpcqp_admm_kernel<4> : nullptr;
    case K_LDS: return k.reuse ? mpcqp_kernel_res_lds_r1(k.nw, k.minw) : mpcqp_kernel_res_lds_r0(k.nw, k.minw);
    case K_GB: return k.reuse ? mpcqp_kernel_res_gb_r1(k.nw, k.minw, k.zyg != 0) : mpcqp_kernel_res_gb_r0(k.nw, k.minw, k.zyg != 0);
    case K_OC_MONO: return k.reuse ? mpcqp_kernel_oc_mono_r1(k.nw, k.ng, k.nh, k.tiles != 0) : mpcqp_kernel_oc_mono_r0(k.nw, k.ng, k.nh, k.tiles != 0);
    case K_OC_SETUP: return mpcqp_kernel_oc_setup(k.nw, k.hub != 0, k.reuse != 0);
    case K_OC_RESCALE: return mpcqp_kernel_oc_rescale(k.nw, k.hub != 0);
    case K_OC_ADMM: return k.soft ? mpcqp_kernel_oc_admm_soft(k.nw, k.ng, k.nh) : mpcqp_kernel_oc_admm(k.nw, k.ng, k.nh);
    case K_OC_ADMM_RF: return k.soft ? mpcqp_kernel_oc_admm_soft_rf(k.nw, k.ng, k.nh) : mpcqp_kernel_oc_admm_rf(k.nw, k.ng, k.nh);
    case K_OC_ADMM_P4: return k.soft ? mpcqp_kernel_oc_admm_soft_p4(k.rf) : mpcqp_kernel_oc_admm_p4(k.rf);
    case K_OC_ADMM_TL: return mpcqp_kernel_oc_admm_tl(k.nw, k.ng, k.nh);
  }
  return nullptr;
}
// waves per QP, register budget, factor location, and -- as its own instance so that the full-setup kernels carry no code for it -- the kept-workspace
// entry (mpcqp_update_vectors).  (On-chip: the single-kernel form; eight waves without an arrow head have none, such handles run the two-kernel form.)
static const void *res_kernel_of(const mpcqp_handle *h, bool reuse) { return kernel_of(res_kernel_id_of(h->sel, reuse)); }
static const void *stream_kernel_of(const mpcqp_handle *h) { return kernel_of(stream_kernel_id_of(h->sel)); }
// the two kernels of the on-chip mode (kernel_oc_split.hpp): CuCaQP::initSolver and CuCaQP::solve
static const void *oc_setup_of(const mpcqp_handle *h, bool reuse) { return kernel_of(oc_setup_kernel_id_of(h->sel, reuse)); }
// ... and the kernel that takes the set-up's place after mpcqp_update_matrices (kernel_oc_rescale.hpp): in the set-up's launch shape
static const void *oc_rescale_of(const mpcqp_handle *h) { return kernel_of(oc_rescale_kernel_id_of(h->sel)); }
// which handles mpcqp_update_matrices takes: the two-kernel on-chip form without the tile experiment
static bool takes_matrix_updates(const mpcqp_handle *h) {
  const Selection &s = h->sel;
  return s.waves > 0 && s.oc && s.split && !s.tiles && !s.vtiles && oc_rescale_of(h) != nullptr;
}
static const void *oc_admm_of(const mpcqp_handle *h, bool rf = false) { return kernel_of(oc_admm_kernel_id_of(h->sel, rf, h->soft)); }
// the soft-row twins of a handle's iteration kernels (whether or not soft rows are set)
static const void *oc_admm_soft_of(const mpcqp_handle *h, bool rf) { return kernel_of(oc_admm_kernel_id_of(h->sel, rf, true)); }
// One solve of the two-kernel on-chip mode on stream s: set-up, iteration; then, for instances whose adaptive-rho step asked for a new factor
// (kernel_oc_split.hpp: they leave the iteration kernel marked OC_PENDING), `resume_rounds` pairs of {re-factorisation, iteration} in which every other
// workgroup returns at once, and a last pair whose iteration kernel re-factorises in place, so that any number of rho updates is served.
// The idle waves' L2 touch during the backward chains (kernel_oc_split.hpp idle_touch): off for the eight-wave instances (one QP's sweeps do not fit a CU's share of
// the L2; MPCQP_TOUCH8 turns it on) and, since round 4, for the four-wave instances of the two-kernel form as well -- with the sweeps' gathers batched and three set-up
// workgroups per CU the touch only competes with them (quadrotor N=20 x 8192 iteration kernel 5.25 -> 5.15 ms without it, N=15 3.98 -> 3.82, N=10 3.02 -> 2.94;
// cart-pole N=50 and double integrator N=60 unchanged; MPCQP_TOUCH4 turns it on).  The single-kernel form keeps it.
static int no_touch_of(const mpcqp_handle *h) {
  if (h->knobs.no_touch) return 1;
  if (h->sel.oc8) return h->knobs.touch8 ? 0 : 1;
  if (h->sel.split) return h->knobs.touch4 ? 0 : 1;
  return 0;
}
static int launch_oc_split(mpcqp_handle *h, DevIO &io, int count, bool reuse, hipStream_t s, hipEvent_t after_setup, int qslot) {
  const Selection &sl = h->sel;
  const dim3 grid(count), block(sl.waves * WAVE), block_s(sl.setup.nw * WAVE);
  const size_t lds = (size_t)sl.lds, lds_setup = (size_t)sl.setup.lds;
  // the iteration kernel as resident workgroups that draw instances from one counter (kernel_oc_split.hpp) when the batch is more than the GPU holds at once
  const bool queued = sl.oc8 != 0;      // (the eight-wave instances are compiled as resident workgroups; the four-wave ones are not)
  int *qc = queued ? h->qctr + 16 * qslot : nullptr;
  if (queued) HIPCHK(hipMemsetAsync(qc, 0, 16 * sizeof(int), s));
  const dim3 grid_it(queued ? std::min(h->qslots, count) : count);
  int nlaunch = 0;
  DevIO ioq[10];
  auto io_of = [&]() -> void * { DevIO &q = ioq[nlaunch]; q = io; q.queue = queued ? qc + nlaunch : nullptr; q.count = count; return (void *)&ioq[nlaunch++]; };
  DevOc doc0 = h->doc; doc0.resume = 0;
  DevOc docr = doc0; docr.resume = 1;
  DevOc docs0 = h->doc_setup; docs0.resume = 0;
  DevOc docsr = docs0; docsr.resume = 1;
  // (the sixth entry is the soft twins' own argument: hipLaunchKernel reads as many entries as the kernel has parameters, five for every other kernel)
  void *args[] = {(void *)&h->dp, (void *)&h->dres, (void *)&h->st, (void *)&io, (void *)&doc0, (void *)&h->dsoft};
  void *argr[] = {(void *)&h->dp, (void *)&h->dres, (void *)&h->st, (void *)&io, (void *)&docr, (void *)&h->dsoft};
  void *sargs[] = {(void *)&h->dp, (void *)&h->dres_setup, (void *)&h->st, (void *)&io, (void *)&docs0};
  void *sargr[] = {(void *)&h->dp, (void *)&h->dres_setup, (void *)&h->st, (void *)&io, (void *)&docsr};
  HIPCHK(hipLaunchKernel(io.reuse == 2 ? oc_rescale_of(h) : oc_setup_of(h, reuse), grid, block_s, sargs, lds_setup, s));      // (DevIO.reuse 2: new matrices on the kept scaling)
  if (after_setup) HIPCHK(hipEventRecord(after_setup, s));
  const bool rho_updates = h->st.adaptive_rho != 0;
  args[3] = io_of();
  HIPCHK(hipLaunchKernel(oc_admm_of(h, !rho_updates), grid_it, block, args, lds, s));     // (without adaptive rho nothing ever leaves: either instance serves)
  if (!rho_updates) return MPCQP_OK;
  for (int r = 0; r <= sl.resume_rounds; r++) {
    HIPCHK(hipLaunchKernel(oc_setup_of(h, false), grid, block_s, sargr, lds_setup, s));
    argr[3] = io_of();
    HIPCHK(hipLaunchKernel(oc_admm_of(h, r == sl.resume_rounds), grid_it, block, argr, lds, s));
  }
  return MPCQP_OK;
}
// `count` instances on stream s through the handle's kernel(s), then the check of what they wrote; every per-instance pointer of io is at the first of them
// (the kernels index by blockIdx).  Events, where given: after the set-up kernel of the two-kernel form, after the last kernel of the solve.
static int launch_batch(mpcqp_handle *h, DevIO &io, int count, bool reuse, hipStream_t s, hipEvent_t after_setup, hipEvent_t after_kernel, int qslot, const int *skip = nullptr) {
  const Selection &sl = h->sel;
  if (sl.waves > 0 && sl.split) {     // CuCaQP::initSolver, then CuCaQP::solve
    int rc = launch_oc_split(h, io, count, reuse, s, after_setup, qslot);
    if (rc) return rc;
  }
  else if (sl.waves > 0) {
    void *args[] = {(void *)&h->dp, (void *)&h->dres, (void *)&h->st, (void *)&io, (void *)&h->doc};
    HIPCHK(hipLaunchKernel(res_kernel_of(h, reuse), dim3(count), dim3(sl.waves * WAVE), args, (size_t)sl.lds, s));
  }
  else {
    void *args[] = {(void *)&h->dp, (void *)&h->st, (void *)&io};
    HIPCHK(hipLaunchKernel(stream_kernel_of(h), dim3(count), dim3(WAVE), args, (size_t)sl.lds, s));
  }
  HIPCHK(hipGetLastError());
  if (after_kernel) HIPCHK(hipEventRecord(after_kernel, s));
  if (h->m > 0) {
    hipLaunchKernelGGL(mpcqp_validate_kernel, dim3((count + 3) / 4), dim3(256), 0, s, count, h->n, h->m, io.l, io.sl, io.u, io.su, io.x, io.y, io.z,
                       io.status, io.iters, io.info, skip);
    HIPCHK(hipGetLastError());
  }
  if (h->polish) {      // OSQP's polish() behind osqp_solve's loop: on the final status (the validation above included), ahead of anything that reads the outputs
    const long b0 = io.status - h->ostatus;      // (a slice of mpcqp_solve_host: the handle's own buffers are advanced like io's)
    DevPolish po;
    po.q = io.q; po.sq = io.sq; po.x = io.x; po.y = io.y; po.z = io.z; po.status = io.status; po.info = io.info; po.ws = io.ws; po.cscale = io.cscale;
    po.fac = h->pfac + b0 * h->pfac_stride; po.fac_stride = h->pfac_stride; po.pstatus = h->opstatus + b0; po.pinfo = h->opinfo + 4 * b0;
    po.delta = h->pol_delta; po.refine = h->pol_refine; po.skip = skip;
    const bool timed = after_kernel != nullptr;
    if (timed) HIPCHK(hipEventRecord(h->evp0, s));
    if (int rc = mpcqp_polish_launch(h->dp, h->st, po, count, s)) return rc;
    if (timed) HIPCHK(hipEventRecord(h->evp1, s));
    h->polish_timed = timed;
  }
  return MPCQP_OK;
}
// the handle's inputs as they stand + its own outputs, workspace and solve-time switches: what every launch starts from
static DevIO io_of_handle(const mpcqp_handle *h) {
  DevIO io = h->io;
  io.x = h->ox; io.y = h->oy; io.z = h->oz; io.status = h->ostatus; io.iters = h->oiters; io.info = h->oinfo; io.ws = h->ws; io.no_remap = h->knobs.no_remap ? 1 : 0; io.no_touch = no_touch_of(h); io.cscale = h->ocs; io.dbg = h->odbg;
  io.reuse = 0; io.keep = h->keep ? 1 : 0; io.order = nullptr;
  return io;
}
// a CSC pattern as the create entries take it: column pointers monotone (from 0 where the entry asks for that), row indices in range.  Pp = null: A alone
static int check_csc(int n, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai, bool from_zero) {
  if (from_zero && ((Pp && Pp[0] != 0) || Ap[0] != 0)) return fail(MPCQP_ERR_ARG, "colptr must start at 0");
  for (int j = 0; j < n; j++) if ((Pp && Pp[j + 1] < Pp[j]) || Ap[j + 1] < Ap[j]) return fail(MPCQP_ERR_ARG, "colptr not monotone");
  if (Pp) for (int k = Pp[0]; k < Pp[n]; k++) if (Pi[k] < 0 || Pi[k] >= n) return fail(MPCQP_ERR_ARG, "P row index out of range");
  for (int k = Ap[0]; k < Ap[n]; k++) if (Ai[k] < 0 || Ai[k] >= m) return fail(MPCQP_ERR_ARG, "A row index out of range");
  return MPCQP_OK;
}

// ---- mpcqp_create, step by step: what select_kernel chose goes to the device
#define UP(expr) do { if (int rc_ = (expr)) return rc_; } while (0)
// the plan's tables (every family reads them) and the offsets of the per-QP slab
static int upload_plan(mpcqp_handle *h) {
  const Plan &pl = h->sel.plan; const WsLayout &w = h->sel.wl; DevPlan &dp = h->dp;
  memset(&dp, 0, sizeof(dp));
  dp.n = h->n; dp.m = h->m; dp.npad = pl.npad; dp.mpad = pl.mpad; dp.nb = pl.nb; dp.nblk = pl.nblk; dp.nfac = (int)pl.fac.size(); dp.nT = pl.nT;
  UP(upload_ell(h, pl.A, &dp.A)); UP(upload_ell(h, pl.At, &dp.At)); UP(upload_ell(h, pl.P, &dp.P));
  UP(upload(h, pl.pos, &dp.pos)); UP(upload(h, pl.perm, &dp.perm));
  UP(upload(h, pl.fwd_ops, &dp.fwd_ops)); UP(upload(h, pl.bwd_ops, &dp.bwd_ops)); UP(upload(h, pl.bwd_of, &dp.bwd_of));
  std::vector<int4> f(pl.fac.size());
  for (size_t i = 0; i < f.size(); i++) f[i] = make_int4(pl.fac[i].type, pl.fac[i].dst, pl.fac[i].a, pl.fac[i].b);
  UP(upload(h, f, &dp.fac));
  UP(upload(h, pl.tpos, &dp.tpos)); UP(upload(h, pl.asm_ptr, &dp.asm_ptr)); UP(upload(h, pl.asm_a, &dp.asm_a));
  UP(upload(h, pl.asm_b, &dp.asm_b)); UP(upload(h, pl.asm_pidx, &dp.asm_pidx)); UP(upload(h, pl.blk_diag, &dp.blk_diag));
  dp.o_ellA = w.ellA; dp.o_ellAt = w.ellAt; dp.o_ellP = w.ellP; dp.o_Lf = w.Lf; dp.o_Lb = w.Lb; dp.o_T = w.T;
  dp.o_l = w.l; dp.o_u = w.u; dp.o_D = w.D; dp.o_E = w.E; dp.o_dx = w.dx; dp.o_dy = w.dy; dp.o_Zg = w.Zg; dp.o_Yg = w.Yg; dp.ws_stride = w.stride;
  return MPCQP_OK;
}
// resident families: the level-parallel LDL' plan and the solve schedule
static int upload_resident(mpcqp_handle *h) {
  const Selection &s = h->sel; const Plan &pl = s.plan; const ResPlan &rp = s.rplan; DevRes &dr = h->dres;
  dr.nphase = rp.nphase; dr.ntemp = rp.ntemp; dr.nconst = rp.nconst; dr.rext = rp.rext;
  dr.nlev = rp.nlev;
  UP(upload(h, rp.lv_ptr, &dr.lv_ptr)); UP(upload(h, rp.lv_diag, &dr.lv_diag)); UP(upload(h, rp.lw_ptr, &dr.lw_ptr));
  UP(upload(h, rp.lw_slot, &dr.lw_slot)); UP(upload(h, rp.lw_g, &dr.lw_g)); UP(upload(h, rp.lu_ptr, &dr.lu_ptr));
  UP(upload(h, rp.lu_dst, &dr.lu_dst)); UP(upload(h, rp.lu_tmp, &dr.lu_tmp)); UP(upload(h, rp.lu_b, &dr.lu_b));
  UP(upload(h, rp.g_ptr, &dr.g_ptr)); UP(upload(h, rp.g_seg, &dr.g_seg)); dr.n_seg = (int)rp.g_seg.size() / 8; dr.stage = s.gblocks ? res_stage_doubles_gb(pl, rp) : res_stage_doubles(pl, rp);
  dr.tmp_alias = s.gblocks && !s.oc && gb_tmp_alias(pl, rp) ? 1 : 0;
  memset(&h->doc, 0, sizeof(h->doc));
  return MPCQP_OK;
}
// on-chip kernels with dense tiles of A (the MPCQP_TILES / MPCQP_VTILES experiments): the tiles and the remainder ELL layouts
static int upload_tiles(mpcqp_handle *h) {
  const Selection &s = h->sel; const Plan &pl = s.plan; const TilePlan &tp = s.tplan; DevTile &t = h->doc.tl;
  t.on = 1; t.ntile = tp.ntile; t.nAr = tp.Ar.nchunks; t.nAtr = tp.Atr.nchunks; t.Ar_entries = tp.Ar.entries(); t.Atr_entries = tp.Atr.entries();
  UP(upload(h, tp.Ar.chunk_off, &t.Ar_off)); UP(upload(h, tp.Ar.idx, &t.Ar_idx)); UP(upload(h, tp.Ar.src, &t.Ar_src));
  UP(upload(h, tp.Atr.chunk_off, &t.Atr_off)); UP(upload(h, tp.Atr.idx, &t.Atr_idx)); UP(upload(h, tp.Atr.src, &t.Atr_src));
  UP(upload(h, tp.tJ, &t.tJ)); UP(upload(h, tp.rowid, &t.rowid));
  if (s.vtiles) {      // row-major tiles for the vector-ALU form: element (r, c) at 16 r + c (the plan keeps the MFMA operand order [r + 16 (c & 3)][c >> 2])
    std::vector<int> rm(tp.tsrc.size(), -1);
    for (size_t tt = 0; tt < tp.tsrc.size() / BLK; tt++) for (int r = 0; r < BS; r++) for (int c = 0; c < BS; c++)
      rm[tt * BLK + r * BS + c] = tp.tsrc[tt * BLK + (r + BS * (c & 3)) * 4 + (c >> 2)];
    UP(upload(h, rm, &t.tsrc));
  } else UP(upload(h, tp.tsrc, &t.tsrc));
  {   // per-chunk records of fixed size (kernel_onchip.hpp oc_tiles_a / oc_tiles_at): {tile, column block, first row, rows}, padded with the zero tile
    auto first = [&](int tt) { for (int r = 0; r < BS; r++) if (tp.rowid[(size_t)tt * BS + r] >= 0) return tp.rowid[(size_t)tt * BS + r]; return 0; };
    auto rows = [&](int tt) { int k = 0; for (int r = 0; r < BS; r++) k += tp.rowid[(size_t)tt * BS + r] >= 0; return k; };
    std::vector<int> ai(32 * (size_t)pl.A.nchunks, 0), ac(pl.A.nchunks, 0);
    for (int c = 0; c < pl.A.nchunks; c++) {
      ac[c] = tp.ta_ptr[c + 1] - tp.ta_ptr[c];
      for (int u = 0; u < 8; u++) {
        const int tt = u < ac[c] ? tp.ta_tid[tp.ta_ptr[c] + u] : tp.ntile;
        int rec[4] = {tt, tp.tJ[tt], first(tt), rows(tt)};
        std::copy(rec, rec + 4, ai.begin() + 32 * (size_t)c + 4 * u);
      }
    }
    UP(upload(h, ai, &t.ta_info)); UP(upload(h, ac, &t.ta_cnt));
    std::vector<int> ti(16 * (size_t)pl.At.nchunks, 0);
    for (int J = 0; J < 4 * pl.At.nchunks; J++) {
      const int tt = (J < pl.nb && tp.tt_ptr[J + 1] > tp.tt_ptr[J]) ? tp.tt_tid[tp.tt_ptr[J]] : tp.ntile;
      int rec[4] = {tt, first(tt), rows(tt), 0};
      std::copy(rec, rec + 4, ti.begin() + 4 * (size_t)J);
    }
    UP(upload(h, ti, &t.tt_info));
  }
  std::vector<unsigned long long> mask(pl.A.nchunks, 0ull);
  for (size_t k = 0; k < (size_t)tp.ntile * BS; k++) if (tp.rowid[k] >= 0) mask[tp.rowid[k] / WAVE] |= 1ull << (tp.rowid[k] % WAVE);
  UP(upload(h, mask, &t.ta_mask));
  t.o_tile = s.wl.tile; t.o_ellAr = s.wl.ellAr; t.o_ellAtr = s.wl.ellAtr;
  return MPCQP_OK;
}
// on-chip mode: the chain / hub tables, the set-up kernel's copies of the arguments in its own launch shape, and what only the device knows --
// whether the table has the tile instance, and how many iteration workgroups it holds at once
static int upload_onchip(mpcqp_handle *h, int cus) {
  Selection &s = h->sel; const Plan &pl = s.plan; const OcPlan &o = s.ocplan; const ResPlan &rp = s.rplan; DevRes &dr = h->dres; DevOc &d = h->doc;
  dr.stage = s.stage; dr.rext = oc_rext(rp.nw, std::max<int>(1, (int)o.pairs.size())); dr.nconst = 0; dr.n_seg = 0;
  d.nbc = o.nbc; d.has_hub = o.has_hub; d.junc = o.junc; d.npw = o.npw; d.nhr = o.nhr; d.nlds = o.nlds; d.ntab = (int)o.tab.size();
  d.o_chainE = o.o_chainE; d.o_chainF = o.o_chainF; d.o_pos = o.o_pos; d.o_fill = o.o_fill; d.ghub_slot = o.ghub_slot; d.ghub_src = o.ghub_src;
  d.npair = (int)o.pairs.size(); d.o_pair = o.o_pair; d.nfill = o.nfill; d.o_s = o.o_s; d.o_dbl = o.o_dbl; d.ndbl = (int)o.dbl.size(); d.o_pp = o.o_pp;
  d.at_poll = s.at_poll; d.at_free = s.at_free;
  d.a_lds = s.a_lds; d.p_lds = s.p_lds;
  if (s.vtiles && !mpcqp_kernel_oc_admm_tl(s.waves, s.oc_ng(), s.oc_nh())) s.vtiles = false;      // (the table has the tile instance for two of the shapes only)
  UP(upload(h, o.tab, &d.tab));
  UP(upload(h, oc_setup_tables(pl, s.tlds, s.sing, s.at_map), &d.asm_rec));
  if (s.tiles || s.vtiles) UP(upload_tiles(h));
  // (after the tables are uploaded: the set-up kernel's copies of the arguments)
  const SetupShape &su = s.setup; DevRes &ds = h->dres_setup; DevOc &dd = h->doc_setup;
  ds = dr; dd = d;
  dd.a_lds = su.a_lds; dd.p_lds = su.p_lds; dd.ix16 = su.ix16; dd.zpad = su.zpad; dd.ixo_a = su.ixo_a; dd.ixo_p = su.ixo_p;
  dd.no_ruiz_regs = h->knobs.no_ruiz_regs ? 1 : 0;
  dd.su_path = setup_path_bits(s);
  ds.stage = su.stage;
  if (!s.split) return MPCQP_OK;
  if (s.oc8 && !s.vtiles && !s.a_assign.empty()) UP(upload(h, s.a_assign, &d.a_assign));
  if (s.oc8) {
    int nb = 0; h->qslots = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, oc_admm_of(h, false), s.waves * WAVE, (size_t)s.lds) == hipSuccess && nb > 0) {
      h->qslots = nb * (cus > 0 ? cus : 256);
    } else (void)hipGetLastError();
    UP(dalloc(h, &h->qctr, 16 * 16));
  }
  if (h->knobs.verbose) fprintf(stderr, "%s, %d resident workgroups\n", setup_shape_text(s).c_str(), h->qslots);
  return MPCQP_OK;
}
// the per-QP slabs and the outputs
static int alloc_workspace(mpcqp_handle *h) {
  const size_t stride = (size_t)h->sel.wl.stride, batch = (size_t)h->batch; const int n = h->n, m = h->m;
  UP(dalloc(h, &h->ws, stride * batch));
  // the resident kernels only ever write the structural non-zeros of the T tiles (fixed positions, plan.hpp tpos): their zeros are set here, once
  HIPCHK(hipMemset(h->ws, 0, stride * batch * sizeof(double))); HIPCHK(hipStreamSynchronize(0));
  UP(dalloc(h, &h->ox, batch * n)); UP(dalloc(h, &h->oy, batch * std::max(m, 1))); UP(dalloc(h, &h->oz, batch * std::max(m, 1)));
  UP(dalloc(h, &h->oinfo, batch * 4)); UP(dalloc(h, &h->ocs, batch));
  UP(dalloc(h, &h->ostatus, batch)); UP(dalloc(h, &h->oiters, batch));
#ifdef MPCQP_TIMING
  UP(dalloc(h, &h->odbg, batch * 16 + 128));
#endif
  // dispatch-hint buffers up front: nothing is allocated inside mpcqp_solve, so a solve can be captured in a HIP graph
  UP(dalloc(h, &h->order[0], batch)); UP(dalloc(h, &h->order[1], batch));
  return MPCQP_OK;
}
#undef UP
// the handle's kernel instances: their dynamic-LDS limit, and that the table has them at all
static int prepare_kernels(mpcqp_handle *h) {
  const Selection &s = h->sel;
  if (s.lds > 48 * 1024) {
    // MaxDynamicSharedMemorySize is a property of the kernel function, shared by every handle that launches it: keep a running
    // maximum per function so that a later handle with a smaller footprint never lowers the limit under an earlier one
    static std::mutex mu; static std::map<std::pair<const void *, int>, long> limit;   // (function, device)
    const void *fns[7] = {res_kernel_of(h, false), res_kernel_of(h, true), nullptr, nullptr, nullptr, nullptr, nullptr};
    if (s.waves == 0) fns[0] = fns[1] = stream_kernel_of(h);
    if (s.split) { fns[0] = oc_setup_of(h, false); fns[1] = oc_setup_of(h, true); fns[2] = oc_admm_of(h, false); fns[3] = oc_admm_of(h, true); fns[4] = oc_rescale_of(h); }
    if (takes_soft_rows(s)) { fns[5] = oc_admm_soft_of(h, false); fns[6] = oc_admm_soft_of(h, true); }      // (the twins a later mpcqp_set_soft_rows switches to: the limit is set here, once)
    std::lock_guard<std::mutex> lock(mu);
    for (int k = 0; k < 7; k++) {
      const void *fn = fns[k];
      if (!fn) continue;
      const long want_lds = (s.split && (k < 2 || k == 4)) ? s.setup.lds : s.lds;
      long &cur = limit[{fn, h->device}];
      if (want_lds <= cur) continue;
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want_lds) != hipSuccess)
        return fail(MPCQP_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      cur = want_lds;
    }
  }
  if (s.waves > 0 && !(s.split ? oc_setup_of(h, false) && oc_setup_of(h, true) && oc_admm_of(h, false) && oc_admm_of(h, true) : res_kernel_of(h, false) && res_kernel_of(h, true)))
    return fail(MPCQP_ERR_STATE, "no kernel instance for this handle (kernel_table.hpp)");
  return MPCQP_OK;
}
// A handle on `family` ("" = the rule's choice, null = MPCQP_VARIANT if set, else the rule): arguments are checked by the callers.
static int create_handle(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                         const mpcqp_settings *settings, const char *family, const Knobs &knobs, mpcqp_handle **out) {
  mpcqp_settings st;
  if (settings) st = *settings; else mpcqp_default_settings(&st);
  int dev = 0, cus = 0, rc;
  if ((rc = mpcqp_pick_device(st.device, &dev))) return rc;
  if (hipSetDevice(dev) != hipSuccess) return fail(MPCQP_ERR_HIP, "hipSetDevice failed");
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
  mpcqp_handle *h = new mpcqp_handle();
  h->st = st; h->device = dev; h->n = n; h->m = m; h->batch = batch; h->knobs = knobs;
  h->sel = select_kernel(n, m, batch, Pp, Pi, Ap, Ai, cus, family, knobs);
  const Selection &s = h->sel;
  rc = s.err ? fail(s.err, s.error) : MPCQP_OK;
  if (!rc) rc = upload_plan(h);
  if (!rc && s.waves > 0) rc = upload_resident(h);
  if (!rc && s.oc) rc = upload_onchip(h, cus);
  if (!rc) rc = alloc_workspace(h);
  if (!rc) rc = prepare_kernels(h);
  if (!rc && (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess || hipEventCreate(&h->ev_mid) != hipSuccess ||
              hipEventCreateWithFlags(&h->ev_order, hipEventDisableTiming) != hipSuccess)) rc = fail(MPCQP_ERR_HIP, "hipEventCreate failed");
  if (rc) { mpcqp_destroy(h); return rc; }
  memset(&h->io, 0, sizeof(h->io));
  h->lpt = !knobs.no_lpt;
  *out = h;
  return MPCQP_OK;
}

extern "C" {

void mpcqp_default_settings(mpcqp_settings *s) {
  if (!s) return;
  s->rho = 0.1; s->sigma = 1e-6; s->alpha = 1.6; s->eps_abs = 1e-3; s->eps_rel = 1e-3;
  s->eps_prim_inf = 1e-4; s->eps_dual_inf = 1e-4; s->adaptive_rho_tolerance = 5.0;
  s->max_iter = 10000; s->check_termination = 25; s->scaling = 10; s->adaptive_rho = 1;
  s->adaptive_rho_interval = 0; s->scaled_termination = 0; s->warm_start = 0; s->device = -1;
}

const char *mpcqp_strerror(int code) {
  static thread_local std::string buf;
  const char *base = "unknown error";
  switch (code) {
    case MPCQP_OK: base = "ok"; break;
    case MPCQP_ERR_ARG: base = "invalid argument"; break;
    case MPCQP_ERR_HIP: base = "HIP runtime error"; break;
    case MPCQP_ERR_NO_GPU: base = "no usable gfx950 GPU (this library has no CPU fallback)"; break;
    case MPCQP_ERR_STATE: base = "call order violated"; break;
    case MPCQP_ERR_LIMIT: base = "problem exceeds on-chip budget"; break;
  }
  buf = base;
  if (code != MPCQP_OK && !g_last_error.empty()) buf += ": " + g_last_error;
  return buf.c_str();
}

int mpcqp_create(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                 const mpcqp_settings *settings, mpcqp_handle **out) {
  if (!out) return fail(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (n <= 0 || m < 0 || batch <= 0 || !Pp || !Pi || !Ap || !Ai) return fail(MPCQP_ERR_ARG, "Invalid dimensions.");
  const Knobs knobs = Knobs::from_env();
  if (!knobs.variant_named && knobs.autotune) return mpcqp_create_tuned(n, m, batch, Pp, Pi, Ap, Ai, settings, out);
  return create_handle(n, m, batch, Pp, Pi, Ap, Ai, settings, nullptr, knobs, out);
}

// ---- kernel family by measurement (include/mpcqp.h mpcqp_create_tuned)
static std::mutex g_tune_mu;
static std::map<std::string, std::string> g_tune_cache;     // pattern + batch + device -> family
static std::string tune_key(int n, int m, int batch, int dev, const int *Pp, const int *Pi, const int *Ap, const int *Ai) {
  unsigned long long hsh = 1469598103934665603ULL;          // FNV-1a over the index arrays
  auto mix = [&](const int *p, long cnt) { for (long k = 0; k < cnt; k++) { hsh ^= (unsigned)p[k]; hsh *= 1099511628211ULL; } };
  mix(Pp, n + 1); mix(Pi, Pp[n]); mix(Ap, n + 1); mix(Ai, Ap[n]);
  return std::to_string(n) + "x" + std::to_string(m) + "x" + std::to_string(batch) + "@" + std::to_string(dev) + ":" + std::to_string(hsh);
}
int mpcqp_create_tuned(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                       const mpcqp_settings *settings, mpcqp_handle **out) {
  if (!out) return fail(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (n <= 0 || m < 0 || batch <= 0 || !Pp || !Pi || !Ap || !Ai) return fail(MPCQP_ERR_ARG, "Invalid dimensions.");
  if (int rc = check_csc(n, m, Pp, Pi, Ap, Ai, true)) return rc;      // (before the pattern is hashed and a synthetic QP filled through it)
  const Knobs knobs = Knobs::from_env();
  auto create = [&](const std::string &family, const mpcqp_settings *sts, mpcqp_handle **o) { return create_handle(n, m, batch, Pp, Pi, Ap, Ai, sts, family == "rule" ? "" : family.c_str(), knobs, o); };
  mpcqp_settings st; if (settings) st = *settings; else mpcqp_default_settings(&st);
  int dev = st.device; if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  const std::string key = tune_key(n, m, batch, dev, Pp, Pi, Ap, Ai);
  {
    std::string cached;
    { std::lock_guard<std::mutex> lock(g_tune_mu); auto it = g_tune_cache.find(key); if (it != g_tune_cache.end()) cached = it->second; }
    if (!cached.empty()) {
      const int rc = create(cached, settings, out);
      if (rc != MPCQP_ERR_LIMIT || cached == "rule") return rc;
      return create("rule", settings, out);       // the cached family no longer takes the size (other settings): the rule's choice instead of an error
    }
  }
  // the synthetic QP on this pattern: P = unit diagonal (other entries 0: positive semidefinite whatever the pattern), A pseudo-random in
  // [-1, 1], q pseudo-random, -1 <= A x <= 1 (feasible at the origin); one instance shared by the batch (stride 0)
  const long nnzP = Pp[n], nnzA = Ap[n];
  std::vector<double> Pv(std::max<long>(nnzP, 1), 0.0), Av(std::max<long>(nnzA, 1), 0.0), qv(n), lv(std::max(m, 1), -1.0), uv(std::max(m, 1), 1.0);
  unsigned long long seed = 88172645463325252ULL;
  auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  for (int j = 0; j < n; j++) for (int k = Pp[j]; k < Pp[j + 1]; k++) if (Pi[k] == j) Pv[k] = 1.0;
  for (long k = 0; k < nnzA; k++) Av[k] = rnd();
  for (int j = 0; j < n; j++) qv[j] = rnd();
  // fixed work: set-up + TUNE_ITERS ADMM iterations, no early exit (eps = 0), no adaptive rho -- what a typical MPC solve costs (25 - 50 iterations)
  mpcqp_settings ts = st;
  ts.max_iter = 50; ts.eps_abs = ts.eps_rel = 0.0; ts.eps_prim_inf = ts.eps_dual_inf = 0.0; ts.adaptive_rho = 0; ts.warm_start = 0;
  const char *families[] = {"", "oc4", "oc8", "gres4", "gres2", "res4", "res2", "res1"};
  mpcqp_handle *best = nullptr; float best_ms = 0.f; std::string best_family; long seen_codes[8]; int nseen = 0;
  std::vector<double> xref;
  int last_rc = MPCQP_ERR_LIMIT;
  for (const char *fam : families) {
    mpcqp_handle *h = nullptr;
    const int rc = create(fam, &ts, &h);
    if (rc != MPCQP_OK) { if (rc != MPCQP_ERR_LIMIT) last_rc = rc; continue; }
    long info[16]; mpcqp_plan_info(h, info);
    const long code = info[15] * 1000000 + info[7];                 // family + LDS footprint: the same kernel instance is timed once
    bool dup = false; for (int k = 0; k < nseen; k++) dup |= seen_codes[k] == code;
    if (dup) { mpcqp_destroy(h); continue; }
    seen_codes[nseen++] = code;
    float ms = 0.f; bool ok = true;
    mpcqp_set_dispatch_hint(h, 0);
    ok = mpcqp_update(h, Pv.data(), 0, qv.data(), 0, Av.data(), 0, lv.data(), 0, uv.data(), 0, MPCQP_MEM_HOST) == MPCQP_OK;
    for (int rep = 0; rep < 2 && ok; rep++) ok = mpcqp_solve(h, nullptr) == MPCQP_OK && mpcqp_last_kernel_ms(h, &ms) == MPCQP_OK;     // (the first launch warms the code object)
    // a candidate only counts if it did the work: every instance ran the full iteration count, and its x agrees with the first
    // candidate's (the families are the same algorithm: the first and the last instance of the batch are compared to 1e-6)
    if (ok) {
      std::vector<int> stt(batch), itr(batch); std::vector<double> xs((size_t)batch * n);
      ok = mpcqp_get(h, xs.data(), nullptr, nullptr, stt.data(), itr.data(), nullptr, MPCQP_MEM_HOST) == MPCQP_OK;
      for (int b = 0; b < batch && ok; b++) ok = itr[b] == ts.max_iter && (stt[b] == MPCQP_MAX_ITER_REACHED || stt[b] == MPCQP_SOLVED || stt[b] == MPCQP_SOLVED_INACCURATE);
      if (ok) {
        std::vector<double> x0(xs.begin(), xs.begin() + n), x1(xs.end() - n, xs.end());
        if (xref.empty()) xref = x0;
        double scale = 1.0, err = 0.0;
        for (int j = 0; j < n; j++) { scale = std::max(scale, std::fabs(xref[j])); err = std::max(err, std::max(std::fabs(x0[j] - xref[j]), std::fabs(x1[j] - xref[j]))); }
        ok = err == err && err <= 1e-6 * scale;
      }
    }
    if (!ok) { mpcqp_destroy(h); continue; }
    if (!best || ms < best_ms) { if (best) mpcqp_destroy(best); best = h; best_ms = ms; best_family = fam[0] ? fam : "rule"; }
    else mpcqp_destroy(h);
  }
  if (!best) return last_rc == MPCQP_ERR_LIMIT ? fail(MPCQP_ERR_LIMIT, "no kernel family takes this pattern / size") : last_rc;
  mpcqp_destroy(best);       // (its settings were the tuning run's: the handle that is returned is created afresh with the caller's)
  { std::lock_guard<std::mutex> lock(g_tune_mu); g_tune_cache[key] = best_family; }
  return create(best_family, settings, out);
}

int mpcqp_create_reduced(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                         int nfixed, const int *fixed_rows, const mpcqp_settings *settings, mpcqp_handle **out) {
  if (!out) return fail(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (n <= 0 || m <= 0 || batch <= 0 || !Pp || !Pi || !Ap || !Ai || nfixed < 0 || (nfixed > 0 && !fixed_rows)) return fail(MPCQP_ERR_ARG, "Invalid dimensions.");
  if (int rc = check_csc(n, m, Pp, Pi, Ap, Ai, false)) return rc;
  RedMaps rm = build_red_maps(n, m, Pp, Pi, Ap, Ai, nfixed, fixed_rows);
  if (!rm.error.empty()) return fail(MPCQP_ERR_ARG, rm.error);
  mpcqp_handle *inner = nullptr;
  int rc = mpcqp_create(rm.nr, rm.mr, batch, rm.Ppr.data(), rm.Pir.data(), rm.Apr.data(), rm.Air.data(), settings, &inner);
  if (rc) return rc;
  mpcqp_handle *h = new mpcqp_handle();
  h->inner = inner; h->st = inner->st; h->device = inner->device; h->n = n; h->m = m; h->batch = batch; h->sel.waves = -1;
  h->sel.plan.n = n; h->sel.plan.m = m; h->sel.plan.nnzP_in = Pp[n]; h->sel.plan.nnzA_in = Ap[n];
  h->red = rm;
  auto bail = [&](int code) { mpcqp_destroy(h); return code; };
  DevRed &d = h->dred;
  memset(&d, 0, sizeof(d));
  d.n = n; d.m = m; d.nr = rm.nr; d.mr = rm.mr; d.nfix = rm.nfix; d.nnzPr = (int)rm.Pir.size(); d.nnzAr = (int)rm.Air.size();
#define UP(expr) if ((rc = (expr))) return bail(rc)
  UP(upload(h, rm.Psrc, &d.Psrc)); UP(upload(h, rm.Asrc, &d.Asrc)); UP(upload(h, rm.fix_var, &d.fix_var)); UP(upload(h, rm.fix_row, &d.fix_row));
  UP(upload(h, rm.fix_src, &d.fix_src)); UP(upload(h, rm.free_var, &d.free_var)); UP(upload(h, rm.kept_row, &d.kept_row));
  UP(upload(h, rm.var_of, &d.var_of)); UP(upload(h, rm.row_of, &d.row_of));
  UP(upload(h, rm.qc_ptr, &d.qc_ptr)); UP(upload(h, rm.qc_k, &d.qc_k)); UP(upload(h, rm.qc_src, &d.qc_src));
  UP(upload(h, rm.lc_ptr, &d.lc_ptr)); UP(upload(h, rm.lc_k, &d.lc_k)); UP(upload(h, rm.lc_src, &d.lc_src));
  UP(upload(h, rm.yp_ptr, &d.yp_ptr)); UP(upload(h, rm.yp_var, &d.yp_var)); UP(upload(h, rm.yp_src, &d.yp_src));
  UP(upload(h, rm.ya_ptr, &d.ya_ptr)); UP(upload(h, rm.ya_row, &d.ya_row)); UP(upload(h, rm.ya_src, &d.ya_src));
  const size_t B = batch;
  UP(dalloc(h, &d.Pr, B * std::max(d.nnzPr, 1))); UP(dalloc(h, &d.qr, B * rm.nr)); UP(dalloc(h, &d.Ar, B * std::max(d.nnzAr, 1)));
  UP(dalloc(h, &d.lr, B * std::max(rm.mr, 1))); UP(dalloc(h, &d.ur, B * std::max(rm.mr, 1))); UP(dalloc(h, &d.xfix, B * std::max(rm.nfix, 1)));
  UP(dalloc(h, &d.bad, B));
  if (h->st.warm_start) { UP(dalloc(h, &h->rx0, B * rm.nr)); UP(dalloc(h, &h->ry0, B * std::max(rm.mr, 1))); }     // (nothing is allocated inside a solve: it stays graph-capturable)
  UP(dalloc(h, &h->ox, B * n)); UP(dalloc(h, &h->oy, B * m)); UP(dalloc(h, &h->oz, B * m));
  UP(dalloc(h, &h->oinfo, B * 4)); UP(dalloc(h, &h->ostatus, B)); UP(dalloc(h, &h->oiters, B));
#undef UP
  memset(&h->io, 0, sizeof(h->io));
  if (hipEventCreateWithFlags(&h->ev0r, hipEventDisableTiming) != hipSuccess) return bail(fail(MPCQP_ERR_HIP, "hipEventCreate failed"));
  *out = h;
  return MPCQP_OK;
}

int mpcqp_create_presolved(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                           const double *l, long sl, const double *u, long su, int mem,
                           const mpcqp_settings *settings, mpcqp_handle **out, int *nfixed_out) {
  if (!out) return fail(MPCQP_ERR_ARG, "out is null");
  *out = nullptr;
  if (nfixed_out) *nfixed_out = 0;
  if (n <= 0 || m <= 0 || batch <= 0 || !Pp || !Pi || !Ap || !Ai || !l || !u) return fail(MPCQP_ERR_ARG, "Invalid dimensions.");
  if (sl < 0 || su < 0 || (sl && sl < m) || (su && su < m)) return fail(MPCQP_ERR_ARG, "stride smaller than the array it strides (dimension mismatch)");
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  if (int rc = check_csc(n, m, nullptr, nullptr, Ap, Ai, true)) return rc;
  // the bounds of the first update on the host (device arrays: one copy, at creation only)
  const size_t nl = sl ? (size_t)sl * (batch - 1) + m : (size_t)m, nu = su ? (size_t)su * (batch - 1) + m : (size_t)m;
  std::vector<double> hl, hu;
  if (mem == MPCQP_MEM_DEVICE) {
    hl.resize(nl); hu.resize(nu);
    HIPCHK(hipMemcpy(hl.data(), l, nl * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hu.data(), u, nu * sizeof(double), hipMemcpyDeviceToHost));
    l = hl.data(); u = hu.data();
  }
  // rows with a single entry in A whose bounds coincide in EVERY instance; one row per variable (a second one stays an ordinary row)
  std::vector<int> cnt(m, 0), col(m, -1);
  for (int j = 0; j < n; j++) for (int k = Ap[j]; k < Ap[j + 1]; k++) { cnt[Ai[k]]++; col[Ai[k]] = j; }
  std::vector<char> taken(n, 0);
  std::vector<int> rows;
  for (int i = 0; i < m; i++) {
    if (cnt[i] != 1 || taken[col[i]]) continue;
    bool eq = true;
    for (int b = 0; b < (sl || su ? batch : 1) && eq; b++) {
      const double lo = l[(size_t)b * sl + i], up = u[(size_t)b * su + i];
      eq = std::fabs(up - lo) <= 1e-9 * std::max(1.0, std::fabs(lo)) && std::fabs(lo) < 1e20;      // (the presolve kernel's own test of the promise)
    }
    if (eq) { rows.push_back(i); taken[col[i]] = 1; }
  }
  if ((int)rows.size() >= n) rows.resize(n - 1);       // (a QP with every variable fixed keeps one: the reduced pattern needs a variable)
  if (nfixed_out) *nfixed_out = (int)rows.size();      // (what is eliminated: after the clip)
  if (rows.empty()) return mpcqp_create(n, m, batch, Pp, Pi, Ap, Ai, settings, out);      // nothing to eliminate: the ordinary handle
  return mpcqp_create_reduced(n, m, batch, Pp, Pi, Ap, Ai, (int)rows.size(), rows.data(), settings, out);
}

// the solve of a reduced handle: substitute the fixed variables, hand the smaller QP to the inner handle, expand its result
static int solve_reduced(mpcqp_handle *h, hipStream_t s) {
  mpcqp_handle *in = h->inner; const DevRed &d = h->dred;
  const bool vectors = h->reuse_next, matrices = h->rescale_next;
  // the presolve overwrites the reduced arrays the previous solve of this handle read: if that one ran on another stream, wait for it
  if (h->solved && h->last_stream != s) { HIPCHK(hipEventRecord(h->ev0r, h->last_stream)); HIPCHK(hipStreamWaitEvent(s, h->ev0r, 0)); }
  hipLaunchKernelGGL(mpcqp_presolve_kernel, dim3(h->batch), dim3(256), 0, s, d, h->io, vectors ? 1 : 0, h->skip);
  HIPCHK(hipGetLastError());
  int rc;
  if (vectors) rc = mpcqp_update_vectors(in, d.qr, d.nr, d.lr, d.mr, d.ur, d.mr, MPCQP_MEM_DEVICE);
  else if (matrices) rc = mpcqp_update_matrices(in, d.Pr, d.nnzPr, d.qr, d.nr, d.Ar, d.nnzAr, d.lr, d.mr, d.ur, d.mr, MPCQP_MEM_DEVICE);
  else rc = mpcqp_update(in, d.Pr, d.nnzPr, d.qr, d.nr, d.Ar, d.nnzAr, d.lr, d.mr, d.ur, d.mr, MPCQP_MEM_DEVICE);
  if (rc) return rc;
  if (h->st.warm_start && h->io.x0 && h->io.y0) {
    if (!h->rx0) return fail(MPCQP_ERR_STATE, "warm start on a reduced handle: settings.warm_start must be set when the handle is created");
    hipLaunchKernelGGL(mpcqp_red_gather_kernel, dim3(h->batch), dim3(256), 0, s, d, h->io.x0, h->io.y0, h->rx0, h->ry0, h->skip);
    HIPCHK(hipGetLastError());
    if ((rc = mpcqp_warm_start(in, h->rx0, h->ry0, MPCQP_MEM_DEVICE))) return rc;
  }
  if ((rc = mpcqp_solve(in, (void *)s))) return rc;
  const bool pol = in->polish && h->opinfo;      // (the inner handle's polish outcome comes back with the objective's constant, like info[0])
  hipLaunchKernelGGL(mpcqp_postsolve_kernel, dim3(h->batch), dim3(256), 0, s, d, h->io, in->ox, in->oy, in->oz, in->ostatus, in->oiters, in->oinfo,
                     pol ? in->opstatus : (const int *)nullptr, pol ? in->opinfo : (const double *)nullptr,
                     h->ox, h->oy, h->oz, h->ostatus, h->oiters, h->oinfo, h->opstatus, h->opinfo, h->skip);
  HIPCHK(hipGetLastError());
  note_skip_state(h, vectors ? 1 : matrices ? 2 : 0);
  h->last_stream = s; h->solved = true; h->have_factor = h->keep; h->reuse_next = false; h->rescale_next = false;
  return MPCQP_OK;
}

static int stage(mpcqp_handle *h, double **own, const double *src, long stride, long width, const double **dst, long *dstride) {
  // host-memory update: copy into an owned device buffer
  size_t count = stride == 0 ? (size_t)width : (size_t)stride * (h->batch - 1) + width;
  if (!*own) { int rc = dalloc(h, own, (size_t)std::max<long>(width, 1) * h->batch); if (rc) return rc; }
  if (stride != 0 && stride != width) {
    for (int b = 0; b < h->batch; b++) HIPCHK(hipMemcpy(*own + (size_t)b * width, src + (size_t)b * stride, width * sizeof(double), hipMemcpyHostToDevice));
    *dstride = width;
  } else {
    HIPCHK(hipMemcpy(*own, src, count * sizeof(double), hipMemcpyHostToDevice));
    *dstride = stride;
  }
  *dst = *own;
  return MPCQP_OK;
}

// what mpcqp_update and mpcqp_update_matrices share: the argument checks, and the five arrays borrowed (device memory) or copied into the handle's own buffers
static int set_problem_data(mpcqp_handle *h, const double *P, long sP, const double *q, long sq, const double *A, long sA,
                            const double *l, long sl, const double *u, long su, int mem) {
  if (!q || (h->sel.plan.nnzP_in > 0 && !P) || (h->sel.plan.nnzA_in > 0 && !A) || (h->m > 0 && (!l || !u))) return fail(MPCQP_ERR_ARG, "null data pointer");
  if (sP < 0 || sq < 0 || sA < 0 || sl < 0 || su < 0) return fail(MPCQP_ERR_ARG, "negative stride");
  if ((sP && sP < h->sel.plan.nnzP_in) || (sq && sq < h->n) || (sA && sA < h->sel.plan.nnzA_in) || (sl && sl < h->m) || (su && su < h->m))
    return fail(MPCQP_ERR_ARG, "stride smaller than the array it strides (dimension mismatch)");
  HIPCHK(hipSetDevice(h->device));
  DevIO &io = h->io;
  if (mem == MPCQP_MEM_DEVICE) {
    // (an array that may be NULL because it is empty is pointed at q, as on the host path: the gathers of the set-up kernels load element 0 for a phantom slot
    // before they discard it -- gather8, rz_fill_p -- and must find memory there)
    io.P = P ? P : q; io.sP = P ? sP : 0; io.q = q; io.sq = sq; io.A = A ? A : q; io.sA = A ? sA : 0;
    io.l = l ? l : q; io.sl = l ? sl : 0; io.u = u ? u : q; io.su = u ? su : 0;
  } else if (mem == MPCQP_MEM_HOST) {
    if (h->last_stream || h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));
    int rc;
    if ((rc = stage(h, &h->dP, P ? P : q, sP, h->sel.plan.nnzP_in, &io.P, &io.sP))) return rc;
    if ((rc = stage(h, &h->dq, q, sq, h->n, &io.q, &io.sq))) return rc;
    if ((rc = stage(h, &h->dA, A ? A : q, sA, h->sel.plan.nnzA_in, &io.A, &io.sA))) return rc;
    if ((rc = stage(h, &h->dl, l ? l : q, sl, h->m, &io.l, &io.sl))) return rc;
    if ((rc = stage(h, &h->du, u ? u : q, su, h->m, &io.u, &io.su))) return rc;
  } else return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  return MPCQP_OK;
}

int mpcqp_update(mpcqp_handle *h, const double *P, long sP, const double *q, long sq, const double *A, long sA,
                 const double *l, long sl, const double *u, long su, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (int rc = set_problem_data(h, P, sP, q, sq, A, sA, l, sl, u, su, mem)) return rc;
  h->have_data = true; h->reuse_next = false; h->rescale_next = false;
  return MPCQP_OK;
}

int mpcqp_update_matrices(mpcqp_handle *h, const double *P, long sP, const double *q, long sq, const double *A, long sA,
                          const double *l, long sl, const double *u, long su, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->keep || !h->have_factor)
    return fail(MPCQP_ERR_STATE, "mpcqp_update_matrices needs mpcqp_keep_workspace(h, 1) and a completed mpcqp_update + mpcqp_solve before it");
  if (h->skip_full)
    return fail(MPCQP_ERR_STATE, "mpcqp_update_matrices: the last full set-up ran under a skip array (mpcqp_set_skip), so the skipped instances hold no scaling "
                                 "of this handle's data; run mpcqp_update + mpcqp_solve without a skip array first");
  if (!takes_matrix_updates(h->inner ? h->inner : h))
    return fail(MPCQP_ERR_LIMIT, "mpcqp_update_matrices: this handle does not run the two-kernel on-chip form (use mpcqp_update)");
  if (int rc = set_problem_data(h, P, sP, q, sq, A, sA, l, sl, u, su, mem)) return rc;
  h->reuse_next = false; h->rescale_next = true; h->rescale_done = false;
  return MPCQP_OK;
}

int mpcqp_warm_start(mpcqp_handle *h, const double *x0, const double *y0, int mem) {
  if (!h || !x0 || !y0) return fail(MPCQP_ERR_ARG, "null pointer");
  HIPCHK(hipSetDevice(h->device));
  if (mem == MPCQP_MEM_DEVICE) { h->io.x0 = x0; h->io.y0 = y0; return MPCQP_OK; }
  int rc;
  if (!h->dx0) { if ((rc = dalloc(h, &h->dx0, (size_t)h->batch * h->n))) return rc; if ((rc = dalloc(h, &h->dy0, (size_t)h->batch * std::max(h->m, 1)))) return rc; }
  HIPCHK(hipMemcpy(h->dx0, x0, (size_t)h->batch * h->n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->dy0, y0, (size_t)h->batch * h->m * sizeof(double), hipMemcpyHostToDevice));
  h->io.x0 = h->dx0; h->io.y0 = h->dy0;
  return MPCQP_OK;
}

int mpcqp_set_dispatch_hint(mpcqp_handle *h, int enable) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (h->inner) return mpcqp_set_dispatch_hint(h->inner, enable);
  h->lpt = enable != 0;
  if (!h->lpt) h->order_cur = -1;
  return MPCQP_OK;
}

int mpcqp_keep_workspace(mpcqp_handle *h, int enable) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (h->inner) {
    const int rc = mpcqp_keep_workspace(h->inner, enable);
    if (rc) return rc;
    h->keep = enable != 0;
    if (!h->keep) { h->have_factor = false; h->reuse_next = false; h->rescale_next = false; }
    return MPCQP_OK;
  }
  if (enable && h->sel.waves == 0) return fail(MPCQP_ERR_LIMIT, "the streaming kernel variant does not keep its workspace");
  h->keep = enable != 0;
  if (!h->keep) { h->have_factor = false; h->reuse_next = false; h->rescale_next = false; }
  return MPCQP_OK;
}

int mpcqp_update_vectors(mpcqp_handle *h, const double *q, long sq, const double *l, long sl, const double *u, long su, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->keep || !h->have_factor)
    return fail(MPCQP_ERR_STATE, "mpcqp_update_vectors needs mpcqp_keep_workspace(h, 1) and a completed mpcqp_update + mpcqp_solve before it");
  if (h->skip_full)
    return fail(MPCQP_ERR_STATE, "mpcqp_update_vectors: the last full set-up ran under a skip array (mpcqp_set_skip), so the skipped instances hold no factor "
                                 "of this handle's matrices; run mpcqp_update + mpcqp_solve without a skip array first");
  if (h->skip_mat && !(h->rescale_next && !h->rescale_done))
    return fail(MPCQP_ERR_STATE, "mpcqp_update_vectors: the last mpcqp_update_matrices solve ran under a skip array (mpcqp_set_skip), so the skipped instances' "
                                 "factors are of older matrices; run an mpcqp_update_matrices or mpcqp_update solve without a skip array first");
  if (!q || (h->m > 0 && (!l || !u))) return fail(MPCQP_ERR_ARG, "null data pointer");
  if (sq < 0 || sl < 0 || su < 0 || (sq && sq < h->n) || (sl && sl < h->m) || (su && su < h->m)) return fail(MPCQP_ERR_ARG, "dimension mismatch: stride shorter than the array");
  HIPCHK(hipSetDevice(h->device));
  DevIO &io = h->io;
  if (mem == MPCQP_MEM_DEVICE) {
    io.q = q; io.sq = sq; io.l = l ? l : q; io.sl = l ? sl : 0; io.u = u ? u : q; io.su = u ? su : 0;      // (m = 0: as in set_problem_data)
  } else if (mem == MPCQP_MEM_HOST) {
    if (h->last_stream || h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));
    int rc;
    if ((rc = stage(h, &h->dq, q, sq, h->n, &io.q, &io.sq))) return rc;
    if ((rc = stage(h, &h->dl, l ? l : q, sl, h->m, &io.l, &io.sl))) return rc;
    if ((rc = stage(h, &h->du, u ? u : q, su, h->m, &io.u, &io.su))) return rc;
  } else return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  // (between mpcqp_update_matrices and its solve: that solve scales these vectors with the rest; behind it, the factor it left is kept)
  if (!(h->rescale_next && !h->rescale_done)) { h->reuse_next = true; h->rescale_next = false; }
  return MPCQP_OK;
}

int mpcqp_set_rho(mpcqp_handle *h, const double *rho0, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (h->inner) return mpcqp_set_rho(h->inner, rho0, mem);
  HIPCHK(hipSetDevice(h->device));
  if (!rho0) { h->io.rho0 = nullptr; return MPCQP_OK; }
  if (mem == MPCQP_MEM_DEVICE) { h->io.rho0 = rho0; return MPCQP_OK; }
  if (mem != MPCQP_MEM_HOST) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  int rc;
  if (!h->drho0) { if ((rc = dalloc(h, &h->drho0, (size_t)h->batch))) return rc; }
  HIPCHK(hipMemcpy(h->drho0, rho0, (size_t)h->batch * sizeof(double), hipMemcpyHostToDevice));
  h->io.rho0 = h->drho0;
  return MPCQP_OK;
}

int mpcqp_set_skip(mpcqp_handle *h, const int *skip, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!skip) { h->skip = nullptr; return h->inner ? mpcqp_set_skip(h->inner, nullptr, mem) : MPCQP_OK; }
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if (mem == MPCQP_MEM_HOST) {
    if (!h->dskip) { if ((rc = dalloc(h, &h->dskip, (size_t)h->batch))) return rc; }
    if (h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));      // (a solve in flight may still read the buffer)
    HIPCHK(hipMemcpy(h->dskip, skip, (size_t)h->batch * sizeof(int), hipMemcpyHostToDevice));
    skip = h->dskip;
  }
  if (h->inner) {      // the handle that runs reads the same array (this handle's copy of a host array)
    if ((rc = mpcqp_set_skip(h->inner, skip, MPCQP_MEM_DEVICE))) return rc;
    h->skip = skip;
    return MPCQP_OK;
  }
  if (!h->skip_list) { if ((rc = dalloc(h, &h->skip_list, (size_t)h->batch))) return rc; }
  if (!h->ev_guard) HIPCHK(hipEventCreateWithFlags(&h->ev_guard, hipEventDisableTiming));
  h->skip = skip;
  return MPCQP_OK;
}

int mpcqp_set_soft_rows(mpcqp_handle *h, const double *w1, long stride1, const double *w2, long stride2, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!w1) { h->soft = false; return MPCQP_OK; }      // (the buffers stay the handle's: a later set call reuses them)
  if (h->inner) return fail(MPCQP_ERR_LIMIT, "mpcqp_set_soft_rows: a reduced or presolved handle does not take soft rows (its rows are not the caller's)");
  if (!takes_soft_rows(h->sel) || !oc_admm_soft_of(h, false) || !oc_admm_soft_of(h, true))
    return fail(MPCQP_ERR_LIMIT, "mpcqp_set_soft_rows: this handle does not run the two-kernel on-chip form (MPCQP_VARIANT=oc4 / oc8 at create names it, where the pattern admits it)");
  if (h->polish) return fail(MPCQP_ERR_STATE, "mpcqp_set_soft_rows: polishing is on (mpcqp_set_polish); its active-set guess assumes hard bounds");
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  const long m = h->m;
  if (m <= 0) return fail(MPCQP_ERR_ARG, "mpcqp_set_soft_rows: the QP has no rows");
  if (stride1 < 0 || stride2 < 0 || (stride1 && stride1 < m) || (w2 && stride2 && stride2 < m)) return fail(MPCQP_ERR_ARG, "stride smaller than the array it strides (dimension mismatch)");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  const size_t B = h->batch;
  if (!h->dsoft.buf) {
    const Plan &pl = h->sel.plan;
    h->dsoft.ms = std::max((pl.mpad + WAVE - 1) / WAVE, pl.A.nchunks) * WAVE;
    if ((rc = dalloc(h, &h->dsoft.buf, B * 2 * (size_t)h->dsoft.ms))) return rc;
  }
  if (mem == MPCQP_MEM_HOST) {
    if (h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));      // (a solve in flight may still read the copies)
    auto bad = [&](const double *w, long st_) {      // (host arrays are checked: weights are >= 0 and not NaN)
      for (long k = 0; w && k < (st_ ? (long)B : 1L); k++) for (long i = 0; i < m; i++) if (!(w[k * st_ + i] >= 0.0)) return true;
      return false;
    };
    if (bad(w1, stride1) || bad(w2, stride2)) return fail(MPCQP_ERR_ARG, "mpcqp_set_soft_rows: a weight is negative or NaN");
    if ((rc = stage(h, &h->dsw1, w1, stride1, m, &h->dsoft.w1, &h->dsoft.s1))) return rc;
    if (w2) { if ((rc = stage(h, &h->dsw2, w2, stride2, m, &h->dsoft.w2, &h->dsoft.s2))) return rc; }
    else { h->dsoft.w2 = nullptr; h->dsoft.s2 = 0; }
  } else {
    h->dsoft.w1 = w1; h->dsoft.s1 = stride1; h->dsoft.w2 = w2; h->dsoft.s2 = w2 ? stride2 : 0;
  }
  h->soft = true;
  return MPCQP_OK;
}

int mpcqp_debug_skip_list(mpcqp_handle *h, int *list, int mem) {
  if (!h || !list) return fail(MPCQP_ERR_ARG, "null pointer");
  if (h->inner) return mpcqp_debug_skip_list(h->inner, list, mem);
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  if (!h->solved || !h->skip_listed) return fail(MPCQP_ERR_STATE, "the last solve of this handle ran without a skip array (mpcqp_set_skip), or none has been issued");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->last_stream));
  HIPCHK(hipMemcpy(list, h->skip_list, (size_t)h->batch * sizeof(int), mem == MPCQP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return MPCQP_OK;
}

int mpcqp_solve(mpcqp_handle *h, void *stream) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->have_data) return fail(MPCQP_ERR_STATE, "Solver not initialized. Call mpcqp_update() first.");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  if (h->inner) return solve_reduced(h, s);
  DevIO io = io_of_handle(h);
  io.reuse = h->rescale_next ? 2 : h->reuse_next ? 1 : 0;
  io.order = (h->lpt && h->order_cur >= 0) ? h->order[h->order_cur] : nullptr;
  if (io.order && h->last_stream != s) HIPCHK(hipStreamWaitEvent(s, h->ev_order, 0));    // the hint was written on another stream
  if (h->skip) {
    // the dispatch list of this solve: the hint's order (or the identity) without the skipped instances, then -1 (kernels_util.hpp); the list of the
    // solve before may still be read on another stream
    if (h->solved && h->last_stream != s) { HIPCHK(hipEventRecord(h->ev_guard, h->last_stream)); HIPCHK(hipStreamWaitEvent(s, h->ev_guard, 0)); }
    hipLaunchKernelGGL(mpcqp_skip_list_kernel, dim3(1), dim3(1024), 0, s, h->skip, io.order, h->skip_list, h->batch);
    HIPCHK(hipGetLastError());
    io.order = h->skip_list;
  }
  HIPCHK(hipEventRecord(h->ev0, s));
  if (int rc = launch_batch(h, io, h->batch, io.reuse != 0, s, h->ev_mid, h->ev1, 0, h->skip)) return rc;
  if (h->lpt && h->batch > 1) {   // order of the next solve from this solve's iteration counts
    const int nxt = h->order_cur == 0 ? 1 : 0;
    hipLaunchKernelGGL(mpcqp_order_kernel, dim3(1), dim3(1024), 0, s, (const int *)h->oiters, h->order[nxt], h->batch, std::max(1, h->st.check_termination));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_order, s));
    h->order_cur = nxt;
  }
  note_skip_state(h, io.reuse);
  h->last_stream = s; h->solved = true; h->have_factor = h->keep; h->rescale_done = h->rescale_next;
  return MPCQP_OK;
}

// launch of instances [b0, b0 + count) on stream s: every per-instance pointer of `io` is advanced, the kernels index by blockIdx
static int launch_slice(mpcqp_handle *h, DevIO io, int b0, int count, hipStream_t s, int qslot) {
  const long n = h->n, m = h->m;
  io.P += (long)b0 * io.sP; io.q += (long)b0 * io.sq; io.A += (long)b0 * io.sA; io.l += (long)b0 * io.sl; io.u += (long)b0 * io.su;
  if (io.x0) io.x0 += b0 * n;
  if (io.y0) io.y0 += b0 * m;
  if (io.rho0) io.rho0 += b0;
  io.x += b0 * n; io.y += b0 * m; io.z += b0 * m; io.status += b0; io.iters += b0; io.info += 4L * b0;
  io.ws += (long)b0 * h->dp.ws_stride; io.cscale += b0;
  if (io.dbg) io.dbg += 16L * b0;
  return launch_batch(h, io, count, false, s, nullptr, nullptr, qslot);
}

int mpcqp_solve_host(mpcqp_handle *h, const double *P, long sP, const double *q, long sq, const double *A, long sA,
                     const double *l, long sl, const double *u, long su,
                     double *x, double *y, int *status, int *iters, int chunks) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!q || (h->sel.plan.nnzP_in > 0 && !P) || (h->sel.plan.nnzA_in > 0 && !A) || (h->m > 0 && (!l || !u))) return fail(MPCQP_ERR_ARG, "null data pointer");
  const long wP = h->sel.plan.nnzP_in, wA = h->sel.plan.nnzA_in, n = h->n, m = h->m;
  if (h->inner) return fail(MPCQP_ERR_STATE, "mpcqp_solve_host is not available on a reduced handle");
  if (h->skip) return fail(MPCQP_ERR_STATE, "mpcqp_solve_host solves the whole batch: clear the skip array first (mpcqp_set_skip(h, NULL, 0))");
  if (h->soft) return fail(MPCQP_ERR_STATE, "mpcqp_solve_host does not take soft rows: clear them first (mpcqp_set_soft_rows(h, NULL, 0, NULL, 0, 0)) or use mpcqp_update + mpcqp_solve");
  if ((sP && sP != wP) || sq != n || (sA && sA != wA) || (m > 0 && (sl != m || su != m)))
    return fail(MPCQP_ERR_ARG, "dimension mismatch: mpcqp_solve_host takes dense instance-major arrays (stride = width; 0 shares P or A)");
  HIPCHK(hipSetDevice(h->device));
  if (h->last_stream || h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));
  chunks = std::max(1, std::min(chunks > 0 ? chunks : 6, h->batch));
  int rc;
  const size_t B = h->batch;
  if (!h->dP) { if ((rc = dalloc(h, &h->dP, (size_t)std::max<long>(wP, 1) * B))) return rc; }
  if (!h->dq) { if ((rc = dalloc(h, &h->dq, (size_t)n * B))) return rc; }
  if (!h->dA) { if ((rc = dalloc(h, &h->dA, (size_t)std::max<long>(wA, 1) * B))) return rc; }
  if (!h->dl) { if ((rc = dalloc(h, &h->dl, (size_t)std::max<long>(m, 1) * B))) return rc; }
  if (!h->du) { if ((rc = dalloc(h, &h->du, (size_t)std::max<long>(m, 1) * B))) return rc; }
  // a slice's kernel ends with a tail (its slowest instance); two slices in flight fill each other's tails.  Two compute streams, not one per slice: the
  // runtime maps streams onto a few hardware queues (four by default), and with eight compute streams beside the copy stream the copies of a later slice
  // queued up behind kernels of earlier ones (rocprofv3 memory-copy trace: gaps of 0.9 - 1.7 ms in the transfer; 12.3 -> 10.3 ms per step on the north-star
  // batch, against a bound of ~10 ms = transfer of one slice + the launch).  MPCQP_PIPE_STREAMS overrides (1 .. 8).
  const int ns = std::min(chunks, std::min(h->knobs.pipe_streams, (int)mpcqp_handle::NPIPE));
  for (int i = 0; i < ns; i++) if (!h->pipe[i]) HIPCHK(hipStreamCreateWithFlags(&h->pipe[i], hipStreamNonBlocking));
  DevIO io = io_of_handle(h);
  io.P = h->dP; io.sP = sP; io.q = h->dq; io.sq = n; io.A = h->dA; io.sA = sA; io.l = h->dl; io.sl = m; io.u = h->du; io.su = m;
  if (sP == 0 && wP) HIPCHK(hipMemcpy(h->dP, P, wP * sizeof(double), hipMemcpyHostToDevice));      // shared matrices: once
  if (sA == 0 && wA) HIPCHK(hipMemcpy(h->dA, A, wA * sizeof(double), hipMemcpyHostToDevice));
  if (!h->pipe_copy) HIPCHK(hipStreamCreateWithFlags(&h->pipe_copy, hipStreamNonBlocking));
  while ((int)h->pipe_ev.size() < chunks) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->pipe_ev.push_back(e); }
  for (int c = 0; c < chunks; c++) {
    const int b0 = (int)((long)h->batch * c / chunks), b1 = (int)((long)h->batch * (c + 1) / chunks), cnt = b1 - b0;
    if (cnt <= 0) continue;
    // inputs of all slices queue on ONE stream, in slice order, so that slice 0 is complete after 1/chunks of the transfer
    // (copies spread over several streams share the link and all finish late)
    hipStream_t cs = h->pipe_copy, s = h->pipe[c % ns];
    if (sP) HIPCHK(hipMemcpyAsync(h->dP + (size_t)b0 * wP, P + (size_t)b0 * wP, (size_t)cnt * wP * sizeof(double), hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(h->dq + (size_t)b0 * n, q + (size_t)b0 * n, (size_t)cnt * n * sizeof(double), hipMemcpyHostToDevice, cs));
    if (sA) HIPCHK(hipMemcpyAsync(h->dA + (size_t)b0 * wA, A + (size_t)b0 * wA, (size_t)cnt * wA * sizeof(double), hipMemcpyHostToDevice, cs));
    if (m) {
      HIPCHK(hipMemcpyAsync(h->dl + (size_t)b0 * m, l + (size_t)b0 * m, (size_t)cnt * m * sizeof(double), hipMemcpyHostToDevice, cs));
      HIPCHK(hipMemcpyAsync(h->du + (size_t)b0 * m, u + (size_t)b0 * m, (size_t)cnt * m * sizeof(double), hipMemcpyHostToDevice, cs));
    }
    HIPCHK(hipEventRecord(h->pipe_ev[c], cs));
    HIPCHK(hipStreamWaitEvent(s, h->pipe_ev[c], 0));
    if ((rc = launch_slice(h, io, b0, cnt, s, 1 + c % ns))) return rc;      // (one set of ticket counters per compute stream: the slices of a stream run one after the other)
    if (x) HIPCHK(hipMemcpyAsync(x + (size_t)b0 * n, h->ox + (size_t)b0 * n, (size_t)cnt * n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (y && m) HIPCHK(hipMemcpyAsync(y + (size_t)b0 * m, h->oy + (size_t)b0 * m, (size_t)cnt * m * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status + b0, h->ostatus + b0, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, s));
    if (iters) HIPCHK(hipMemcpyAsync(iters + b0, h->oiters + b0, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(h->pipe_copy));
  for (int i = 0; i < ns; i++) HIPCHK(hipStreamSynchronize(h->pipe[i]));
  h->io.P = io.P; h->io.sP = io.sP; h->io.q = io.q; h->io.sq = io.sq; h->io.A = io.A; h->io.sA = io.sA; h->io.l = io.l; h->io.sl = io.sl; h->io.u = io.u; h->io.su = io.su;
  h->have_data = true; h->reuse_next = false; h->rescale_next = false; h->solved = true; h->have_factor = h->keep; h->last_stream = nullptr; h->order_cur = -1;
  note_skip_state(h, 0);
  return MPCQP_OK;
}

int mpcqp_get(mpcqp_handle *h, double *x, double *y, double *z, int *status, int *iters, double *info, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->solved) return fail(MPCQP_ERR_STATE, "no solve has been issued");
  HIPCHK(hipSetDevice(h->device));
  hipMemcpyKind k = mem == MPCQP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  hipStream_t s = h->last_stream;
  const size_t B = h->batch;
  if (x) HIPCHK(hipMemcpyAsync(x, h->ox, B * h->n * sizeof(double), k, s));
  if (y && h->m) HIPCHK(hipMemcpyAsync(y, h->oy, B * h->m * sizeof(double), k, s));
  if (z && h->m) HIPCHK(hipMemcpyAsync(z, h->oz, B * h->m * sizeof(double), k, s));
  if (status) HIPCHK(hipMemcpyAsync(status, h->ostatus, B * sizeof(int), k, s));
  if (iters) HIPCHK(hipMemcpyAsync(iters, h->oiters, B * sizeof(int), k, s));
  if (info) HIPCHK(hipMemcpyAsync(info, h->oinfo, B * 4 * sizeof(double), k, s));
  if (mem != MPCQP_MEM_DEVICE) HIPCHK(hipStreamSynchronize(s));
  return MPCQP_OK;
}

int mpcqp_sync(mpcqp_handle *h) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->last_stream));
  return MPCQP_OK;
}

void mpcqp_destroy(mpcqp_handle *h) {
  if (!h) return;
  if (h->inner) { mpcqp_destroy(h->inner); h->inner = nullptr; }
  (void)hipSetDevice(h->device);
  if (h->solved) (void)hipStreamSynchronize(h->last_stream);
  for (void *p : h->dev_allocs) (void)hipFree(p);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev_mid) (void)hipEventDestroy(h->ev_mid);
  if (h->ev_guard) (void)hipEventDestroy(h->ev_guard);
  if (h->ev_order) (void)hipEventDestroy(h->ev_order);
  if (h->ev0r) (void)hipEventDestroy(h->ev0r);
  if (h->evp0) (void)hipEventDestroy(h->evp0);
  if (h->evp1) (void)hipEventDestroy(h->evp1);
  for (int i = 0; i < mpcqp_handle::NPIPE; i++) if (h->pipe[i]) (void)hipStreamDestroy(h->pipe[i]);
  if (h->pipe_copy) (void)hipStreamDestroy(h->pipe_copy);
  for (hipEvent_t e : h->pipe_ev) (void)hipEventDestroy(e);
  delete h;
}

int mpcqp_last_kernel_ms(mpcqp_handle *h, float *ms) {
  if (!h || !ms) return fail(MPCQP_ERR_ARG, "null pointer");
  if (!h->solved) return fail(MPCQP_ERR_STATE, "no solve has been issued");
  if (h->inner) return mpcqp_last_kernel_ms(h->inner, ms);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return MPCQP_OK;
}

int mpcqp_last_phase_ms(mpcqp_handle *h, float *setup_ms, float *solve_ms) {
  if (!h || !setup_ms || !solve_ms) return fail(MPCQP_ERR_ARG, "null pointer");
  if (!h->solved) return fail(MPCQP_ERR_STATE, "no solve has been issued");
  if (h->inner) return mpcqp_last_phase_ms(h->inner, setup_ms, solve_ms);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventSynchronize(h->ev1));
  if (!h->sel.split) { *setup_ms = 0.f; HIPCHK(hipEventElapsedTime(solve_ms, h->ev0, h->ev1)); return MPCQP_OK; }
  HIPCHK(hipEventElapsedTime(setup_ms, h->ev0, h->ev_mid));
  HIPCHK(hipEventElapsedTime(solve_ms, h->ev_mid, h->ev1));
  return MPCQP_OK;
}

int mpcqp_set_polish(mpcqp_handle *h, int enable, double delta, int refine_iter) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (h->inner) {
    int rc = mpcqp_set_polish(h->inner, enable, delta, refine_iter);
    if (!rc && h->inner->polish && !h->opinfo) {      // the expansion's copy of the polish outcome (nothing is allocated inside a solve)
      HIPCHK(hipSetDevice(h->device));
      const size_t B = h->batch;
      if ((rc = dalloc(h, &h->opstatus, B))) return rc;
      if ((rc = dalloc(h, &h->opinfo, B * 4))) return rc;
      HIPCHK(hipMemset(h->opstatus, 0, B * sizeof(int))); HIPCHK(hipMemset(h->opinfo, 0, B * 4 * sizeof(double)));
    }
    if (!rc) h->polish = h->inner->polish;
    return rc;
  }
  if (!enable) { h->polish = false; h->polish_timed = false; return MPCQP_OK; }
  if (h->soft) return fail(MPCQP_ERR_STATE, "mpcqp_set_polish: the handle has soft rows set (mpcqp_set_soft_rows); the polish's active-set guess assumes hard bounds");
  HIPCHK(hipSetDevice(h->device));
  if (!h->pfac) {
    if (int rc = mpcqp_polish_prepare(h->dp, h->device)) return rc;
    if (h->solved) HIPCHK(hipStreamSynchronize(h->last_stream));
    const size_t B = h->batch;
    h->pfac_stride = mpcqp_polish_fac_doubles(h->dp);
    int rc;
    if ((rc = dalloc(h, &h->pfac, B * (size_t)h->pfac_stride))) return rc;
    if ((rc = dalloc(h, &h->opstatus, B))) return rc;
    if ((rc = dalloc(h, &h->opinfo, B * 4))) return rc;
    HIPCHK(hipMemset(h->opstatus, 0, B * sizeof(int))); HIPCHK(hipMemset(h->opinfo, 0, B * 4 * sizeof(double)));
    HIPCHK(hipEventCreate(&h->evp0)); HIPCHK(hipEventCreate(&h->evp1));
  }
  h->pol_delta = delta > 0.0 ? delta : 1e-6;
  h->pol_refine = refine_iter >= 0 ? refine_iter : 3;
  h->polish = true;
  return MPCQP_OK;
}

int mpcqp_get_polish(mpcqp_handle *h, int *polish_status, double *polish_info, int mem) {
  if (!h) return fail(MPCQP_ERR_ARG, "null handle");
  if (!h->polish) return fail(MPCQP_ERR_STATE, "polishing is off (mpcqp_set_polish)");
  if (!h->solved) return fail(MPCQP_ERR_STATE, "no solve has been issued");
  // (a reduced handle: its own copy, which the expansion wrote -- the inner handle's outcome with the candidate's objective in the caller's terms)
  if (mem != MPCQP_MEM_HOST && mem != MPCQP_MEM_DEVICE) return fail(MPCQP_ERR_ARG, "mem must be MPCQP_MEM_HOST or MPCQP_MEM_DEVICE");
  HIPCHK(hipSetDevice(h->device));
  const hipMemcpyKind k = mem == MPCQP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  hipStream_t s = h->last_stream;
  const size_t B = h->batch;
  if (polish_status) HIPCHK(hipMemcpyAsync(polish_status, h->opstatus, B * sizeof(int), k, s));
  if (polish_info) HIPCHK(hipMemcpyAsync(polish_info, h->opinfo, B * 4 * sizeof(double), k, s));
  if (mem != MPCQP_MEM_DEVICE) HIPCHK(hipStreamSynchronize(s));
  return MPCQP_OK;
}

int mpcqp_last_polish_ms(mpcqp_handle *h, float *ms) {
  if (!h || !ms) return fail(MPCQP_ERR_ARG, "null pointer");
  if (h->inner) return mpcqp_last_polish_ms(h->inner, ms);
  if (!h->solved || !h->polish || !h->polish_timed) return fail(MPCQP_ERR_STATE, "no polish kernel has run behind an mpcqp_solve");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipEventSynchronize(h->evp1));
  HIPCHK(hipEventElapsedTime(ms, h->evp0, h->evp1));
  return MPCQP_OK;
}

int mpcqp_plan_info(const mpcqp_handle *h, long *o) {
  if (!h || !o) return fail(MPCQP_ERR_ARG, "null pointer");
  if (h->inner) return mpcqp_plan_info(h->inner, o);        // the plan that runs: the reduced pattern's
  plan_info_of(h->sel, h->n, h->m, h->batch, o);
  return MPCQP_OK;
}

int mpcqp_oc_info(const mpcqp_handle *h, long *o) {
  if (!h || !o) return fail(MPCQP_ERR_ARG, "null pointer");
  if (h->inner) return mpcqp_oc_info(h->inner, o);
  oc_info_of(h->sel, o);
  return MPCQP_OK;
}

int mpcqp_debug_scaling(mpcqp_handle *h, int b, double *D, double *E, double *c) {
  if (!h || b < 0 || b >= h->batch) return fail(MPCQP_ERR_ARG, "bad instance index");
  if (h->inner) return fail(MPCQP_ERR_STATE, "scaling of a reduced handle lives in the reduced dimensions");
  if (!h->solved) return fail(MPCQP_ERR_STATE, "no solve has been issued");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->last_stream));
  const Plan &pl = h->sel.plan;
  std::vector<double> Dp(pl.npad);
  const double *base = h->ws + (size_t)b * h->sel.wl.stride;
  if (D) { HIPCHK(hipMemcpy(Dp.data(), base + h->sel.wl.D, pl.npad * sizeof(double), hipMemcpyDeviceToHost)); for (int j = 0; j < h->n; j++) D[j] = Dp[pl.pos[j]]; }
  if (E && h->m) HIPCHK(hipMemcpy(E, base + h->sel.wl.E, h->m * sizeof(double), hipMemcpyDeviceToHost));
  if (c) HIPCHK(hipMemcpy(c, h->ocs + b, sizeof(double), hipMemcpyDeviceToHost));
  return MPCQP_OK;
}

#ifdef MPCQP_TIMING
// timing build only: per-QP cycle counts of the 16 instrumented segments (copied to host)
int mpcqp_debug_timing(mpcqp_handle *h, long long *out) {
  if (!h || !out || !h->odbg) return fail(MPCQP_ERR_ARG, "no timing data");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->last_stream));
  HIPCHK(hipMemcpy(out, h->odbg, ((size_t)h->batch * 16 + 128) * sizeof(long long), hipMemcpyDeviceToHost));
  return MPCQP_OK;
}
#endif

int mpcqp_debug_blockops(const double *A, const double *B, const double *C, const double *S, double *out_gemm, double *out_linv, int *potrf_fail) {
  if (!A || !B || !C || !S || !out_gemm || !out_linv || !potrf_fail) return fail(MPCQP_ERR_ARG, "null pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MPCQP_ERR_NO_GPU, "no device");
  double *d = nullptr; int *df = nullptr;
  HIPCHK(hipMalloc((void **)&d, 6 * BLK * sizeof(double)));
  HIPCHK(hipMalloc((void **)&df, sizeof(int)));
  HIPCHK(hipMemcpy(d, A, BLK * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d + BLK, B, BLK * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + 2 * BLK, C, BLK * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d + 3 * BLK, S, BLK * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mpcqp_blockops_kernel, dim3(1), dim3(WAVE), 0, 0, d, d + BLK, d + 2 * BLK, d + 3 * BLK, d + 4 * BLK, d + 5 * BLK, df);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_gemm, d + 4 * BLK, BLK * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_linv, d + 3 * BLK, BLK * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(potrf_fail, df, sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(d); (void)hipFree(df);
  return MPCQP_OK;
}

}  // extern "C"
