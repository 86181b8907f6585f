/*
 * mpcqp.h -- C ABI of the MI355X-native batched QP engine (libmpcqp.so).
 *
 * Drop-in boundary.  The reference has no FFI; its seam is the C++ class CuCaQP
 * (reference include/optimal_control_problem/sqp_solver/CuCaQP.h:27-102), driven from one place in the
 * order setDimension -> settings -> [ setSystem(P,q,A,l,u) -> initSolver -> solve -> getSolution ]
 * (reference src/sqp_solver/SQPOptimizationSolver.cpp:80-85,155-167).  Each entry point below names the
 * CuCaQP member(s) it replaces.  One handle owns one batch of QPs that share a sparsity pattern (the
 * reference's batch is 1); distinct handles are independent (one per GPU when sharding a batch).
 *
 * Plain C: no exceptions cross the ABI, integer status codes, caller owns every I/O buffer, the library
 * owns its device workspace.  A handle is not thread-safe (neither is CuCaQP).
 */
#ifndef MPCQP_H
#define MPCQP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_OK 0
#define MPCQP_ERR_ARG 1       /* bad dimensions / null pointers / malformed CSC   (CuCaQP.cpp:23-27,49-52) */
#define MPCQP_ERR_HIP 2       /* a HIP runtime call failed; mpcqp_strerror() carries the HIP message        */
#define MPCQP_ERR_NO_GPU 3    /* no gfx950 device / code object missing: the product path has no CPU fallback */
#define MPCQP_ERR_STATE 4     /* call order violated (solve before update, ...)   (CuCaQP.cpp:199-203)      */
#define MPCQP_ERR_LIMIT 5     /* problem does not fit the kernel's on-chip budget                          */

/* per-QP solver status, numerically identical to OSQP 1.0's osqp_status_type */
#define MPCQP_SOLVED 1
#define MPCQP_SOLVED_INACCURATE 2
#define MPCQP_PRIMAL_INFEASIBLE 3
#define MPCQP_PRIMAL_INFEASIBLE_INACCURATE 4
#define MPCQP_DUAL_INFEASIBLE 5
#define MPCQP_DUAL_INFEASIBLE_INACCURATE 6
#define MPCQP_MAX_ITER_REACHED 7
#define MPCQP_NON_CVX 9
#define MPCQP_UNSOLVED 11      /* also: data refused -- an instance with l_i > u_i on some row is not solved (OSQP's setup validation,
                                * which makes CuCaQP::initSolver return false, CuCaQP.cpp:183-197): 0 iterations, NaN in x, y, z */

#define MPCQP_MEM_HOST 0      /* pointer is host memory (pageable or pinned) */
#define MPCQP_MEM_DEVICE 1    /* pointer is device memory on the handle's GPU */

/* Replaces CuCaQP::setVerbosity/setWarmStart/setAbsoluteTolerance/setRelativeTolerance/setMaxIteration
 * (reference src/sqp_solver/CuCaQP.cpp:163-181).  Defaults = OSQP defaults with the values the reference
 * fixes at src/sqp_solver/SQPOptimizationSolver.cpp:81-85 (eps_abs = eps_rel = 1e-3, max_iter = 10000). */
typedef struct mpcqp_settings {
  double rho;                    /* 0.1   */
  double sigma;                  /* 1e-6  */
  double alpha;                  /* 1.6   */
  double eps_abs;                /* 1e-3  */
  double eps_rel;                /* 1e-3  */
  double eps_prim_inf;           /* 1e-4  */
  double eps_dual_inf;           /* 1e-4  */
  double adaptive_rho_tolerance; /* 5     */
  int max_iter;                  /* 10000 */
  int check_termination;         /* 25    */
  int scaling;                   /* 10 Ruiz passes */
  int adaptive_rho;              /* 1     */
  int adaptive_rho_interval;     /* 0 -> 4 * check_termination (deterministic; OSQP's wall-clock rule is not reproducible) */
  int scaled_termination;        /* 0     */
  int warm_start;                /* 0 = cold start from x = z = y = 0, which is what the reference does
                                    because CuCaQP::setSystem clears the solver (CuCaQP.cpp:271-288) */
  int device;                    /* HIP device ordinal, -1 = current device */
} mpcqp_settings;

typedef struct mpcqp_handle mpcqp_handle;

void mpcqp_default_settings(mpcqp_settings *s);

/* Replaces CuCaQP::CuCaQP + setDimension (CuCaQP.cpp:5-41) and the pattern-dependent part of initSolver
 * (CuCaQP.cpp:183-197): n variables, m constraint rows, `batch` QP instances sharing one sparsity.
 * P is CSC n x n -- either triangle or both (CasADi hands the reference both triangles; like OsqpEigen,
 * only entries with row <= col are used); A is CSC m x n.  Index arrays are copied. */
int mpcqp_create(int n, int m, int batch,
                 const int *P_colptr, const int *P_rowidx,
                 const int *A_colptr, const int *A_rowidx,
                 const mpcqp_settings *settings, mpcqp_handle **out);

/* Opt-in: mpcqp_create with the kernel family chosen by MEASUREMENT instead of by the rules tuned on the MPC workloads (for patterns those
 * rules have never seen).  Every family that takes the pattern and size (the rule's own choice, the on-chip modes, the LDS-resident and the
 * global-block kernels) gets a handle, runs a synthetic QP on this pattern (unit diagonal P, pseudo-random A, box around the origin, a fixed
 * number of ADMM iterations), and the fastest one is returned; the others are destroyed.  The handle that comes back IS a handle of that
 * family: results are bitwise what MPCQP_VARIANT=<family> gives.  The choice is cached per (pattern, batch) for the life of the process.
 * Costs a few hundred milliseconds at create -- the pattern-dependent part of what the reference pays in initSolver for every QP
 * (CuCaQP.cpp:183-197).  The environment variable MPCQP_AUTOTUNE=1 makes mpcqp_create behave like this entry point; default: off. */
int mpcqp_create_tuned(int n, int m, int batch,
                       const int *P_colptr, const int *P_rowidx,
                       const int *A_colptr, const int *A_rowidx,
                       const mpcqp_settings *settings, mpcqp_handle **out);

/* Opt-in reduced form.  The reference's QP carries variables that are fixed by construction: the parameter block p, whose rows
 * read p <= p + dp <= p (SQPOptimizationSolver.cpp:47-60,117), and the first frame, pinned through lbx = ubx
 * (src/OptimalControlProblem.cpp:93-96).  OSQP iterates on them like on any other variable, and so does a handle from
 * mpcqp_create.  Here the caller names `nfixed` rows of A that have a single entry and l = u in every instance and every
 * update; their variables are substituted (x_j = l_i / a_ij) before the solve, the remaining QP -- smaller, and without the
 * parameter block's coupling to every stage -- is solved on its own pattern, and x, y, z are returned in the caller's
 * dimensions (the multiplier of an eliminated row from stationarity of its variable).  The handle is used like any other
 * (update / update_vectors / warm_start / set_rho / solve / get; mpcqp_solve_host and mpcqp_debug_scaling are not available).
 * It is a different, shorter ADMM run on an equivalent QP: x agrees with the full form within the termination tolerance, not
 * in the last digits, and status / iteration counts / info are the reduced run's, stated for the caller's QP: info[0] is the
 * caller's objective at the returned x (the constant q_f'x_f + 1/2 x_f'P_ff x_f of the eliminated variables is added to the
 * reduced run's objective; mpcqp_get_polish reports the candidate's objective the same way), info[1] and info[2] are the
 * residuals of the caller's QP at the returned point (the eliminated rows and the stationarity of the eliminated variables hold
 * to rounding).  An instance without a point -- a certificate of infeasibility, MPCQP_NON_CVX, crossed bounds -- is NaN in all
 * of x, y, z, as from mpcqp_create.  An instance that breaks the promise (l != u on a named row) is refused like one with
 * crossed bounds (MPCQP_UNSOLVED, x, y, z and info[0..2] NaN, 0 iterations).  mpcqp_update_vectors reads the P and A arrays of the last mpcqp_update again (the eliminated
 * columns enter q, l, u): device pointers borrowed there must still be valid.  The default stays the full form. */
int mpcqp_create_reduced(int n, int m, int batch,
                         const int *P_colptr, const int *P_rowidx,
                         const int *A_colptr, const int *A_rowidx,
                         int nfixed, const int *fixed_rows,
                         const mpcqp_settings *settings, mpcqp_handle **out);

/* The same without the caller naming rows: the rows to eliminate are FOUND -- every row of A with a single entry whose bounds coincide in every
 * instance of (l, u), the bounds of the first update (host or device arrays, strides as in mpcqp_update; read once, here) -- which is what the
 * reference's formulation produces by itself: 0 <= dp <= 0 on the parameter block (SQPOptimizationSolver.cpp:117) and the first frame pinned
 * through lbx = ubx (src/OptimalControlProblem.cpp:93-96).  A caller that arrives through CuCaQP / OptimalControlProblem and cannot name rows
 * gets the reduced form this way (CuCaQP::setPresolveFixedRows(true) in cpp/CuCaQP.hpp).  Returns the handle of mpcqp_create_reduced on those rows
 * (an ordinary handle when there are none) and the number of rows it eliminates in *nfixed (may be NULL; a QP whose every variable is pinned keeps
 * one variable, so n - 1 at the most).  The promise "l = u on these rows in every later update" is
 * checked per instance as there (MPCQP_UNSOLVED, NaN for an instance that breaks it).  The default stays the full form. */
int mpcqp_create_presolved(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                           const double *l, long sl, const double *u, long su, int mem,
                           const mpcqp_settings *settings, mpcqp_handle **out, int *nfixed);

/* Replaces CuCaQP::setSystem -> setHessianMatrix/setGradient/setLinearConstraintsMatrix/setLowerBound/
 * setUpperBound (CuCaQP.cpp:43-103,271-288), argument order P,q,A,l,u as at CuCaQP.cpp:283-287.
 * Value arrays are instance-major: QP b reads P + b*strideP (in doubles) ... ; stride 0 shares one array
 * across the batch.  mem = MPCQP_MEM_HOST: values are copied (caller may free at once, as with CuCaQP,
 * which copies into its members CuCaQP.h:83-87).  mem = MPCQP_MEM_DEVICE: pointers are borrowed until
 * the next mpcqp_solve on this handle has completed. */
int mpcqp_update(mpcqp_handle *h,
                 const double *P, long strideP, const double *q, long strideq,
                 const double *A, long strideA, const double *l, long stridel,
                 const double *u, long strideu, int mem);

/* The (unused, private) CuCaQP::update* fast path made real (CuCaQP.cpp:106-161): primal/dual start
 * x0 [batch*n], y0 [batch*m]; honoured by the next solve when settings.warm_start != 0. */
int mpcqp_warm_start(mpcqp_handle *h, const double *x0, const double *y0, int mem);

/* Kept workspace -- the fast path the reference's private, never-called CuCaQP::updateGradient / updateLowerBound /
 * updateUpperBound were written for (CuCaQP.cpp:117-161), with the semantics of OSQP's osqp_update_data_vec: P and A, their
 * scaling (D, E, c), the KKT factorisation and every instance's current (possibly adapted) rho stay from the previous solve on
 * this handle; only q, l, u are replaced.  The next mpcqp_solve skips equilibration and factorisation; an instance is
 * re-factorised only if one of its rows moved between loose / inequality / equality (its rho_i changes then), and an instance
 * whose matrices were found non-convex stays MPCQP_NON_CVX.  x / y start from zero, or from mpcqp_warm_start when
 * settings.warm_start is set.  Call order: mpcqp_keep_workspace(h, 1) -> mpcqp_update -> mpcqp_solve ->
 * { mpcqp_update_vectors -> mpcqp_solve }*; mpcqp_update returns to a full setup.  Strides and mem as in mpcqp_update.
 * MPCQP_ERR_STATE when there is no kept solve yet; MPCQP_ERR_LIMIT on the streaming kernel variant. */
int mpcqp_keep_workspace(mpcqp_handle *h, int enable);
int mpcqp_update_vectors(mpcqp_handle *h, const double *q, long strideq, const double *l, long stridel,
                         const double *u, long strideu, int mem);

/* Kept workspace, new matrices -- what the reference's private, never-called CuCaQP::updateHessianMatrix / updateLinearConstraintsMatrix
 * (CuCaQP.cpp:106-116,129-140) map to through OsqpEigen: OSQP's osqp_update_data_mat.  The scaling D, E, c of the handle's last full
 * set-up (mpcqp_update + mpcqp_solve) and every instance's current rho stay; the new P, q, A, l, u are scaled with them (c D P D, c D q,
 * E A D, E l, E u) and the KKT matrix is factorised again.  The next mpcqp_solve skips the equilibration passes only.  Every instance is
 * re-factorised: an instance that was MPCQP_NON_CVX gets a fresh verdict from its new matrices.  x / y start from zero, or from
 * mpcqp_warm_start when settings.warm_start is set.  Strides, mem, borrowing rules and argument checks as in mpcqp_update.
 * Call order: mpcqp_keep_workspace(h, 1) -> mpcqp_update -> mpcqp_solve -> { mpcqp_update_matrices | mpcqp_update_vectors -> mpcqp_solve }*;
 * mpcqp_update returns to a full set-up (and to a new scaling); mpcqp_update_vectors behind a matrices solve works on the factor that
 * solve left; mpcqp_update_vectors between mpcqp_update_matrices and its solve only replaces q, l, u of that solve.
 * An instance with l_i > u_i on some row is refused as always (MPCQP_UNSOLVED, NaN), for that solve only.  An instance that the last
 * full set-up refused for that reason has its D, E, c all the same -- the bounds take no part in the scaling -- and is solved here like
 * every other instance once its bounds are in order.
 * MPCQP_ERR_STATE without mpcqp_keep_workspace(h, 1) or without a kept solve.  MPCQP_ERR_LIMIT, at this call, on a handle that does not run
 * the two-kernel on-chip form (streaming, LDS-resident, global-block, MPCQP_OC_MONO, the tile experiments): the handle stays as it was, and
 * the caller falls back to mpcqp_update.  Reduced handles forward to their inner handle. */
int mpcqp_update_matrices(mpcqp_handle *h, const double *P, long strideP, const double *q, long strideq,
                          const double *A, long strideA, const double *l, long stridel,
                          const double *u, long strideu, int mem);

/* Per-instance starting rho for the following solves (rho0 [batch]; entries <= 0 mean settings.rho; NULL returns to
 * settings.rho for all).  A kept OSQP workspace carries its adapted rho from one problem to the next
 * (osqp_update_* do not reset it) -- the behaviour the reference's unused update* members would have had
 * (CuCaQP.cpp:106-161); feed info[3] of the previous solve back in. */
int mpcqp_set_rho(mpcqp_handle *h, const double *rho0, int mem);

/* Replaces CuCaQP::initSolver + CuCaQP::solve (CuCaQP.cpp:183-211): per QP, Ruiz scaling, KKT
 * factorisation and the ADMM loop run in one launch on `stream` (a hipStream_t, NULL = default stream).
 * Asynchronous: returns after the launch; results are ordered on `stream`. */
int mpcqp_solve(mpcqp_handle *h, void *stream);

/* Fused host-buffer step for large batches: CuCaQP::setSystem + initSolver + solve + getSolution (CuCaQP.cpp:183-224,271-288) in
 * one call, pipelined -- the batch is cut into `chunks` slices (0 = 6); all host-to-device copies queue on one internal stream
 * in slice order, each slice's kernel and its device-to-host copies run on one of several compute streams as soon as its inputs
 * have landed, so transfers overlap the kernels of earlier slices ("streams matrices via pinned hipMemcpyAsync").  Arrays are dense and instance-major (stride = width; strideP / strideA may be 0 for matrices shared by the
 * batch); x [batch*n], y [batch*m], status, iters [batch] may be NULL.  The copies are asynchronous only from / to pinned host
 * memory (hipHostMalloc, hipHostRegister); pageable memory works but serialises.  Returns when everything has completed.
 * Cold start, full setup, batch-order dispatch; the results also stay on the device for mpcqp_get. */
int mpcqp_solve_host(mpcqp_handle *h, const double *P, long strideP, const double *q, long strideq,
                     const double *A, long strideA, const double *l, long stridel, const double *u, long strideu,
                     double *x, double *y, int *status, int *iters, int chunks);

/* Scheduling hint (on by default; MPCQP_NO_LPT=1 in the environment turns it off at create): after every solve the instances
 * are ranked by their ADMM iteration count, and the next solve on the handle hands them to workgroups in that order, longest
 * first.  Instances are independent, so no output changes by a bit; what changes is the tail of the launch -- with one QP per
 * workgroup and 25- and 100-iteration instances mixed, in-order dispatch leaves CUs idle while the last long instance
 * finishes.  The predictor is exact when the same batch is solved again and good in an MPC loop (consecutive solves of the
 * same plants); a stale hint is harmless.  No reference counterpart (the reference solves one QP at a time). */
int mpcqp_set_dispatch_hint(mpcqp_handle *h, int enable);

/* Solve a subset of the batch (opt-in; a handle that never sets a skip array launches exactly what it launched before).  skip [batch]: a nonzero
 * entry (any value) leaves that instance out of the following mpcqp_solve calls -- the polarity of mpcqp_kkt_args.frozen, so the verdict array of
 * mpcqp_stage_kkt / mpcqp_nlp_kkt can be passed as it is.  NULL clears the skip array.  MPCQP_MEM_DEVICE: the pointer is borrowed and every following
 * mpcqp_solve reads it on its stream, so the contents may change between solves (and between replays of a captured solve) without another call;
 * MPCQP_MEM_HOST: the array is copied into a buffer of the handle.  Everything the feature needs is allocated here, never inside mpcqp_solve, which
 * stays capturable in a HIP graph.  No value comes back to the host.
 * A skipped instance: none of its inputs is read (P, q, A, l, u, x0, y0, rho0), its bounds are not validated, and nothing of it is written -- x, y, z,
 * status, iters, info, polish_status, polish_info and its slab of the workspace (factor, D, E, c, rho, parked factor) keep their bits; on a handle
 * that never solved it they are whatever the buffers held.  An active instance gets, bit for bit, the result of the same solve without a skip array.
 * How: one small kernel ahead of the solve compacts the dispatch order -- the hint's order where there is one, else the identity -- to the active
 * instances, in that order, followed by -1 up to batch entries; the grids stay as they are and a workgroup whose entry is negative returns at once
 * (the ticket loop of the eight-wave iteration kernel ends at the first negative entry).  Reduced handles forward the array to the handle that runs.
 * Kept workspaces, tracked per handle (not per instance):
 *   - after a full set-up (mpcqp_update + mpcqp_solve) under a skip array, mpcqp_update_vectors and mpcqp_update_matrices answer MPCQP_ERR_STATE
 *     until a full set-up without one has run: a skipped instance would reuse a factor or a scaling of other matrices;
 *   - after an mpcqp_update_matrices solve under a skip array, mpcqp_update_vectors answers MPCQP_ERR_STATE (a skipped instance's factor is of
 *     older matrices) until an mpcqp_update_matrices solve or a full set-up without one; mpcqp_update_matrices still works (D, E, c are those of
 *     the unskipped full set-up);
 *   - an mpcqp_update_vectors solve under a skip array leaves everything valid: a skipped instance's factor, rho and parked state are not touched.
 * mpcqp_solve_host with a skip array set answers MPCQP_ERR_STATE.  No reference counterpart (the reference solves one QP at a time). */
int mpcqp_set_skip(mpcqp_handle *h, const int *skip, int mem);
/* The compacted dispatch list of the last mpcqp_solve (list [batch]: the active instances in dispatch order, then -1), for tests of the compaction
 * kernel; waits for the solve.  MPCQP_ERR_STATE when the last solve ran without a skip array (or none ran). */
int mpcqp_debug_skip_list(mpcqp_handle *h, int *list, int mem);

/* Soft constraint rows.  With weights set, the following solves minimise
 *     1/2 x'Px + q'x + sum_i [ w1_i d_i + 1/2 w2_i d_i^2 ],   d_i = dist((Ax)_i, [l_i, u_i]),
 * with no new variables and the same P, A, pattern, row classes, rho and factorisation: only the z update of the ADMM changes, from the projection onto
 * [l, u] to the proximal map of the penalty (past a bound by max(0, (rho_i d - w1) / (rho_i + w2)) in the scaled problem).  w1, w2 [m] per instance, >= 0;
 * stride 0 = one array shared by the batch; w2 = NULL means zeros; a row with w1_i >= 1e30 (the library's infinity, as for bounds) is hard, and a handle whose
 * rows are all hard returns the bits of the plain solve.  w1 = NULL clears the setting: the plain kernels run again.  Device arrays are borrowed and read by
 * every following solve on its stream (like the skip array); host arrays are copied.  The set call allocates what the solves need (nothing is allocated inside
 * mpcqp_solve: a soft solve stays capturable in a graph).
 * Outputs: z is the minimiser's row activity and may lie outside [l, u] on soft rows (the penalty can be read off it); y_i is a subgradient of the penalty at
 * z_i: 0 inside, |y_i| <= w1_i on a bound, +-(w1_i + w2_i d_i) outside; info[0] stays 1/2 x'Px + q'x.  The primal-infeasibility certificate treats a soft row
 * like a row with both bounds infinite; the dual-infeasibility certificate still counts it as bounded, so a problem that is unbounded only through soft rows with
 * w2 = 0 (and singular P) ends on the iteration limit.
 * Only the two-kernel on-chip form has soft twins of its iteration kernel: every other family, and the tile experiment, answers MPCQP_ERR_LIMIT (the precedent
 * of mpcqp_update_matrices), and so do reduced and presolved handles.  Polishing and soft rows exclude each other -- the active-set guess assumes hard bounds:
 * whichever of mpcqp_set_polish / mpcqp_set_soft_rows comes second answers MPCQP_ERR_STATE.  mpcqp_solve_host with soft rows set answers MPCQP_ERR_STATE.
 * Kept workspaces (mpcqp_update_vectors, mpcqp_update_matrices), warm starts, mpcqp_set_rho, the dispatch hint and mpcqp_set_skip work as before.
 * No reference counterpart (OSQP has hard rows only; the reference models slack as extra inputs). */
int mpcqp_set_soft_rows(mpcqp_handle *h, const double *w1, long stride1, const double *w2, long stride2, int mem);

/* Replaces CuCaQP::getSolution / getSolutionAsDM (CuCaQP.cpp:213-224), and additionally surfaces what the
 * reference drops: duals y, row activities z, per-QP status, iteration count and
 * info[4] = {objective, primal residual, dual residual, final rho}.  Any output pointer may be NULL.
 * Copies are issued on the stream of the last solve; with MPCQP_MEM_HOST the call returns after they
 * have completed. */
int mpcqp_get(mpcqp_handle *h, double *x, double *y, double *z, int *status, int *iters, double *info, int mem);

/* Solution polishing -- OSQP's `polishing` setting (OsqpEigen::Settings::setPolish) with its `delta` and `polish_refine_iter`; the per-QP outcome is
 * OSQP's info->status_polish.  The reference never switches it on (its settings are the five of src/sqp_solver/CuCaQP.cpp:163-181), so the default is
 * off and a handle that never calls mpcqp_set_polish, or calls it with enable = 0, launches exactly what it launched before.  When on, a polish kernel is
 * queued behind every solve on the solve's stream (mpcqp_solve_host: on each slice's compute stream, ahead of its device-to-host copies): for every instance
 * that ended MPCQP_SOLVED it guesses the active rows from the iterate (lower: z - l < -y, upper: u - z < y), solves the
 * regularised KKT system [P + delta I, A_a'; A_a, -delta I] on them (delta in the caller's units: the result does not depend on the equilibration), refines the result refine_iter times against the unregularised matrix, and keeps
 * it -- x, y, z and info[0..2] are overwritten -- iff OSQP's rule holds (both residuals smaller than ADMM's, or one smaller while the other was below
 * 1e-10).  status, iters and info[3] never change; an instance that is not polished, or whose candidate is rejected, keeps the ADMM result bit for bit.
 * The factor of the polish system lives in scratch allocated here (nothing is allocated inside a solve), so a kept workspace's factor survives.
 * delta <= 0 -> 1e-6, refine_iter < 0 -> 3 (OSQP's defaults).  Reduced handles forward the setting to the handle that runs. */
#define MPCQP_POLISH_LINSYS_ERROR  -2   /* the polish system had a non-positive pivot: ADMM solution kept */
#define MPCQP_POLISH_FAILED        -1   /* candidate rejected: ADMM solution kept */
#define MPCQP_POLISH_NOT_PERFORMED  0   /* polishing off, or status != MPCQP_SOLVED */
#define MPCQP_POLISH_SUCCESS        1
int mpcqp_set_polish(mpcqp_handle *h, int enable, double delta, int refine_iter);
/* OSQP's info->status_polish per QP (polish_status [batch]) and polish_info[4*b ..] = {objective, primal residual, dual residual of the candidate --
 * accepted or not; NaN when none was built --, number of active rows}.  Either pointer may be NULL.  Of the last solve, ordered on its stream like
 * mpcqp_get; a reduced handle reports its inner handle's, with the objective in the caller's terms.  MPCQP_ERR_STATE when polishing is off. */
int mpcqp_get_polish(mpcqp_handle *h, int *polish_status, double *polish_info, int mem);
/* Duration of the polish kernel of the last mpcqp_solve from HIP events around its launch (OSQP's info->polish_time); mpcqp_last_kernel_ms and
 * mpcqp_last_phase_ms keep their meaning -- the polish is timed apart.  MPCQP_ERR_STATE when none ran. */
int mpcqp_last_polish_ms(mpcqp_handle *h, float *ms);

int mpcqp_sync(mpcqp_handle *h);                 /* wait for the last solve / copies */
void mpcqp_destroy(mpcqp_handle *h);             /* replaces CuCaQP::~CuCaQP (CuCaQP.cpp:16-21) */
const char *mpcqp_strerror(int code);            /* replaces the std::cerr messages of CuCaQP.cpp */

/* Measurement hooks (no reference counterpart; the reference times setSystem+initSolver+solve with
 * std::chrono, SQPOptimizationSolver.cpp:153-160).  Duration of the last solve kernel from HIP events
 * recorded around the launch on its stream (waits for the kernel). */
int mpcqp_last_kernel_ms(mpcqp_handle *h, float *ms);
/* The same split by the reference's two calls, where the handle runs them as two kernels (the on-chip mode: variant 200 + NW):
 * setup_ms = the set-up kernel (CuCaQP::initSolver, CuCaQP.cpp:183-197), solve_ms = the iteration kernel (CuCaQP::solve,
 * CuCaQP.cpp:199-211).  Handles that do both in one kernel report setup_ms = 0 and the whole kernel in solve_ms. */
int mpcqp_last_phase_ms(mpcqp_handle *h, float *setup_ms, float *solve_ms);
/* info[0..15]: n, m, batch, npad, mpad, n_blocks(n/16), L_blocks, lds_bytes_per_qp, workspace_bytes_per_qp,
 * ordering(0 natural,1 hubs-last,2 twisted), nnzP_triu, nnzA, T_blocks, factor_ops (on-chip kernels: the number of dense 16 x 16 tiles of A the
 * iteration's two sweeps run on, 0 = ELL only), ell_slots_total,
 * variant (0 = streaming kernel, NW > 0 = LDS-resident factor with NW waves per QP, 100 + NW = same kernels with
 * the factor blocks left in the HBM slab, 200 + NW = on-chip mode: factor in LDS + registers) */
int mpcqp_plan_info(const mpcqp_handle *h, long *info16);

/* What bench.py prices a launch of the on-chip mode with (variant 200 + NW; info[0..7] are zero for other kernel families).  info[0..7]: chain blocks of the factor, 1 if
 * the pattern has an arrow head (the parameter block), lengths of the two elimination chains (the critical path of each triangular sweep: one
 * dependent 16 x 16 mat-vec per position), factor blocks resident in LDS, positions per wave, hub blocks per wave in registers, and -- two-kernel
 * form -- the number of {re-factorisation, iteration} launch pairs queued behind a solve for adaptive-rho steps (0 = single kernel);
 * info[8..10]: 64-lane ELL slots of A (by row), A' (by variable) and P that a sweep walks; info[11]: twisted pairs of chains (1: plain or twisted order; more: the dissected order, whose chains info[2], info[3] describe pair 0).  No reference counterpart (the
 * reference's instruments are the two timers of SQPOptimizationSolver.cpp:133-164). */
int mpcqp_oc_info(const mpcqp_handle *h, long *info12);

/* Replaces CuCaQP::printSolverData (CuCaQP.cpp:226-269): copies the scaled problem data the kernel holds
 * for instance b back to the host (D [n], E [m], c; any pointer may be NULL). */
int mpcqp_debug_scaling(mpcqp_handle *h, int b, double *D, double *E, double *c);

/* Kernel self-test of the 16x16 block primitives (MFMA f64 A*B^T, Cholesky+inverse) on caller data:
 * A, B, C are row-major 16x16; out_gemm = C - A*B^T; out_linv = inverse of chol(S) for SPD S (lower). */
int mpcqp_debug_blockops(const double *A, const double *B, const double *C, const double *S,
                         double *out_gemm, double *out_linv, int *potrf_fail);

/* ---------------------------------------------------------------------------------------------------------------
 * Local-system evaluation on device.
 *
 * Replaces SQPOptimizationSolver::getLocalSystem (reference src/sqp_solver/SQPOptimizationSolver.cpp:100-120): the
 * CasADi function localSystemFunction_(p, x, l, u) -> (H, grad f, J_c, l - c, u - c) built at
 * SQPOptimizationSolver.cpp:47-77 with augmented variables w = [p; x] and rows c = [p; x; g(p, x)], evaluated at the
 * current SQP iterate.  Here the evaluation is a HIP kernel over a batch of instances of one stage OCP
 *     min sum_k (s_k - p)' Q (s_k - p) + u_k' R u_k   s.t.  s_{k+1} = F(s_k, u_k),   frame_k = [s_k; u_k], k < horizon
 * (cost as OptimalControlProblem::addVectorCost sums it, reference src/OptimalControlProblem.cpp:574-600; dynamics rows
 * as addEquationConstraint stacks them, :448-470; stage-interleaved frames, src/OCP_config/OCPConfig.cpp:29-46,102),
 * and its outputs are written straight into the device arrays mpcqp_update borrows (MPCQP_MEM_DEVICE), in the CSC value
 * order of mpcqp_stage_pattern -- so an SQP iteration never leaves the GPU.  Jacobians of F come from forward-mode dual
 * numbers inside the kernel (one thread per instance and QP column), not from finite differences.
 * np = nx (p is the reference state), n = np + horizon * (nx + nu), m = n + (horizon - 1) * nx + horizon * nh, where nh is the
 * number of rows of an optional per-frame path constraint lo <= h(s_k, u_k) <= hi (generated libraries only; rows [p; x; g; h],
 * their bounds travel in lbg / ubg behind the dynamics rows). */
#define MPCQP_MODEL_DOUBLE_INTEGRATOR 0   /* nx 2, nu 1, exact discrete map; no parameters                       */
#define MPCQP_MODEL_QUADROTOR 1           /* nx 12, nu 4, RK4; par = {mass, grav, arm, kappa, Jx, Jy, Jz}        */
#define MPCQP_MODEL_CARTPOLE 2            /* nx 4, nu 1, RK4; par = {m_cart, m_pole, length, grav}               */
#define MPCQP_MODEL_USER 3                /* dynamics from a generated library, see mpcqp_stage_create_user       */

typedef struct mpcqp_stage_desc {
  int model;        /* MPCQP_MODEL_*            */
  int horizon;      /* number of frames N >= 2  */
  double dt;        /* step of the discrete map */
  double Q[16];     /* diagonal state weights (first nx used)  */
  double R[8];      /* diagonal input weights (first nu used)  */
  double par[8];    /* model parameters, see MPCQP_MODEL_*     */
  int device;       /* HIP device ordinal, -1 = current device */
} mpcqp_stage_desc;

typedef struct mpcqp_stage mpcqp_stage;

/* fills `d` with the zoo's defaults for `model` (weights, parameters and dt of SURVEY.md section 8d) */
int mpcqp_stage_default(int model, int horizon, mpcqp_stage_desc *d);
/* the once-per-problem part (the reference's constructor builds the symbolic function once, SQPOptimizationSolver.cpp:12-92) */
int mpcqp_stage_create(const mpcqp_stage_desc *d, mpcqp_stage **out);
/* User-defined dynamics: the native form of the reference's gen_code / load_lib flow (solver_settings.gen_code writes the
 * CasADi function out as C, gcc builds a shared library, load_lib loads it; reference src/OptimalControlProblem.cpp:263-287,
 * 602-640).  `library_path` is a shared library generated by optimal_control_problem_amd/codegen.py from a traced discrete
 * map s_{k+1} = F(s_k, u_k): a scalar-generic functor instantiated into the same evaluation kernels (hipcc, gfx950), exporting
 * mpcqp_user_abi / _dims / _eval / _merit.  d->model and d->par are ignored (constants are baked into the generated code);
 * nx <= 16, nu <= 8.  A library generated with a stage cost l(s, u, r) (and optionally a terminal one) -- the general form of the
 * SX cost terms the reference sums in addScalarCost, src/OptimalControlProblem.cpp:491-497 -- also exports mpcqp_user_cost: the
 * objective is then sum_k l(s_k, u_k, p) with its exact Hessian (the reference's hessian(f, w), SQPOptimizationSolver.cpp:55-60) in
 * the structure the generated code reports (mpcqp_stage_pattern), and d->Q, d->R, mpcqp_stage_set_weights do not apply. */
int mpcqp_stage_create_user(const mpcqp_stage_desc *d, const char *library_path, mpcqp_stage **out);
/* Opt-in trajectory tracking: one reference state per frame.  In the reference this needs nothing special -- setReference takes an SX of any size
 * (src/OptimalControlProblem.cpp:570-572), computeOptimalTrajectory checks only that the size matches (:85-90), and the user subtracts slice k of
 * the reference in the cost term of step k.  In the formulation w = [p; x], rows [p; x; g] (SQPOptimizationSolver.cpp:47-77) the parameter block
 * is then p = [r_0; ...; r_{horizon-1}], np = horizon * nx, every p_k coupled to its own frame only: the objective is
 *     sum_k (s_k - r_k)' Q_k (s_k - r_k) + u_k' R_k u_k      or, with a generated stage cost,      sum_k l(s_k, u_k, r_k).
 * library_path NULL: a zoo model (d->model); else a library generated with per_frame_reference (it exports mpcqp_user_pref, which returns 1).
 * MPCQP_ERR_ARG for a library generated without it -- and mpcqp_stage_create_user returns MPCQP_ERR_ARG for one generated with it.
 * Every other mpcqp_stage_* entry works on the handle unchanged, with p [batch * horizon * nx]. */
int mpcqp_stage_create_tracking(const mpcqp_stage_desc *d, const char *library_path /* NULL = zoo model */, mpcqp_stage **out);
void mpcqp_stage_destroy(mpcqp_stage *s);
/* Per-frame diagonal weights (terminal costs, ramps): Qk [horizon * nx], Rk [horizon * nu], host pointers, copied; frame k is
 * weighted by Qk[k*nx ...], Rk[k*nu ...] instead of desc.Q, desc.R (the reference calls addVectorCost once per step, so weights may
 * differ by step, reference readme.md:121-128).  NULL, NULL returns to desc.Q, desc.R.  MPCQP_ERR_ARG for an evaluator generated
 * with its own stage cost. */
int mpcqp_stage_set_weights(mpcqp_stage *s, const double *Qk, const double *Rk);
/* Per-frame bounds of the path constraint, lo / hi [horizon * nh] host pointers, copied: what mpcqp_stage_merit measures violations
 * against when the bounds differ by frame -- a terminal constraint is a path constraint that is loose (-inf, +inf) on every frame
 * but the last (addInequalityConstraint is called per frame in the reference, src/OptimalControlProblem.cpp:448-470, so bounds may
 * differ by frame).  The QP itself takes its bounds from lbg / ubg of mpcqp_stage_eval either way.  NULL, NULL returns to the
 * bounds baked into the generated library. */
int mpcqp_stage_set_path_bounds(mpcqp_stage *s, const double *lo, const double *hi);
/* Per-instance plant parameters: a batch of different robots on one handle (opt-in).  Without this entry every instance of a
 * launch shares desc.par (a generated library: the defaults it was generated with).  theta [batch * MPCQP_STAGE_NPAR], row b = instance b's
 * parameters in the order of the MPCQP_MODEL_* comments above (a generated library: the order of the model's theta); entries past
 * mpcqp_stage_param_count are never read.  The values are copied into a buffer the handle owns (mem = MPCQP_MEM_HOST or MPCQP_MEM_DEVICE) before
 * the call returns.  which = MPCQP_PARAMS_MODEL: what mpcqp_stage_eval, _merit, _linesearch and the rollout tail of mpcqp_stage_advance use;
 * which = MPCQP_PARAMS_PLANT: what the plant step F(s_0, u_0) of mpcqp_stage_advance uses (not read when s_meas is given) -- as long as it is
 * not set, the plant is the model.  theta = NULL returns that set to the shared values.  The parameters are data of the dynamics: they are not QP
 * variables, do not join p, and the QP pattern does not depend on them.  A launch whose batch exceeds a stored set's is MPCQP_ERR_ARG, a smaller
 * one uses the first rows.  MPCQP_ERR_ARG as well for a handle whose mpcqp_stage_param_count is 0 (the double integrator; a library generated
 * without parameters, every library from before this entry included), a bad `which`, or batch <= 0 with a non-NULL theta. */
#define MPCQP_STAGE_NPAR 8
#define MPCQP_PARAMS_MODEL 0
#define MPCQP_PARAMS_PLANT 1
/* 7 quadrotor, 4 cart-pole, 0 double integrator, ntheta of a generated library */
int mpcqp_stage_param_count(const mpcqp_stage *s);
int mpcqp_stage_set_instance_params(mpcqp_stage *s, int which, int batch, const double *theta, int mem);
/* Stage data: per-frame, per-instance values in the path constraint and the costs -- a batch of different worlds on one handle (opt-in; DESIGN.md
 * 6.15).  In the reference the parameter SX may appear in any constraint or cost term (src/OptimalControlProblem.cpp:444-497); acados and ACADO
 * know the same as stage-wise parameters / online data.  A library generated from a model that declares nsd = k (1 <= k <= MPCQP_STAGE_MAXSD) reads
 * k values d[0..k-1] inside hfun, lcost and lterm (not in F, kfun or llink): an obstacle's centre, a corridor's width, a scheduled weight.  Without
 * a stored set every frame of every instance takes the defaults the library was generated with.  The values are data: they are not QP variables,
 * add no column, row or entry of P or A, and mpcqp_stage_pattern / _dims are those of the same model with the numbers written as constants.
 * mpcqp_stage_data_count: k of a generated library, 0 for the zoo models and for a library generated without stage data (every library from before
 * this entry included), 0 for a null handle.
 * mpcqp_stage_set_stage_data: d [batch * horizon * nsd], row (b, k) = what frame k of instance b takes, copied into a buffer the handle owns
 * (mem = MPCQP_MEM_HOST or MPCQP_MEM_DEVICE) before the call returns; mpcqp_stage_eval, _merit, _linesearch and the stage_cost log of
 * mpcqp_stage_advance (the k = 0 term, with d_0 as it stands before any shift) use it from then on.  d = NULL returns to the defaults (batch and
 * mem are then ignored).  A launch whose batch exceeds the stored set's is MPCQP_ERR_ARG, a smaller one uses the first rows.  MPCQP_ERR_ARG as
 * well for a null handle, a handle whose mpcqp_stage_data_count is 0, batch <= 0 with a non-NULL d, or a bad mem; MPCQP_ERR_HIP when the
 * allocation or the copy fails.
 * mpcqp_stage_shift_data: the receding-horizon hand-over of the stored set, one kernel on `stream`: row (b, k) becomes row (b, k + 1) for
 * k < horizon - 1, the last row d_new[b] (d_new [batch * nsd], device memory) or, with d_new = NULL, the old last row again.  Out of place between
 * two buffers of the handle, which are then swapped: launches enqueued on the same stream afterwards see the shifted set.  The data describe the
 * world, so they shift whatever the QP's status was, as the per-frame references do in mpcqp_stage_advance; call it after that entry, which
 * still reads d_0.  MPCQP_ERR_STATE when no set is stored (the defaults do not shift); MPCQP_ERR_ARG for a null handle, a handle without stage
 * data, or a batch that is not the stored set's (every stored row shifts). */
#define MPCQP_STAGE_MAXSD 8
int mpcqp_stage_data_count(const mpcqp_stage *s);
int mpcqp_stage_set_stage_data(mpcqp_stage *s, int batch, const double *d, int mem);
int mpcqp_stage_shift_data(mpcqp_stage *s, int batch, const double *d_new /* [batch * nsd], device, may be NULL */, void *stream);
/* Transition data: the stage data in the dynamics (opt-in).  A library generated from a model that also sets transition_data reads
 * d[0..k-1] inside F / cdyn, kfun and llink as well: a step length per frame (a non-uniform time grid), a previewed disturbance, a schedule.  The
 * functions of the transition k -> k + 1 take row k of the instance.  mpcqp_stage_eval, _merit, _linesearch, _rollout and _lagrangian use the rows of
 * the stored set; mpcqp_stage_advance takes row 0 for the plant step and row horizon - 1 for the rollout tail, both as they stand before
 * mpcqp_stage_shift_data, which stays a separate call after it.  The rows stay data: pattern and sizes are those of the same model with the numbers
 * written as constants.
 * mpcqp_stage_has_transition_data: 1 for such a library, 0 for every other handle (the zoo, a library generated without the flag or before this
 * entry) and for a null handle. */
int mpcqp_stage_has_transition_data(const mpcqp_stage *s);
/* dims[8] = {nx, nu, np, n, m, nnz(P), nnz(A), horizon * (nx + nu)} */
int mpcqp_stage_dims(const mpcqp_stage *s, int *dims8);
/* 1 when the evaluator was generated with its own stage cost (mpcqp_stage_create_user above), 0 for diagonal tracking weights */
int mpcqp_stage_has_cost(const mpcqp_stage *s);
/* 1 when the library was generated with a link cost llink(s_k, u_k, s_{k+1}, u_{k+1}), summed over the stages k = 0 .. horizon-2 on top of the
 * frame cost (diagonal weights or a generated stage cost): a move penalty (u_{k+1} - u_k)' S (u_{k+1} - u_k), a slew penalty on a state.  In the
 * reference any SX over two frames is a cost term (addScalarCost, src/OptimalControlProblem.cpp:491-497); here the library exports
 * mpcqp_user_link_cost, the structure of the term's Hessian over [s; u; s_next; u_next], and P couples frame k to frame k + 1 in exactly that
 * structure (both triangles; mpcqp_stage_pattern and nnz(P) of mpcqp_stage_dims report it) with the exact Hessian of the objective.  The term
 * takes no reference and no parameters; mpcqp_stage_merit and _linesearch include it, the stage_cost log of mpcqp_stage_advance (the k = 0 frame
 * term) does not.  0 for the zoo models and for a library without the export (every one generated before this entry). */
int mpcqp_stage_has_link_cost(const mpcqp_stage *s);
/* The number of residual rows nr when the library was generated with a Gauss-Newton frame cost f = sum_k |rcost(s_k, u_k, r)|^2 (the reference's
 * addVectorCost, sum w_i e_i^2 without 1/2, with a nonlinear e; an optional terminal residual on the last frame): the library exports
 * mpcqp_user_residual_cost, q is the exact gradient 2 J' r and P takes 2 J'J over [s_k; u_k; r] -- positive semidefinite by construction -- in
 * place of the exact Hessian.  mpcqp_stage_has_cost is 1 for such a handle as well; mpcqp_stage_has_convexify and _has_exact_hessian are 0.
 * 0 for the zoo models, for a scalar stage cost and for a library without the export (every one generated before this entry). */
int mpcqp_stage_has_residual_cost(const mpcqp_stage *s);
/* CSC sparsity of P (n x n, both triangles, as CasADi hands it to CuCaQP) and A = [I; dg/dw] (m x n): the arrays
 * mpcqp_create takes.  Pp, Ap: n + 1 entries; Pi: nnz(P); Ai: nnz(A).  Host pointers. */
int mpcqp_stage_pattern(const mpcqp_stage *s, int *Pp, int *Pi, int *Ap, int *Ai);
/* getLocalSystem for `batch` instances.  All pointers are device memory, instance-major and dense: p [batch*np],
 * x, lbx, ubx [batch*horizon*(nx+nu)], lbg, ubg [batch*(horizon-1)*nx]  ->  P [batch*nnzP], q [batch*n],
 * A [batch*nnzA], l, u [batch*m] with l = [p; lbx; lbg] - c, u = [p; ubx; ubg] - c.  Asynchronous on `stream`. */
int mpcqp_stage_eval(mpcqp_stage *s, int batch, const double *p, const double *x,
                     const double *lbx, const double *ubx, const double *lbg, const double *ubg,
                     double *P, double *q, double *A, double *l, double *u, void *stream);
/* objective f [batch] (SQPOptimizationSolver.cpp:180-181) and max-norm of the dynamics violation gmax [batch]
 * (either may be NULL) at iterate x; device pointers */
int mpcqp_stage_merit(mpcqp_stage *s, int batch, const double *p, const double *x, double *f, double *gmax, void *stream);
/* the damped update result.x += alpha * solution[pSize:] (SQPOptimizationSolver.cpp:171-177): x [batch*nvar] +=
 * alpha * dw[b*n + np ...]; device pointers.  step_max [batch] (may be NULL) receives max|alpha * dx| per instance.
 * status [batch] (may be NULL = the reference's behaviour: every step is taken, NaN from an infeasible QP included):
 * when given, instances whose QP status is not MPCQP_SOLVED / _SOLVED_INACCURATE / _MAX_ITER_REACHED keep their x. */
int mpcqp_stage_step(mpcqp_stage *s, int batch, double alpha, const double *dw, double *x, double *step_max,
                     const int *status, void *stream);
/* Receding-horizon hand-over between two MPC ticks, one kernel for the batch.  In the reference the step between two calls of
 * computeOptimalTrajectory is the caller's: the new first frame is pinned through lbx / ubx (src/OptimalControlProblem.cpp:93-96), the plant is
 * the caller's own code, and the next solve starts from the previous trajectory unshifted because result_ persists (SQPOptimizationSolver.cpp:88-91,
 * OptimalControlProblem.cpp:113).  Here, per instance b, with X_k = [s_k; u_k] the frames of x_in, f = nx + nu, and ok = (status == NULL or
 * status[b] is MPCQP_SOLVED / _SOLVED_INACCURATE / _MAX_ITER_REACHED, the set mpcqp_stage_step uses):
 *   plant       s+ = s_meas[b] when s_meas is given, else F(s_0, u_0) by the handle's own discrete map, plus w[b] when w is given;
 *               u+ = ok ? u_1 : u_0 (a failed QP holds the applied input)
 *   trajectory  x_out = [s+; u+], X_2, ..., X_{N-1}, tail, with tail = X_{N-1} (MPCQP_TAIL_REPEAT) or [F(s_{N-1}, u_{N-1}); u_{N-1}] (MPCQP_TAIL_ROLLOUT)
 *   pin         the first f entries of lbx[b] and ubx[b] become [s+; u+], in place; nothing else in those arrays is touched
 *   references  tracking handles only: p_out = r_1, ..., r_{N-1}, then r_new[b] (NULL: r_{N-1} again)
 *   QP start    dw_out [batch * n] from dw_in (both or neither): the parameter part copied (tracking: shifted by nx, zero last block), the frames
 *               shifted by f with a zero last block; y_out [batch * m] from y_in (both or neither): each row block of [p; x; dynamics; path; link]
 *               shifted by its own stage width (nx or as dw; f; nx; nh; nk) with a zero last block.  An instance that is not ok gets all zeros
 *               (its dw and y are NaN after an infeasible QP).
 *   logs        applied [batch * f] = X_0; stage_cost [batch] = the k = 0 term of mpcqp_stage_merit's objective at X_0, against r_0 on a tracking
 *               handle and against p[b] [batch * nx] otherwise (p is read for this only and must be given with stage_cost there)
 * All pointers are device memory; x_in, x_out, lbx, ubx are required, the rest may be NULL.  Out of place: x_out != x_in, dw_out != dw_in,
 * y_out != y_in, p_out != p_in.  Asynchronous on `stream`.  MPCQP_ERR_ARG for a bad argument; MPCQP_ERR_LIMIT for a generated library
 * from before this entry (it does not export mpcqp_user_advance; regenerate it). */
#define MPCQP_TAIL_REPEAT 0
#define MPCQP_TAIL_ROLLOUT 1
typedef struct mpcqp_stage_advance_args {
  const double *x_in; double *x_out;   /* [batch * horizon * f]                                      */
  double *lbx, *ubx;                   /* [batch * horizon * f], first f entries per instance written */
  const int *status;                   /* [batch], optional                                          */
  const double *s_meas, *w;            /* [batch * nx], optional, at most one of them                */
  const double *p;                     /* [batch * nx], non-tracking handles, for stage_cost only    */
  const double *p_in; double *p_out;   /* [batch * horizon * nx], tracking handles (required there)  */
  const double *r_new;                 /* [batch * nx], tracking handles, optional                   */
  const double *dw_in; double *dw_out; /* [batch * n], optional pair                                 */
  const double *y_in; double *y_out;   /* [batch * m], optional pair                                 */
  double *applied, *stage_cost;        /* [batch * f], [batch], optional                             */
  int tail;                            /* MPCQP_TAIL_*                                               */
} mpcqp_stage_advance_args;
int mpcqp_stage_advance(mpcqp_stage *s, int batch, const mpcqp_stage_advance_args *a, void *stream);
/* A dynamically feasible trajectory from a first frame and a sequence of inputs, one kernel for the batch (opt-in: the reference starts its SQP loop
 * at x = 0, SQPOptimizationSolver.cpp:88-91, and has no such step).  Linearised about a trajectory with s_{k+1} = F(s_k, u_k) the dynamics rows of
 * the local system are satisfied by dx = 0, so the first QP can only be infeasible through the boxes.  Per instance b, with
 * X_k = [s_k; u_k] the frames, f = nx + nu, and clip(v, lo, hi) = (v < lo ? lo : v), then (v > hi ? hi : v), elementwise against the same entries of
 * lbx / ubx (the identity without the pair; a NaN passes through):
 *   first frame  X_0 = clip(x_in[0:f]): a first frame pinned through lbx = ubx comes out as pinned, bit for bit
 *   inputs       u_k = clip(u_in_k) for k >= 1, u_in_k being x_in's own input of frame k (MPCQP_ROLLOUT_INPUTS_ITERATE) or u_0
 *                (MPCQP_ROLLOUT_INPUTS_HOLD); the states of x_in's frames k >= 1 are not read
 *   states       s_{k+1} = F(s_k, u_k), k = 0 .. N - 2, by the handle's own discrete map under the instance's stored model parameter row
 *                (MPCQP_PARAMS_MODEL) where one is set, as the rollout tail of mpcqp_stage_advance; stage data and references take no part; states
 *                are not clipped
 *   divergence   step k fails when an entry of s_k, u_k or F(s_k, u_k) is not finite: diverged[b] = the first such k, and every later state
 *                holds s_k (the inputs are still written); -1 when no step fails.  No state is written that F did not produce from finite data,
 *                but for a non-finite X_0 the caller handed in, which is held and reported as diverged[b] = 0
 *   box_viol[b]  max over all nvar entries of max(lbx - x_out, x_out - ubx, 0): 0 without the pair, an infinite bound contributes 0; with
 *                lbx <= ubx only the states of the frames k >= 1 can contribute
 *   frozen       an instance with frozen[b] != 0 is neither read nor written: its rows of x_out, diverged and box_viol keep what they held
 * One thread per instance, one writer per element, no atomics: bitwise repeatable, independent of the batch size and of the instance's position, and
 * the same in place (x_out == x_in) and out of place.  All pointers are device memory.  Asynchronous on `stream`; nothing is allocated, so a
 * captured graph replays it.  MPCQP_ERR_ARG for a null s, a, x_in or x_out, only one of lbx / ubx, an unknown `inputs`, batch < 1 or a batch larger
 * than the stored parameter rows; MPCQP_ERR_LIMIT for a generated library from before this entry (it does not export mpcqp_user_rollout;
 * regenerate it). */
#define MPCQP_ROLLOUT_INPUTS_ITERATE 0   /* u_k = the inputs of x_in's frame k                      */
#define MPCQP_ROLLOUT_INPUTS_HOLD    1   /* u_k = u_0 for every k                                   */
typedef struct mpcqp_stage_rollout_args {
  const double *x_in;  double *x_out;    /* [batch * nvar]; x_out may be x_in (in place)             */
  const double *lbx, *ubx;               /* [batch * nvar], optional pair: the box to project onto   */
  const int *frozen;                     /* [batch], optional: nonzero = neither read nor written    */
  int *diverged;                         /* [batch], optional                                        */
  double *box_viol;                      /* [batch], optional                                        */
  int inputs;                            /* MPCQP_ROLLOUT_INPUTS_*                                   */
} mpcqp_stage_rollout_args;
int mpcqp_stage_rollout(mpcqp_stage *s, int batch, const mpcqp_stage_rollout_args *a, void *stream);
/* Per-instance step length by an l1-merit backtracking search, one kernel for the batch (opt-in; replaces one mpcqp_stage_step + mpcqp_stage_merit
 * pair).  The reference takes result.x += alpha * solution[pSize:] with one alpha for every iteration (SQPOptimizationSolver.cpp:171-177: no
 * line search, no merit function); this entry departs from those lines.  Per instance b, with dx = dw[np:] and ok = (status == NULL or status[b] is
 * MPCQP_SOLVED / _SOLVED_INACCURATE / _MAX_ITER_REACHED, the set mpcqp_stage_step uses):
 *   violation  v(x) = sum |s_{k+1} - F(s_k, u_k)| + sum over the path and link rows of max(lo - h, 0) + max(h - hi, 0) (the bounds
 *              mpcqp_stage_merit uses) + sum over all nvar entries of max(lbx - x, 0) + max(x - ubx, 0); an infinite bound contributes 0
 *   merit      phi(x) = f(p, x) + mu_b v(x), f being mpcqp_stage_merit's objective
 *   penalty    mu_b = max(mu[b] if given, mu_min, mu_factor * max_{np <= i < m} |y_i|), y the multipliers of the QP just solved; written back to
 *              mu[b], so the penalty never decreases from one call to the next
 *   slope      D = min(0, sum_{j >= np} q_j dw_j - mu_b v(x)), q the gradient mpcqp_stage_eval wrote at x
 *   search     alpha_j = alpha0 * beta^j, j = 0 .. candidates - 1: the first j with phi(x + alpha_j dx) finite and <= phi(x) + c1 alpha_j D is
 *              taken, accepted[b] = j.  None: alpha_{candidates-1} if its merit is finite, accepted[b] = -1; else alpha = 0, accepted[b] = -2.
 *              An instance that is not ok keeps x bit for bit, alpha = 0, accepted[b] = -2, mu[b] untouched (its dw and y are not read).
 *   update     x += alpha dx in place, by mpcqp_stage_step's expression: candidates = 1 reproduces mpcqp_stage_step(alpha0) on finite data
 *   outputs    alpha_out, step_max = max |alpha dx|, f_out and gmax_out = what mpcqp_stage_merit returns at the new x (taken from the chosen
 *              candidate's evaluation), phi [batch * 2] = {phi(x_old), phi(x_new)} under mu_b
 * All pointers are device memory.  Asynchronous on `stream`.  MPCQP_ERR_ARG for a null required pointer, candidates outside 1..8, beta outside
 * (0, 1), alpha0 <= 0, c1 outside [0, 1); MPCQP_ERR_LIMIT for a generated library from before this entry (it does not export
 * mpcqp_user_linesearch; regenerate it). */
#define MPCQP_LINESEARCH_MAX_CANDIDATES 8
typedef struct mpcqp_stage_linesearch_args {
  const double *p;                     /* [batch * np]                                               */
  double *x;                           /* [batch * nvar], in / out                                   */
  const double *lbx, *ubx;             /* [batch * nvar]                                             */
  const double *q, *dw;                /* [batch * n]: gradient at x, QP solution                    */
  const double *y;                     /* [batch * m]: QP multipliers                                */
  const int *status;                   /* [batch], optional                                          */
  double *mu;                          /* [batch], optional, in / out                                */
  double *alpha_out;                   /* [batch], optional                                          */
  int *accepted;                       /* [batch], optional                                          */
  double *step_max, *f_out, *gmax_out; /* [batch], optional                                          */
  double *phi;                         /* [batch * 2], optional                                      */
  double alpha0, beta, c1, mu_min, mu_factor;
  int candidates;                      /* 1 .. MPCQP_LINESEARCH_MAX_CANDIDATES                       */
} mpcqp_stage_linesearch_args;
int mpcqp_stage_linesearch(mpcqp_stage *s, int batch, const mpcqp_stage_linesearch_args *a, void *stream);
/* Convexify the frame term of a general stage cost on the device (opt-in).  mpcqp_stage_eval writes the exact Hessian of the traced
 * cost into P, and a non-convex lcost / lterm makes the QP MPCQP_NON_CVX, as OSQP rejects it in the reference.  This entry, called on the P
 * mpcqp_stage_eval just wrote at the same (p, x), replaces every frame's Hessian H_k over [s_k; u_k; r] (the terminal cost's on the last frame) by
 * V f(Lambda) V', H_k = V Lambda V':
 *   MPCQP_CONVEXIFY_PROJECT  f(lam) = max(lam, eps)         MPCQP_CONVEXIFY_MIRROR  f(lam) = max(|lam|, eps)
 * A frame with lam_min(H_k) >= eps is untouched: nothing of it is written, and an instance without a touched frame keeps every bit of P.  For a
 * touched frame the correction f(H_k) - H_k is ADDED to the frame's slots of P, both triangles; in a handle with one shared reference the
 * p-p block takes the sum of the corrections over the touched frames, k ascending, in a second pass.  q, A, l, u are not arguments: the gradient
 * stays exact, only the curvature the QP sees changes.  A link cost's own entries are not convexified (it must be convex for P to be positive
 * semidefinite).  No floating-point atomics: the result is bitwise repeatable and does not depend on the batch size or the instance's position.
 * Needs a library generated from a model with convexify = True: its cost pattern is closed under the fill-in of V f(Lambda) V' (every pair of
 * indices inside one connected component of the Hessian's sparsity graph), and it exports mpcqp_user_convexify.  The handle's stored stage
 * data and per-frame references are honoured.  Stateless but for a scratch buffer the handle grows on first use; asynchronous on `stream`.
 * touched[b]: the number of touched frames of instance b; lam_min[b * horizon + k]: lam_min(H_k) before the change.
 * MPCQP_ERR_LIMIT (with the reason) for a built-in model or a library without the export; MPCQP_ERR_ARG for a mode other than the two, eps <= 0
 * or not finite, a null a, P, x or p, batch < 1, or a batch larger than the stored stage data. */
#define MPCQP_CONVEXIFY_PROJECT 1
#define MPCQP_CONVEXIFY_MIRROR  2
typedef struct mpcqp_stage_convexify_args {
  int mode; double eps;                /* MPCQP_CONVEXIFY_*; eps > 0, finite                          */
  const double *p, *x;                 /* [batch * np], [batch * nvar]: as mpcqp_stage_eval           */
  double *P;                           /* [batch * nnzP], in / out: as mpcqp_stage_eval wrote it      */
  int *touched;                        /* [batch], optional                                          */
  double *lam_min;                     /* [batch * horizon], optional                                */
} mpcqp_stage_convexify_args;
int mpcqp_stage_has_convexify(const mpcqp_stage *s);
int mpcqp_stage_convexify(mpcqp_stage *s, int batch, const mpcqp_stage_convexify_args *a, void *stream);
/* The exact Hessian of the Lagrangian on the device (opt-in).  The reference's QP takes hessian(f, w), the Hessian of the cost alone
 * (src/sqp_solver/SQPOptimizationSolver.cpp:55-60), and so does mpcqp_stage_eval; this entry departs from those lines.  With the rows
 * c(w) = [p; x; s_{k+1} - F(s_k, u_k); h(s_k, u_k); kfun(...)] and their multipliers y [m] -- what mpcqp_get returns and mpcqp_stage_linesearch takes --
 * the Lagrangian is L = f + y'c, and since the rows p and x are linear its Hessian is that of f plus, on every frame's [s_k; u_k] block,
 *   C_k = - sum_i y_dyn[k, i] d2F_i(s_k, u_k)  (k < horizon - 1)  + sum_i y_path[k, i] d2h_i(s_k, u_k),
 *   y_dyn[k, i] = y[np + nvar + k nx + i],  y_path[k, i] = y[np + nvar + (horizon - 1) nx + k nh + i].
 * Called on the P mpcqp_stage_eval just wrote at the same (p, x), it ADDS C_k to the frame's slots of P, both triangles: one thread per
 * (instance, frame, column), the column formed as -FG.d + HG.d by one pass each of the generated gradients of lam'F and mu'h on dual numbers, each
 * entry read, added to and written by one thread.  No floating-point atomics: the result is bitwise repeatable and does not depend on the batch size
 * or the instance's position.  F takes the instance's stored parameter row, h the frame's stored stage data, as in mpcqp_stage_eval.  With
 * mode = MPCQP_CONVEXIFY_PROJECT / _MIRROR the rule of mpcqp_stage_convexify then runs on H_k^L = H_k + C_k (C_k zero-padded over r) in place of H_k,
 * on the updated P: a frame it does not touch holds the bits mode = 0 gives; touched and lam_min are written as there (mode = 0 writes neither).
 * status [batch], when given: an instance whose QP status is not MPCQP_SOLVED / _SOLVED_INACCURATE / _MAX_ITER_REACHED is neither read nor
 * written (its y is NaN after an infeasible QP); with a mode its touched is 0 and its lam_min stays.  q, A, l, u are not arguments.
 * Link constraints are not covered: their curvature couples two frames, and a model with a nonlinear kfun is refused when it is traced (a linear
 * one contributes nothing); a link cost is a cost and already exact.  Needs a library generated from a model with lcost and exact_hessian = True:
 * the structure of C_k is part of its cost pattern and it exports mpcqp_user_lagrangian.  Asynchronous on `stream`.
 * MPCQP_ERR_LIMIT (with the reason) for a built-in model, a library without the export, and mode != 0 on a library without convexify = True;
 * MPCQP_ERR_ARG for a null a, x, y, P (or p with a mode), a mode other than 0 and the two, eps <= 0 or not finite with a mode, batch < 1, or a batch
 * larger than the stored stage data or parameter rows. */
typedef struct mpcqp_stage_lagrangian_args {
  const double *p, *x;                 /* [batch * np], [batch * nvar]: as mpcqp_stage_eval           */
  const double *y;                     /* [batch * m]: multiplier estimate, rows [p; x; dyn; path; link] */
  const int *status;                   /* [batch], optional                                          */
  double *P;                           /* [batch * nnzP], in / out: as mpcqp_stage_eval wrote it      */
  int mode; double eps;                /* 0 = add only; MPCQP_CONVEXIFY_PROJECT / _MIRROR with eps    */
  int *touched;                        /* [batch], optional, as mpcqp_stage_convexify                */
  double *lam_min;                     /* [batch * horizon], optional, as mpcqp_stage_convexify      */
} mpcqp_stage_lagrangian_args;
int mpcqp_stage_has_exact_hessian(const mpcqp_stage *s);
int mpcqp_stage_lagrangian(mpcqp_stage *s, int batch, const mpcqp_stage_lagrangian_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Local-system evaluation on device for a general (non-stage) NLP.
 *
 * The reference hands ANY problem to its SQP: cost and constraints are arbitrary SX over the whole decision vector, CasADi
 * differentiates them with their true sparsity -- hessian(f, w), jacobian([p; x; g], w), w = [p; x] (reference
 * src/sqp_solver/SQPOptimizationSolver.cpp:47-77) -- and getLocalSystem is one compiled call per iteration (:100-120), followed by
 * the damped update and the objective (:171-181).  mpcqp_stage_* above does that on the device for the stage pattern; the entries
 * below do it for everything else.  `library_path` is a shared library generated by optimal_control_problem_amd/codegen.py
 * (build_general_device_library) from the traced cost and constraints: one scalar-generic functor with the cost, its
 * reverse-derived gradient and the constraints, instantiated into the kernels of csrc/general_kernels.hpp (hipcc, gfx950), with
 * the CSC pattern and the colouring tables that compress the Hessian and Jacobian passes.  Rows [p; x; g], l = [p; lbx; lbg] - c,
 * u = [p; ubx; ubg] - c with c = [p; x; g(p, x)]; infinite bounds stay infinite.  np = 0 and ng = 0 are allowed (their arrays
 * have no elements and may be NULL).
 * Errors: MPCQP_ERR_ARG for null pointers, batch <= 0, a library that cannot be loaded, lacks a symbol or was generated for another
 * version of the kernels; MPCQP_ERR_NO_GPU without a device. */
typedef struct mpcqp_nlp mpcqp_nlp;

/* dlopen, ABI version check, tables uploaded once (SQPOptimizationSolver.cpp:47-77: the once-per-problem part); device: HIP
 * ordinal, -1 = current device */
int mpcqp_nlp_create(const char *library_path, int device, mpcqp_nlp **out);
void mpcqp_nlp_destroy(mpcqp_nlp *s);
/* dims[8] = {nvar, np, ng, n, m, nnz(P), nnz(A), passes}: passes = evaluations of the functor per instance and call (the colours
 * of the Hessian plus those of the Jacobian; SQPOptimizationSolver.cpp:47-77) */
int mpcqp_nlp_dims(const mpcqp_nlp *s, int *dims8);
/* CSC sparsity of P (n x n, both triangles) and A = [I; dg/dw] (m x n), as mpcqp_create takes them (SQPOptimizationSolver.cpp:47-77).
 * Pp, Ap: n + 1 entries; Pi: nnz(P); Ai: nnz(A).  Host pointers. */
int mpcqp_nlp_pattern(const mpcqp_nlp *s, int *Pp, int *Pi, int *Ap, int *Ai);
/* getLocalSystem for `batch` instances (SQPOptimizationSolver.cpp:100-120).  Device pointers, instance-major and dense: p [batch*np],
 * x, lbx, ubx [batch*nvar], lbg, ubg [batch*ng]  ->  P [batch*nnzP], q [batch*n], A [batch*nnzA], l, u [batch*m].  Every output
 * element has one writer: two calls on the same input give the same bits.  Asynchronous on `stream`. */
int mpcqp_nlp_eval(mpcqp_nlp *s, int batch, const double *p, const double *x, const double *lbx, const double *ubx,
                   const double *lbg, const double *ubg, double *P, double *q, double *A, double *l, double *u, void *stream);
/* objective f [batch] (SQPOptimizationSolver.cpp:180-181) and gmax [batch], the max-norm violation of lbg <= g(p, x) <= ubg (0 when
 * feasible or ng = 0); either output may be NULL; device pointers */
int mpcqp_nlp_merit(mpcqp_nlp *s, int batch, const double *p, const double *x, const double *lbg, const double *ubg,
                    double *f, double *gmax, void *stream);
/* the damped update of SQPOptimizationSolver.cpp:171-177, with the semantics of mpcqp_stage_step (step_max and status optional) */
int mpcqp_nlp_step(mpcqp_nlp *s, int batch, double alpha, const double *dw, double *x, double *step_max, const int *status, void *stream);
/* Per-instance step length by an l1-merit backtracking search for a general NLP, one kernel for the batch (opt-in; replaces one mpcqp_nlp_step +
 * mpcqp_nlp_merit pair).  The reference takes result.x += alpha * solution[pSize:] with one alpha for every iteration
 * (SQPOptimizationSolver.cpp:171-177: no line search, no merit function); this entry departs from those lines.  The rule is the one of
 * mpcqp_stage_linesearch above, word for word -- penalty, slope, search, update, outputs, the treatment of an instance that is not ok -- with
 * these two measures:
 *   violation  v(x) = sum over the ng general rows of max(lbg - g, 0) + max(g - ubg, 0) + sum over all nvar entries of max(lbx - x, 0) +
 *              max(x - ubx, 0); an infinite bound contributes 0
 *   objective  f(p, x) and gmax_out are what mpcqp_nlp_merit returns (gmax: general rows only, floor 0), bit for bit at the new x
 *   update     x += alpha dx in place, by mpcqp_nlp_step's expression: candidates = 1 reproduces mpcqp_nlp_step(alpha0) bit for bit on finite data
 * The result is bitwise repeatable and does not depend on the batch size or on the instance's position in the batch.  All pointers are device
 * memory (p may be NULL when np = 0, lbg / ubg when ng = 0).  Asynchronous on `stream`; nothing is allocated, a captured graph replays it.
 * MPCQP_ERR_ARG for a null handle, batch <= 0, a null argument block or required pointer, candidates outside 1..8, beta outside (0, 1),
 * alpha0 <= 0, c1 outside [0, 1), mu_min or mu_factor negative or not finite; MPCQP_ERR_LIMIT for a generated library without the export
 * mpcqp_general_linesearch -- one generated before this entry, or with line_search=False; regenerate it.  The handle stays usable after either.
 * mpcqp_nlp_has_linesearch: 1 when the handle's library carries the kernel, 0 otherwise or for a null handle. */
typedef struct mpcqp_nlp_linesearch_args {
  const double *p;                     /* [batch * np]                                               */
  double *x;                           /* [batch * nvar], in / out                                   */
  const double *lbx, *ubx;             /* [batch * nvar]                                             */
  const double *lbg, *ubg;             /* [batch * ng]                                               */
  const double *q, *dw;                /* [batch * n]: gradient at x, QP solution                    */
  const double *y;                     /* [batch * m]: QP multipliers                                */
  const int *status;                   /* [batch], optional                                          */
  double *mu;                          /* [batch], optional, in / out                                */
  double *alpha_out;                   /* [batch], optional                                          */
  int *accepted;                       /* [batch], optional                                          */
  double *step_max, *f_out, *gmax_out; /* [batch], optional                                          */
  double *phi;                         /* [batch * 2], optional                                      */
  double alpha0, beta, c1, mu_min, mu_factor;
  int candidates;                      /* 1 .. MPCQP_LINESEARCH_MAX_CANDIDATES                       */
} mpcqp_nlp_linesearch_args;
int mpcqp_nlp_has_linesearch(const mpcqp_nlp *s);
int mpcqp_nlp_linesearch(mpcqp_nlp *s, int batch, const mpcqp_nlp_linesearch_args *a, void *stream);
/* The exact Hessian of the Lagrangian for a general NLP (opt-in).  The reference's QP takes hessian(f, w), the Hessian of the cost
 * alone (src/sqp_solver/SQPOptimizationSolver.cpp:55-60), and so does mpcqp_nlp_eval; this entry departs from those lines, as mpcqp_stage_lagrangian
 * does for the stage pattern.  With the rows c(w) = [p; x; g(w)], w = [p; x], and their multipliers y [m] -- what mpcqp_get returns and
 * mpcqp_nlp_linesearch takes -- the Lagrangian is L = f + y'c, and since the rows p and x are linear its Hessian is that of f plus
 *   C(w, y) = sum_i y[n + i] d2 g_i(w) / dw2     over the whole of w, parameter columns included, as P is.
 * Called on the P mpcqp_nlp_eval just wrote at the same (p, x):
 *   mode 0                   P <- P + C on the slots of C's structure.  With a workspace C [batch * nnzP] the curvature is written there first
 *                            (its slots outside C's structure are not touched) and added by a second kernel; without one it is added to P
 *                            directly.  Both give the same bits.
 *   MPCQP_NLP_DOMINANT       the convexity safeguard: with R_c = sum_{r != c} |C_rc| and d_c = max(0, R_c - C_cc), P <- (P + C) + diag(d).
 *                            C + diag(d) is diagonally dominant with a non-negative diagonal, hence positive semidefinite: P' is at least the
 *                            Hessian of f whatever the multipliers are, d_c = 0 wherever C is already dominant, and y = 0 leaves P as it is.
 *                            The rule is conservative -- it does not keep all of the curvature.  Needs the workspace.  shift [batch * n], when
 *                            given, receives d_c for every column c with curvature of every instance that is read; nothing else is written to
 *                            it, so zero it beforehand.
 * A slot whose addend is zero keeps its bits.  status [batch], when given: an instance whose QP status is not MPCQP_SOLVED / _SOLVED_INACCURATE /
 * _MAX_ITER_REACHED is neither read nor written (its y is NaN after an infeasible QP).  q, A, l, u are not arguments: the gradient, the merit and
 * the fixed points stay exact.  Every entry has one writer and there are no atomics: the result is bitwise repeatable and does not depend on the
 * batch size or the instance's position.  Asynchronous on `stream`; nothing is allocated, a captured graph replays it.  Needs a library generated
 * from a model with exact_hessian=True (general_nlp.GeneralNLP): the structure of C is part of its pattern of P -- mpcqp_nlp_eval writes 0 to the
 * added slots -- and it exports mpcqp_general_lagrangian.  A flagged model without curvature (linear constraints, ng = 0) makes the call a no-op.
 * MPCQP_ERR_ARG for a null handle, a, x, y or P, a null p when np > 0, a null C with MPCQP_NLP_DOMINANT, any other mode, batch < 1;
 * MPCQP_ERR_LIMIT (with the reason) for a library without the export.  The handle stays usable after either.
 * mpcqp_nlp_has_exact_hessian: 1 when the handle's library carries the kernels, 0 otherwise or for a null handle. */
#define MPCQP_NLP_DOMINANT 1
typedef struct mpcqp_nlp_lagrangian_args {
  const double *p, *x;                 /* [batch * np], [batch * nvar]: as mpcqp_nlp_eval             */
  const double *y;                     /* [batch * m]: multiplier estimate, rows [p; x; g]           */
  const int *status;                   /* [batch], optional                                          */
  double *P;                           /* [batch * nnzP], in / out: as mpcqp_nlp_eval wrote it at the same (p, x) */
  double *C;                           /* [batch * nnzP] workspace; optional with mode 0, required with MPCQP_NLP_DOMINANT */
  int mode;                            /* 0 or MPCQP_NLP_DOMINANT                                    */
  double *shift;                       /* [batch * n], optional out; written only with MPCQP_NLP_DOMINANT */
} mpcqp_nlp_lagrangian_args;
int mpcqp_nlp_has_exact_hessian(const mpcqp_nlp *s);
int mpcqp_nlp_lagrangian(mpcqp_nlp *s, int batch, const mpcqp_nlp_lagrangian_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * First-order optimality residuals of the NLP, per instance, one kernel for the batch (opt-in).  The reference's loop has no
 * convergence test (src/sqp_solver/SQPOptimizationSolver.cpp:127-216: a fixed number of iterations; the ||dx|| < 1e-6 stop exists only when
 * verbose, :183-197); these entries depart from those lines.  They read what an SQP iteration already holds on the device: the local system
 * (q, A, l, u) mpcqp_stage_eval / mpcqp_nlp_eval just wrote at w = [p; x] -- q = grad f(w), A = d[p; x; g]/dw in the CSC value order of the
 * handle's pattern, l = [p; lbx; lbg] - c(w), u = [p; ubx; ubg] - c(w) -- and multipliers y [m], rows [p; x; g], in the sign convention of
 * mpcqp_get (P x + q + A'y = 0, y_i > 0 on an active upper bound).  With col0 = np (the parameter columns are skipped: their pinned rows
 * absorb any value):
 *   t_j    = sum_k A_kj y_k, the entries of column j added in storage order, each product and each sum rounded (no fused multiply-add)
 *   stat   = max_{j >= col0} |q_j + t_j|                  scale = max_{j >= col0} max(|q_j|, |t_j|)
 *   feas   = max_i max(l_i, -u_i, 0)                      (the distance of 0 from [l_i, u_i]: the violation of the NLP's own bounds at w)
 *   compl  = max_i max( min(max(y_i, 0), max(u_i, 0)), min(max(-y_i, 0), max(-l_i, 0)) )
 *            (the min form: no product with an infinite bound; a multiplier pushing on a bound that is +-inf or +-1e30 counts in full, an
 *            equality row at a feasible point counts 0)
 *   converged = stat <= tol_stat * max(1, scale)  and  feas <= tol_feas  and  compl <= tol_compl
 * res[4 b ..] = {stat, feas, compl, scale}.  A NaN anywhere in the instance's q, A, l, u, y -- the parameter columns included -- or in a q_j + t_j
 * makes all four NaN and converged 0: an instance whose last QP returned no point has a NaN y and never reads as converged.
 * frozen [batch], when given: an instance with a nonzero entry is neither read nor written (its res and converged keep their bits).
 * One lane group of 16, 32 or 64 lanes per instance, chosen from max(n - col0, m); a lane owns columns lane, lane + G, ... and then rows
 * lane, lane + G, ...; the maxima are reduced by a fixed xor butterfly inside the group and one lane writes.  No atomics, no LDS: the result
 * is bitwise repeatable and does not depend on the batch size or on the instance's position in the batch.  All pointers are device memory,
 * instance-major and dense.  Asynchronous on `stream`; the handle keeps the pattern of A on the device from its creation, so a call allocates
 * nothing, copies nothing, and a captured graph replays it.  Generated libraries take no part: every handle has the entry.
 * MPCQP_ERR_ARG for a null handle, batch <= 0, a null argument block, a null q, A, l, u, y or res, or a tolerance that is negative or NaN. */
typedef struct mpcqp_kkt_args {
  const double *q, *A, *l, *u, *y;     /* [batch * n | nnzA | m | m | m]                              */
  double *res;                         /* [batch * 4]: stat, feas, compl, scale                      */
  int *converged;                      /* [batch], optional                                          */
  const int *frozen;                   /* [batch], optional: nonzero = neither read nor written      */
  double tol_stat, tol_feas, tol_compl;
} mpcqp_kkt_args;
int mpcqp_stage_kkt(mpcqp_stage *s, int batch, const mpcqp_kkt_args *a, void *stream);
int mpcqp_nlp_kkt(mpcqp_nlp *s, int batch, const mpcqp_kkt_args *a, void *stream);

/* Time-varying LQR feedback gains along the plan, one backward Riccati sweep per instance in one kernel (opt-in; the reference hands the plant
 * X_0 only and has no such step), and the feedback law u = u_k + K_k (s - s_k) applied in a second one (DESIGN 6.29;
 * models.StageOCP.riccati_gains and StageOCP.feedback are the host statements).  The gains are those of the equality-constrained tangent problem
 * of the local system mpcqp_stage_eval wrote (and mpcqp_stage_convexify / mpcqp_stage_lagrangian may have made positive definite):
 * inequalities enter only through the clamp.  Per instance b of a handle with N frames, f = nx + nu:
 *   H_k [f x f]      frame k's block of P: rows and columns np + k f + (0 .. f-1).  Both triangles are stored and each entry is read from its
 *                    own slot; an entry outside the pattern is 0
 *   [A_k B_k]        [nx x f], MINUS the dynamics block of A: rows n + k nx + r, columns np + k f + c, k = 0 .. N-2 (mpcqp_stage_eval writes
 *                    -dF there); an entry outside the pattern is 0
 *   not read         the reference columns and rows, the path rows, the link rows (nk > 0 is accepted, the rows are ignored like the path
 *                    rows), q, l, u
 * Backwards from k = N-1, with Q = [Q_ss Q_su; Q_us Q_uu] split at nx and acc(...) a sum in ascending index order from 0:
 *   Q          k = N-1: Q = H_{N-1} as read.  k < N-1: T = V_{k+1} [A_k B_k], then for r <= c
 *              Q[r][c] = Q[c][r] = H_k[r][c] + acc_j [A_k B_k][j][r] T[j][c]: the upper triangle is formed once and mirrored, so Q is
 *              symmetric bit for bit (the lower triangle of H_k is then not used)
 *   clamp      optional, needs x, lbx, ubx together: input i of frame k is clamped when x - lbx <= clamp_tol or ubx - x <= clamp_tol at entry
 *              k f + nx + i (a NaN there compares false: not clamped); a pinned first frame is therefore always clamped.  Row and column i of
 *              Q_uu become the unit vector and row i of Q_us becomes 0 -- the control-limited DDP rule: row i of K_k is 0 and the input does
 *              not enter V_k
 *   reg        added to the diagonal of Q_uu, free inputs only (>= 0, default 0)
 *   Cholesky   Q_uu = U' U from the upper triangle of Q_uu, by rows, together with the forward solve Y = U'^-1 Q_us: for jj = 0 .. nu-1
 *              d = Q_uu[jj][jj] - acc_t U[t][jj]^2 (t < jj);  the frame FAILS when !(d > thr), thr = MPCQP_RICCATI_PIVOT * max(1, max_i |Q_uu[i][i]|)
 *              (the diagonal after clamp and reg, a NaN entry skipped by the max; a non-finite pivot fails);  U[jj][jj] = sqrt(d);
 *              M[jj][c] = (M[jj][c] - acc_t U[t][jj] M[t][c]) / U[jj][jj] for the columns c > jj of Q_uu (giving U) and every column of Q_us (giving Y)
 *   gain       K_k = -U^-1 Y [nu x nx] by back substitution: z_i = (Y[i][j] - acc_t U[i][t] z_t (t = i+1 .. nu-1)) / U[i][i], K_k[i][j] = -z_i
 *   value      V_k[r][c] = V_k[c][r] = Q_ss[r][c] - acc_i Y[i][r] Y[i][c] for r <= c: symmetric bit for bit
 *   failure    failed[b] = the frame whose pivot failed (the first one met, walking backwards), -1 if none.  K_j and V_j for every j <= failed[b]
 *              are written as zeros -- a zero gain is the open-loop plan, the safe answer; the frames above keep what was computed
 *   frozen     an instance with frozen[b] != 0 is neither read nor written
 * The device runs the same operations with fused multiply-adds, so it agrees with the statement to rounding, not bit for bit.  One lane group of
 * 16 (f <= 16) or 32 lanes per instance, lanes own columns, the tiles V, Q, [A B], T in LDS; one writer per element, no atomics: bitwise repeatable
 * and independent of the batch size and of the instance's position.  The handle builds two slot tables from its own pattern on the first call
 * and frees them in mpcqp_stage_destroy: a first call while `stream` is capturing answers MPCQP_ERR_STATE (call once before the capture); after
 * that nothing is allocated and a captured graph replays the launch.  No model code takes part, so a generated library needs no export.
 * MPCQP_ERR_ARG for a null s, a, P, A or K, a partial clamp triple, a negative (or NaN) clamp_tol or reg, batch < 1; MPCQP_ERR_LIMIT (with the
 * reason) for a handle with a link cost (mpcqp_stage_has_link_cost): its P couples neighbouring frames, and a sweep that dropped those blocks
 * would be silently wrong. */
#define MPCQP_RICCATI_PIVOT 1e-12
typedef struct mpcqp_stage_riccati_args {
  const double *P, *A;          /* [batch * nnzP], [batch * nnzA] on the handle's pattern      */
  const double *x, *lbx, *ubx;  /* [batch * nvar], all three or none: the clamp                */
  double clamp_tol, reg;
  const int *frozen;            /* [batch], optional: nonzero = neither read nor written       */
  double *K;                    /* [batch * N * nu * nx], (k, i, j) row-major, required        */
  double *V;                    /* [batch * N * nx * nx], optional                             */
  int *failed;                  /* [batch], optional                                           */
} mpcqp_stage_riccati_args;
int mpcqp_stage_riccati(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_args *a, void *stream);
/* The direct solve of the stage QP where no inequality is active (opt-in; models.StageOCP.direct_qp is the host statement).  The
 * QP  min 1/2 w'P w + q'w  s.t.  l <= A w <= u  of a local system is, with every inequality slack, the equality-constrained tangent problem:
 * one Riccati recursion with its affine terms solves that exactly.  The entry solves it per instance, tests the result against every inequality
 * row, and reports in direct[b] whether the result IS the QP's solution; only the instances it does not accept need mpcqp_solve (direct > 0 is
 * the array mpcqp_set_skip takes).  H_k, [A_k B_k] and acc(...) are those of mpcqp_stage_riccati above; w = [dp; d_0 .. d_{N-1}], d_k = [ds_k; du_k],
 * variable c of frame k is column and identity row j = np + k f + c; q_k = q[np + k f ..]; dynamics row n + k nx + r reads
 * ds_{k+1}[r] - ([A_k B_k] d_k)[r] and its entry on ds_{k+1} is taken as 1 (not read); path rows n + (N-1) nx + k nh + r, link rows behind them.
 *   eligible   read from l, u alone.  All of: l_j == u_j == 0 on every parameter row; l == u on every state row of frame 0 (ds_0 = l there);
 *              every input row of frame 0 either pinned (l == u: du = l) or free, no NaN in its l, u; on every identity row of the frames
 *              k >= 1 no NaN in l, u and not l == u; l == u on every dynamics row (b_k = l there).  A NaN compares unequal.  Otherwise
 *              direct[b] = -1 and nothing else is written.
 *   backwards  k = N-1 .. 0.  Q as in mpcqp_stage_riccati.  g [f]: k = N-1: g = q_k.  k < N-1: h[j] = acc_i V_{k+1}[j][i] b_k[i] + v_{k+1}[j], then
 *              g[c] = q_k[c] + acc_j [A_k B_k][j][c] h[j].
 *              k = 0 only, the pins (P the pinned inputs, in ascending order): a free input i gets g_u[i] += acc_{p in P} Q_uu[p][i] l_p; a pinned
 *              input p gets g_u[p] = -l_p, row p of Q_us = 0, row and column p of Q_uu = the unit vector.  There is no clamp in the frames k >= 1.
 *              reg (>= 0) is added to the diagonal of Q_uu, free inputs only.
 *              Cholesky and pivot test as in mpcqp_stage_riccati, with g_u as one more column: y0[jj] = (g_u[jj] - acc_t U[t][jj] y0[t]) / U[jj][jj].
 *              A failed pivot at any frame ends the instance: direct[b] = -2, nothing else is written.
 *              K_k as there; kappa_k: z_i = (y0[i] - acc_t U[i][t] z_t (t = i+1 .. nu-1)) / U[i][i], kappa_k[i] = -z_i.
 *              k >= 1: V_k as there, v_k[r] = g_s[r] - acc_i Y[i][r] y0[i].
 *   forwards   ds_0 = l.  du_k[i] = acc_j K_k[i][j] ds_k[j] + kappa_k[i] (a pinned input of frame 0: l, exactly);
 *              ds_{k+1}[r] = acc_c [A_k B_k][r][c] d_k[c] + b_k[r].
 *   adjoint    k = N-1 .. 0, in the convention of mpcqp_get (P w + q + A'y = 0):  e[c] = acc_r H_k[r][c] d_k[r] + q_k[c] (column c of H_k: P
 *              stores both triangles),  t[c] = acc_r [A_k B_k][r][c] y_k[r] (0 at k = N-1),  val[c] = t[c] - e[c].  k >= 1: the multiplier of
 *              dynamics row n + (k-1) nx + c is y_{k-1}[c] = val[c], c < nx: the state columns are stationary by construction, the input columns
 *              by the gain.  k = 0: a pinned identity row j = np + c (every state, the pinned inputs) closes its own column, y_j = val[c].
 *              A parameter row j closes its column too: y_j = -(acc_e P_e w_row(e) + q_j) over the entries of column j of P in rows >= np, in
 *              storage order (dp = 0: the entries in the parameter rows are not read).  Every other row -- the identity rows of free
 *              variables, the path rows, the link rows -- gets 0.
 *   z          z_j = w_j on the identity rows, z = l on the dynamics rows (A w there, up to rounding), and on a path or link row the entries of
 *              the row times w in ascending column order (a link row: frame k, then frame k + 1; a structural zero is skipped).
 *   accepted   direct[b] = 1 iff l_i - feas_tol <= z_i <= u_i + feas_tol on every identity row of a free variable, every path row and every link
 *              row (a NaN compares false and rejects); otherwise direct[b] = 0.  Only an accepted instance has w, y, z written; a rejected,
 *              ineligible or failed one writes direct[b] alone, and a frozen one (frozen[b] != 0) is neither read nor written, direct[b] included.
 * Why accepted means optimal: positive pivots make the objective strictly convex on the set the equalities (pins, dynamics) leave, so (w, y) is
 * that set's unique minimiser with its multipliers; a minimiser over a set that also lies in a subset of it minimises over the subset, and zero
 * multipliers on the slack inequalities complete the KKT conditions of the QP.  This needs no P >= 0 on the whole space: the entry can accept an
 * instance mpcqp_solve would report as MPCQP_NON_CVX, and its answer is then the minimiser the tangent problem does have.
 * The device runs the same operations with fused multiply-adds: it agrees with the statement to rounding.  stage_direct_kernel uses the size
 * classes, lane groups and tiles of the gain sweep plus six vectors per group; K_k, kappa_k and d_k go through a workspace the handle owns
 * (batch N (nu (nx + 1) + f) doubles, grown when a larger batch arrives); forward and adjoint passes run in the same kernel by the same group.  One
 * writer per element, no atomics: bitwise repeatable, independent of the batch size and of the instance's position.  The first call builds the
 * slot tables (those of mpcqp_stage_riccati included), and the first call at a batch allocates the workspace: either while `stream` is capturing
 * answers MPCQP_ERR_STATE (call once before the capture); after that nothing is allocated and a captured graph replays the launch.
 * MPCQP_ERR_ARG for a null s, a, P, q, A, l, u, w, y or direct, a negative (or NaN) feas_tol or reg, batch < 1; MPCQP_ERR_LIMIT (with the reason)
 * for a handle with a link cost, as mpcqp_stage_riccati answers. */
typedef struct mpcqp_stage_riccati_solve_args {
  const double *P, *q, *A, *l, *u;   /* [batch * nnzP | n | nnzA | m | m], the local system          */
  double feas_tol, reg;
  const int *frozen;            /* [batch], optional: nonzero = neither read nor written       */
  double *w;                    /* [batch * n], required                                       */
  double *y;                    /* [batch * m], required                                       */
  double *z;                    /* [batch * m], optional                                       */
  int *direct;                  /* [batch], required: 1 accepted, 0 rejected, -1 ineligible, -2 a pivot failed */
} mpcqp_stage_riccati_solve_args;
int mpcqp_stage_riccati_solve(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_args *a, void *stream);
/* The direct solve with active input bounds (opt-in; models.StageOCP.direct_qp_active is the host statement): the entry above, then
 * up to `rounds` primal-dual active-set rounds over the INPUT box rows, all in one kernel.  An input held at its bound is a pinned input, and the
 * recursion absorbs a pin at no cost; state bounds, path rows and link rows are still only tested.  Notation, eligibility, reg, frozen, z and the
 * pivot test are those of mpcqp_stage_riccati_solve.  The set S holds inputs (k, i) of any frame, each at its lower or its upper bound; the
 * inputs of frame 0 that the bounds pin (l == u) stay pinned, are not part of S, and their entries of act_in / act_out are neither read nor written.
 *   round 0    the entry above with S empty, operation for operation.  A failed pivot: direct[b] = -2.  An instance accepted here has that entry's
 *              bits in w, y, z, direct[b] = 1 and rounds_used[b] = 0.
 *   hopeless   after the forward pass of any round: some identity row of a state of a frame k >= 1, some path row or some link row has
 *              !(l_i - feas_tol <= z_i <= u_i + feas_tol) (a NaN counts).  No set over the inputs repairs those rows here: direct[b] = 0 at once.
 *   violation  a free input (not pinned, not in S) with du < l - feas_tol violates its lower bound, else with du > u + feas_tol its upper bound.
 *   round 1's set   every violating input, held at the bound it violates; and every entry of act_in (when given) -1 / +1 whose input does not
 *              violate, is not pinned and whose named bound is finite, held at that bound (an infinite bound cannot be held: the entry is ignored;
 *              where guess and violation disagree the violation decides).
 *   a round with S   the three passes of the entry above with the pin rule of frame 0 applied at every frame: the held set C of frame k is S's
 *              inputs of that frame (and, k = 0, the pins), c_p the bound input p is held at (the pins: l).  After Q and g are formed, with Q as
 *              it stands before any of it is rewritten and p in ascending order: a free input i gets g_u[i] += acc_{p in C} Q_uu[p][i] c_p;
 *              for k >= 1 a state column j gets g_s[j] += acc_{p in C} Q_us[p][j] c_p (this enters v_k.  Frame 0 has no v_0, so the entry above
 *              could leave the state columns out, and frame 0 still does); a held input p gets g_u[p] = -c_p, row p of Q_us = 0, row and column p
 *              of Q_uu = the unit vector; reg is added on free inputs only.  Forwards a held input takes c_p exactly.  Adjoint: the identity row of
 *              a held input closes its own column, y_j = val[c], as the pinned rows of frame 0 do.  A failed pivot in a round >= 1 rejects
 *              (direct[b] = 0): with positive pivots in round 0 it can only be rounding.
 *   test       primal as above: every identity row of a free variable, every path row, every link row within feas_tol.  Dual, in the sign
 *              convention of mpcqp_get: a row held at its upper bound needs y_j >= -dual_tol, one held at its lower bound y_j <= dual_tol (a NaN
 *              fails).  Both hold: direct[b] = 1, w, y, z are written, rounds_used[b] = the round.
 *   update     test failed, not hopeless, rounds remain: every violating input joins S at the bound it violates, every held input whose
 *              multiplier fails the dual test leaves S.  After round `rounds` the instance is rejected: direct[b] = 0.
 *   act_out    the last set formed, i.e. the set of the last round the instance ran (round 0: empty), -1 / +1 / 0 per input, for accepted and
 *              rejected instances alike: the next tick's guess.  rounds_used[b] = that round.  An ineligible (-1), failed (-2) or frozen instance
 *              writes neither.  act_out may be act_in: an entry is read in round 0 and written at the end by the same thread.
 * Why accepted means optimal: the argument of the entry above (a minimiser over a set that lies in a subset) does not carry over -- a held bound
 * makes the round's feasible set SMALLER than the QP's.  What carries it is round 0: its positive pivots make the objective strictly convex on
 * the set the pins and the dynamics leave, and the QP's feasible set lies in that set, so the QP has at most one KKT point and a KKT point is its
 * minimiser.  A round's point with the primal and the dual test passed IS a KKT point of the QP: stationary by construction, feasible, zero
 * multipliers on slack rows, the right sign on held ones.
 * stage_direct_active_kernel uses the size classes, lane groups and tiles of stage_direct_kernel; its workspace (the handle's, grown with the
 * batch: batch N (nu (nx + 1) + 2 f + 1) doubles) also holds val and the set words of the round at work and of the next.  The loop over rounds is
 * uniform over the block; one writer per element, no atomics: bitwise repeatable, independent of the batch size and of the instance's position.
 * Capture rules as above (the first call, and the first at a larger batch, answer MPCQP_ERR_STATE under capture).  MPCQP_ERR_ARG and
 * MPCQP_ERR_LIMIT as above, MPCQP_ERR_ARG also for rounds outside 1 .. MPCQP_ACTIVE_MAX_ROUNDS and a negative (or NaN) dual_tol. */
#define MPCQP_ACTIVE_MAX_ROUNDS 8
typedef struct mpcqp_stage_riccati_solve_active_args {
  const double *P, *q, *A, *l, *u;   /* [batch * nnzP | n | nnzA | m | m], the local system          */
  double feas_tol, reg;
  const int *frozen;            /* [batch], optional: nonzero = neither read nor written       */
  double *w;                    /* [batch * n], required                                       */
  double *y;                    /* [batch * m], required                                       */
  double *z;                    /* [batch * m], optional                                       */
  int *direct;                  /* [batch], required: 1 accepted, 0 rejected, -1 ineligible, -2 a pivot failed in round 0 */
  int rounds;                   /* 1 .. MPCQP_ACTIVE_MAX_ROUNDS: the rounds after round 0      */
  double dual_tol;              /* >= 0                                                        */
  const int *act_in;            /* [batch * N * nu], optional: the guess, -1 / 0 / +1          */
  int *act_out;                 /* [batch * N * nu], optional; may alias act_in                */
  int *rounds_used;             /* [batch], optional                                           */
} mpcqp_stage_riccati_solve_active_args;
int mpcqp_stage_riccati_solve_active(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_active_args *a, void *stream);
/* The interior-point direct solve (opt-in; models.StageOCP.direct_qp_ipm is the host statement): mpcqp_stage_riccati_solve as
 * iteration 0, then up to `iters` iterations of a primal-dual interior-point method over the box rows of the free variables -- STATES and inputs,
 * either side, any frame -- all in one kernel.  A bound on a state cannot be pinned; it can be barriered: a log-barrier on a box row adds a
 * positive term to the diagonal of H_k and a term to q_k and changes nothing else, so an iteration is the backward and the forward pass of the
 * entry above on modified data.  Notation, eligibility (-1), reg, frozen, z, the pivot test and the capture rules are those of
 * mpcqp_stage_riccati_solve.
 *   barriered rows   every identity row of a free variable: states and inputs of the frames k >= 1, the inputs of frame 0 that are not pinned.
 *              Each finite side has a slack t > 0 and a multiplier lambda > 0 of its own; an infinite side has neither.  Path rows and link rows
 *              are NOT barriered: they are tested at a candidate, and a violation there rejects the instance.
 *   inside     w is inside when every barriered row has l_j - feas_tol <= w_j <= u_j + feas_tol (a NaN fails): the test of the entry above.
 *   iteration 0  the entry above, operation for operation: w0.  A failed pivot: direct[b] = -2.  w0 inside: w0 is a candidate with no
 *              multipliers; path and link rows within feas_tol: direct[b] = 1 with that entry's bits in w, y, z, iters_used[b] = 0; else
 *              direct[b] = 0, iters_used[b] = 0.  w0 satisfies the dynamics and the pins exactly, and every later iterate is an affine
 *              combination of such points: the dynamics rows never carry a residual, z = l there as before.
 *   start      w0 not inside: per finite side t = max(w0 - l, MPCQP_IPM_T0) resp. max(u - w0, MPCQP_IPM_T0) (the slack where it is larger,
 *              else T0), lambda = MPCQP_IPM_MU0 / t.
 *   mu         the mean of lambda t over all finite sides: per column the frames in ascending order (lower side, then upper side), then the
 *              columns by the butterfly of the lane group (v + v[lane ^ o], o = W / 2 .. 1; W = 16 for f <= 16, else 32), divided by the count.
 *   sigma      1 when the last iterate was a candidate whose stationarity was too large (re-centre: mu is not driven further); else
 *              MPCQP_IPM_SIGMA when the last alpha >= MPCQP_IPM_ALPHA_SHORT (also in iteration 1), else MPCQP_IPM_SIGMA_SHORT.
 *   target     s = max(sigma mu, MPCQP_IPM_TARGET * comp_tol): the loop never drives mu below what the stop test asks for (rounding, below).
 *   iteration  with that s and r = lambda / t per side: a lower side of column c adds r to H_k[c][c] and -((s / t + lambda) + r l) to
 *              q_k[c]; an upper side adds r and +((s / t + lambda) - r u); both sides of a column are summed before they are added.  The
 *              backward and the forward pass of the entry above on this data (reg and the pins of frame 0 as there) give w+.  dw = w+ - w;
 *              lower side dt = dw + ((w - l) - t), upper side dt = ((u - w) - t) - dw; dlambda = (s / t - lambda) - r dt.
 *              alpha = min(1, MPCQP_IPM_FRAC * min over all t and lambda with a negative direction of -v / dv); w, t, lambda += alpha times
 *              their directions.  A failed pivot, or an alpha that is not in (0, 1] (a NaN), rejects: direct[b] = 0 (with positive pivots in
 *              iteration 0 this can only be rounding).
 *   candidate  the new w is inside, max lambda t <= comp_tol and mu <= comp_tol (a NaN fails).  Then the adjoint pass of the entry above runs
 *              at w with y_j = lambda_U - lambda_L (the sign convention of mpcqp_get) on the barriered rows: val = [A_k B_k]' lam_k -
 *              (H_k w_k + q_k) - y; the state columns give the dynamics multipliers lam_{k-1}, frame 0's pinned rows close their own columns,
 *              and stat = max |val - reg w| over the barriered INPUT columns is what the iterate leaves of the stationarity condition of the QP the
 *              passes solve, reg on the free inputs' diagonal included (the gain closes
 *              these columns exactly only after a full step).  Path and link rows are tested at w: a violation rejects, direct[b] = 0.
 *              stat <= stat_tol: direct[b] = 1, w, y, z written.  Else the loop goes on (sigma = 1).
 *   the end    after `iters` iterations an open instance is rejected: direct[b] = 0, iters_used[b] = iters.
 *   iters_used, res   the last iteration the instance ran; res[3 b ..] = the largest violation of a barriered row, max lambda t (0 in iteration
 *              0) and stat (NaN when the exit point was not a candidate), all at the exit point -- for accepted and rejected instances alike.  An
 *              ineligible (-1), failed (-2) or frozen instance writes neither; a rejected instance writes nothing else.
 * What accepted means: unlike the two entries above, an accepted point of an iteration >= 1 is an APPROXIMATE KKT point of the QP: primal
 * feasible within feas_tol (exactly on the dynamics and the pins), multipliers of the right sign, lambda t <= comp_tol on every side, stationary
 * within stat_tol.  Iteration 0's positive pivots make the objective strictly convex on the set the pins and the dynamics leave, so the QP has one
 * KKT point: the accepted point is close to the minimiser and cannot be near a different stationary point.  How close depends on comp_tol, on
 * the smallest active multiplier and on the conditioning (DESIGN 6.32 has measured distances).  Rounding: lambda carries an error of about
 * eps * (lambda / t) * |w|, and t = mu / lambda on an active row: stat cannot be driven below about 1e-16 lambda^2 / mu, which is why the target
 * stops at MPCQP_IPM_TARGET * comp_tol and why a comp_tol below 1e-8 is out of reach in double precision (DESIGN 6.32 has the measurements).
 * stage_direct_ipm_kernel uses the size classes, lane groups and tiles of stage_direct_kernel; its workspace (the handle's, grown with the batch:
 * batch N (nu (nx + 1) + 7 f) doubles) holds the gains, w, dw, val, t_L, t_U, lambda_L, lambda_U.  The loop over the iterations is uniform over
 * the block; one writer per element, no atomics: bitwise repeatable, independent of the batch size and of the instance's position.  No state is
 * kept between calls.  MPCQP_ERR_ARG and MPCQP_ERR_LIMIT as above, MPCQP_ERR_ARG also for iters outside 1 .. MPCQP_IPM_MAX_ITERS and a negative
 * (or NaN) comp_tol or stat_tol. */
#define MPCQP_IPM_MAX_ITERS 50
#define MPCQP_IPM_T0 0.1
#define MPCQP_IPM_MU0 1.0
#define MPCQP_IPM_FRAC 0.995
#define MPCQP_IPM_SIGMA 0.1
#define MPCQP_IPM_SIGMA_SHORT 0.5
#define MPCQP_IPM_ALPHA_SHORT 0.5
#define MPCQP_IPM_TARGET 0.5
typedef struct mpcqp_stage_riccati_solve_ipm_args {
  const double *P, *q, *A, *l, *u;   /* [batch * nnzP | n | nnzA | m | m], the local system          */
  double feas_tol, reg;
  const int *frozen;            /* [batch], optional: nonzero = neither read nor written       */
  double *w;                    /* [batch * n], required                                       */
  double *y;                    /* [batch * m], required                                       */
  double *z;                    /* [batch * m], optional                                       */
  int *direct;                  /* [batch], required: 1 accepted, 0 rejected, -1 ineligible, -2 a pivot failed in iteration 0 */
  int iters;                    /* 1 .. MPCQP_IPM_MAX_ITERS: the iterations after iteration 0  */
  double comp_tol, stat_tol;    /* >= 0                                                        */
  int *iters_used;              /* [batch], optional                                           */
  double *res;                  /* [batch * 3], optional                                       */
} mpcqp_stage_riccati_solve_ipm_args;
int mpcqp_stage_riccati_solve_ipm(mpcqp_stage *s, int batch, const mpcqp_stage_riccati_solve_ipm_args *a, void *stream);
/* The feedback law at one frame, one thread per (instance, input): with row(v, stride) = v + b * stride,
 *   acc = acc_j K[b][k][i][j] * (s[j] - s_nom[j])     (each product and each sum rounded, no fused multiply-add: bitwise the host statement)
 *   u   = clip(u_nom[i] + acc), clip the two selects of mpcqp_stage_rollout against lo[i] / hi[i] (the identity without the pair)
 *   x_out[b * nvar + nx + i] = u, and the same entry of lbx[b] and ubx[b] when that pair is given -- the corrected input is what the next tick
 *   sees pinned;  du[b * nu + i] = u - u_nom[i] when given.
 * s, s_nom, u_nom, lo, hi are pointers with row strides (in doubles), so a caller points them into its trajectory buffers and bound arrays without
 * copies; they may lie inside x_out, lbx, ubx as long as no entry that is written (nx .. f-1 of each row) is also read through another name.
 * k is one frame for the launch.  An instance whose sweep failed at a frame >= k has a zero gain there and gets clip(u_nom).  Nothing is
 * allocated: a captured graph replays it.  MPCQP_ERR_ARG for a null s, a, K, s, s_nom, u_nom or x_out, only one of lo / hi or of lbx / ubx,
 * batch < 1, k outside 0 .. N-1. */
typedef struct mpcqp_stage_feedback_args {
  const double *K;              /* [batch * N * nu * nx], what mpcqp_stage_riccati wrote        */
  int k;                        /* the frame whose gain is applied                             */
  const double *s, *s_nom, *u_nom;                 /* rows of nx, nx, nu doubles               */
  long s_stride, s_nom_stride, u_nom_stride;       /* distance between two instances' rows     */
  const double *lo, *hi;        /* rows of nu doubles, optional pair                           */
  long lo_stride, hi_stride;
  double *x_out;                /* [batch * nvar]: entries nx .. f-1 of each row are written    */
  double *lbx, *ubx;            /* [batch * nvar], optional pair: the same entries              */
  double *du;                   /* [batch * nu], optional                                      */
} mpcqp_stage_feedback_args;
int mpcqp_stage_feedback(mpcqp_stage *s, int batch, const mpcqp_stage_feedback_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Structured stage form: the same QP, given by its stage blocks instead of CSC value arrays.
 *
 * The reference only ever produces OCP-structured QPs: the decision vector is the stage-interleaved list of frames
 * [s_k; u_k] (src/OCP_config/OCPConfig.cpp:29-46,102) behind a parameter block p, and the local QP has w = [p; frames] and rows
 * [p; frames; g] (src/sqp_solver/SQPOptimizationSolver.cpp:47-77).  A caller that has the blocks -- an LTV / linearised MPC that
 * never went through CasADi -- would have to scatter them into CSC arrays itself to call mpcqp_update.  Here it names the stage
 * dimensions once and hands over, per instance (instance-major, dense, row-major):
 *     H   [N][f][f]       Hessian block of frame k, f = nx + nu (symmetric; both triangles are read as given)
 *     Hp  [N][np][f]      P[p, frame_k]  (its transpose fills P[frame_k, p]);   Hpp [np][np]  P[p, p]      (both NULL when np = 0)
 *     AB  [N-1][nx][f]    [A_k B_k] of  s_{k+1} = A_k s_k + B_k u_k + c_k : dynamics row block k reads
 *                         lg_k <= s_{k+1} - A_k s_k - B_k u_k <= ug_k  (an equality when lg_k = ug_k = c_k), the sign convention of the
 *                         reference's rows (+1 on s_{k+1}, -dF/d[s_k; u_k]; compare mpcqp_stage_eval above)
 *     q [n], l [m], u [m] as in mpcqp_update: n = np + N f in the order [p; frames], m = n + (N - 1) nx in the order
 *                         [p; frames; dynamics] (the identity rows carry the box bounds; the reference pins p with l = u)
 * The QP is the one mpcqp_create / mpcqp_update would get for the CSC pattern mpcqp_stageqp_pattern returns -- for np = nx and dense
 * masks exactly mpcqp_stage_pattern's -- and it runs on an ordinary handle on that pattern: blocks and CSC arrays holding the same
 * numbers give bitwise the same x, y, z, status and iteration counts (tests/test_gpu_stageqp.py).  One gather kernel per update writes
 * the CSC value arrays (algorithmic bytes: blocks in, nnz(P) + nnz(A) values out); the ADMM kernels are not aware of this form.
 * Optional masks keep structural zeros out of the pattern (a diagonal tracking cost, a sparse Jacobian): entries masked out are not
 * read.  np = 0: a plain LQ-structured QP without the reference's parameter block. */
typedef struct mpcqp_stageqp_dims {
  int N;                            /* frames, >= 2 */
  int nx, nu;                       /* frame k = [s_k (nx); u_k (nu)] */
  int np;                           /* leading parameter block (0 = none) */
  const unsigned char *cost_mask;   /* optional [(f + np)^2] row-major over the local variables [s; u; p]: which entries of H_k, Hp_k, Hpp exist
                                       (symmetric, diagonal set; the same for every frame); NULL = dense blocks */
  const unsigned char *dyn_mask;    /* optional [nx * f] row-major: which entries of [A_k B_k] exist; NULL = dense */
} mpcqp_stageqp_dims;

typedef struct mpcqp_stageqp mpcqp_stageqp;

/* CSC pattern of the stage form (host only; no GPU needed): sizes4 = {n, m, nnz(P), nnz(A)}; any of the arrays may be NULL (query the
 * sizes first).  P has both triangles, rows ascending inside a column -- what CasADi hands CuCaQP::setHessianMatrix. */
int mpcqp_stageqp_pattern(const mpcqp_stageqp_dims *d, int *sizes4, int *P_colptr, int *P_rowidx, int *A_colptr, int *A_rowidx);
/* mpcqp_create on that pattern plus the maps and value arrays of the gather kernel */
int mpcqp_stageqp_create(const mpcqp_stageqp_dims *d, int batch, const mpcqp_settings *settings, mpcqp_stageqp **out);
/* the ordinary handle underneath: mpcqp_solve / _get / _warm_start / _set_rho / _keep_workspace / _update_vectors / _plan_info apply to it
 * (x, y, z come back in the orders given above).  Owned by the mpcqp_stageqp: do not destroy it. */
mpcqp_handle *mpcqp_stageqp_handle(mpcqp_stageqp *s);
/* mpcqp_update in blocks.  mem = MPCQP_MEM_DEVICE: the gather kernel is queued on `stream` -- the stream of the mpcqp_solve calls on this
 * handle -- and q, l, u are borrowed until that solve has completed, like in mpcqp_update; the block arrays are free once the kernel
 * has run.  mem = MPCQP_MEM_HOST: everything is copied before the call returns. */
int mpcqp_stageqp_update(mpcqp_stageqp *s, const double *H, const double *Hp, const double *Hpp, const double *AB,
                         const double *q, const double *l, const double *u, int mem, void *stream);
void mpcqp_stageqp_destroy(mpcqp_stageqp *s);

#ifdef __cplusplus
}
#endif
#endif
