/*
 * ldsr_hip.h -- C ABI of libldsr_hip.so, the MI355X (gfx950) engine for ldsr's
 * EM/Kalman restart path.  Plain pointers and sizes only; no torch / Rcpp types.
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *
 *   ldsr_em_restart_grid     LDS_EM_restart (R/LDS_reconstruction.R:42-62) for one series, and
 *                            the fold loop of cvLDS (R/LDS_reconstruction.R:373-375 ->
 *                            one_lds_cv :270-285) for several: the foreach fan-out :46, the
 *                            selection :50-58 and the winner's model {theta, fit, liks, lik} in
 *                            ONE call -- only the winners' fit / liks cross PCIe
 *   ldsr_em_restart_groups   the ensemble loop R/LDS_reconstruction.R:242-246 (members differ in
 *                            p, q: tests/testthat/test-ensemble.R:4-5): one grid per member,
 *                            run concurrently
 *   ldsr_em_batch            the bare fan-out  foreach(theta0 = init) %dopar% LDS_EM(...)
 *                            of R/LDS_reconstruction.R:46, i.e. n_cells calls of
 *                            _ldsr_LDS_EM (src/RcppExports.cpp:40-53 -> src/EM.cpp:245-280),
 *                            batched over restarts and over series / CV folds
 *   ldsr_em_batch_multi      same, sharded over several GPUs by host threads (no collective)
 *   ldsr_em_batch_device     same, operands already resident in HBM (bench + torch callers)
 *   ldsr_smooth_batch        _ldsr_Kalman_smoother (src/RcppExports.cpp:11-24 ->
 *                            src/EM.cpp:22-131), one E-step per (series, theta) cell;
 *                            also yields the winner's `fit` list of LDS_EM (src/EM.cpp:276-279)
 *   ldsr_mstep_batch         _ldsr_Mstep (src/RcppExports.cpp:26-38 -> src/EM.cpp:139-229)
 *   ldsr_propagate_batch     _ldsr_propagate (src/RcppExports.cpp:56-69 -> src/EM.cpp:295-356)
 *   ldsr_penalized_lik_batch penalized_likelihood of R/LDS_GA.R:28-44 for a whole GA population
 *   ldsr_ga_batch            LDS_GA (R/LDS_GA.R:54-82): the whole island GA -- fitness, selection,
 *                            crossover, mutation, elitism, migration, the stop rule -- for one series
 *                            or the folds of cvLDS(method = "GA") in ONE call; the population never
 *                            leaves HBM.  An island GA of GA::gaisl's family by this project's own
 *                            specification, NOT gaisl's random stream
 *   ldsr_bfgs_batch          LDS_BFGS (R/LDS_GA.R:155-184) and the BFGS / BFGS_smooth arms of call_method
 *                            (R/LDS_reconstruction.R:70-86): every restart's whole bound-constrained
 *                            L-BFGS run over ssqTrain inside one kernel launch, the selection of
 *                            R/LDS_GA.R:174 and the winner's propagate / Kalman_smoother fit in ONE call.
 *                            This project's own L-BFGS, NOT the iterates of the
 *                            L-BFGS-B code behind stats::optim
 *   ldsr_bfgs_update_batch   LDS_BFGS_with_update (R/LDS_GA.R:90-127): the same L-BFGS on -penalized_likelihood
 *   ldsr_pl_grad_batch       penalized_likelihood (R/LDS_GA.R:28-44) and its exact gradient for a batch of thetas
 *   ldsr_ssq_grad_batch      ssqTrain (R/LDS_GA.R:143-147) and its exact gradient for a batch of thetas
 *   ldsr_select_restart      the argmax-with-C>0 rule of R/LDS_reconstruction.R:50-58
 *   ldsr_simulate_batch      LDS_rep / one_LDS_rep (R/stochastics.R:18-63): num_reps stochastic
 *                            replicates of each of n_models thetas in one launch; with the uniforms
 *                            R would draw (ldsr_simulate_draw_count) the result is set.seed(k);
 *                            LDS_rep(...) draw for draw
 *   ldsr_pcr_batch           the benchmark model R/PCR.R: every (member, fold) least-squares fit of cvPCR /
 *                            PCR_ensemble_selection (one_pcr_cv :101-107) and PCR_reconstruction's lm + predict
 *   ldsr_filter_batch        replaces nothing the reference exports: it returns what Kalman_smoother computes on its
 *                            way and discards (src/EM.cpp:43-90,115-120: Xp, Vp, Yp, Xu, Vu, delta, Sigma), the
 *                            per-step likelihood terms and the statistics of the standardised innovations
 *
 * Data conventions (identical to the bytes R hands to .Call):
 *   y      [n_series][T]        double, NaN / NA_real_ = missing
 *   u      [n_series][T][p]     double; an R p x T matrix is column-major, i.e. exactly
 *                               this time-major layout (u[t*p + k]).  NULL = input absent
 *                               (the reference's 1x1 `matrix(0)` sentinel, src/EM.cpp:71)
 *   v      [n_series][T][q]     likewise (src/EM.cpp:77)
 *   shared_uv != 0              u and v hold ONE series ([T][p], [T][q]) shared by every
 *                               y series (cvLDS folds: same inputs, different NA masks,
 *                               R/LDS_reconstruction.R:274)
 *   theta  [n_cells][6+p+q]     packed  A, B[p], C, D[q], Q, R, mu1, V1  (list order of
 *                               src/EM.cpp:221-228).  With u (v) absent p (q) is 1, the
 *                               B (D) slot is ignored on input and returned as 0, as
 *                               B.zeros(1, p) at src/EM.cpp:186 (:154)
 *   cell_offsets [n_series+1]   HOST array: cells [cell_offsets[s], cell_offsets[s+1]) are
 *                               the restarts of series s
 *
 * Limits of this build: 1 <= p, q <= 16 (larger returns LDSR_EUNSUPPORTED; the scan kernel
 * covers p, q <= 8 = every BASELINE config and the reference's tests, wider inputs run on the
 * serial kernel), T >= 2, niter >= 2 (the reference indexes lik[1]
 * unconditionally, src/EM.cpp:256).
 *
 * Every function returns LDSR_OK (0) or an error code; ldsr_last_error() gives the
 * message of the calling thread's last failure.
 *
 * Ownership: the library never keeps a pointer of the caller after a call returns.  The
 * host-pointer entry points cache their device buffers, pinned staging buffers and one stream
 * per concurrent caller and device (grow-only arenas; a call on a busy device gets its own), so
 * repeated calls do no hipMalloc / hipFree; ldsr_shutdown() frees everything.  All entry
 * points may be called from several threads.
 */
#ifndef LDSR_HIP_H
#define LDSR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDSR_OK 0
#define LDSR_EINVAL 1        /* bad argument */
#define LDSR_EUNSUPPORTED 2  /* p or q above the compiled limit */
#define LDSR_EHIP 3          /* a HIP runtime call failed (no device, OOM, launch error) */
#define LDSR_EINTERRUPTED 4  /* the interrupt callback asked to stop; outputs are incomplete */
#define LDSR_EINTERNAL 5     /* the library's own pre-launch check refused a launch; nothing ran */

/* per-cell status words */
#define LDSR_CELL_OK 0
#define LDSR_CELL_NONFINITE 1 /* final lik is NaN/Inf (tolerated by the reference's selection, na.rm) */
#define LDSR_CELL_SINGULAR 2  /* Svv or Tuu of the series is singular: arma::inv would throw */
#define LDSR_CELL_INTERRUPTED 3 /* stopped early by the interrupt callback (theta = last E-step's) */

/* algorithm selector */
#define LDSR_ALGO_AUTO 0
#define LDSR_ALGO_SERIAL 1 /* one thread per cell, sequential in time (any T) */
#define LDSR_ALGO_SCAN 2   /* one to four wavefronts per cell, parallel-in-time scans (T <= 8192,
                              p, q <= 8); AUTO picks it whenever it applies and PAIR does not */
#define LDSR_ALGO_PAIR 3   /* the same scans with TWO cells per wavefront (one per 32-lane half):
                              65 <= T <= 1024, p, q <= 4, narrower ranges of T for the wider inputs
                              (ldsr_em_plan tells); AUTO's first choice where it applies -- with
                              tol > 0 only for fully observed series.  Its LEAD form
                              (a closed-form all-missing lead, tails <= 512 steps: ldsr_em_plan_lead)
                              also exists for padded p or q = 8 */
#define LDSR_ALGO_QUAD 4   /* FOUR cells per wavefront (one per 16-lane DPP row): 65 <= T <= 512,
                              p, q <= 4; AUTO's first choice there for launches that fill the device */

const char *ldsr_last_error(void);
const char *ldsr_version(void);
/* first 16 hex digits of the SHA-256 over the library's sources (every .hip, .h and .inc file of
 * ldsr_amd/csrc, its Makefile and this header) it was built from: a caller that has the tree can tell a
 * stale binary (ldsr_amd/_lib.py refuses one) */
const char *ldsr_source_hash(void);
int ldsr_device_count(void);
void ldsr_shutdown(void);

/* LDS_EM_restart for a whole grid of series / CV folds in one call: runs every (series,
 * restart) cell (cells are cut into contiguous slices over devices[0..n_devices), host threads,
 * no collective), picks each series' winner by the reference's rule (highest lik among
 * restarts with C > 0 if any, NaN ignored, first index on ties), and returns per series the
 * winner's model exactly as LDS_EM returns it (src/EM.cpp:276-279):
 *   winner   [n_series]          global cell index, or -1 if nothing is selectable
 *   theta_w  [n_series][6+p+q]   lik_w [n_series]   n_iter_w [n_series]
 *   liks_w   [n_series][niter]   the winner's likelihood trace, NaN beyond n_iter_w[s]
 *   X, Y, V, J [n_series][T]     the winner's fit (Kalman_smoother at theta_w, stdlik = TRUE)
 * Rows of a series without a winner are NaN.  liks_w, X, Y, V, J may each be NULL.
 * The per-cell results (theta_all [n_cells][6+p+q], lik_all, n_iter_all, status_all) are
 * optional: pass NULL to leave them on the device side of PCIe. */
int ldsr_em_restart_grid(int n_devices, const int *devices, int n_series, int T, int p, int q,
                         const double *y, const double *u, const double *v, int shared_uv,
                         const int *cell_offsets, const double *theta0, int niter, double tol,
                         int algo, double *theta_all, double *lik_all, int *n_iter_all,
                         int *status_all, int *winner, double *theta_w, double *lik_w,
                         int *n_iter_w, double *liks_w, double *X, double *Y, double *V,
                         double *J);

/* Heterogeneous ensembles (R/LDS_reconstruction.R:242-246: list members differ in p and q):
 * one ldsr_em_restart_grid per group, groups run concurrently (one host thread and one stream
 * each; group g starts on devices[g % n_devices]).  Fields are the arguments of
 * ldsr_em_restart_grid; rc receives each group's return code. */
typedef struct ldsr_group {
    int n_series, T, p, q, shared_uv;
    const double *y, *u, *v;
    const int *cell_offsets;
    const double *theta0;
    double *theta_all, *lik_all;
    int *n_iter_all, *status_all;
    int *winner;
    double *theta_w, *lik_w;
    int *n_iter_w;
    double *liks_w, *X, *Y, *V, *J;
    int rc;
} ldsr_group;
int ldsr_em_restart_groups(int n_devices, const int *devices, int n_groups, ldsr_group *groups,
                           int niter, double tol, int algo);

/* Batched LDS_EM.  Host pointers; copies in, runs on `device`, copies out.
 * liks may be NULL; otherwise [n_cells][niter], entries beyond n_iter[c] are NaN. */
int ldsr_em_batch(int device, int n_series, int T, int p, int q, const double *y,
                  const double *u, const double *v, int shared_uv, const int *cell_offsets,
                  const double *theta0, int niter, double tol, int algo,
                  double *theta, double *lik, int *n_iter, int *status, double *liks);

/* Same over several GPUs of one node: the cell grid is cut into n_devices contiguous slices,
 * one host thread per listed device, no collective (restarts never communicate,
 * R/LDS_reconstruction.R:46).  devices[] may repeat an id. */
int ldsr_em_batch_multi(int n_devices, const int *devices, int n_series, int T, int p, int q,
                        const double *y, const double *u, const double *v, int shared_uv,
                        const int *cell_offsets, const double *theta0, int niter, double tol,
                        int algo, double *theta, double *lik, int *n_iter, int *status,
                        double *liks);

/* Same with DEVICE pointers (cell_offsets stays a host array and may be reused or freed as
 * soon as the call returns).  Asynchronous on `stream` (a hipStream_t passed as void*; NULL =
 * default stream): the call only enqueues work -- the block table travels through a pinned
 * staging ring owned by the library -- and never waits for the device.  workspace: device
 * buffer of at least ldsr_em_workspace_bytes(...) bytes, 256-byte aligned; it holds the
 * prepared series, the block table and the work-queue heads of THIS call, so calls that may
 * overlap in time (different streams) need separate workspaces. */
size_t ldsr_em_workspace_bytes(int n_series, int T, int p, int q, int n_cells, int algo);
int ldsr_em_batch_device(int device, void *stream, int n_series, int T, int p, int q,
                         const double *d_y, const double *d_u, const double *d_v,
                         int shared_uv, const int *cell_offsets, const double *d_theta0,
                         int niter, double tol, int algo, double *d_theta, double *d_lik,
                         int *d_n_iter, int *d_status, double *d_liks, void *d_workspace,
                         size_t workspace_bytes);

/* Which kernel a call with these arguments launches: writes its name as rocprofv3 prints it
 * (e.g. "em_pair_kernel<1, 2, 32, 32, false, false>") into buf and returns the resolved algorithm
 * (LDSR_ALGO_SERIAL / LDSR_ALGO_SCAN / LDSR_ALGO_PAIR / LDSR_ALGO_QUAD), or a negative value for
 * unsupported arguments.  With LDSR_ALGO_AUTO it assumes a launch large enough to fill the device
 * (smaller launches keep the scan kernel, whose smaller workgroups spread over more CUs; how many cells
 * fill the device depends on the shape, tol and the lead -- ldsr_last_em_kernel tells what a launch
 * ran), and with tol > 0 it reports what ldsr_em_batch_device runs (the scan kernel, except for short
 * series); the host-pointer entries additionally take the pair family when every series is fully
 * observed (ldsr_em_plan_lead with lead_steps = -1). */
int ldsr_em_plan(int T, int p, int q, int niter, double tol, int algo, char *buf, size_t len);

/* The same two with one more piece of knowledge about the data: the first lead_steps time steps of
 * EVERY series are missing (paleo-type series: centuries before the instrumental period; 0 = none
 * or unknown).  LDSR_ALGO_AUTO then handles that lead in closed form and sweeps only the tail
 * (em_pair_impl.h, LEAD).  lead_steps = -1 says the opposite: every y_t of every series is
 * observed -- AUTO then keeps the pair / quad kernels with tol > 0 as the host-pointer entries do
 * for such series (a wrong claim costs speed, not correctness: the kernels look at the mask
 * themselves).  The host-pointer entries find both facts in y. */
int ldsr_em_batch_device_lead(int device, void *stream, int n_series, int T, int p, int q,
                              const double *d_y, const double *d_u, const double *d_v,
                              int shared_uv, const int *cell_offsets, const double *d_theta0,
                              int niter, double tol, int algo, double *d_theta, double *d_lik,
                              int *d_n_iter, int *d_status, double *d_liks, void *d_workspace,
                              size_t workspace_bytes, int lead_steps);
int ldsr_em_plan_lead(int T, int p, int q, int niter, double tol, int algo, int lead_steps,
                      char *buf, size_t len);
/* The kernel one Kalman_smoother pass of this shape runs: LDSR_ALGO_SCAN and the name of the scan
 * kernel's FIT form, or LDSR_ALGO_SERIAL (empty name) beyond its shapes; -1 for bad arguments. */
int ldsr_smooth_plan(int T, int p, int q, char *buf, size_t len);
/* Names (as rocprofv3 prints them, one per line) of every instantiation of the parallel-in-time kernel
 * families compiled into this library; returns the buffer length needed.  The library is built to hold
 * exactly what the plans above can return (tests/test_abi_and_host.py). */
size_t ldsr_kernel_inventory(char *buf, size_t len);
/* Name of the EM kernel of the most recent EM launch on `device` (what AUTO actually chose for that
 * launch's size and data); -1 if there was none. */
int ldsr_last_em_kernel(int device, char *buf, size_t len);

/* Batched Kalman_smoother: one E-step for each cell's theta.  Host pointers.
 * X, Y, V, J: [n_cells][T] (any may be NULL); lik: [n_cells].  stdlik as src/EM.cpp:124.
 * A series whose Svv / Tuu is singular (an EM call flags it LDSR_CELL_SINGULAR) has a smoother all the same:
 * this entry and ldsr_penalized_lik_batch run its cells on the serial kernel. */
int ldsr_smooth_batch(int device, int n_series, int T, int p, int q, const double *y,
                      const double *u, const double *v, int shared_uv,
                      const int *cell_offsets, const double *theta, int stdlik, double *X,
                      double *Y, double *V, double *J, double *lik);

/* Batched Mstep: fit (X, V, J: [n_cells][T]) -> theta [n_cells][6+p+q].  Host pointers. */
int ldsr_mstep_batch(int device, int n_series, int T, int p, int q, const double *y,
                     const double *u, const double *v, int shared_uv,
                     const int *cell_offsets, const double *X, const double *V,
                     const double *J, double *theta, int *status);

/* Batched propagate (no measurement update).  X, Y, V: [n_cells][T]; lik [n_cells]. */
int ldsr_propagate_batch(int device, int n_series, int T, int p, int q, const double *y,
                         const double *u, const double *v, int shared_uv,
                         const int *cell_offsets, const double *theta, int stdlik, double *X,
                         double *Y, double *V, double *lik);

/* Batched penalized_likelihood (R/LDS_GA.R:28-44, the GA / BFGS fitness): for every theta,
 * Kalman_smoother(..., stdlik = FALSE)$lik - lambda * sum_t (Xs[t+1] - A Xs[t] - B u[t])^2.
 * pl: [n_cells].  Only the scalar leaves the device. */
int ldsr_penalized_lik_batch(int device, int n_series, int T, int p, int q, const double *y,
                             const double *u, const double *v, int shared_uv,
                             const int *cell_offsets, const double *theta, double lambda,
                             double *pl);

/* LDS_GA (R/LDS_GA.R:54-82): an island genetic algorithm that maximises penalized_likelihood over
 * packed thetas inside the box [lb, ub], entirely on the device.  The algorithm -- operators, stop rule,
 * the layout of the counter-mode random streams -- is specified in INTEGRATION.md ("The island GA");
 * it is of the family of GA::gaisl, which the reference calls, and does not reproduce gaisl's stream.
 * n_series independent problems (the folds of cvLDS: shared_uv) run side by side, each with num_islands
 * islands of pop_per_island individuals (2 .. LDSR_GA_MAX_POP); problem s draws under seed + s, so it
 * evolves exactly as problem 0 of a one-problem call with that seed, whatever else shares the call.
 *   lb, ub       [6+p+q] finite, lb <= ub           lambda   the penalty weight of R/LDS_GA.R:41
 *   maxiter      generations at most (>= 1)         run      stop after this many generations without
 *                                                            a new best (>= 1; the reference: 100)
 *   suggestions  [n_series][n_suggestions][6+p+q] or NULL: the first individuals of island 0, clipped
 *                to the box (n_suggestions <= pop_per_island)
 *   theta_best   [n_series][6+p+q]   pl_best [n_series] (-inf, theta NaN: no finite fitness ever)
 *   n_gen        [n_series] generations evaluated
 *   trace        [n_series][maxiter] best so far after each generation, NaN beyond n_gen; may be NULL
 *   population   [n_series][num_islands][pop_per_island][6+p+q], fitness [n_series][num_islands]
 *                [pop_per_island]: the LAST EVALUATED generation (index n_gen - 1) and its fitness;
 *                each may be NULL
 * Host pointers.  The series are uploaded and prepared once; a generation is two launches (the
 * smoother's scalar-only pass, then breeding), enqueued LDSR_GA_CHUNK generations at a time with one
 * small read-back in between; the interrupt callback is polled there (LDSR_EINTERRUPTED).  One problem of
 * the reference's default size is 400 cells and cannot fill the device: batch problems into one call. */
#define LDSR_GA_MAX_POP 1024
#define LDSR_GA_PCROSSOVER 0.8          /* probability that a selected pair is crossed */
#define LDSR_GA_PMUTATION 0.1           /* probability that a child has one gene redrawn */
#define LDSR_GA_ELITE_PCT 5             /* elites: max(1, (5 n + 50) / 100), 5 % rounded half up */
#define LDSR_GA_MIGRATION_PCT 10        /* migrants: max(1, 10 n / 100), 10 % rounded down */
#define LDSR_GA_MIGRATION_INTERVAL 10   /* migrate after every 10th generation */
#define LDSR_GA_CHUNK 32                /* generations enqueued between two looks at the stop flags */
int ldsr_ga_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                  const double *v, int shared_uv, const double *lb, const double *ub, double lambda,
                  int num_islands, int pop_per_island, int maxiter, int run, unsigned long long seed,
                  const double *suggestions, int n_suggestions, double *theta_best, double *pl_best,
                  int *n_gen, double *trace, double *population, double *fitness);

/* ssqTrain of R/LDS_GA.R:143-147 and its gradient: for every theta, with propagate's recursion
 *   x_1 = mu1, x_{t+1} = A x_t + B u_t, Y_t = C x_t + D v_t  (src/EM.cpp:295-356, no measurement update),
 *   ssq = sum over the observed y_t of (y_t - Y_t)^2   (NaN and +-Inf in y: missing),
 * and grad = d ssq / d theta by the adjoint recursion: exact, one forward and one
 * backward pass over the series.  The Q, R, V1 slots and the slots of an absent input have gradient 0.
 *   ssq [n_cells]   grad [n_cells][6+p+q], may be NULL (values only).  Host pointers. */
int ldsr_ssq_grad_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                        const double *v, int shared_uv, const int *cell_offsets, const double *theta,
                        double *ssq, double *grad);

/* LDS_BFGS (R/LDS_GA.R:155-184): a bound-constrained L-BFGS from every start point par0[c] that minimises
 * ssq over the box [lb, ub], one persistent wavefront per (series, restart) cell: iterates, gradients and
 * the curvature pairs never leave the wave, the whole run of a cell is one kernel launch.  The optimiser
 * -- active set, two-loop direction, projected backtracking, stop rules -- is specified in INTEGRATION.md
 * ("The bound-constrained L-BFGS"); it is NOT the L-BFGS-B code that stats::optim calls and does not
 * reproduce its iterates.
 *   par0    [n_cells][6+p+q] start points (projected into the box)     lb, ub [6+p+q] finite, lb <= ub
 *   maxit   iterations at most (>= 1; optim: 100)      lmm   curvature pairs kept, 1 .. 8 (optim: 5)
 *   factr   stop when (f_k - f_k+1) / max(|f_k|, |f_k+1|, 1) <= factr * 2^-52 (>= 0; optim: 1e7)
 *   pgtol   stop when the projected gradient's largest entry is <= pgtol (>= 0; optim: 0)
 *   select_max != 0: each series' winner is the restart with the LARGEST minimised value, the reference's
 *           literal which.max(optim.vals) (R/LDS_GA.R:174); 0: the smallest.  NaN ignored, first index on
 *           ties, -1 when no restart of the series has a finite value
 *   fit_mode 0: the winner's fit is propagate(theta_w) (method = "BFGS"; J untouched), 1: Kalman_smoother
 *           (theta_w) (method = "BFGS_smooth"); lik_w is that fit's standardised likelihood
 *   par_all [n_cells][6+p+q], value_all, n_iter_all, n_eval_all (forward passes), status_all [n_cells]:
 *           each may be NULL
 *   winner [n_series] global cell index, theta_w [n_series][6+p+q], value_w [n_series]: required;
 *   lik_w [n_series], X, Y, V, J [n_series][T]: each may be NULL.  Rows without a winner are NaN.
 * Host pointers; only the winners' rows cross PCIe.  The interrupt callback is polled while the call waits,
 * and the kernel looks at its flag every 8 iterations (LDSR_EINTERRUPTED).  One problem of the reference's
 * default size is 100 cells and cannot fill the device: batch the folds of cvLDS into one call. */
#define LDSR_BFGS_CONVERGED 0    /* a stop rule fired */
#define LDSR_BFGS_MAXIT 1        /* maxit iterations ran */
#define LDSR_BFGS_LINESEARCH 2   /* no acceptable step in 20 halvings: the cell keeps its best point */
#define LDSR_BFGS_NONFINITE 3    /* f is not finite at the start: value NaN, par = par0 */
#define LDSR_BFGS_INTERRUPTED 4  /* stopped by the interrupt callback (the call returns LDSR_EINTERRUPTED) */
int ldsr_bfgs_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                    const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                    const double *lb, const double *ub, int maxit, int lmm, double factr, double pgtol,
                    int select_max, int fit_mode, double *par_all, double *value_all, int *n_iter_all,
                    int *n_eval_all, int *status_all, int *winner, double *theta_w, double *value_w,
                    double *lik_w, double *X, double *Y, double *V, double *J);

/* penalized_likelihood (R/LDS_GA.R:28-44) and its gradient: pl = lik - lambda ssq with lik the likelihood of
 * Kalman_smoother (stdlik = FALSE) and ssq = sum (Xs_{t+1} - A Xs_t - B u_t)^2 over the smoothed means; grad =
 * d pl / d theta in all of A, B, C, D, Q, R, mu1, V1 by reverse mode over the smoother:
 * exact, five passes over the series, each a scan over the 64 lanes of the cell's wavefront.  pl is bit-identical
 * with and without grad.  The slots of an absent input have gradient 0; NaN and +-Inf in y: missing.
 *   pl [n_cells]   grad [n_cells][6+p+q], may be NULL (values only).  Host pointers; lambda finite.
 * Before the launch the bytes the kernel will touch behind every device pointer are checked against the call's
 * block; a mismatch returns LDSR_EINTERNAL with the pointer's name in ldsr_last_error() and launches nothing. */
int ldsr_pl_grad_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                       const double *v, int shared_uv, const int *cell_offsets, const double *theta,
                       double lambda, double *pl, double *grad);

/* LDS_BFGS_with_update (R/LDS_GA.R:90-127): ldsr_bfgs_batch's optimiser, arguments and outputs with the
 * objective f = -pl at the given lambda (finite).  value_all / value_w are the minimised -pl; a start with some
 * S_t <= 0 is LDSR_BFGS_NONFINITE.  select_max != 0 is the reference's literal which.max(optim.vals)
 * (R/LDS_GA.R:116), the LARGEST minimised value.  There is no fit_mode: the winners' fit is always
 * Kalman_smoother(theta_w) with the standardised likelihood, J included.  The pre-launch check of
 * ldsr_pl_grad_batch applies. */
int ldsr_bfgs_update_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                           const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                           const double *lb, const double *ub, double lambda, int maxit, int lmm, double factr,
                           double pgtol, int select_max, double *par_all, double *value_all, int *n_iter_all,
                           int *n_eval_all, int *status_all, int *winner, double *theta_w, double *value_w,
                           double *lik_w, double *X, double *Y, double *V, double *J);

/* Test hook of that pre-launch check, no device needed: lays out the block of ldsr_pl_grad_batch (kernel = 0) or
 * ldsr_bfgs_update_batch (kernel = 1) for the given shape at a made-up base address, reserves strip_short bytes
 * less for the strip, moves grad (kernel 0) or par (kernel 1) up by out_shift bytes, and runs the check on the
 * kernel's parameter struct.  -> LDSR_OK, or LDSR_EINTERNAL with the field's name in ldsr_last_error(). */
int ldsr_plg_extent_check(int kernel, int n_series, int T, int p, int q, int has_u, int has_v, int shared_uv,
                          const int *cell_offsets, int with_grad, long strip_short, long out_shift);

/* The Kalman filter's own outputs and the innovation diagnostics: for every cell's theta
 * the forward pass of Kalman_smoother (src/EM.cpp:43-90,115-120), kept instead of discarded.  Time is 0-based;
 * obs_t = isfinite(y_t) (NaN, NA and +-Inf: missing); an absent u (v) drops the B u (D v) term.
 *   Xp_0 = mu1, Vp_0 = V1;  t >= 1: Xp_t = A Xu_{t-1} + B u_{t-1}, Vp_t = A Vu_{t-1} A + Q
 *   Yp_t = C Xp_t + D v_t;  S_t = C Vp_t C + R (every t);  e_t = y_t - Yp_t where obs_t, NaN elsewhere
 *   obs_t: K = Vp_t C / S_t, Xu_t = Xp_t + K e_t, Vu_t = (1 - K C) Vp_t;  otherwise Xu_t = Xp_t, Vu_t = Vp_t
 *   ll_t = -1/2 (log(2 pi) + log S_t + e_t^2 / S_t) where obs_t, 0 elsewhere
 *   lik  = sum_t ll_t, divided by n_obs when stdlik: Kalman_smoother's lik (n_obs = 0: 0, NaN with stdlik)
 *   z_t  = e_t / sqrt(S_t) at observed t;  zmean = their mean;  zvar = sum (z_t - zmean)^2 / n_obs
 *   acf_k = sum over t with obs_t and obs_{t+k} of (z_t - zmean)(z_{t+k} - zmean) / sum over observed t of
 *           (z_t - zmean)^2, k = 1 .. n_lags; NaN when no such pair exists or the denominator is 0 (this project's
 *           own specification for series with holes)
 * Outputs: the rows Xp, Vp, Yp, Xu, Vu, e, S, ll are [n_cells][T], each may be NULL (not written, not copied);
 * lik [n_cells]; zstat [n_cells][2] = (zmean, zvar), may be NULL; acf [n_cells][n_lags], required exactly when
 * n_lags > 0 (0 <= n_lags <= LDSR_FILTER_MAX_LAGS, n_lags < T); status [n_cells], may be NULL: LDSR_CELL_NONFINITE
 * when sum_t ll_t is not finite (some S_t <= 0 at an observed step: the rows hold what the recursion produced), else
 * LDSR_CELL_OK -- the sum before the division, so status does not depend on stdlik.  The filter does not whiten by
 * Svv / Tuu: a series an EM call flags LDSR_CELL_SINGULAR is answered like any other.  One wavefront per cell, any T
 * (filter.hip); a cell's numbers do not depend on the rows requested, on its place in the batch or on stdlik (lik
 * apart), and are the same from both entries. */
#define LDSR_FILTER_MAX_LAGS 32
int ldsr_filter_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                      const double *v, int shared_uv, const int *cell_offsets, const double *theta, int stdlik,
                      int n_lags, double *Xp, double *Vp, double *Yp, double *Xu, double *Vu, double *e, double *S,
                      double *ll, double *lik, double *zstat, double *acf, int *status);
/* The same with DEVICE pointers (cell_offsets stays a host array), asynchronous on `stream` (NULL = default stream):
 * the call only enqueues.  d_workspace: at least ldsr_filter_workspace_bytes(...) bytes (0: unsupported arguments),
 * 256-byte aligned; it holds the cell -> series map and, when n_lags > 0, the [n_cells][T] strip of z the lag pass
 * reads.  A short workspace is refused before anything is written. */
size_t ldsr_filter_workspace_bytes(int n_series, int T, int p, int q, int n_cells, int n_lags);
int ldsr_filter_batch_device(int device, void *stream, int n_series, int T, int p, int q, const double *d_y,
                             const double *d_u, const double *d_v, int shared_uv, const int *cell_offsets,
                             const double *d_theta, int stdlik, int n_lags, double *d_Xp, double *d_Vp, double *d_Yp,
                             double *d_Xu, double *d_Vu, double *d_e, double *d_S, double *d_ll, double *d_lik,
                             double *d_zstat, double *d_acf, int *d_status, void *d_workspace, size_t workspace_bytes);

/* Test hooks of the arenas' guard mode (LDSR_ARENA_GUARD=1 in the environment when the library is loaded; off, and
 * free, by default).  In that mode every buffer a host-pointer entry carves out of its arena is followed by a band of
 * at least 256 bytes and the block by one of 64 KiB, the whole block is filled with 0xFF before the entry uploads
 * anything, and when the call's lease ends the bands are read back: every band with a changed byte is one violation.
 *   ldsr_arena_guard_report    number of violations since the last report; their descriptions, one per line (entry,
 *                              carve index, offsets, byte count), go into buf (may be NULL)
 *   ldsr_arena_guard_selftest  leases an arena, carves two buffers, sets ONE byte of the band between them with
 *                              hipMemset from the host, and releases: the next report counts exactly one violation,
 *                              "band behind carve 0".  Launches no kernel and touches only memory the arena owns.
 *                              LDSR_EINVAL when the mode is off. */
int ldsr_arena_guard_report(char *buf, size_t len);
int ldsr_arena_guard_selftest(int device);

/* Stochastic replicates: one_LDS_rep / LDS_rep (R/stochastics.R:18-63) for n_models thetas x
 * num_reps replicates of T steps,
 *   x_1 ~ N(0, V1), x_{t+1} = A x_t + B u_t + q_t, y_t = C x_t + D v_t + r_t, q_t ~ N(0, Q), r_t ~ N(0, R),
 *   simQ_t = exp(y_t + mu) if exp_trans, else y_t + mu   (x_1 has mean 0: mu1 is not used).
 *   theta  [n_models][6+p+q]; u [n_models][T][p] / v [n_models][T][q] (shared_uv: one [T][p] / [T][q]
 *          for all models), either NULL = that term dropped (no upper limit on p, q); mu [n_models]
 *          or NULL (= 0).
 *   uniforms  NULL: counter mode -- uniform i of replicate r of model m is SplitMix64 of (seed,
 *          m * 2^32 + first_rep + r, i), so replicates do not depend on how they are split over calls;
 *          otherwise R-stream mode: R's unif_rand() values in the order LDS_rep consumes them (models
 *          one after the other, each model's replicates one after the other; first_rep is unused).
 *          Normals are R's "Inversion" rule: two uniforms each, none for a zero, NaN, negative or
 *          infinite variance (R's rnorm returns 0 / NaN there without drawing).
 *   simX, simY, simQ  [n_models][num_reps][T], each may be NULL (not computed).
 * Host pointers; copies in, runs on `device`, copies out. */
int ldsr_simulate_batch(int device, int n_models, int T, int p, int q, const double *u,
                        const double *v, int shared_uv, const double *theta, const double *mu,
                        int num_reps, int first_rep, int exp_trans, unsigned long long seed,
                        const double *uniforms, double *simX, double *simY, double *simQ);
/* Uniforms one such call consumes in R-stream mode (host code); offsets [n_models + 1] (may be NULL)
 * receives where each model's uniforms start.  A negative value (-LDSR_EINVAL) for bad arguments. */
long long ldsr_simulate_draw_count(int n_models, int T, int p, int q, const double *theta,
                                   int num_reps, long long *offsets);
/* Same as ldsr_simulate_batch with DEVICE pointers, asynchronous on `stream` (NULL = default
 * stream).  R-stream mode also takes d_offsets: the first n_models offsets of
 * ldsr_simulate_draw_count, copied to the device (NULL in counter mode). */
int ldsr_simulate_batch_device(int device, void *stream, int n_models, int T, int p, int q,
                               const double *d_u, const double *d_v, int shared_uv,
                               const double *d_theta, const double *d_mu, int num_reps,
                               int first_rep, int exp_trans, unsigned long long seed,
                               const double *d_uniforms, const long long *d_offsets,
                               double *d_simX, double *d_simY, double *d_simQ);

/* Principal-component regression, the reference's benchmark model (R/PCR.R): one_pcr_cv (:101-107) for every
 * (member, fold) cell of cvPCR / PCR_ensemble_selection (:164, :220, :228) and the lm + predict of
 * PCR_reconstruction (:49-50, :76-77), all cells in ONE launch.  Cell (m, f) fits y ~ 1 + X_m by a Householder QR
 * (intercept first, the member's columns in order, no pivoting -- the method class of stats::.lm.fit, not the
 * normal equations) on the rows with heldout[f][i] == 0 and y[i] finite, then predicts the rows of Xpred_m.
 *   k        [n_members] columns of each member, 1 .. 16 (larger: LDSR_EUNSUPPORTED); members may differ
 *   X        member blocks, each n x k[m] column-major (the bytes of an R matrix), concatenated
 *   y        [n]; NaN, NA and +-Inf rows never train (na.omit)
 *   heldout  [n_folds][n] bytes, 0 / 1; n_folds = 1 with an all-zero row is the plain fit
 *   Xpred    member blocks, each N x k[m] column-major, concatenated; NULL: predict X's own rows (N must be n)
 *   pred     [n_members][n_folds][N] x_t' beta        lev   likewise, h_t = |R^-T x_t|^2 = x_t'(X'X)^-1 x_t
 *   coef     [n_members][n_folds][17]: intercept, slopes, NaN beyond k[m] + 1
 *   sigma    [n_members][n_folds] sqrt(RSS / df), NaN when df = 0      df  likewise, n_train - (k[m] + 1)
 *   status   [n_members][n_folds] LDSR_CELL_OK, or LDSR_CELL_SINGULAR (pred, lev, coef, sigma NaN): fewer
 *            training rows than k[m] + 1, or a column whose norm after the reflections before it is <= 1e-7 of
 *            its original norm -- .lm.fit's tolerance used as a flag where LINPACK would pivot
 * lev, coef, sigma, df may each be NULL.  Host pointers.  A cell's result does not depend on the other cells of
 * the call.  Limits: n >= 2 and n * (max k + 2) <= 18432 (a cell's design lives in LDS: n <= 1024 at k = 16,
 * n <= 6144 at k = 1; larger: LDSR_EUNSUPPORTED); N is unbounded. */
int ldsr_pcr_batch(int device, int n_members, int n, const int *k, const double *X, const double *y, int n_folds,
                   const unsigned char *heldout, int N, const double *Xpred, double *pred, double *lev,
                   double *coef, double *sigma, int *df, int *status);

/* User interrupts during a run (the reference calls Rcpp::checkUserInterrupt() every 100 EM
 * iterations, src/EM.cpp:261-262).  While a callback is registered, the thread that called an
 * EM entry point (ldsr_em_batch[_multi], ldsr_em_restart_grid / _groups) invokes it about once
 * per millisecond while it waits for the device -- never from the library's worker threads; a
 * non-zero return raises a host-pinned flag that every running EM kernel polls every 64
 * iterations: cells stop with status LDSR_CELL_INTERRUPTED and the call returns
 * LDSR_EINTERRUPTED.  NULL unregisters.  The R shim registers R_CheckUserInterrupt wrapped in
 * R_ToplevelExec. */
int ldsr_set_interrupt_callback(int (*callback)(void *), void *arg);

/* Optional kernel timer.  While enabled, every ldsr_em_batch_device call brackets its EM
 * kernel with HIP events on the launch stream; collect() waits for them and returns the summed
 * kernel time and the number of launches since the last collect / enable. */
void ldsr_profile_enable(int on);
int ldsr_profile_collect(double *total_ms, int *n_launches);

/* Restart selection on the host: index of the winning cell among n, or -1. */
int ldsr_select_restart(int n, const double *lik, const double *theta, int p, int q);

/* The reference's five skill metrics (/root/reference/src/utils.cpp: NSE :13, nRMSE :36, corr :49,
 * KGE :68, RE :93; .Call entries _ldsr_NSE .. _ldsr_RE, src/RcppExports.cpp:71-130,137-141).  Host
 * code on n points -- cross-validation folds of 12..46 values: they are here because a DLL that
 * replaces ldsr.so must keep them registered, not because they are hot.  Same argument order as
 * the reference: model output first, observation second. */
double ldsr_metric_nse(int n, const double *yhat, const double *y);
double ldsr_metric_nrmse(int n, const double *yhat, const double *y, double norm_const);
double ldsr_metric_corr(int n, const double *x, const double *y);
double ldsr_metric_kge(int n, const double *yhat, const double *y);
double ldsr_metric_re(int n, const double *yhat, const double *y, double yc_bar);

#ifdef __cplusplus
}
#endif
#endif
