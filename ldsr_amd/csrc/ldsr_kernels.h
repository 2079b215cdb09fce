// ldsr_kernels.h -- host-visible launch interface between the C ABI (api_*.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "ldsr_device.h"

struct PrepParams {
    int T, p, q, PP, QQ, shared_uv;
    const double *y, *u, *v;  // raw inputs as handed over the ABI (u / v may be null)
    double *yp, *up, *vp;     // prepared copies in the workspace
    double *yz;               // y with 0 where missing
    double *img;              // scan kernel: chunk-transposed series images [n_series][img_stride], or null
    long img_stride;          // doubles per image
    int L, NL;                // chunk length and virtual lanes (64 W) of the image layout
    double *img2;             // pair kernel: second image per series (NL2 virtual lanes, chunk length L2), or null
    long img2_stride;
    int L2, NL2;
    int lead;                 // pair kernel's LEAD form: img2 covers the tail [lead, T) only ...
    double *img3;             // ... and img3 the (whitened) u_t of the lead, [step of the lane][NL2 lanes][PP], or null
    long img3_stride;
    SeriesConst *sc;
    int *queue;               // [n_series] work-queue heads, reset to 0 here
    // Cell order of the pair kernel's steady form (em_pair_impl.h em_pair_body_steady): n_series more
    // workgroups sort every series' cells by the predicted number of steps its variance recursion needs
    // to settle at theta0, slowest first -- perm[position] = cell.  Null: no ordering.
    int *perm;                // [n_cells]
    int *perm_key;            // [n_cells] scratch (the cells' buckets)
    const int *cell_off;      // [n_series + 1] device copy of the cell offsets
    const double *theta0;     // [n_cells][6 + p + q]
    int n_series;
    int order_cpb;            // static schedule: cells per workgroup (positions are dealt across the workgroups); 0 = work queue
    int order_ntr;            // steps of the transient block (L - 1)
};

struct SmoothParams {
    int T, p, q, has_u, has_v, n_cells, stdlik, mode;
    const double *yp, *up, *vp;
    long u_stride, v_stride;
    const SeriesConst *sc;
    const int *series_of_cell;
    const double *theta;  // [n_cells][P] input (smooth / propagate)
    double *X, *Y, *V, *J, *lik;
    double *theta_out;    // mstep
    int *status;
    double *pen;          // smoother: lik - lambda * ssq (penalized_likelihood), may be null
    double lambda;
    int scalar_only;      // only lik / pen leave the kernel: Y and J are not written
};

// Restart selection on the device (R/LDS_reconstruction.R:50-58), one workgroup per series.
struct SelectParams {
    int n_series, P, c_index;     // c_index: position of C in a packed theta (1 + p)
    const int *off;               // [n_series + 1] cell offsets
    const double *theta, *lik;    // [n_cells][P], [n_cells]
    int *winner;                  // [n_series] cell index or -1
};

// Winner extraction of the restart-grid entry: row i of the *_w arrays = cell[i] of the batch
// (cell[i] < 0: no winner -- NaN rows), and the FIT launch's block table, one winner per block
// (its series, cell i, one cell or none).
struct GatherParams {
    int n_w, P, niter;
    const int *cell;          // [n_w] cell index of each winner, or -1
    const int *ser;           // [n_w] series of each winner, or null: winner i is series i's
    const double *theta;      // [n_cells][P] fitted
    const double *theta0;     // [n_cells][P] initial
    const double *lik;        // [n_cells]
    const int *n_iter;        // [n_cells]
    const double *liks;       // [n_cells][niter] traces (entries beyond n_iter undefined), or null
    double *theta_w, *theta0_w;   // [n_w][P]
    double *liks_w;           // [n_w][niter], NaN padded (untouched when liks is null)
    double *lik_w;            // [n_w]
    int *n_iter_w;            // [n_w]
    int *blk;                 // [3][n_w] block table (series, first cell, cells)
};

static inline int ldsr_pad_dim(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }

hipError_t launch_series_prep(const PrepParams &prm, int n_series, hipStream_t stream);
hipError_t launch_em_serial(const EmParams &prm, int PP, int QQ, int n_blocks, hipStream_t stream);
hipError_t launch_em_scan(const EmParams &prm, int PP, int QQ, int n_blocks, bool queue, bool fit,
                          hipStream_t stream);
void em_scan_layout(int T, int PP, int QQ, int *L, int *NL, long *img_doubles);
bool em_scan_global_image(int T, int PP, int QQ);   // series image too large for LDS: read from L2
bool em_scan_queue_only(int T, int PP, int QQ);     // shapes compiled with the work-queue schedule only
bool em_scan_supported(int T, int PP, int QQ);
int em_scan_cells_per_block(int T, int PP, int QQ);
// two (lpc = 32) or four (lpc = 16) cells per wave (em_pair_impl.h): T <= lpc * 32, padded p, q <= 4
bool em_pair_supported(int T, int PP, int QQ, int lpc, bool lead_form = false);   // lead_form: T = the tail of a closed-form lead
int em_pair_cells_per_block(int T, int PP, int QQ, int lpc, int lead = 0);   // T: the steps the sweeps work on
int em_pair_waves_per_block(int T, int PP, int QQ, int lpc, int lead = 0);
void em_pair_layout(int T, int PP, int QQ, int lpc, int *L, long *img_doubles, bool lead_form = false);
hipError_t launch_em_pair(const EmParams &prm, int PP, int QQ, int lpc, int n_blocks, bool queue, hipStream_t stream);
void em_pair_kernel_name(int T, int PP, int QQ, int lpc, bool queue, char *buf, size_t len, bool lead = false);
// kernel names as rocprofv3 prints them (ldsr_em_plan)
void em_scan_kernel_name(int T, int PP, int QQ, bool queue, bool fit, char *buf, size_t len);
void em_serial_kernel_name(int T, int PP, int QQ, char *buf, size_t len);
#include <string>
void em_kernel_inventory(std::string &out);      // names of every compiled scan / pair instantiation, one per line

// Which EM kernel a launch runs (em_plan.hip): the one place that decides it, for the launches and
// for the plan queries of the C ABI.  Host code, no HIP calls.
struct EmPlanIn {
    int T = 0, p = 0, q = 0, niter = 0, algo = 0;     // algo: the requested LDSR_ALGO_*
    double tol = 0.0;
    int lead_steps = 0;            // data facts: -1 every y_t observed, 0 unknown, > 0 the first lead_steps steps of every series missing
    int lead_force = 0;            // > 0: the pair family runs with this lead (a re-run of part of a batch)
    const int *off = nullptr;      // the whole call's cell offsets [n_series + 1] on a device of cus CUs;
    int n_series = 0, cus = 0;     // off = null: a launch that fills the device
};
struct EmPlan {
    bool ok = false;
    int err = 0;                   // !ok: LDSR_E* code and message
    const char *msg = "";
    int T = 0, PP = 0, QQ = 0;
    int algo_layout = 0, layout_cpb = 0;    // what the workspace is sized and laid out for (the resolved request)
    int algo = 0;                  // what runs: LDSR_ALGO_SERIAL, _SCAN, _PAIR or _QUAD
    bool cpw = false;              // the pair family (PAIR or QUAD) with lpc lanes per cell (32: two cells per wave, 16: four)
    int lpc = 32, chunk = 0;       // ... and chunk length of its series image
    int lead = 0, Te = 0;          // closed-form lead, and the steps the sweeps work on (T - lead)
    bool queue = false;            // per-series work queue (else static schedule)
    int cpb = 0;                   // cells per workgroup
    bool steady_order = false;     // series_prep orders the cells for the steady form
};
EmPlan em_plan(const EmPlanIn &in);
void em_plan_kernel_name(const EmPlan &pl, char *buf, size_t len);   // as rocprofv3 prints it
hipError_t launch_gather_winners(const GatherParams &prm, hipStream_t stream);
hipError_t launch_select_winners(const SelectParams &prm, hipStream_t stream);
hipError_t launch_smooth(const SmoothParams &prm, int PP, int QQ, hipStream_t stream);
hipError_t launch_mstep(const SmoothParams &prm, int PP, int QQ, hipStream_t stream);

// Stochastic replicates (simulate.hip): one_LDS_rep / LDS_rep, R/stochastics.R:18-63.
// R's rnorm(n, 0, sd) with sd = sqrt(var) (nmath rnorm): a NaN, negative or infinite sd gives NaN and
// a zero sd gives 0, both without consuming a uniform; otherwise one norm_rand() = two unif_rand().
// Returns 1 if R draws, else 0 with the returned value in *fixed.
__host__ __device__ inline int sim_draws(double var, double *fixed) {
    const double sd = sqrt(var);
    if (!(sd >= 0.0) || sd == INFINITY) { *fixed = NAN; return 0; }
    if (sd == 0.0) { *fixed = 0.0; return 0; }
    *fixed = 0.0;
    return 1;
}
// uniforms one replicate consumes: [x_1 from V1] [q_1..q_T from Q] [r_1..r_T from R], two per draw
__host__ __device__ inline long long sim_draws_per_rep(const double *theta, int p, int q, int T) {
    double f;
    const int P = 6 + p + q;
    return 2 * ((long long)sim_draws(theta[P - 1], &f) + (long long)T * sim_draws(theta[2 + p + q], &f) +
                (long long)T * sim_draws(theta[3 + p + q], &f));
}
struct SimParams {
    int n_models, T, p, q, num_reps, first_rep, exp_trans;
    const double *u, *v;           // [.][T][p] / [.][T][q] time-major, or null (term dropped)
    long long u_stride, v_stride;  // doubles from one model's inputs to the next (0: one shared series)
    const double *theta;           // [n_models][6 + p + q]
    const double *mu;              // [n_models] or null (0)
    unsigned long long seed;       // counter mode
    const double *uniforms;        // R-stream mode (null: counter mode) ...
    const long long *draw_off;     // ... and [n_models] index of each model's first uniform there
    double *simX, *simY, *simQ;    // [n_models][num_reps][T], each may be null
};
hipError_t launch_simulate(const SimParams &prm, hipStream_t stream);
