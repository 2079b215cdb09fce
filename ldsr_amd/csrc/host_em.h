// host_em.h -- what api_em.hip gives the other host units: the workspace layout, one EM launch on device data,
// and one smoother pass on prepared series.
#pragma once
#include <vector>

#include "host_runtime.h"
#include "ldsr_kernels.h"

namespace ldsr_host {

struct WsLayout {
    size_t sc, yp, yz, up, vp, img, img2, img3, blk, soc, queue, perm, perm_key, scratch, total;
    long scratch_stride, img_stride;   // img_stride: doubles per series image (0 = no image)
    long img2_stride;                  // pair kernel's image (0 = none)
    long img3_stride;                  // ... and its lead image
    int max_blocks, img_L, img_NL;
};

WsLayout ws_layout(int n_series, int T, int PP, int QQ, int shared_uv, int n_cells, int algo, int cpb);
PrepParams prep_params(int n_series, int T, int p, int q, int PP, int QQ, const double *d_y, const double *d_u,
                       const double *d_v, int shared_uv, char *ws, const WsLayout &L, bool scan_img);

// One EM launch on device data (cell_offsets: a host array).  em_batch_device_impl fills in the plan it
// chose and the workspace layout it carved.
struct EmLaunch {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_series = 0, T = 0, p = 0, q = 0, shared_uv = 0, niter = 0, algo = LDSR_ALGO_AUTO;
    double tol = 0.0;
    const double *y = nullptr, *u = nullptr, *v = nullptr, *theta0 = nullptr;
    const int *cell_offsets = nullptr;
    double *theta = nullptr, *lik = nullptr, *liks = nullptr;
    int *n_iter = nullptr, *status = nullptr;
    int liks_nanfill = 1;           // liks beyond a cell's n_iter set to NaN (the batch ABI; the restart grid reads n_iter)
    void *workspace = nullptr;
    size_t workspace_bytes = 0;
    const int *abort_flag = nullptr;
    int lead_steps = 0, lead_force = 0;     // EmPlanIn's data facts and forced lead
    const int *plan_off = nullptr;  // the whole call's offsets (plan_ns series; null: cell_offsets): AUTO's kernel,
    int plan_ns = 0;                // hence the rounding of the results, must not depend on how many devices share it
    bool fit_follows = true;        // the winners' FIT pass follows: series_prep builds the scan kernel's image even
                                    // behind a pair-family launch (the bare device entries skip it: 4096 values at config 2)
    EmPlan plan;                    // out
    WsLayout layout;                // out
};

int em_batch_device_impl(EmLaunch &E);

// Series that series_prep has prepared in the workspace ws (layout *L); what reads them goes on `stream`
struct PreparedSeries {
    int device;
    hipStream_t stream;
    int T, p, q, PP, QQ, shared_uv;
    bool has_u, has_v;
    char *ws;
    const WsLayout *L;
};

// Where a smoother pass writes, on the device: rows [n][T] of X, Y, V, J and [n] of lik, pen, status.  pen set:
// only the scalars leave the kernel, and X and V are the serial smoother's filtered-state strip.
struct FitOut {
    double *X = nullptr, *Y = nullptr, *V = nullptr, *J = nullptr, *lik = nullptr, *pen = nullptr;
    int *status = nullptr;
};

// the prepared-series fields of a kernel's parameters (EmParams, SmoothParams)
template <class Params>
static void set_prepared_series(Params &prm, const PreparedSeries &S) {
    prm.T = S.T; prm.p = S.p; prm.q = S.q; prm.has_u = S.has_u; prm.has_v = S.has_v;
    prm.yp = (const double *)(S.ws + S.L->yp);
    prm.up = (const double *)(S.ws + S.L->up);
    prm.vp = (const double *)(S.ws + S.L->vp);
    prm.u_stride = S.shared_uv ? 0 : (long)S.T * S.PP; prm.v_stride = S.shared_uv ? 0 : (long)S.T * S.QQ;
    prm.sc = (const SeriesConst *)(S.ws + S.L->sc);
}

// One Kalman_smoother pass (src/EM.cpp:22-131) for n cells on prepared series: the FIT form of
// the scan kernel (one wave group per cell) whenever the shape is supported, else the serial
// one-thread-per-cell kernel.  mode: 0 smoother, 1 propagate (serial kernel only).
// It comes in two parts, so that a caller that runs the same cells again and again (the GA's fitness
// pass) pays the host work once: smoother_tables uploads what depends on the cell -> series map alone,
// smoother_enqueue launches and touches no host memory.
struct SmootherTables {
    bool scan = false;              // the scan kernel's FIT form runs
    const int *d_tab = nullptr;     // its block table [3][n_blocks] on the device
    int n_blocks = 0;
};

bool smoother_is_scan(int T, int PP, int QQ, const WsLayout &L, int mode);
int smoother_tables(const PreparedSeries &S, int n, const int *series_of_cell, int mode, int *d_soc,
                    SmootherTables *out, const std::vector<char> *skip_series = nullptr);
int smoother_enqueue(const PreparedSeries &S, int n, const SmootherTables &tb, const int *d_soc,
                     const double *d_theta, int stdlik, int mode, double lambda, const FitOut &out);
int launch_smoother(const PreparedSeries &S, int n, const int *series_of_cell, const double *d_theta, int stdlik,
                    int mode, double lambda, const FitOut &out, int *d_soc, const int *d_tab_prebuilt = nullptr);

}  // namespace ldsr_host
