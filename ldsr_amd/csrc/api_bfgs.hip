// api_bfgs.hip -- the L-BFGS learners' entries of the C ABI: ssqTrain, the two optimisers, the penalised
// likelihood's gradient and the extent check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "host_series.h"
#include "bfgs.h"
#include "plgrad.h"

namespace ldsr_host {

// Every entry uploads the raw series (the kernels read the ABI's time-major u, v as they are and find the
// missing y_t themselves), the cell -> series map and the cells' thetas: a SeriesUpload with its cells, whose
// view() is the series side of the launch.  The strip of the workspace is the objective's own.
// ssqTrain (LDS_BFGS, bfgs.hip): for the gradient, where T is beyond the LDS
static size_t ssq_strip_bytes(int n_cells, int T) {
    return T <= BFGS_LDS_MAX_T ? 0 : sizeof(double) * 2 * (size_t)T * (size_t)bfgs_waves(n_cells, T);
}
// the penalised likelihood (LDS_BFGS_with_update, plgrad.hip): always
static size_t plg_strip_bytes(int n_cells, int T) {
    return n_cells > 0 ? sizeof(double) * plg_launch_strip_doubles(n_cells, T) : 0;
}
// bytes the block reserves for y, u, v, series_of_cell and the strip (SeriesUpload::carve)
struct PlgSeriesHave { size_t b[5]; };
static PlgSeriesHave plg_series_have(const SeriesUpload &U, size_t strip_bytes) {
    return PlgSeriesHave{{sizeof(double) * (size_t)U.n_series * U.T, U.uv_bytes(U.u, U.p), U.uv_bytes(U.v, U.q),
                          sizeof(int) * (size_t)U.cell_offsets[U.n_series], strip_bytes}};
}
// The pre-launch check: every extent inside what was reserved for it and inside the call's block, no required
// pointer null -- else LDSR_EINTERNAL with the field's name, and the caller does not launch.
static int refuse_bad_extent(const char *kernel, const PlgExtent *e, int n, const char *dev, size_t block_bytes) {
    const int bad = plg_first_bad_extent(e, n, dev, block_bytes);
    if (bad < 0) return LDSR_OK;
    const PlgExtent &x = e[bad];
    if (!x.ptr) return fail(LDSR_EINTERNAL, std::string("internal: ") + kernel + " not launched: " + x.name + " is NULL");
    return fail(LDSR_EINTERNAL, std::string("internal: ") + kernel + " not launched: the kernel touches " +
                std::to_string(x.need) + " bytes of " + x.name + ", " + std::to_string(x.have) + " are reserved at offset " +
                std::to_string((long long)((const char *)x.ptr - dev)) + " of a block of " + std::to_string(block_bytes));
}
static int check_bfgs_update_extents(const BfgsParams &up, int n_series, const PlgSeriesHave &have, const char *dev,
                                     size_t block_bytes) {
    const int n_cells = up.S.n_cells, P = 6 + up.S.p + up.S.q;
    const size_t rows = sizeof(double) * (size_t)n_cells * P, vals = sizeof(double) * (size_t)n_cells;
    const size_t ints = sizeof(int) * (size_t)n_cells, box = sizeof(double) * (size_t)P;
    PlgExtent e[PLG_MAX_EXTENTS];
    int n = plg_series_extents(up.S, n_series, have.b, e);
    e[n++] = PlgExtent{"par0", up.par0, sizeof(double) * plg_rows_doubles(n_cells, P), rows, 1};
    e[n++] = PlgExtent{"lb", up.lb, sizeof(double) * plg_rows_doubles(1, P), box, 1};
    e[n++] = PlgExtent{"ub", up.ub, sizeof(double) * plg_rows_doubles(1, P), box, 1};
    e[n++] = PlgExtent{"par", up.par, sizeof(double) * plg_rows_doubles(n_cells, P), rows, 1};
    e[n++] = PlgExtent{"value", up.value, sizeof(double) * plg_rows_doubles(n_cells, 1), vals, 1};
    e[n++] = PlgExtent{"n_iter", up.n_iter, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    e[n++] = PlgExtent{"n_eval", up.n_eval, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    e[n++] = PlgExtent{"status", up.status, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    return refuse_bad_extent("ldsr_bfgs_update_kernel", e, n, dev, block_bytes);
}

// The block of ldsr_bfgs_batch / ldsr_bfgs_update_batch: [series | map | par0 | lb | ub | offsets] go up in one
// copy; then what the host always reads, the optional per-cell results, the winners' fit, the strip, the workspace.
struct BfgsCall {
    SeriesUpload U;
    bool update;
    int n_cells, P;
    WsLayout L;
    size_t nT, o_lb, o_ub, o_off, in_bytes, o_win, o_thw, o_vw, sel_bytes, o_par, o_val, o_nit, o_nev, o_st, cell_bytes,
           o_lik, o_X, o_Y, o_V, o_J, o_fst, fit_bytes, o_fsoc, o_fth, strip_bytes, o_strip, o_ws, total;
    Carver c;
    BfgsCall(const SeriesUpload &series, const int *cell_offsets, const double *par0, bool update_)
        : U(series), update(update_) {
        const int n_series = U.n_series, T = U.T;
        n_cells = cell_offsets[n_series]; P = 6 + U.p + U.q;
        L = ws_layout(n_series, T, ldsr_pad_dim(U.p), ldsr_pad_dim(U.q), U.shared_uv, n_series, LDSR_ALGO_SCAN, 1);
        nT = (size_t)n_series * T;
        U.carve(c, cell_offsets, par0);
        o_lb = c.take(sizeof(double) * (size_t)P);
        o_ub = c.take(sizeof(double) * (size_t)P);
        o_off = c.take(sizeof(int) * ((size_t)n_series + 1));
        in_bytes = c.o;
        o_win = c.take(sizeof(int) * (size_t)n_series);
        o_thw = c.take(sizeof(double) * (size_t)n_series * P);
        o_vw = c.take(sizeof(double) * (size_t)n_series);
        sel_bytes = c.o - o_win;
        o_par = c.take(sizeof(double) * (size_t)n_cells * P);
        o_val = c.take(sizeof(double) * (size_t)n_cells);
        o_nit = c.take(sizeof(int) * (size_t)n_cells);
        o_nev = c.take(sizeof(int) * (size_t)n_cells);
        o_st = c.take(sizeof(int) * (size_t)n_cells);
        cell_bytes = c.o - o_par;
        o_lik = c.take(sizeof(double) * (size_t)n_series);
        o_X = c.take(sizeof(double) * nT);
        o_Y = c.take(sizeof(double) * nT);
        o_V = c.take(sizeof(double) * nT);
        o_J = c.take(sizeof(double) * nT);
        o_fst = c.take(sizeof(int) * (size_t)n_series);
        fit_bytes = c.o - o_lik;
        o_fsoc = c.take(sizeof(int) * (size_t)n_series);
        o_fth = c.take(sizeof(double) * (size_t)n_series * P);
        strip_bytes = update ? plg_strip_bytes(n_cells, T) : ssq_strip_bytes(n_cells, T);
        o_strip = c.take(strip_bytes);
        o_ws = c.take(L.total);
        total = c.o;
    }
    // the pointers of the optimiser's launch (its scalars are the caller's)
    BfgsParams params(char *dev) const {
        BfgsParams bp;
        memset(&bp, 0, sizeof(bp));
        bp.S = U.view(dev, strip_bytes ? (double *)(dev + o_strip) : nullptr);
        bp.par0 = (const double *)(dev + U.o_th);
        bp.lb = (const double *)(dev + o_lb);
        bp.ub = (const double *)(dev + o_ub);
        bp.par = (double *)(dev + o_par);
        bp.value = (double *)(dev + o_val);
        bp.n_iter = (int *)(dev + o_nit);
        bp.n_eval = (int *)(dev + o_nev);
        bp.status = (int *)(dev + o_st);
        return bp;
    }
    int check(const BfgsParams &up, size_t strip_have, const char *dev) const {
        return check_bfgs_update_extents(up, U.n_series, plg_series_have(U, strip_have), dev, total);
    }
};

// One launch runs every cell's optimisation from start to stop; a second picks the winners; the host then
// sees winner / theta_w / value_w, and the winners' fit is one pass of the existing propagate / FIT
// kernels on the prepared series.
// update: the objective is -pl at lambda (LDS_BFGS_with_update, plgrad.hip) instead of ssqTrain.
static int run_bfgs(bool update, double lambda, int device, int n_series, int T, int p, int q, const double *y,
                    const double *u, const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                    const double *lb, const double *ub, int maxit, int lmm, double factr, double pgtol,
                    int select_max, int fit_mode, double *par_all, double *value_all, int *n_iter_all,
                    int *n_eval_all, int *status_all, int *winner, double *theta_w, double *value_w, double *lik_w,
                    double *X, double *Y, double *V, double *J) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    const int P = 6 + p + q;
    rc = check_box(lb, ub, P, "variable");
    if (rc) return rc;
    if (!std::isfinite(lambda)) return fail(LDSR_EINVAL, "lambda must be finite");
    if (maxit < 1) return fail(LDSR_EINVAL, "maxit must be >= 1");
    if (lmm < 1 || lmm > BFGS_MAX_LMM) return fail(LDSR_EINVAL, "lmm must be in 1 .. 8");
    if (!(factr >= 0.0) || !std::isfinite(factr)) return fail(LDSR_EINVAL, "factr must be finite and >= 0");
    if (!(pgtol >= 0.0) || !std::isfinite(pgtol)) return fail(LDSR_EINVAL, "pgtol must be finite and >= 0");
    if (fit_mode != 0 && fit_mode != 1) return fail(LDSR_EINVAL, "fit_mode must be 0 (propagate) or 1 (Kalman_smoother)");
    if (!par0) return fail(LDSR_EINVAL, "par0 must not be NULL");
    if (!winner || !theta_w || !value_w) return fail(LDSR_EINVAL, "winner, theta_w and value_w must not be NULL");
    const int n_cells = cell_offsets[n_series];
    const bool want_fit = lik_w || X || Y || V || (J && fit_mode == 1);
    IntrScope intr_scope;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    BfgsCall B(SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, par0, update);
    SeriesUpload &U = B.U;
    const size_t nT = B.nT;
    const bool want_cells = par_all || value_all || n_iter_all || n_eval_all || status_all;
    rc = arena_reserve(A, B.c, B.in_bytes + align256(B.sel_bytes) + align256(std::max(B.cell_bytes, B.fit_bytes)),
                       update ? "ldsr_bfgs_update_batch" : "ldsr_bfgs_batch");
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    U.stage(A);
    memcpy(pin + B.o_lb, lb, sizeof(double) * (size_t)P);
    memcpy(pin + B.o_ub, ub, sizeof(double) * (size_t)P);
    memcpy(pin + B.o_off, cell_offsets, sizeof(int) * ((size_t)n_series + 1));
    BfgsParams bp = B.params(dev);
    bp.lambda = lambda;
    bp.maxit = maxit; bp.lmm = lmm;
    bp.ftol = factr * 0x1p-52; bp.pgtol = pgtol;
    bp.intr = intr_flag_for_kernels();
    if (update && n_cells > 0) {        // (before anything is enqueued)
        rc = B.check(bp, B.strip_bytes, dev);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(dev, pin, B.in_bytes, hipMemcpyHostToDevice, A->stream));
    HIPCHK(update ? launch_bfgs_update(bp, A->stream) : launch_bfgs(bp, A->stream));
    BfgsSelectParams sl;
    sl.n_series = n_series; sl.P = P; sl.select_max = select_max;
    sl.cell_offsets = (const int *)(dev + B.o_off);
    sl.par = bp.par; sl.value = bp.value;
    sl.winner = (int *)(dev + B.o_win);
    sl.theta_w = (double *)(dev + B.o_thw);
    sl.value_w = (double *)(dev + B.o_vw);
    HIPCHK(launch_bfgs_select(sl, A->stream));
    char *psel = pin + B.in_bytes, *pbig = psel + align256(B.sel_bytes);
    HIPCHK(hipMemcpyAsync(psel, dev + B.o_win, B.sel_bytes, hipMemcpyDeviceToHost, A->stream));
    if (want_cells) HIPCHK(hipMemcpyAsync(pbig, dev + B.o_par, B.cell_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(wait_stream(A->stream));
    intr_poll();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    memcpy(winner, psel, sizeof(int) * (size_t)n_series);
    memcpy(theta_w, psel + (B.o_thw - B.o_win), sizeof(double) * (size_t)n_series * P);
    memcpy(value_w, psel + (B.o_vw - B.o_win), sizeof(double) * (size_t)n_series);
    if (par_all) memcpy(par_all, pbig, sizeof(double) * (size_t)n_cells * P);
    if (value_all) memcpy(value_all, pbig + (B.o_val - B.o_par), sizeof(double) * (size_t)n_cells);
    if (n_iter_all) memcpy(n_iter_all, pbig + (B.o_nit - B.o_par), sizeof(int) * (size_t)n_cells);
    if (n_eval_all) memcpy(n_eval_all, pbig + (B.o_nev - B.o_par), sizeof(int) * (size_t)n_cells);
    if (status_all) memcpy(status_all, pbig + (B.o_st - B.o_par), sizeof(int) * (size_t)n_cells);
    if (!want_fit) return LDSR_OK;

    // the winners' fit: the series that have one, their thetas packed side by side
    std::vector<int> ws_series;
    std::vector<double> th((size_t)n_series * P);
    for (int s = 0; s < n_series; s++)
        if (winner[s] >= 0) {
            memcpy(&th[ws_series.size() * P], theta_w + (size_t)s * P, sizeof(double) * (size_t)P);
            ws_series.push_back(s);
        }
    const int n_w = (int)ws_series.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto fill = [&](double *a, size_t n) { if (a) std::fill(a, a + n, nan); };
    if (n_w < n_series) {
        fill(lik_w, (size_t)n_series); fill(X, nT); fill(Y, nT); fill(V, nT);
        if (fit_mode == 1) fill(J, nT);
    }
    if (n_w == 0) return LDSR_OK;
    HIPCHK(U.prep(device, A->stream, dev + B.o_ws, &B.L));
    rc = stage_h2d_async(device, A->stream, dev + B.o_fth, th.data(), sizeof(double) * (size_t)n_w * P);
    if (rc) return rc;
    const FitOut fit{(double *)(dev + B.o_X), (double *)(dev + B.o_Y), (double *)(dev + B.o_V), (double *)(dev + B.o_J),
                     (double *)(dev + B.o_lik), nullptr, (int *)(dev + B.o_fst)};
    rc = launch_smoother(U.ps, n_w, ws_series.data(), (const double *)(dev + B.o_fth), 1, fit_mode == 0 ? 1 : 0, 0.0, fit,
                         (int *)(dev + B.o_fsoc));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pbig, dev + B.o_lik, B.fit_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(wait_stream(A->stream));
    for (int i = 0; i < n_w; i++) {
        const size_t s = (size_t)ws_series[(size_t)i], row = sizeof(double) * (size_t)i * T;
        if (lik_w) lik_w[s] = ((const double *)pbig)[i];
        if (X) memcpy(X + s * T, pbig + (B.o_X - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (Y) memcpy(Y + s * T, pbig + (B.o_Y - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (V) memcpy(V + s * T, pbig + (B.o_V - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (J && fit_mode == 1) memcpy(J + s * T, pbig + (B.o_J - B.o_lik) + row, sizeof(double) * (size_t)T);
    }
    // A series the scan kernel flagged (singular Svv / Tuu) has a smoother all the same: its winner takes the
    // serial kernel in a call of its own, which is what ldsr_smooth_batch gives for that theta.
    const int *fst = (const int *)(pbig + (B.o_fst - B.o_lik));
    const int off1[2] = {0, 1};
    for (int i = 0; i < n_w && smoother_is_scan(T, U.ps.PP, U.ps.QQ, B.L, fit_mode == 0 ? 1 : 0); i++) {
        if (fst[i] != LDSR_CELL_SINGULAR) continue;
        const size_t s = (size_t)ws_series[(size_t)i], uv = shared_uv ? 0 : s * T;
        auto row = [&](double *a) { return a ? a + s * T : nullptr; };
        double lik1;
        rc = run_fit_kernel(FIT_SMOOTH, device,
                            SeriesUpload{1, T, p, q, y + s * T, u ? u + uv * p : nullptr, v ? v + uv * q : nullptr, shared_uv},
                            off1, theta_w + s * P, 1, 0.0, FitOut{row(X), row(Y), row(V), row(J), &lik1}, true);
        if (rc) return rc;
        if (lik_w) lik_w[s] = lik1;
    }
    return LDSR_OK;
}

extern "C" int ldsr_bfgs_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                               const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                               const double *lb, const double *ub, int maxit, int lmm, double factr,
                               double pgtol, int select_max, int fit_mode, double *par_all, double *value_all,
                               int *n_iter_all, int *n_eval_all, int *status_all, int *winner, double *theta_w,
                               double *value_w, double *lik_w, double *X, double *Y, double *V, double *J) {
    return run_bfgs(false, 0.0, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, par0, lb, ub, maxit, lmm,
                    factr, pgtol, select_max, fit_mode, par_all, value_all, n_iter_all, n_eval_all, status_all, winner,
                    theta_w, value_w, lik_w, X, Y, V, J);
}

extern "C" int ldsr_bfgs_update_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                                      const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                                      const double *lb, const double *ub, double lambda, int maxit, int lmm,
                                      double factr, double pgtol, int select_max, double *par_all, double *value_all,
                                      int *n_iter_all, int *n_eval_all, int *status_all, int *winner, double *theta_w,
                                      double *value_w, double *lik_w, double *X, double *Y, double *V, double *J) {
    return run_bfgs(true, lambda, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, par0, lb, ub, maxit, lmm,
                    factr, pgtol, select_max, 1, par_all, value_all, n_iter_all, n_eval_all, status_all, winner,
                    theta_w, value_w, lik_w, X, Y, V, J);
}

// The block of ldsr_ssq_grad_batch / ldsr_pl_grad_batch: [series | map | theta] go up in one copy, [value | grad]
// come back in one; then the objective's strip (pl: the penalised likelihood, else ssqTrain).
struct GradCall {
    SeriesUpload U;
    int n_cells, P;
    size_t in_bytes, o_f, o_g, g_bytes, out_bytes, o_strip, strip_bytes, total;
    Carver c;
    GradCall(const SeriesUpload &series, const int *cell_offsets, const double *theta, bool pl, bool grad) : U(series) {
        n_cells = cell_offsets[U.n_series]; P = 6 + U.p + U.q;
        U.carve(c, cell_offsets, theta);
        in_bytes = c.o;
        o_f = c.take(sizeof(double) * (size_t)n_cells);
        g_bytes = grad ? sizeof(double) * (size_t)n_cells * P : 0;
        o_g = c.take(g_bytes);
        out_bytes = c.o - o_f;
        strip_bytes = pl ? plg_strip_bytes(n_cells, U.T) : grad ? ssq_strip_bytes(n_cells, U.T) : 0;
        o_strip = c.take(strip_bytes);
        total = c.o;
    }
    // the launch's parameters: those of ldsr_pl_grad_kernel; ldsr_ssq_grad_kernel's are the same without lambda
    PlGradParams params(char *dev, double lambda) const {
        PlGradParams pp;
        pp.S = U.view(dev, strip_bytes ? (double *)(dev + o_strip) : nullptr);
        pp.theta = (const double *)(dev + U.o_th);
        pp.lambda = lambda;
        pp.pl = (double *)(dev + o_f);
        pp.grad = g_bytes ? (double *)(dev + o_g) : nullptr;
        return pp;
    }
    int check(const PlGradParams &pp, size_t strip_have, const char *dev) const {
        PlgExtent e[PLG_MAX_EXTENTS];
        int n = plg_series_extents(pp.S, U.n_series, plg_series_have(U, strip_have).b, e);
        e[n++] = PlgExtent{"theta", pp.theta, sizeof(double) * plg_rows_doubles(n_cells, P), sizeof(double) * (size_t)n_cells * P, 1};
        e[n++] = PlgExtent{"pl", pp.pl, sizeof(double) * plg_rows_doubles(n_cells, 1), sizeof(double) * (size_t)n_cells, 1};
        e[n++] = PlgExtent{"grad", pp.grad, sizeof(double) * plg_rows_doubles(n_cells, P), g_bytes, 0};
        return refuse_bad_extent("ldsr_pl_grad_kernel", e, n, dev, total);
    }
};

// One launch: the objective's value per cell and, where grad is asked for, its gradient.  pl: the penalised
// likelihood at lambda, with the pre-launch extent check; else ssqTrain.
static int run_value_grad(bool pl, double lambda, int device, int n_series, int T, int p, int q, const double *y,
                          const double *u, const double *v, int shared_uv, const int *cell_offsets, const double *theta,
                          double *value, double *grad) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    if (!theta || !value) return fail(LDSR_EINVAL, pl ? "theta and pl must not be NULL" : "theta and ssq must not be NULL");
    if (!std::isfinite(lambda)) return fail(LDSR_EINVAL, "lambda must be finite");
    if (cell_offsets[n_series] == 0) return LDSR_OK;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    GradCall call(SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, theta, pl, grad != nullptr);
    rc = arena_reserve(A, call.c, call.in_bytes + align256(call.out_bytes), pl ? "ldsr_pl_grad_batch" : "ldsr_ssq_grad_batch");
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    call.U.stage(A);
    const PlGradParams pp = call.params(dev, lambda);
    if (pl) {
        rc = call.check(pp, call.strip_bytes, dev);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(dev, pin, call.in_bytes, hipMemcpyHostToDevice, A->stream));
    HIPCHK(pl ? launch_pl_grad(pp, A->stream) : launch_ssq_grad(SsqParams{pp.S, pp.theta, pp.pl, pp.grad}, A->stream));
    char *pout = pin + call.in_bytes;
    HIPCHK(hipMemcpyAsync(pout, dev + call.o_f, call.out_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    memcpy(value, pout, sizeof(double) * (size_t)call.n_cells);
    if (grad) memcpy(grad, pout + (call.o_g - call.o_f), sizeof(double) * (size_t)call.n_cells * call.P);
    return LDSR_OK;
}

extern "C" int ldsr_ssq_grad_batch(int device, int n_series, int T, int p, int q, const double *y,
                                   const double *u, const double *v, int shared_uv, const int *cell_offsets,
                                   const double *theta, double *ssq, double *grad) {
    return run_value_grad(false, 0.0, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta, ssq, grad);
}

extern "C" int ldsr_pl_grad_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                                  const double *v, int shared_uv, const int *cell_offsets, const double *theta,
                                  double lambda, double *pl, double *grad) {
    return run_value_grad(true, lambda, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta, pl, grad);
}

extern "C" int ldsr_plg_extent_check(int kernel, int n_series, int T, int p, int q, int has_u, int has_v, int shared_uv,
                                     const int *cell_offsets, int with_grad, long strip_short, long out_shift) {
    static const double present = 0.0;      // (y, u, v: only whether they are null matters here)
    int rc = check_common(n_series, T, p, q, &present, cell_offsets);
    if (rc) return rc;
    if (cell_offsets[n_series] < 1) return fail(LDSR_EINVAL, "the check needs at least one cell");
    char *const dev = (char *)(uintptr_t)0x100000;      // never dereferenced
    GradCall call(SeriesUpload{n_series, T, p, q, &present, has_u ? &present : nullptr, has_v ? &present : nullptr,
                               shared_uv}, cell_offsets, nullptr, true, kernel == 1 || with_grad != 0);
    const PlGradParams pp0 = call.params(dev, 1.0);
    const size_t strip_have = call.strip_bytes - (size_t)strip_short;
    if (kernel == 0) {
        PlGradParams pp = pp0;
        if (pp.grad) pp.grad = (double *)((char *)pp.grad + out_shift);
        return call.check(pp, strip_have, dev);
    }
    // ldsr_bfgs_update_batch's own block
    const BfgsCall B(call.U, cell_offsets, nullptr, true);
    BfgsParams bp = B.params(dev);
    bp.par = (double *)((char *)bp.par + out_shift);
    return B.check(bp, B.strip_bytes - (size_t)strip_short, dev);
}

}  // namespace ldsr_host
