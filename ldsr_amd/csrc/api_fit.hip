// api_fit.hip -- the smoother, propagate, mstep and penalised-likelihood entries of the C ABI.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "host_series.h"

namespace ldsr_host {

// The arena block of one such call, uploaded and prepared (begin): [series | map | theta] go up in one copy;
// d.lik, d.pen, d.status and d_theta_out come back in one (small_out bytes, host() says where); the rows stay.
struct FitCall {
    ArenaLease lease;
    WsLayout L;
    SeriesUpload U;
    size_t n_cells, row_bytes, small_out;
    FitOut d;       // (d.pen: FIT_PENLIK only)
    double *d_theta_out;
    char *pout;     // (pinned: the small outputs)

    const char *host(const void *small) const { return pout + ((const char *)small - (const char *)d.lik); }
    // (the serial kernels use X / V as their filtered-state strip; only FIT_PENLIK writes no rows)
    int begin(FitKind kind, int device, const SeriesUpload &series, const int *cell_offsets, const double *theta,
              bool serial = false) {
        U = series;
        int rc = arena_acquire(device, &lease.a);
        if (rc) return rc;
        Arena *A = lease.a;
        const int PP = ldsr_pad_dim(U.p), QQ = ldsr_pad_dim(U.q);
        n_cells = (size_t)cell_offsets[U.n_series]; row_bytes = sizeof(double) * n_cells * U.T;
        L = ws_layout(U.n_series, U.T, PP, QQ, U.shared_uv, (int)n_cells, LDSR_ALGO_SCAN, 1);
        const bool need_strip = kind == FIT_PROPAGATE || kind == FIT_MSTEP || serial || !em_scan_supported(U.T, PP, QQ);
        const size_t yj_bytes = kind == FIT_PENLIK ? 0 : row_bytes, xv_bytes = need_strip ? row_bytes : yj_bytes;
        Carver c;
        U.carve(c, cell_offsets, theta);
        const size_t in_bytes = c.o;
        const size_t o_lik = c.take(sizeof(double) * n_cells), o_pen = c.take(sizeof(double) * n_cells);
        const size_t o_st = c.take(sizeof(int) * n_cells), o_tho = c.take(sizeof(double) * n_cells * (6 + U.p + U.q));
        small_out = c.o - o_lik;
        const size_t o_X = c.take(xv_bytes), o_V = c.take(xv_bytes), o_Y = c.take(yj_bytes), o_J = c.take(yj_bytes);
        const size_t o_ws = c.take(L.total);
        static const char *const entry[] = {"ldsr_smooth_batch", "ldsr_propagate_batch", "ldsr_mstep_batch", "ldsr_penalized_lik_batch"};
        rc = arena_reserve(A, c, in_bytes + align256(small_out), entry[kind]);
        if (rc) return rc;
        char *dev = A->dev;
        pout = A->pin + in_bytes;
        d.X = (double *)(dev + o_X); d.Y = (double *)(dev + o_Y); d.V = (double *)(dev + o_V); d.J = (double *)(dev + o_J);
        d.lik = (double *)(dev + o_lik); d.status = (int *)(dev + o_st); d_theta_out = (double *)(dev + o_tho);
        d.pen = kind == FIT_PENLIK ? (double *)(dev + o_pen) : nullptr;
        U.stage(A);
        HIPCHK(hipMemcpyAsync(dev, A->pin, in_bytes, hipMemcpyHostToDevice, A->stream));
        HIPCHK(U.prep(device, A->stream, dev + o_ws, &L));
        return LDSR_OK;
    }
};

// Mstep (src/EM.cpp:139-229): the fit arrives from the caller, its X, V, J rows go straight into the device arrays
static int run_mstep(int device, const SeriesUpload &U, const int *cell_offsets, const double *X, const double *V,
                     const double *J, double *theta_out, int *status) {
    int rc = check_common(U.n_series, U.T, U.p, U.q, U.y, cell_offsets);
    if (rc || cell_offsets[U.n_series] == 0) return rc;
    if (!X || !V || !J || !theta_out) return fail(LDSR_EINVAL, "mstep needs X, V, J and theta");
    FitCall F;
    rc = F.begin(FIT_MSTEP, device, U, cell_offsets, nullptr);
    if (rc) return rc;
    SmoothParams sp;
    memset(&sp, 0, sizeof(sp));
    set_prepared_series(sp, F.U.ps);
    sp.n_cells = (int)F.n_cells; sp.series_of_cell = F.U.d_soc;
    sp.X = F.d.X; sp.V = F.d.V; sp.J = F.d.J; sp.status = F.d.status; sp.theta_out = F.d_theta_out;
    HIPCHK(hipMemcpyAsync(sp.X, X, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(sp.V, V, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(sp.J, J, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(launch_mstep(sp, F.U.ps.PP, F.U.ps.QQ, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(F.pout, F.d.lik, F.small_out, hipMemcpyDeviceToHost, F.U.ps.stream));
    HIPCHK(hipStreamSynchronize(F.U.ps.stream));
    memcpy(theta_out, F.host(F.d_theta_out), sizeof(double) * F.n_cells * (6 + U.p + U.q));
    if (status) memcpy(status, F.host(F.d.status), sizeof(int) * F.n_cells);
    return LDSR_OK;
}

// host: the caller's arrays, null where a row is not wanted (lik: for FIT_PENLIK the penalised likelihood).
// The scan kernel whitens the inputs by Svv / Tuu and flags a series where one of them is singular (fewer
// observations than columns of v, say) instead of answering, but Kalman_smoother needs neither: the cells of
// such a series then go through the serial smoother (serial: this call is that second pass), in a call of
// their own, so that a cell's result does not depend on what shares the call (LDS_GA does the same).
int run_fit_kernel(FitKind kind, int device, const SeriesUpload &U, const int *cell_offsets,
                   const double *theta, int stdlik, double lambda, const FitOut &host, bool serial) {
    int rc = check_common(U.n_series, U.T, U.p, U.q, U.y, cell_offsets);
    if (rc || cell_offsets[U.n_series] == 0) return rc;
    if (!theta || !host.lik) return fail(LDSR_EINVAL, "theta and lik must not be NULL");
    const int mode = kind == FIT_PROPAGATE ? 1 : 0;
    std::vector<int> redo;      // the series the scan kernel flagged
    {
        FitCall F;
        rc = F.begin(kind, device, U, cell_offsets, theta, serial);
        if (rc) return rc;
        const FitOut &d = F.d;
        const bool scan = !serial && smoother_is_scan(U.T, F.U.ps.PP, F.U.ps.QQ, F.L, mode);
        rc = serial ? smoother_enqueue(F.U.ps, (int)F.n_cells, SmootherTables(), F.U.d_soc, F.U.d_theta, stdlik, mode,
                                       lambda, d)
                    : launch_smoother(F.U.ps, (int)F.n_cells, F.U.h_soc, F.U.d_theta, stdlik, mode, lambda, d, F.U.d_soc);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(F.pout, d.lik, F.small_out, hipMemcpyDeviceToHost, F.U.ps.stream));
        HIPCHK(hipStreamSynchronize(F.U.ps.stream));
        memcpy(host.lik, F.host(d.pen ? d.pen : d.lik), sizeof(double) * F.n_cells);
        const int *st = (const int *)F.host(d.status);
        for (int s = 0; s < U.n_series && scan; s++)        // (singular is a fact of the series: its first cell tells)
            if (cell_offsets[s + 1] > cell_offsets[s] && st[cell_offsets[s]] == LDSR_CELL_SINGULAR) redo.push_back(s);
        if (!d.pen) {
            if (host.X) HIPCHK(hipMemcpy(host.X, d.X, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.Y) HIPCHK(hipMemcpy(host.Y, d.Y, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.V) HIPCHK(hipMemcpy(host.V, d.V, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.J) HIPCHK(hipMemcpy(host.J, d.J, F.row_bytes, hipMemcpyDeviceToHost));
        }
    }
    for (int s : redo) {
        const size_t c0 = (size_t)cell_offsets[s], uv = U.shared_uv ? 0 : (size_t)s * U.T;
        const int off1[2] = {0, cell_offsets[s + 1] - cell_offsets[s]};
        auto rows = [&](double *a) { return a ? a + c0 * U.T : nullptr; };
        rc = run_fit_kernel(kind, device,
                            SeriesUpload{1, U.T, U.p, U.q, U.y + (size_t)s * U.T, U.u ? U.u + uv * U.p : nullptr,
                                         U.v ? U.v + uv * U.q : nullptr, U.shared_uv},
                            off1, theta + c0 * (6 + U.p + U.q), stdlik, lambda,
                            FitOut{rows(host.X), rows(host.Y), rows(host.V), rows(host.J), host.lik + c0}, true);
        if (rc) return rc;
    }
    return LDSR_OK;
}

extern "C" int ldsr_smooth_batch(int device, int n_series, int T, int p, int q, const double *y,
                                 const double *u, const double *v, int shared_uv,
                                 const int *cell_offsets, const double *theta, int stdlik,
                                 double *X, double *Y, double *V, double *J, double *lik) {
    return run_fit_kernel(FIT_SMOOTH, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, stdlik, 0.0, FitOut{X, Y, V, J, lik});
}

extern "C" int ldsr_propagate_batch(int device, int n_series, int T, int p, int q, const double *y,
                                    const double *u, const double *v, int shared_uv,
                                    const int *cell_offsets, const double *theta, int stdlik,
                                    double *X, double *Y, double *V, double *lik) {
    return run_fit_kernel(FIT_PROPAGATE, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, stdlik, 0.0, FitOut{X, Y, V, nullptr, lik});
}

extern "C" int ldsr_penalized_lik_batch(int device, int n_series, int T, int p, int q,
                                        const double *y, const double *u, const double *v,
                                        int shared_uv, const int *cell_offsets, const double *theta,
                                        double lambda, double *pl) {
    return run_fit_kernel(FIT_PENLIK, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, 0, lambda, FitOut{nullptr, nullptr, nullptr, nullptr, pl});
}

extern "C" int ldsr_mstep_batch(int device, int n_series, int T, int p, int q, const double *y,
                                const double *u, const double *v, int shared_uv,
                                const int *cell_offsets, const double *X, const double *V,
                                const double *J, double *theta, int *status) {
    return run_mstep(device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, X, V, J, theta,
                     status);
}

}  // namespace ldsr_host
