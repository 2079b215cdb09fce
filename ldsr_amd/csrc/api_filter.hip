// api_filter.hip -- the Kalman filter's entries of the C ABI: ldsr_filter_batch,
// ldsr_filter_workspace_bytes and ldsr_filter_batch_device over filter.hip's kernel.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "host_series.h"
#include "filter.h"

namespace ldsr_host {

// the caller's eight rows in the header's order, Xp .. ll
struct FilterRows {
    double *r[8];
};
static void set_rows(FilterParams &fp, const FilterRows &rows) {
    fp.Xp = rows.r[0]; fp.Vp = rows.r[1]; fp.Yp = rows.r[2]; fp.Xu = rows.r[3];
    fp.Vu = rows.r[4]; fp.e = rows.r[5]; fp.Sv = rows.r[6]; fp.ll = rows.r[7];
}

// The argument checks of both entries; nothing is touched before they pass.
static int check_filter(int n_series, int T, int p, int q, const double *y, const int *cell_offsets, const double *theta,
                        int n_lags, const double *lik, const double *acf) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    if (!theta || !lik) return fail(LDSR_EINVAL, "theta and lik must not be NULL");
    if (n_lags < 0 || n_lags > LDSR_FILTER_MAX_LAGS)
        return fail(LDSR_EINVAL, "n_lags must be in 0 .. " + std::to_string(LDSR_FILTER_MAX_LAGS));
    if (n_lags >= T) return fail(LDSR_EINVAL, "n_lags must be smaller than T");
    if (n_lags > 0 && !acf) return fail(LDSR_EINVAL, "acf must not be NULL when n_lags > 0");
    return LDSR_OK;
}

extern "C" size_t ldsr_filter_workspace_bytes(int n_series, int T, int p, int q, int n_cells, int n_lags) {
    if (n_series < 1 || T < 2 || p < 1 || q < 1 || p > LDSR_MAXPQ || q > LDSR_MAXPQ || n_cells < 0) return 0;
    if (n_lags < 0 || n_lags > LDSR_FILTER_MAX_LAGS || n_lags >= T) return 0;
    return flt_ws_bytes(n_cells, T, n_lags);
}

extern "C" int ldsr_filter_batch_device(int device, void *stream_, int n_series, int T, int p, int q, const double *d_y,
                                        const double *d_u, const double *d_v, int shared_uv, const int *cell_offsets,
                                        const double *d_theta, int stdlik, int n_lags, double *d_Xp, double *d_Vp,
                                        double *d_Yp, double *d_Xu, double *d_Vu, double *d_e, double *d_S, double *d_ll,
                                        double *d_lik, double *d_zstat, double *d_acf, int *d_status, void *d_workspace,
                                        size_t workspace_bytes) {
    int rc = check_filter(n_series, T, p, q, d_y, cell_offsets, d_theta, n_lags, d_lik, d_acf);
    if (rc) return rc;
    const int n_cells = cell_offsets[n_series];
    if (n_cells == 0) return LDSR_OK;
    if (!d_workspace) return fail(LDSR_EINVAL, "workspace must not be NULL");
    const size_t need = flt_ws_bytes(n_cells, T, n_lags);
    if (workspace_bytes < need) return fail(LDSR_EINVAL, "workspace too small: need " + std::to_string(need) + " bytes");
    if (((size_t)d_workspace & 255) != 0) return fail(LDSR_EINVAL, "workspace must be 256-byte aligned");
    HIPCHK(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)d_workspace;
    // the cell -> series map travels through the pinned staging ring: the call only enqueues
    std::vector<int> soc((size_t)n_cells);
    for (int s = 0; s < n_series; s++)
        for (int c = cell_offsets[s]; c < cell_offsets[s + 1]; c++) soc[(size_t)c] = s;
    rc = stage_h2d_async(device, stream, ws, soc.data(), sizeof(int) * (size_t)n_cells);
    if (rc) return rc;
    FilterParams fp;
    fp.S = cell_series(n_cells, T, p, q, d_y, d_u, d_v, shared_uv, (const int *)ws, nullptr);
    fp.theta = d_theta; fp.stdlik = stdlik != 0; fp.n_lags = n_lags;
    set_rows(fp, FilterRows{{d_Xp, d_Vp, d_Yp, d_Xu, d_Vu, d_e, d_S, d_ll}});
    fp.lik = d_lik; fp.zstat = d_zstat; fp.acf = d_acf; fp.status = d_status;
    fp.z = n_lags > 0 ? (double *)(ws + flt_ws_soc_bytes(n_cells)) : nullptr;
    HIPCHK(launch_filter(fp, stream));
    return LDSR_OK;
}

// [series | map | theta] go up in one copy; [lik | zstat | acf | status] come back in one, each requested row in one.
extern "C" int ldsr_filter_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                                 const double *v, int shared_uv, const int *cell_offsets, const double *theta, int stdlik,
                                 int n_lags, double *Xp, double *Vp, double *Yp, double *Xu, double *Vu, double *e,
                                 double *S, double *ll, double *lik, double *zstat, double *acf, int *status) {
    int rc = check_filter(n_series, T, p, q, y, cell_offsets, theta, n_lags, lik, acf);
    if (rc) return rc;
    const size_t n_cells = (size_t)cell_offsets[n_series];
    if (n_cells == 0) return LDSR_OK;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    const FilterRows host{{Xp, Vp, Yp, Xu, Vu, e, S, ll}};
    const size_t row_bytes = sizeof(double) * n_cells * T;
    SeriesUpload U{n_series, T, p, q, y, u, v, shared_uv};
    Carver c;
    U.carve(c, cell_offsets, theta);
    const size_t in_bytes = c.o;
    const size_t o_lik = c.take(sizeof(double) * n_cells), o_zs = c.take(sizeof(double) * n_cells * 2);
    const size_t o_acf = c.take(sizeof(double) * n_cells * (size_t)n_lags), o_st = c.take(sizeof(int) * n_cells);
    const size_t small_out = c.o - o_lik;
    size_t o_row[8];
    for (int i = 0; i < 8; i++) o_row[i] = c.take(host.r[i] ? row_bytes : 0);
    const size_t o_z = c.take(flt_z_bytes((int)n_cells, T, n_lags));
    rc = arena_reserve(A, c, in_bytes + align256(small_out), "ldsr_filter_batch");
    if (rc) return rc;
    char *dev = A->dev, *pout = A->pin + in_bytes;
    U.stage(A);
    HIPCHK(hipMemcpyAsync(dev, A->pin, in_bytes, hipMemcpyHostToDevice, A->stream));
    FilterParams fp;
    fp.S = U.view(dev, nullptr);
    fp.theta = U.d_theta; fp.stdlik = stdlik != 0; fp.n_lags = n_lags;
    FilterRows d;
    for (int i = 0; i < 8; i++) d.r[i] = host.r[i] ? (double *)(dev + o_row[i]) : nullptr;
    set_rows(fp, d);
    fp.lik = (double *)(dev + o_lik); fp.zstat = (double *)(dev + o_zs);
    fp.acf = n_lags > 0 ? (double *)(dev + o_acf) : nullptr;
    fp.status = (int *)(dev + o_st);
    fp.z = n_lags > 0 ? (double *)(dev + o_z) : nullptr;
    HIPCHK(launch_filter(fp, A->stream));
    HIPCHK(hipMemcpyAsync(pout, dev + o_lik, small_out, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    memcpy(lik, pout, sizeof(double) * n_cells);
    if (zstat) memcpy(zstat, pout + (o_zs - o_lik), sizeof(double) * n_cells * 2);
    if (acf) memcpy(acf, pout + (o_acf - o_lik), sizeof(double) * n_cells * (size_t)n_lags);
    if (status) memcpy(status, pout + (o_st - o_lik), sizeof(int) * n_cells);
    for (int i = 0; i < 8; i++)
        if (host.r[i]) HIPCHK(hipMemcpy(host.r[i], d.r[i], row_bytes, hipMemcpyDeviceToHost));
    return LDSR_OK;
}

}  // namespace ldsr_host
