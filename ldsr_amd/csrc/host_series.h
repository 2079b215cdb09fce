// host_series.h -- the series of a host-pointer call on their way to the device (api_fit.hip, api_ga.hip,
// api_bfgs.hip, api_filter.hip), the series side of a one-wave-per-cell launch, and api_fit.hip's smoother call for
// the learners' singular series.
#pragma once
#include <cstring>

#include "host_em.h"
#include "plgrad.h"                   // CellSeries

namespace ldsr_host {

// The series side of a one-wave-per-cell launch (bfgs.hip, plgrad.hip, filter.hip) from device pointers as they
// are: u / v null: absent; strip: the kernel's workspace or null.
inline CellSeries cell_series(int n_cells, int T, int p, int q, const double *d_y, const double *d_u, const double *d_v,
                              int shared_uv, const int *d_soc, double *d_strip) {
    CellSeries S;
    S.n_cells = n_cells; S.T = T; S.p = p; S.q = q;
    S.y = d_y; S.u = d_u; S.v = d_v;
    S.u_stride = shared_uv ? 0 : (long)T * p; S.v_stride = shared_uv ? 0 : (long)T * q;
    S.series_of_cell = d_soc; S.strip = d_strip;
    return S;
}

// ---- what the host-pointer entries of the smoother, GA and BFGS families share ----------------
// The series of a call as they cross the ABI (u, v null: absent) and their part of its input block: carve() takes
// y | u | v and, given cell_offsets, the cell -> series map and the theta rows; stage() fills them in the pinned
// block and says where the caller's ONE copy of its whole input block puts them on the device.
struct SeriesUpload {
    int n_series, T, p, q;
    const double *y, *u, *v;
    int shared_uv;
    const int *cell_offsets = nullptr;
    const double *theta = nullptr;      // (null with cell_offsets: the rows are reserved and go up as they are)
    size_t o_y = 0, o_u = 0, o_v = 0, o_soc = 0, o_th = 0;
    const double *d_y = nullptr, *d_u = nullptr, *d_v = nullptr, *d_theta = nullptr;
    int *d_soc = nullptr, *h_soc = nullptr;     // (h_soc: the staged map, for the block tables)
    PreparedSeries ps;                          // prep(): the series as series_prep leaves them
    size_t uv_bytes(const double *a, int k) const { return a ? sizeof(double) * (shared_uv ? 1 : (size_t)n_series) * T * k : 0; }
    void carve(Carver &c, const int *offsets = nullptr, const double *theta_rows = nullptr) {
        cell_offsets = offsets; theta = theta_rows;
        o_y = c.take(sizeof(double) * (size_t)n_series * T);
        o_u = c.take(uv_bytes(u, p));
        o_v = c.take(uv_bytes(v, q));
        if (!offsets) return;
        o_soc = c.take(sizeof(int) * (size_t)offsets[n_series]);
        o_th = c.take(sizeof(double) * (size_t)offsets[n_series] * (6 + p + q));
    }
    void stage(const Arena *A) {
        memcpy(A->pin + o_y, y, sizeof(double) * (size_t)n_series * T);
        if (u) memcpy(A->pin + o_u, u, uv_bytes(u, p));
        if (v) memcpy(A->pin + o_v, v, uv_bytes(v, q));
        d_y = (const double *)(A->dev + o_y);
        d_u = u ? (const double *)(A->dev + o_u) : nullptr;
        d_v = v ? (const double *)(A->dev + o_v) : nullptr;
        if (!cell_offsets) return;
        h_soc = (int *)(A->pin + o_soc); d_soc = (int *)(A->dev + o_soc); d_theta = (const double *)(A->dev + o_th);
        for (int s = 0; s < n_series; s++)
            for (int cc = cell_offsets[s]; cc < cell_offsets[s + 1]; cc++) h_soc[cc] = s;
        if (theta) memcpy(A->pin + o_th, theta, sizeof(double) * (size_t)cell_offsets[n_series] * (6 + p + q));
    }
    // ... and of the carved series with their cells in the call's block at dev (what stage() hands out as d_y, d_u,
    // d_v, d_soc; the offsets alone decide, so the extent check can ask before anything is staged)
    CellSeries view(char *dev, double *d_strip) const {
        return cell_series(cell_offsets[n_series], T, p, q, (const double *)(dev + o_y),
                           u ? (const double *)(dev + o_u) : nullptr, v ? (const double *)(dev + o_v) : nullptr, shared_uv,
                           (const int *)(dev + o_soc), d_strip);
    }
    // series_prep of the uploaded series into the workspace ws (layout *L)
    hipError_t prep(int device, hipStream_t stream, char *ws, const WsLayout *L) {
        ps = PreparedSeries{device, stream, T, p, q, ldsr_pad_dim(p), ldsr_pad_dim(q), shared_uv, u != nullptr, v != nullptr,
                            ws, L};
        return launch_series_prep(prep_params(n_series, T, p, q, ps.PP, ps.QQ, d_y, d_u, d_v, shared_uv, ws, *L, true),
                                  n_series, stream);
    }
};

enum FitKind { FIT_SMOOTH, FIT_PROPAGATE, FIT_MSTEP, FIT_PENLIK };     // (PENLIK: only lik - lambda * ssq leaves the device)
int run_fit_kernel(FitKind kind, int device, const SeriesUpload &U, const int *cell_offsets, const double *theta,
                   int stdlik, double lambda, const FitOut &host, bool serial = false);      // (api_fit.hip)

}  // namespace ldsr_host
