// filter.h -- the Kalman filter's own outputs: what src/EM.cpp:43-90,115-120 computes
// as Xp, Vp, Yp, Xu, Vu, delta, Sigma and discards, the per-step likelihood terms and the statistics of the
// standardised innovations.  What filter.hip's kernel and its host unit (api_filter.hip) share.
//
// The per-step arithmetic is plgrad.h's (plg_mob_step, plg_var_step, plg_mean_step, plg_fwd_step_values): the
// forward pass of the penalised likelihood, kept this time.  This file adds what that pass never formed and the
// addresses of the rows; all of it inline host/device functions, so it can be run on a CPU.
#pragma once
#include "plgrad.h"

#pragma clang fp contract(off)

#define FLT_MAX_WAVES (1 << 20)       // waves (= workgroups) of a launch at most; a wave takes cells blockIdx.x, + gridDim.x, ...

// (element i of a cell's row of a [n_cells][T] output, of acf [n_cells][n_lags], of zstat [n_cells][2]: plg_row_at)
PLG_HD int flt_waves(int n_cells) { return n_cells < FLT_MAX_WAVES ? n_cells : FLT_MAX_WAVES; }

// ---- the workspace of ldsr_filter_batch_device: [series_of_cell | z] -------------------------------------------
PLG_HD size_t flt_align256(size_t x) { return (x + 255) & ~(size_t)255; }
PLG_HD size_t flt_ws_soc_bytes(int n_cells) { return flt_align256(sizeof(int) * (size_t)(n_cells > 0 ? n_cells : 1)); }
// the strip of standardised innovations, [n_cells][T]: the lag pass reads z_{t+k} of another lane (and chunk)
PLG_HD size_t flt_z_bytes(int n_cells, int T, int n_lags) {
    return n_lags > 0 ? flt_align256(sizeof(double) * plg_rows_doubles(n_cells > 0 ? n_cells : 1, T)) : 0;
}
PLG_HD size_t flt_ws_bytes(int n_cells, int T, int n_lags) { return flt_ws_soc_bytes(n_cells) + flt_z_bytes(n_cells, T, n_lags); }

struct FilterParams {
    CellSeries S;                     // (S.strip is not used)
    const double *theta;              // [n_cells][P]
    int stdlik, n_lags;
    double *Xp, *Vp, *Yp, *Xu, *Vu, *e, *Sv, *ll;     // [n_cells][T] each, or null: not written
    double *lik;                      // [n_cells]
    double *zstat;                    // [n_cells][2] (zmean, zvar) or null
    double *acf;                      // [n_cells][n_lags]; null exactly when n_lags == 0
    int *status;                      // [n_cells] or null
    double *z;                        // [n_cells][T]; null exactly when n_lags == 0
};

// ---- what the forward step adds to plg_fwd_step_values -----------------------------------------------------------
// Yp_t = C Xp_t + D.v_t
PLG_HD double flt_yp(const PlgCoef &c, double Xp, double dv) { return fma(c.C, Xp, dv); }
// ll_t = -1/2 (log 2 pi + log S_t + e_t^2 / S_t), 0 where y_t is missing (lik_term is 0 there)
PLG_HD double flt_ll(const PlgFwd &f) { return -0.5 * f.lik_term; }
// z_t = e_t / sqrt(S_t); NaN where y_t is missing, as e_t
PLG_HD double flt_z(const PlgFwd &f, bool obs) { return obs ? f.d / sqrt(f.S) : NAN; }

// The running mean and sum of squared deviations of the observed z: (n, mean, M2) of the steps so far takes in
// (cnt, mean_c, M2_c) of a chunk (the pairwise update of Chan, Golub and LeVeque: no cancellation, any T).
struct FltMoments {
    double n, mean, M2;
};
PLG_HD FltMoments flt_moments_merge(const FltMoments &a, double cnt, double mean_c, double M2_c) {
    if (cnt == 0.0) return a;
    const double n = a.n + cnt, delta = mean_c - a.mean;
    return FltMoments{n, fma(delta, cnt / n, a.mean), a.M2 + fma(delta * delta, a.n * cnt / n, M2_c)};
}

#if defined(__HIPCC__)
hipError_t launch_filter(const FilterParams &prm, hipStream_t stream);
#endif
