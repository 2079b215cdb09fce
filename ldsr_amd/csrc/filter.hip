// filter.hip -- the Kalman filter as an output: the one-step-ahead prediction, the
// filtered state, the innovation and its variance, the per-step likelihood terms, and the mean, variance and
// autocorrelations of the standardised innovations.
//
// One wave per (series, restart) cell; lane l of chunk ch owns step 64 ch + l, any T.  The pass is fwd_chunk of
// plgrad_lanes.h, the one plgrad.hip's pl_eval runs forward: Vp_t by the inclusive scan of the Riccati steps as 2 x 2 projective maps, then
// S_t, K_t, Vu_t of each lane's own step from its entry state with the reference's expressions; Xp_t by the
// affine scan with A (1 - K_t C); a carry between chunks.  Every requested row goes straight from the owning
// lane to memory (512 contiguous bytes per chunk).  lik is one wave sum at the end; zmean and zvar merge each
// chunk's moments into the running ones (filter.h).  The autocorrelations are a second pass: lane l reads z_t
// and z_{t+k} from the cell's strip of the workspace, which exists only when lags are asked for.
//
// Every product-sum is an explicit fma and contraction is off: a cell's numbers do not depend on which rows
// are requested, on where the cell sits in the batch or on stdlik (lik apart).
#include "filter.h"
#include "plgrad_lanes.h"     // cell_view, theta_lanes, fwd_chunk, wave_sum1, strip_sync
#include "../../include/ldsr_hip.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(64) void ldsr_filter_kernel(FilterParams prm) {
    const int lane = threadIdx.x;
    const int T = prm.S.T, P = 6 + prm.S.p + prm.S.q;
    const int n_chunks = plg_chunks(T);
    for (int cell = blockIdx.x; cell < prm.S.n_cells; cell += gridDim.x) {
        const CellView c = cell_view(prm.S, cell);
        const double xv = lane < P ? prm.theta[plg_row_at(cell, lane, P)] : 0.0;       // variable i of theta in lane i
        const ThetaLanes th = theta_lanes(c, xv);
        double *const zrow = prm.z ? prm.z + plg_row_at(cell, 0, T) : nullptr;

        // ---- the filter ----
        double ll_sum = 0.0;
        FltMoments mom = {0.0, 0.0, 0.0};
        double carry_V = th.V1, carry_X = th.mu1;
        for (int ch = 0; ch < n_chunks; ch++) {
            const FwdChunk fc = fwd_chunk(c, th, ch, lane, carry_V, carry_X);
            const int t = fc.t;
            const bool in = fc.in, obs = fc.obs;
            const PlgFwd &f = fc.f;
            const double z = flt_z(f, obs);
            if (in) {
                const size_t at = plg_row_at(cell, t, T);
                if (prm.Xp) prm.Xp[at] = fc.Xp;
                if (prm.Vp) prm.Vp[at] = fc.Vp;
                if (prm.Yp) prm.Yp[at] = flt_yp(th.co, fc.Xp, fc.dv);
                if (prm.Xu) prm.Xu[at] = f.Xu;
                if (prm.Vu) prm.Vu[at] = f.Vu;
                if (prm.e) prm.e[at] = obs ? f.d : NAN;
                if (prm.Sv) prm.Sv[at] = f.S;
                if (prm.ll) prm.ll[at] = flt_ll(f);
                if (zrow) zrow[t] = z;
                ll_sum += flt_ll(f);
            }
            // the chunk's moments of z, merged into the running ones (the same in every lane)
            const double cnt = (double)__popcll(__ballot(obs));
            const double sum_c = wave_sum1(obs ? z : 0.0);
            const double mean_c = cnt > 0.0 ? sum_c / cnt : 0.0;
            const double dev = obs ? z - mean_c : 0.0;
            mom = flt_moments_merge(mom, cnt, mean_c, wave_sum1(dev * dev));
        }
        const double lik_sum = wave_sum1(ll_sum);
        if (lane == 0) {
            prm.lik[plg_row_at(cell, 0, 1)] = prm.stdlik ? lik_sum / mom.n : lik_sum;
            if (prm.status) prm.status[plg_row_at(cell, 0, 1)] = isfinite(lik_sum) ? LDSR_CELL_OK : LDSR_CELL_NONFINITE;
            if (prm.zstat) {
                prm.zstat[plg_row_at(cell, 0, 2)] = mom.n > 0.0 ? mom.mean : NAN;
                prm.zstat[plg_row_at(cell, 1, 2)] = mom.M2 / mom.n;
            }
        }
        if (prm.n_lags <= 0) continue;

        // ---- the autocorrelations: pairs (t, t + k) with both steps observed, one mean and one denominator ----
        strip_sync();
        for (int k = 1; k <= prm.n_lags; k++) {
            double num = 0.0;
            bool any = false;
            for (int ch = 0; ch < n_chunks; ch++) {
                const int t = plg_fwd_step(ch, lane);
                if (t < T - k && isfinite(c.y[plg_y_at(0, t, T)]) && isfinite(c.y[plg_y_at(0, t + k, T)])) {
                    num = fma(zrow[t] - mom.mean, zrow[t + k] - mom.mean, num);
                    any = true;
                }
            }
            const double tot = wave_sum1(num);
            const bool pairs = __any(any);
            if (lane == 0) prm.acf[plg_row_at(cell, k - 1, prm.n_lags)] = (pairs && mom.M2 != 0.0) ? tot / mom.M2 : NAN;
        }
    }
}

hipError_t launch_filter(const FilterParams &prm, hipStream_t stream) {
    if (prm.S.n_cells <= 0) return hipSuccess;
    hipLaunchKernelGGL(ldsr_filter_kernel, dim3((unsigned)flt_waves(prm.S.n_cells)), dim3(64), 0, stream, prm);
    return hipGetLastError();
}
