// pcr.hip -- batched principal-component regression: the reference's benchmark model, R/PCR.R.
//
// One cell = one (member m, fold f): fit y ~ 1 + X_m on the rows fold f does not hold out and whose y is
// finite (one_pcr_cv, R/PCR.R:101-107: X2 <- X[-z, ], .lm.fit(X2, y2); lm's na.omit :49, :76), then
// x_t' beta for the rows of a prediction matrix (:106 the member's own rows, :50 / :77 the whole record).
//
// One wavefront per cell, one cell per workgroup.  The fit is a Householder QR of [1 X_m | y] without
// pivoting, the method class of .lm.fit (LINPACK dqrdc2 / dqrsl), NOT the normal equations: a Householder
// step rewrites the columns it has not reached yet, so a cell needs a mutable copy of its design -- its
// training rows, compacted, live in LDS (column-major, row i of every column is read and written by lane
// i & 63 only; n (kmax + 2) doubles, which is what bounds n: pcr.h PCR_MAX_WORK).  Staging X_m once for
// the folds of a member would add a second copy and save reads that hit L2 anyway, so there is none.
//   step j:  s = |a_j[j:]|^2                                     one wave reduction
//            v = a_j[j:] - beta e_1, beta = -sign(a_jj) sqrt(s)   (no cancellation in v_1)
//            d_c = v' a_c[j:] for every column c > j and y        one batched wave reduction (wave_sum_n)
//            a_c[j:] -= (d_c / (sqrt(s) (sqrt(s) + |a_jj|))) v
// Every reduction has a fixed tree and a cell touches nothing another cell writes, so a cell's result does
// not depend on what else is in the call.  The rank rule is .lm.fit's tolerance as a flag: a column whose
// remaining norm is <= 1e-7 of its original norm (or fewer training rows than columns) makes the cell
// LDSR_CELL_SINGULAR with NaN outputs, where dqrdc2 would move the column to the end.
// After the QR: R in the upper triangle, Q'y in y's column, beta by back substitution in every lane,
// RSS = |(Q'y)[k+1:]|^2, and for the prediction sweep lanes run over the rows with beta and R broadcast
// from LDS: pred_t = x_t' beta, leverage h_t = |R^-T x_t|^2 by forward substitution.
#include "pcr.h"

#include "../../include/ldsr_hip.h"
#include "em_scan_impl.h"     // wave_sum_n, uniform_d

// LDS written by one lane of the wave is read by another
__device__ __forceinline__ void pcr_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// KP: compiled number of design columns (intercept included), K = k + 1 <= KP of them live
template <int KP>
__device__ __forceinline__ void pcr_cell(const PcrParams &prm, int m, int f, int k, double *W, int lane) {
    const int n = prm.n, K = k + 1, ld = n;
    const size_t cell = (size_t)m * prm.n_folds + f;
    double *osq = W + (size_t)ld * (prm.kmax + 2);        // [KP] squared original norms of the columns
    const long long coff = prm.coff[m];
    const double *Xm = prm.X + (size_t)coff * n;
    const unsigned char *ho = prm.heldout + (size_t)f * n;
    const double *Xp = prm.Xpred ? prm.Xpred + (size_t)coff * prm.N : Xm;
    const int Np = prm.Xpred ? prm.N : n;
    double *ycol = W + (size_t)K * ld;

    // training rows, compacted in their order: column c of row pos at W[c ld + pos], y in column K
    int nt = 0;
    double sq[KP];
#pragma unroll
    for (int c = 0; c < KP; c++) sq[c] = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        double yi = 0.0;
        bool tr = false;
        if (i < n) {
            yi = prm.y[i];
            tr = ho[i] == 0 && isfinite(yi);
        }
        const unsigned long long mask = __ballot(tr);
        const int pos = nt + __popcll(mask & ((1ull << lane) - 1ull));
        if (tr) {
            W[pos] = 1.0;
            sq[0] += 1.0;
#pragma unroll
            for (int c = 1; c < KP; c++)
                if (c < K) {
                    const double x = Xm[(size_t)(c - 1) * n + i];
                    W[(size_t)c * ld + pos] = x;
                    sq[c] = fma(x, x, sq[c]);
                }
            ycol[pos] = yi;
        }
        nt += __popcll(mask);
    }
    const int df = nt - K;
    bool sing = nt < K;
    if (!sing) {
        wave_sum_n<KP>(sq);
#pragma unroll
        for (int c = 0; c < KP; c++)
            if (lane == c) osq[c] = sq[c];
    }

    for (int j = 0; j < K && !sing; j++) {
        pcr_wave_sync();
        double *aj = W + (size_t)j * ld;
        const int i00 = j & ~63;
        double s1[1] = {0.0};
        for (int i0 = i00; i0 < nt; i0 += 64) {
            const int i = i0 + lane;
            if (i >= j && i < nt) {
                const double x = aj[i];
                s1[0] = fma(x, x, s1[0]);
            }
        }
        wave_sum_n<1>(s1);
        const double s = uniform_d(s1[0]), nrm = sqrt(s);
        if (!(nrm > 1e-7 * sqrt(osq[j]))) {       // (NaN and an all-zero column land here too)
            sing = true;
            break;
        }
        const double alpha = uniform_d(aj[j]);
        const double bet = alpha >= 0.0 ? -nrm : nrm;
        const double vj = alpha - bet;
        const double tau = 1.0 / (nrm * (nrm + fabs(alpha)));     // 2 / v'v
        double d[KP];
#pragma unroll
        for (int c = 0; c < KP; c++) d[c] = 0.0;
        for (int i0 = i00; i0 < nt; i0 += 64) {
            const int i = i0 + lane;
            if (i >= j && i < nt) {
                const double v = i == j ? vj : aj[i];
#pragma unroll
                for (int c = 1; c <= KP; c++)
                    if (c > j && c <= K) d[c - 1] = fma(v, W[(size_t)c * ld + i], d[c - 1]);
            }
        }
        wave_sum_n<KP>(d);
        for (int i0 = i00; i0 < nt; i0 += 64) {
            const int i = i0 + lane;
            if (i >= j && i < nt) {
                const double v = i == j ? vj : aj[i];
#pragma unroll
                for (int c = 1; c <= KP; c++)
                    if (c > j && c <= K) {
                        double *w = W + (size_t)c * ld + i;
                        *w = fma(-(tau * d[c - 1]), v, *w);
                    }
                if (i == j) aj[j] = bet;          // R_jj
            }
        }
    }
    pcr_wave_sync();

    if (lane == 0) {
        prm.status[cell] = sing ? LDSR_CELL_SINGULAR : LDSR_CELL_OK;
        if (prm.df) prm.df[cell] = df;
    }
    if (sing) {
        if (lane == 0 && prm.sigma) prm.sigma[cell] = NAN;
        if (prm.coef && lane < PCR_COEF_STRIDE) prm.coef[cell * PCR_COEF_STRIDE + lane] = NAN;
        for (int t = lane; t < Np; t += 64) {
            prm.pred[cell * Np + t] = NAN;
            if (prm.lev) prm.lev[cell * Np + t] = NAN;
        }
        return;
    }

    if (prm.sigma) {
        double r1[1] = {0.0};
        for (int i = K + lane; i < nt; i += 64) r1[0] = fma(ycol[i], ycol[i], r1[0]);
        wave_sum_n<1>(r1);
        if (lane == 0) prm.sigma[cell] = df > 0 ? sqrt(r1[0] / (double)df) : NAN;
    }

    // R beta = (Q'y)[0:K], the same in every lane
    double b[KP];
#pragma unroll
    for (int r = KP - 1; r >= 0; r--) {
        b[r] = 0.0;
        if (r < K) {
            double acc = ycol[r];
#pragma unroll
            for (int c = r + 1; c < KP; c++)
                if (c < K) acc = fma(-W[(size_t)c * ld + r], b[c], acc);
            b[r] = acc / W[(size_t)r * ld + r];
        }
    }
    if (prm.coef) {
        double mine = NAN;
#pragma unroll
        for (int r = 0; r < KP; r++)
            if (lane == r && r < K) mine = b[r];
        if (lane < PCR_COEF_STRIDE) prm.coef[cell * PCR_COEF_STRIDE + lane] = mine;
    }

    for (int t = lane; t < Np; t += 64) {
        double x[KP];
        x[0] = 1.0;
        double p = b[0];
#pragma unroll
        for (int c = 1; c < KP; c++) {
            x[c] = 0.0;
            if (c < K) {
                x[c] = Xp[(size_t)(c - 1) * Np + t];
                p = fma(x[c], b[c], p);
            }
        }
        prm.pred[cell * Np + t] = p;
        if (prm.lev) {                 // R' z = x_t
            double h = 0.0;
#pragma unroll
            for (int r = 0; r < KP; r++)
                if (r < K) {
                    double acc = x[r];
#pragma unroll
                    for (int c = 0; c < r; c++) acc = fma(-W[(size_t)r * ld + c], x[c], acc);
                    x[r] = acc / W[(size_t)r * ld + r];      // (x[0..r] now holds z)
                    h = fma(x[r], x[r], h);
                }
            prm.lev[cell * Np + t] = h;
        }
    }
}

__global__ __launch_bounds__(64) void ldsr_pcr_kernel(PcrParams prm) {
    extern __shared__ __attribute__((aligned(16))) double pcr_work[];
    const int lane = threadIdx.x;
    const int cell = blockIdx.x, m = cell / prm.n_folds, f = cell - m * prm.n_folds;
    const int k = prm.k[m];
    if (k <= 1) pcr_cell<2>(prm, m, f, k, pcr_work, lane);
    else if (k <= 3) pcr_cell<4>(prm, m, f, k, pcr_work, lane);
    else if (k <= 8) pcr_cell<9>(prm, m, f, k, pcr_work, lane);
    else pcr_cell<PCR_MAXK + 1>(prm, m, f, k, pcr_work, lane);
}

size_t pcr_lds_bytes(int n, int kmax) { return sizeof(double) * ((size_t)n * (kmax + 2) + PCR_AUX); }

hipError_t launch_pcr(const PcrParams &prm, hipStream_t stream) {
    const size_t lds = pcr_lds_bytes(prm.n, prm.kmax);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)ldsr_pcr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ldsr_pcr_kernel, dim3((unsigned)(prm.n_members * prm.n_folds)), dim3(64), lds, stream, prm);
    return hipGetLastError();
}
