// pcr.h -- launch interface of the batched principal-component regression (pcr.hip), the reference's
// R/PCR.R: one_pcr_cv :101-107 for every (member, fold) cell and the lm / predict of PCR_reconstruction
// :49-50, :76-77.
#pragma once
#include <hip/hip_runtime.h>

#define PCR_MAXK 16            // columns of a member at most (LDSR_MAXPQ)
#define PCR_COEF_STRIDE 17     // coef row of a cell: intercept + PCR_MAXK slopes, NaN beyond k + 1
// LDS of a cell: its own copy of the training rows of [1 X_m y], n (kmax + 2) doubles, and PCR_AUX more
#define PCR_AUX 64
#define PCR_MAX_WORK 18432     // n (kmax + 2) at most: 144 KiB + the aux words of the CU's 160 KiB

struct PcrParams {
    int n_members, n, n_folds, N, kmax;
    const int *k;                   // [n_members]
    const long long *coff;          // [n_members] columns in front of member m (sum of k[0..m))
    const double *X;                // member blocks [n x k_m] column-major, concatenated
    const double *y;                // [n]
    const unsigned char *heldout;   // [n_folds][n] 0 / 1
    const double *Xpred;            // member blocks [N x k_m] column-major, or null: predict X's own rows (N = n)
    double *pred;                   // [n_members][n_folds][N]
    double *lev;                    // likewise, or null
    double *coef;                   // [n_members][n_folds][PCR_COEF_STRIDE], or null
    double *sigma;                  // [n_members][n_folds], or null
    int *df;                        // likewise, or null
    int *status;                    // likewise
};

size_t pcr_lds_bytes(int n, int kmax);
hipError_t launch_pcr(const PcrParams &prm, hipStream_t stream);
