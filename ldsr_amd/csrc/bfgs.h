// bfgs.h -- launch interface of the L-BFGS learner (bfgs.hip): LDS_BFGS, R/LDS_GA.R:155-184, by the
// specification in INTEGRATION.md ("The bound-constrained L-BFGS").  Included by bfgs.hip, by plgrad.hip
// (through bfgs_impl.h: the optimiser's parameter block is the same for both objectives) and by api_bfgs.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "plgrad.h"                   // CellSeries

#define BFGS_MAX_LMM 8                // curvature pairs a wave can keep (lmm <= this)
#define BFGS_LS_TRIALS 20             // line-search trials at most
#define BFGS_LDS_MAX_T 4096           // 2 T doubles fit the 64 KiB of one workgroup up to here

struct SsqParams {
    CellSeries S;                     // S.strip: [n_waves][2 T] where T > BFGS_LDS_MAX_T (else null: LDS)
    const double *theta;              // [n_cells][P]
    double *ssq;                      // [n_cells]
    double *grad;                     // [n_cells][P] or null
};

// The optimiser's launch, on ssqTrain (launch_bfgs; S.strip as in SsqParams) or on -pl at lambda
// (launch_bfgs_update, plgrad.h; S.strip as in PlGradParams).
struct BfgsParams {
    CellSeries S;
    const double *par0;               // [n_cells][P]
    const double *lb, *ub;            // [P]
    double lambda;                    // (ssqTrain ignores it)
    int maxit, lmm;
    double ftol, pgtol;               // ftol = factr * 2^-52
    const int *intr;                  // host-pinned interrupt flag, or null (not part of the call's block)
    double *par, *value;              // [n_cells][P], [n_cells]: the minimised ssq resp. -pl
    int *n_iter, *n_eval, *status;    // [n_cells]
};

struct BfgsSelectParams {
    int n_series, P, select_max;
    const int *cell_offsets;          // [n_series + 1], on the device
    const double *par, *value;
    int *winner;                      // [n_series] global cell index or -1
    double *theta_w, *value_w;        // [n_series][P], [n_series] (NaN rows without a winner)
};

// waves (= workgroups) a launch over n_cells cells uses; the strip is [bfgs_waves(..)][2 T] doubles
int bfgs_waves(int n_cells, int T);
hipError_t launch_ssq_grad(const SsqParams &prm, hipStream_t stream);
hipError_t launch_bfgs(const BfgsParams &prm, hipStream_t stream);
hipError_t launch_bfgs_select(const BfgsSelectParams &prm, hipStream_t stream);
