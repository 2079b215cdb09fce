// bfgs_impl.h -- the bound-constrained L-BFGS of INTEGRATION.md ("The bound-constrained L-BFGS") as a device
// function over an objective: one wave runs one cell's optimisation from its start point to a stop rule.
// The objective is a type with
//     template <bool GRAD> double eval(double x, int lane, double *g) const
// -- f at the point whose variable i sits in lane i (the same in every lane) and, with GRAD, variable i of
// the gradient in lane i (0 in the lanes beyond P).  Instantiated for ssqTrain (bfgs.hip: LDS_BFGS) and for
// the negative penalised likelihood (plgrad.hip: LDS_BFGS_with_update).
#pragma once
#include "bfgs.h"
#include "plgrad_lanes.h"     // wave_sum1; em_scan_impl.h: wave_sum_n
#include "../../include/ldsr_hip.h"

#pragma clang fp contract(off)

__device__ __forceinline__ double wave_max1(double x) {      // x >= 0 or NaN; NaN in any lane gives NaN
    bool bad = x != x;
    for (int d = 32; d >= 1; d >>= 1) x = fmax(x, __shfl_xor(x, d, 64));
    return __any(bad) ? NAN : x;
}

// One cell.  prm: the launch's parameters (par0, lb / ub as lo / hi of this lane, maxit, lmm, ftol, pgtol, intr
// and the per-cell outputs par, value, n_iter, n_eval, status); mine: lane < P.
template <class Obj>
__device__ __forceinline__ void bfgs_cell(const Obj &obj, const BfgsParams &prm, int cell, int P, int lane, bool mine,
                                          double lo, double hi) {
    const double x_in = mine ? prm.par0[(size_t)cell * P + lane] : 0.0;
    double x = fmin(fmax(x_in, lo), hi);
    double g = 0.0;
    double f = obj.template eval<true>(x, lane, &g);
    int n_eval = 1, k = 0, status = LDSR_BFGS_MAXIT;
    if (!isfinite(f)) {
        if (mine) prm.par[(size_t)cell * P + lane] = x_in;
        if (lane == 0) {
            prm.value[cell] = NAN;
            prm.n_iter[cell] = 0;
            prm.n_eval[cell] = n_eval;
            prm.status[cell] = LDSR_BFGS_NONFINITE;
        }
        return;
    }
    double sh[BFGS_MAX_LMM], yh[BFGS_MAX_LMM];      // curvature pairs, newest first
#pragma unroll
    for (int j = 0; j < BFGS_MAX_LMM; j++) { sh[j] = 0.0; yh[j] = 0.0; }
    int cnt = 0;
    for (;;) {
        // the active set and the projected gradient
        const bool active = !mine || lo == hi || (x <= lo && g > 0.0) || (x >= hi && g < 0.0);
        const double pg = active ? 0.0 : g;
        const double pgn = wave_max1(fabs(pg));
        if (pgn <= prm.pgtol) { status = LDSR_BFGS_CONVERGED; break; }
        if (k >= prm.maxit) { status = LDSR_BFGS_MAXIT; break; }
        if (prm.intr && (k & 7) == 0 && *(const volatile int *)prm.intr != 0) { status = LDSR_BFGS_INTERRUPTED; break; }

        // the direction: two-loop recursion over the pairs restricted to the free variables
        double d = -pg;
        if (cnt > 0) {
            double sy_yy[2 * BFGS_MAX_LMM];
#pragma unroll
            for (int j = 0; j < BFGS_MAX_LMM; j++) {
                const double sj = active ? 0.0 : sh[j], yj = active ? 0.0 : yh[j];
                sy_yy[2 * j] = sj * yj;
                sy_yy[2 * j + 1] = yj * yj;
            }
            wave_sum_n<2 * BFGS_MAX_LMM>(sy_yy);
            double al[BFGS_MAX_LMM];
            double qv = pg, gamma = 1.0;
            bool have_gamma = false;
#pragma unroll
            for (int j = 0; j < BFGS_MAX_LMM; j++) {
                al[j] = 0.0;
                const double sy = sy_yy[2 * j], yy = sy_yy[2 * j + 1];
                if (j < cnt && sy > 2.2e-16 * yy) {
                    al[j] = wave_sum1(active ? 0.0 : sh[j] * qv) / sy;
                    if (!active) qv = fma(-al[j], yh[j], qv);
                    if (!have_gamma) { gamma = sy / yy; have_gamma = true; }
                }
            }
            qv *= gamma;
#pragma unroll
            for (int j = BFGS_MAX_LMM - 1; j >= 0; j--) {
                const double sy = sy_yy[2 * j], yy = sy_yy[2 * j + 1];
                if (j < cnt && sy > 2.2e-16 * yy) {
                    const double be = wave_sum1(active ? 0.0 : yh[j] * qv) / sy;
                    if (!active) qv = fma(al[j] - be, sh[j], qv);
                }
            }
            d = active ? 0.0 : -qv;
        }
        double gd = wave_sum1(g * d);
        if (cnt > 0 && !(gd < 0.0)) {       // not a descent direction: steepest descent, memory cleared
            cnt = 0;
            d = -pg;
            gd = wave_sum1(g * d);
        }

        // projected backtracking
        double alpha = k == 0 ? fmin(1.0, 1.0 / pgn) : 1.0;
        double xt = x, ft = f;
        bool ok = false;
        for (int trial = 0; trial < BFGS_LS_TRIALS; trial++) {
            xt = fmin(fmax(fma(alpha, d, x), lo), hi);
            ft = obj.template eval<false>(xt, lane, nullptr);
            n_eval++;
            const double slope = wave_sum1(g * (xt - x));
            if (isfinite(ft) && ft <= fma(1e-4, slope, f)) { ok = true; break; }
            alpha *= 0.5;
        }
        if (!ok) { status = LDSR_BFGS_LINESEARCH; break; }

        // the gradient at the accepted point, the new pair, the stop rule
        double gt = 0.0;
        ft = obj.template eval<true>(xt, lane, &gt);
        n_eval++;
        const double sv = xt - x, yv = gt - g;
        double pr[2] = {sv * yv, yv * yv};
        wave_sum_n<2>(pr);
        if (pr[0] > 2.2e-16 * pr[1]) {
#pragma unroll
            for (int j = BFGS_MAX_LMM - 1; j > 0; j--) { sh[j] = sh[j - 1]; yh[j] = yh[j - 1]; }
            sh[0] = sv;
            yh[0] = yv;
            cnt = min(cnt + 1, prm.lmm);
        }
        const double drop = (f - ft) / fmax(fmax(fabs(f), fabs(ft)), 1.0);
        x = xt; f = ft; g = gt;
        k++;
        if (drop <= prm.ftol) { status = LDSR_BFGS_CONVERGED; break; }
    }
    if (mine) prm.par[(size_t)cell * P + lane] = x;
    if (lane == 0) {
        prm.value[cell] = f;
        prm.n_iter[cell] = k;
        prm.n_eval[cell] = n_eval;
        prm.status[cell] = status;
    }
}
