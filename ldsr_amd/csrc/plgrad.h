// plgrad.h -- the penalised likelihood pl = lik - lambda ssq of LDS_BFGS_with_update (R/LDS_GA.R:90-127) and
// its exact gradient: what plgrad.hip's kernels, its host code and the stand-alone host program of the tests
// (tests/plgrad_host/main.cpp) share.  The quantities and recurrences are those of tests/plgrad_model.py.
// Its series descriptor (CellSeries), the addresses of the series and of the per-cell rows and the extent check
// serve every one-wave-per-cell kernel: bfgs.h, filter.h and host_series.h include this file for them.
//
// Everything a kernel computes per step and every address it forms is an inline host/device function of
// this file, so the addressing can be walked and the arithmetic run on a CPU.  This file includes nothing
// else of the project.
//
// Time is 0-based.  Forward passes give lane l of chunk k step 64 k + l, backward passes step 64 k + 63 - l
// (the mirrored mapping: the step above is the lane below, so one scan serves both directions).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLG_HD __host__ __device__ inline
#else
#define PLG_HD inline
#endif

#pragma clang fp contract(off)

#define PLG_LOG_2PI 1.8378770664093453
#define PLG_MAX_WAVES 2048            // waves (= workgroups) of a launch at most: bounds the strip

// ---- the strip: [n_waves][PLG_NSTRIP][T] doubles of device workspace ------------------------------------
// Arrays of a wave's strip.  A pass may reuse the slot of an array no later pass reads: the lane that
// reads step t of the old array is the lane that writes step t of the new one.
enum {
    PLG_J = 0,        // J_t (0 at T-1)                                   forward pass
    PLG_SRC = 1,      // Xu_t - J_t Xp_{t+1}: the source of Xs_t          forward pass (value and gradient)
    PLG_XS = 1,       // Xs_t                                             pass 3, over PLG_SRC
    PLG_BU = 2,       // B.u_t                                            forward pass
    PLG_EB = 2,       // -2 lambda e_t, the adjoint of e_t (0 at T-1)     pass 3, over PLG_BU
    PLG_VP = 3,       // Vp_t                                             forward pass, gradient only from here on
    PLG_K = 4,        // K_t (0 where y_t is missing)
    PLG_XP = 5,       // Xp_t
    PLG_D = 6,        // d_t (0 where y_t is missing)
    PLG_AB = 7,       // a_t, the adjoint of Xs_t                         pass 4
    PLG_JB = 8,       // the adjoint of J_t (0 at T-1)                    pass 4
    PLG_NSTRIP = 9
};

PLG_HD size_t plg_strip_doubles(int T) { return (size_t)PLG_NSTRIP * (size_t)T; }
PLG_HD size_t plg_strip_at(int k, int t, int T) { return (size_t)k * (size_t)T + (size_t)t; }
PLG_HD size_t plg_wave_strip(int wave, int T) { return (size_t)wave * plg_strip_doubles(T); }
PLG_HD int plg_waves(int n_cells) { return n_cells < PLG_MAX_WAVES ? n_cells : PLG_MAX_WAVES; }
PLG_HD int plg_chunks(int T) { return (T + 63) / 64; }
PLG_HD int plg_fwd_step(int chunk, int lane) { return 64 * chunk + lane; }
PLG_HD int plg_rev_step(int chunk, int lane) { return 64 * chunk + 63 - lane; }

// ---- the series and the per-cell rows ---------------------------------------------------------------------
PLG_HD size_t plg_y_at(int s, int t, int T) { return (size_t)s * (size_t)T + (size_t)t; }
// u / v are time-major [.][T][k]; stride: doubles between two series (0: shared by all)
PLG_HD size_t plg_uv_at(int s, long stride, int t, int k, int j) {
    return (size_t)s * (size_t)stride + (size_t)t * (size_t)k + (size_t)j;
}
PLG_HD size_t plg_row_at(int cell, int i, int P) { return (size_t)cell * (size_t)P + (size_t)i; }

// The series side of a one-wave-per-cell launch (bfgs.hip, plgrad.hip, filter.hip): cell c belongs to series
// series_of_cell[c].
struct CellSeries {
    int n_cells, T, p, q;
    const double *y;                  // [n_series][T], NaN / +-Inf = missing
    const double *u, *v;              // time-major [.][T][p] / [.][T][q], or null: absent
    long u_stride, v_stride;          // doubles between two series (0: shared by all)
    const int *series_of_cell;        // [n_cells]
    double *strip;                    // the waves' workspace, as the kernel lays it out (null: it has none)
};

// doubles behind each pointer that a launch over n_series series / n_cells cells can touch: one past the
// largest index the functions above give
PLG_HD size_t plg_y_doubles(int n_series, int T) { return plg_y_at(n_series - 1, T - 1, T) + 1; }
PLG_HD size_t plg_uv_doubles(int n_series, long stride, int T, int k) {
    return plg_uv_at(n_series - 1, stride, T - 1, k, k - 1) + 1;
}
PLG_HD size_t plg_rows_doubles(int n_cells, int P) { return plg_row_at(n_cells - 1, P - 1, P) + 1; }
PLG_HD size_t plg_launch_strip_doubles(int n_cells, int T) {
    return plg_wave_strip(plg_waves(n_cells) - 1, T) + plg_strip_doubles(T);
}

// ---- the parameter structs of the kernels -----------------------------------------------------------------
struct PlGradParams {
    CellSeries S;                     // S.strip: [plg_waves(n_cells)][PLG_NSTRIP][T]
    const double *theta;              // [n_cells][P]
    double lambda;
    double *pl;                       // [n_cells]
    double *grad;                     // [n_cells][P] or null
};

// One device pointer of a launch: the bytes the kernel touches behind it (need), the bytes the host reserved
// for it (have), and whether the kernel dereferences it unconditionally.
struct PlgExtent {
    const char *name;
    const void *ptr;
    size_t need, have;
    int required;
};
#define PLG_MAX_EXTENTS 16

PLG_HD int plg_series_extents(const CellSeries &S, int n_series, const size_t *have, PlgExtent *e) {
    // have: bytes reserved for y, u, v, series_of_cell, strip (the strip of the pl kernels)
    int n = 0;
    e[n++] = PlgExtent{"y", S.y, sizeof(double) * plg_y_doubles(n_series, S.T), have[0], 1};
    e[n++] = PlgExtent{"u", S.u, sizeof(double) * plg_uv_doubles(n_series, S.u_stride, S.T, S.p), have[1], 0};
    e[n++] = PlgExtent{"v", S.v, sizeof(double) * plg_uv_doubles(n_series, S.v_stride, S.T, S.q), have[2], 0};
    e[n++] = PlgExtent{"series_of_cell", S.series_of_cell, sizeof(int) * (size_t)S.n_cells, have[3], 1};
    e[n++] = PlgExtent{"strip", S.strip, sizeof(double) * plg_launch_strip_doubles(S.n_cells, S.T), have[4], 1};
    return n;
}

// Index of the first extent that is null though required, larger than what was reserved for it, or not
// inside the block [base, base + block_bytes); -1 when every extent is fine.
PLG_HD int plg_first_bad_extent(const PlgExtent *e, int n, const void *base, size_t block_bytes) {
    const char *b = (const char *)base;
    for (int i = 0; i < n; i++) {
        const char *p = (const char *)e[i].ptr;
        if (!p) {
            if (e[i].required) return i;
            continue;
        }
        if (e[i].need > e[i].have) return i;
        if (p < b || (size_t)(p - b) > block_bytes || e[i].need > block_bytes - (size_t)(p - b)) return i;
    }
    return -1;
}

// ---- the arithmetic of one step ----------------------------------------------------------------------------
// what every pass needs of theta
struct PlgCoef {
    double A, C, Q, R, A2, C2;
};
PLG_HD PlgCoef plg_coef(double A, double C, double Q, double R) { return PlgCoef{A, C, Q, R, A * A, C * C}; }

// x -> a x + b
struct PlgAff {
    double a, b;
};
PLG_HD PlgAff plg_aff_identity() { return PlgAff{1.0, 0.0}; }
// second after first
PLG_HD PlgAff plg_aff_then(const PlgAff &first, const PlgAff &second) {
    return PlgAff{second.a * first.a, fma(second.a, first.b, second.b)};
}
PLG_HD double plg_aff_apply(const PlgAff &f, double x) { return fma(f.a, x, f.b); }

// V -> (m00 V + m01) / (m10 V + m11): a step of the Riccati recursion Vp_t -> Vp_{t+1}
struct PlgMob {
    double m00, m01, m10, m11;
};
PLG_HD PlgMob plg_mob_identity() { return PlgMob{1.0, 0.0, 0.0, 1.0}; }
// observed: Vp' = A^2 Vp R / (C^2 Vp + R) + Q; missing: the same map with C = 0, Vp' = A^2 Vp + Q
PLG_HD PlgMob plg_mob_step(const PlgCoef &c, bool obs) {
    if (!obs) return PlgMob{c.A2, c.Q, 0.0, 1.0};
    return PlgMob{fma(c.A2, c.R, c.Q * c.C2), c.Q * c.R, c.C2, c.R};
}
PLG_HD int plg_exponent(double x) {      // of frexp; 0 for 0, NaN and +-Inf
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_frexp_exp(x);
#else
    int e = 0;
    if (x == x && fabs(x) <= 1.7976931348623157e308) frexp(x, &e);
    return e;
#endif
}
// second after first, scaled by the power of two that brings the largest entry into [1/2, 1): exact
PLG_HD PlgMob plg_mob_then(const PlgMob &first, const PlgMob &second) {
    PlgMob r;
    r.m00 = fma(second.m00, first.m00, second.m01 * first.m10);
    r.m01 = fma(second.m00, first.m01, second.m01 * first.m11);
    r.m10 = fma(second.m10, first.m00, second.m11 * first.m10);
    r.m11 = fma(second.m10, first.m01, second.m11 * first.m11);
    const int e = -plg_exponent(fmax(fmax(fabs(r.m00), fabs(r.m01)), fmax(fabs(r.m10), fabs(r.m11))));
    r.m00 = ldexp(r.m00, e);
    r.m01 = ldexp(r.m01, e);
    r.m10 = ldexp(r.m10, e);
    r.m11 = ldexp(r.m11, e);
    return r;
}
PLG_HD double plg_mob_apply(const PlgMob &m, double V) { return fma(m.m00, V, m.m01) / fma(m.m10, V, m.m11); }

// the forward step t from its entry state (Vp_t, Xp_t), with the reference's expressions
struct PlgFwd {
    double S, K, Vu, d, Xu;
    double lik_term;      // log 2 pi + log S_t + d_t^2 / S_t (0 where y_t is missing)
};
PLG_HD void plg_var_step(const PlgCoef &c, double Vp, bool obs, double *S, double *K, double *Vu) {
    *S = fma(c.C2, Vp, c.R);
    *K = obs ? Vp * c.C / *S : 0.0;
    *Vu = fma(-*K, c.C, 1.0) * Vp;
}
// Xp_t -> Xp_{t+1} = A (1 - K_t C) Xp_t + A K_t (y_t - D.v_t) + B.u_t   (ymdv = y_t - D.v_t, 0 where missing)
PLG_HD PlgAff plg_mean_step(const PlgCoef &c, double K, double ymdv, double bu) {
    return PlgAff{c.A * fma(-K, c.C, 1.0), fma(c.A * K, ymdv, bu)};
}
PLG_HD PlgFwd plg_fwd_step_values(const PlgCoef &c, double Vp, double Xp, bool obs, double ymdv) {
    PlgFwd f;
    plg_var_step(c, Vp, obs, &f.S, &f.K, &f.Vu);
    f.d = obs ? fma(-c.C, Xp, ymdv) : 0.0;
    f.Xu = fma(f.K, f.d, Xp);
    f.lik_term = obs ? PLG_LOG_2PI + log(f.S) + f.d * f.d / f.S : 0.0;
    return f;
}
// J_t and the source of Xs_t = J_t Xs_{t+1} + src_t; the last step has J = 0, Xs = Xu
PLG_HD PlgAff plg_smooth_step(const PlgCoef &c, double Vu, double Xu, double Vp_next, double Xp_next, bool last) {
    if (last) return PlgAff{0.0, Xu};
    const double J = Vu * c.A / Vp_next;
    return PlgAff{J, fma(-J, Xp_next, Xu)};
}
// e_t = Xs_{t+1} - A Xs_t - B.u_t (0 at the last step)
PLG_HD double plg_resid(const PlgCoef &c, double Xs, double Xs_next, double bu, bool last) {
    return last ? 0.0 : fma(-c.A, Xs, Xs_next) - bu;
}
PLG_HD double plg_value(double lik_terms, double ssq, double lambda) { return fma(-lambda, ssq, -0.5 * lik_terms); }

// pass 4: a_t = J_{t-1} a_{t-1} + (eb_{t-1} - A eb_t); J_prev = eb_prev = 0 at t = 0
PLG_HD PlgAff plg_adj_xs_step(const PlgCoef &c, double J_prev, double eb_prev, double eb) {
    return PlgAff{J_prev, fma(-c.A, eb, eb_prev)};
}
PLG_HD double plg_adj_j(double a, double Xs_next, double Xp_next, bool last) { return last ? 0.0 : a * (Xs_next - Xp_next); }

// pass 5, step t.  What the step holds of the forward pass and of pass 4:
struct PlgBack {
    bool obs, first, last;
    double Vp, Vp_next, K, Xp, d, Xs, eb, a, Jb;     // (Vp_next, Jb: unused at the last step)
    double back;          // J_{t-1} a_{t-1}: what a_{t-1} takes out of xp_t (0 at t = 0)
    double back_v;        // Jb_{t-1} J_{t-1} / Vp_t (0 at t = 0)
    double S, Vu, Xu, omk, jterm;     // derived: plg_back_derive
};
PLG_HD void plg_back_derive(const PlgCoef &c, PlgBack *b) {
    double K;
    plg_var_step(c, b->Vp, b->obs, &b->S, &K, &b->Vu);
    b->Xu = fma(b->K, b->d, b->Xp);
    b->omk = fma(-b->K, c.C, 1.0);
    b->jterm = b->last ? 0.0 : b->Jb * c.A / b->Vp_next;
}
// xp_t = A (1 - K_t C) xp_{t+1} + (1 - K_t C) a_t + [obs] C d_t / S_t - J_{t-1} a_{t-1}
PLG_HD PlgAff plg_adj_xp_step(const PlgCoef &c, const PlgBack &b) {
    const double o = b.obs ? c.C * b.d / b.S : 0.0;
    return PlgAff{c.A * b.omk, fma(b.omk, b.a, o) - b.back};
}
PLG_HD double plg_adj_xu(const PlgCoef &c, const PlgBack &b, double xp_next) { return fma(c.A, xp_next, b.a); }
// vp_t = (A (1 - K_t C))^2 vp_{t+1} + (1 - K_t C)^2 jterm_t
//        + [obs] ((C / S_t)(1 - K_t C) d_t xu_t - C^2 / 2 (1 / S_t - d_t^2 / S_t^2)) - Jb_{t-1} J_{t-1} / Vp_t
PLG_HD PlgAff plg_adj_vp_step(const PlgCoef &c, const PlgBack &b, double xu) {
    const double am = c.A * b.omk;
    double src = b.omk * b.omk * b.jterm;
    if (b.obs) {
        const double h = -0.5 * (1.0 / b.S - b.d * b.d / (b.S * b.S));
        src += fma(c.C / b.S * b.omk * b.d, xu, c.C2 * h);
    }
    return PlgAff{am * am, src - b.back_v};
}
PLG_HD double plg_adj_vu(const PlgCoef &c, const PlgBack &b, double vp_next) { return fma(c.A2, vp_next, b.jterm); }

// the step's share of d pl / d (A, Q, C, R) and the factors of u_t and v_t in d pl / d (B, D)
struct PlgContrib {
    double gA, gQ, gC, gR, fB, fD;
};
PLG_HD PlgContrib plg_contrib(const PlgCoef &c, const PlgBack &b, double xu, double vu, double xp_next,
                              double vp_next) {
    PlgContrib g = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!b.last) {
        g.gA = fma(-b.Xs, b.eb, b.Jb * b.Vu / b.Vp_next) + fma(xp_next, b.Xu, 2.0 * c.A * b.Vu * vp_next);
        g.fB = xp_next - b.eb;
        g.gQ = vp_next;
    }
    if (b.obs) {
        const double Kb = fma(xu, b.d, -(c.C * b.Vp * vu));
        const double Sb = -0.5 * (1.0 / b.S - b.d * b.d / (b.S * b.S)) - Kb * b.K / b.S;
        const double db = fma(b.K, xu, -b.d / b.S);
        g.gC = fma(-b.K * b.Vp, vu, Kb * b.Vp / b.S) + fma(-db, b.Xp, 2.0 * c.C * b.Vp * Sb);
        g.fD = -db;
        g.gR = Sb;
    }
    return g;
}

// ---- launch interface (plgrad.hip) ------------------------------------------------------------------------
#if defined(__HIPCC__)
struct BfgsParams;                    // (bfgs.h)
hipError_t launch_pl_grad(const PlGradParams &prm, hipStream_t stream);
hipError_t launch_bfgs_update(const BfgsParams &prm, hipStream_t stream);
#endif
