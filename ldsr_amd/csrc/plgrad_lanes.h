// plgrad_lanes.h -- the device part every one-wave-per-cell kernel shares: a wave's view of its cell, theta out
// of the lanes, inclusive scans over the 64 lanes of a wavefront by DPP row shifts and broadcasts (no LDS) -- of
// plgrad.h's maps and of x -> A x + e with one A for all lanes --, the value of the lane below, the sum of a value
// over the wave, the fence between two passes over a wave's strip, and one chunk of the Kalman filter.  Included
// by bfgs_impl.h (so by bfgs.hip: ssqTrain, and plgrad.hip: the penalised likelihood, its gradient and the L-BFGS
// learner on it), filter.hip (the Kalman filter's outputs) and simulate.hip (the replicates).  Device code only.
#pragma once
#include "plgrad.h"
#include "em_scan_impl.h"     // dppz / dppd, readlane_d, wave_sum_n

#pragma clang fp contract(off)

// one wave's view of its cell: the rows of the cell's series (u, v null: absent)
struct CellView {
    const double *y, *u, *v;
    int T, p, q;
};
__device__ __forceinline__ CellView cell_view(const CellSeries &S, int cell) {
    const int s = S.series_of_cell[plg_row_at(cell, 0, 1)];
    CellView c;
    c.T = S.T; c.p = S.p; c.q = S.q;
    c.y = S.y + plg_y_at(s, 0, S.T);
    c.u = S.u ? S.u + plg_uv_at(s, S.u_stride, 0, S.p, 0) : nullptr;
    c.v = S.v ? S.v + plg_uv_at(s, S.v_stride, 0, S.q, 0) : nullptr;
    return c;
}

// theta out of the lanes (variable i sits in lane i of xv) into scalars; B_k, D_k are 0 where u, v is absent
struct ThetaLanes {
    PlgCoef co;
    double mu1, V1, Bk[LDSR_MAXPQ], Dk[LDSR_MAXPQ];
};
__device__ __forceinline__ ThetaLanes theta_lanes(const CellView &c, double xv) {
    const int p = c.p, q = c.q;
    ThetaLanes th;
    th.co = plg_coef(readlane_d(xv, 0), readlane_d(xv, 1 + p), readlane_d(xv, 2 + p + q), readlane_d(xv, 3 + p + q));
    th.mu1 = readlane_d(xv, 4 + p + q);
    th.V1 = readlane_d(xv, 5 + p + q);
#pragma unroll
    for (int k = 0; k < LDSR_MAXPQ; k++) {
        th.Bk[k] = (c.u && k < p) ? readlane_d(xv, 1 + k) : 0.0;
        th.Dk[k] = (c.v && k < q) ? readlane_d(xv, 2 + p + k) : 0.0;
    }
    return th;
}

template <int CTRL, int RM>
__device__ __forceinline__ PlgAff aff_from(const PlgAff &x) {       // identity where the DPP source does not exist
    return PlgAff{dppd<CTRL, RM>(1.0, x.a), dppd<CTRL, RM>(0.0, x.b)};
}
// inclusive scan over the lanes: lane l gets (map of lane l) after ... after (map of lane 0)
__device__ __forceinline__ PlgAff aff_scan(PlgAff x) {
    x = plg_aff_then(aff_from<DPP_ROW_SHR(1), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(2), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(4), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(8), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_BCAST15, 0xA>(x), x);          // lane 15 -> row 1, lane 47 -> row 3
    x = plg_aff_then(aff_from<DPP_ROW_BCAST31, 0xC>(x), x);          // lane 31 -> rows 2, 3
    return x;
}

// the same scan where every lane's map has the multiplier A: x_l = A x_{l-1} + e_l, one fma by a power of A per
// round -- A^1, A^2, A^4, A^8 (row shifts), A^((l & 15) + 1) and A^((l & 31) + 1) (the row broadcasts)
struct AffineScan {
    double A, A2, A4, A8, P16, P32;
    __device__ __forceinline__ AffineScan(double A_, int lane) : A(A_) {
        A2 = A * A; A4 = A2 * A2; A8 = A4 * A4;
        const double A16 = A8 * A8;
        P16 = A;
        if (lane & 1) P16 *= A;
        if (lane & 2) P16 *= A2;
        if (lane & 4) P16 *= A4;
        if (lane & 8) P16 *= A8;
        P32 = (lane & 16) ? P16 * A16 : P16;
    }
    __device__ __forceinline__ double run(double x) const {
        x = fma(A, dppz<DPP_ROW_SHR(1)>(x), x);
        x = fma(A2, dppz<DPP_ROW_SHR(2)>(x), x);
        x = fma(A4, dppz<DPP_ROW_SHR(4)>(x), x);
        x = fma(A8, dppz<DPP_ROW_SHR(8)>(x), x);
        x = fma(P16, dppd<DPP_ROW_BCAST15, 0xA>(0.0, x), x);    // lane 15 -> row 1, lane 47 -> row 3
        x = fma(P32, dppd<DPP_ROW_BCAST31, 0xC>(0.0, x), x);    // lane 31 -> rows 2, 3
        return x;
    }
};

template <int CTRL, int RM>
__device__ __forceinline__ PlgMob mob_from(const PlgMob &x) {
    return PlgMob{dppd<CTRL, RM>(1.0, x.m00), dppd<CTRL, RM>(0.0, x.m01), dppd<CTRL, RM>(0.0, x.m10),
                  dppd<CTRL, RM>(1.0, x.m11)};
}
__device__ __forceinline__ PlgMob mob_scan(PlgMob x) {
    x = plg_mob_then(mob_from<DPP_ROW_SHR(1), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(2), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(4), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(8), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_BCAST15, 0xA>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_BCAST31, 0xC>(x), x);
    return x;
}

// the value of the lane below (the step before in a forward pass, the step above in a backward one); lane 0
// gets the carry of the chunk before
__device__ __forceinline__ double lane_below(double carry, double x) { return dppd<DPP_WAVE_SHR1, 0xF>(carry, x); }

// the sum of x over the wave, the same in every lane
__device__ __forceinline__ double wave_sum1(double x) {
    double a[1] = {x};
    wave_sum_n<1>(a);
    return a[0];
}

// a wave's strip is written by one lane and read by another in the next pass
__device__ __forceinline__ void strip_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// One chunk of the Kalman filter: lane l takes step t = 64 ch + l (in: t < T) from its entry state (Vp, Xp) to its
// exit state (Vp_next, Xp_next).  carry_V / carry_X: the state at the chunk's entry (V1 / mu1 before chunk 0), at
// its exit on return.
struct FwdChunk {
    int t;
    bool in, obs;                 // obs: y_t is there and finite
    double bu, dv;                // B.u_t, D.v_t
    double Vp, Xp, Vp_next, Xp_next;
    PlgFwd f;
};
__device__ __forceinline__ FwdChunk fwd_chunk(const CellView &c, const ThetaLanes &th, int ch, int lane, double &carry_V,
                                              double &carry_X) {
    const int T = c.T, p = c.p, q = c.q;
    FwdChunk r;
    r.t = plg_fwd_step(ch, lane);
    r.in = r.t < T;
    r.bu = 0.0;
    r.dv = 0.0;
    double yt = NAN;
    if (r.in) {
        if (c.u) {
#pragma unroll
            for (int k = 0; k < LDSR_MAXPQ; k++)
                if (k < p) r.bu = fma(th.Bk[k], c.u[plg_uv_at(0, 0, r.t, p, k)], r.bu);
        }
        if (c.v) {
#pragma unroll
            for (int k = 0; k < LDSR_MAXPQ; k++)
                if (k < q) r.dv = fma(th.Dk[k], c.v[plg_uv_at(0, 0, r.t, q, k)], r.dv);
        }
        yt = c.y[plg_y_at(0, r.t, T)];
    }
    r.obs = r.in && isfinite(yt);
    const double ymdv = r.obs ? yt - r.dv : 0.0;
    // the variance: Vp at the exit of every step, then each lane's own step from its entry state
    const PlgMob m = mob_scan(r.in ? plg_mob_step(th.co, r.obs) : plg_mob_identity());
    r.Vp_next = plg_mob_apply(m, carry_V);
    r.Vp = lane_below(carry_V, r.Vp_next);
    carry_V = readlane_d(r.Vp_next, 63);
    double S, K, Vu;
    plg_var_step(th.co, r.Vp, r.obs, &S, &K, &Vu);
    // the mean
    const PlgAff a = aff_scan(r.in ? plg_mean_step(th.co, K, ymdv, r.bu) : plg_aff_identity());
    r.Xp_next = plg_aff_apply(a, carry_X);
    r.Xp = lane_below(carry_X, r.Xp_next);
    carry_X = readlane_d(r.Xp_next, 63);
    r.f = plg_fwd_step_values(th.co, r.Vp, r.Xp, r.obs, ymdv);
    return r;
}
