// plgrad.hip -- the penalised likelihood pl = lik - lambda ssq (R/LDS_GA.R:28-44) with its exact gradient on
// the device, and the L-BFGS learner on f = -pl (LDS_BFGS_with_update, R/LDS_GA.R:90-127; the optimiser is
// bfgs_impl.h, the specification INTEGRATION.md "The bound-constrained L-BFGS").
//
// One wave per (series, restart) cell, lane i holds variable i of theta.  The time recursions run over the
// wave in chunks of 64 steps with a carry between chunks; every one of them is an inclusive scan of maps
// under composition (DPP row shifts and broadcasts), affine maps for the means and the adjoints, 2 x 2
// projective maps with an exact power-of-two renormalisation for the variance.  The passes:
//   forward   Vp_t by the scan of the Riccati steps, then S_t, K_t, Vu_t of each lane's own step from its entry
//             state with the reference's expressions; Xp_t by the affine scan with A (1 - K_t C); d_t, Xu_t,
//             the likelihood terms, J_t and the source of Xs_t
//   pass 3    backward: Xs_t = J_t Xs_{t+1} + (Xu_t - J_t Xp_{t+1}), e_t, ssq -- a value-only evaluation ends here
//   pass 4    forward: a_t (adjoint of Xs_t), coefficient J_{t-1}; the adjoint of J_t
//   pass 5    backward: xp_t, then vp_t whose source needs xu_t of the same step; the parameter gradients
// What a later pass needs of a step lies in the wave's strip of the device workspace (plgrad.h).  The per-step
// arithmetic and every address are plgrad.h's host/device functions, the cross-lane part is plgrad_lanes.h.
//
// Every product-sum is an explicit fma and contraction is off: the value is the same with and without the
// gradient.
#include "plgrad.h"
#include "bfgs_impl.h"        // the optimiser
#include "plgrad_lanes.h"     // cell_view, theta_lanes, fwd_chunk, aff_scan, lane_below, strip_sync

#pragma clang fp contract(off)

#define MAXPQ LDSR_MAXPQ

// pl at the theta whose variable i sits in lane i (xv); with GRAD also d pl / d theta, variable i in lane i
// (0 in the lanes beyond P).  The value is the same in every lane.  st: the wave's strip [PLG_NSTRIP][T].
template <bool GRAD>
__device__ __forceinline__ double pl_eval(const CellView &c, double *const st, double lambda, double xv, int lane,
                                          double *g_out) {
    const int T = c.T, p = c.p, q = c.q;
    // (theta_lanes of plgrad_lanes.h written out: through the helper the register allocator reloads more spilled
    //  scalars in this unit, 41 v_readlane more, and ldsr_bfgs_update_kernel is 0.8 % slower at T = 813)
    const PlgCoef co = plg_coef(readlane_d(xv, 0), readlane_d(xv, 1 + p), readlane_d(xv, 2 + p + q),
                                readlane_d(xv, 3 + p + q));
    ThetaLanes th;
    th.co = co;
    th.mu1 = readlane_d(xv, 4 + p + q);
    th.V1 = readlane_d(xv, 5 + p + q);
#pragma unroll
    for (int k = 0; k < MAXPQ; k++) {
        th.Bk[k] = (c.u && k < p) ? readlane_d(xv, 1 + k) : 0.0;
        th.Dk[k] = (c.v && k < q) ? readlane_d(xv, 2 + p + k) : 0.0;
    }
    const int n_chunks = plg_chunks(T);

    // ---- forward: the filter ----
    double lik_terms = 0.0;
    {
        double carry_V = th.V1, carry_X = th.mu1;
        for (int ch = 0; ch < n_chunks; ch++) {
            const FwdChunk fc = fwd_chunk(c, th, ch, lane, carry_V, carry_X);
            const int t = fc.t;
            if (fc.in) {
                lik_terms += fc.f.lik_term;
                const PlgAff sm = plg_smooth_step(co, fc.f.Vu, fc.f.Xu, fc.Vp_next, fc.Xp_next, t == T - 1);
                st[plg_strip_at(PLG_J, t, T)] = sm.a;
                st[plg_strip_at(PLG_SRC, t, T)] = sm.b;
                st[plg_strip_at(PLG_BU, t, T)] = fc.bu;
                if (GRAD) {
                    st[plg_strip_at(PLG_VP, t, T)] = fc.Vp;
                    st[plg_strip_at(PLG_K, t, T)] = fc.f.K;
                    st[plg_strip_at(PLG_XP, t, T)] = fc.Xp;
                    st[plg_strip_at(PLG_D, t, T)] = fc.f.d;
                }
            }
        }
    }
    strip_sync();

    // ---- pass 3, backward: the smoothed means and ssq ----
    double ssq = 0.0;
    {
        double carry = 0.0;     // Xs of the step above the chunk (J = 0 at T - 1: never used there)
        for (int ch = n_chunks - 1; ch >= 0; ch--) {
            const int t = plg_rev_step(ch, lane);
            const bool in = t < T;
            PlgAff sm = plg_aff_identity();
            double bu = 0.0;
            if (in) {
                sm.a = st[plg_strip_at(PLG_J, t, T)];
                sm.b = st[plg_strip_at(PLG_SRC, t, T)];
                bu = st[plg_strip_at(PLG_BU, t, T)];
            }
            const double Xs = plg_aff_apply(aff_scan(sm), carry);
            const double Xs_next = lane_below(carry, Xs);
            carry = readlane_d(Xs, 63);
            if (in) {
                const double e = plg_resid(co, Xs, Xs_next, bu, t == T - 1);
                ssq = fma(e, e, ssq);
                if (GRAD) {
                    st[plg_strip_at(PLG_XS, t, T)] = Xs;
                    st[plg_strip_at(PLG_EB, t, T)] = -2.0 * lambda * e;
                }
            }
        }
    }
    double tot[2] = {lik_terms, ssq};
    wave_sum_n<2>(tot);
    const double pl = plg_value(tot[0], tot[1], lambda);
    strip_sync();           // (the next evaluation's forward pass overwrites what other lanes have just read)
    if (!GRAD) return pl;

    // ---- pass 4, forward: the adjoints of Xs_t and J_t ----
    {
        double carry = 0.0;
        for (int ch = 0; ch < n_chunks; ch++) {
            const int t = plg_fwd_step(ch, lane);
            const bool in = t < T;
            PlgAff ad = plg_aff_identity();
            if (in) {
                const double eb = st[plg_strip_at(PLG_EB, t, T)];
                const double J_prev = t > 0 ? st[plg_strip_at(PLG_J, t - 1, T)] : 0.0;
                const double eb_prev = t > 0 ? st[plg_strip_at(PLG_EB, t - 1, T)] : 0.0;
                ad = plg_adj_xs_step(co, J_prev, eb_prev, eb);
            }
            const double a = plg_aff_apply(aff_scan(ad), carry);
            carry = readlane_d(a, 63);
            if (in) {
                const bool last = t == T - 1;
                const double Xs_next = last ? 0.0 : st[plg_strip_at(PLG_XS, t + 1, T)];
                const double Xp_next = last ? 0.0 : st[plg_strip_at(PLG_XP, t + 1, T)];
                st[plg_strip_at(PLG_AB, t, T)] = a;
                st[plg_strip_at(PLG_JB, t, T)] = plg_adj_j(a, Xs_next, Xp_next, last);
            }
        }
    }
    strip_sync();

    // ---- pass 5, backward: the adjoints of Xp_t and Vp_t, the parameter gradients ----
    double red[4 + 2 * MAXPQ];      // A, Q, C, R, B_k, D_k
#pragma unroll
    for (int k = 0; k < 4 + 2 * MAXPQ; k++) red[k] = 0.0;
    double carry_xp = 0.0, carry_vp = 0.0;
    for (int ch = n_chunks - 1; ch >= 0; ch--) {
        const int t = plg_rev_step(ch, lane);
        const bool in = t < T;
        PlgBack b;
        b.obs = false; b.first = t == 0; b.last = t >= T - 1;
        b.Vp = 1.0; b.Vp_next = 1.0; b.K = 0.0; b.Xp = 0.0; b.d = 0.0; b.Xs = 0.0; b.eb = 0.0; b.a = 0.0; b.Jb = 0.0;
        b.back = 0.0; b.back_v = 0.0;
        if (in) {
            b.obs = isfinite(c.y[plg_y_at(0, t, T)]);
            b.Vp = st[plg_strip_at(PLG_VP, t, T)];
            b.K = st[plg_strip_at(PLG_K, t, T)];
            b.Xp = st[plg_strip_at(PLG_XP, t, T)];
            b.d = st[plg_strip_at(PLG_D, t, T)];
            b.Xs = st[plg_strip_at(PLG_XS, t, T)];
            b.eb = st[plg_strip_at(PLG_EB, t, T)];
            b.a = st[plg_strip_at(PLG_AB, t, T)];
            if (!b.last) {
                b.Vp_next = st[plg_strip_at(PLG_VP, t + 1, T)];
                b.Jb = st[plg_strip_at(PLG_JB, t, T)];
            }
            if (!b.first) {
                const double J_prev = st[plg_strip_at(PLG_J, t - 1, T)];
                b.back = J_prev * st[plg_strip_at(PLG_AB, t - 1, T)];
                b.back_v = st[plg_strip_at(PLG_JB, t - 1, T)] * J_prev / b.Vp;
            }
        }
        plg_back_derive(co, &b);
        const double xp = plg_aff_apply(aff_scan(in ? plg_adj_xp_step(co, b) : plg_aff_identity()), carry_xp);
        const double xp_next = lane_below(carry_xp, xp);
        carry_xp = readlane_d(xp, 63);
        const double xu = plg_adj_xu(co, b, xp_next);
        const double vp = plg_aff_apply(aff_scan(in ? plg_adj_vp_step(co, b, xu) : plg_aff_identity()), carry_vp);
        const double vp_next = lane_below(carry_vp, vp);
        carry_vp = readlane_d(vp, 63);
        if (in) {
            const PlgContrib g = plg_contrib(co, b, xu, plg_adj_vu(co, b, vp_next), xp_next, vp_next);
            red[0] += g.gA; red[1] += g.gQ; red[2] += g.gC; red[3] += g.gR;
            if (c.u) {
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < p) red[4 + k] = fma(g.fB, c.u[plg_uv_at(0, 0, t, p, k)], red[4 + k]);
            }
            if (c.v) {
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < q) red[4 + MAXPQ + k] = fma(g.fD, c.v[plg_uv_at(0, 0, t, q, k)], red[4 + MAXPQ + k]);
            }
        }
    }
    wave_sum_n<4 + 2 * MAXPQ>(red);
    double g = 0.0;
    if (lane == 0) g = red[0];
    if (lane == 1 + p) g = red[2];
    if (lane == 2 + p + q) g = red[1];
    if (lane == 3 + p + q) g = red[3];
    if (lane == 4 + p + q) g = carry_xp;       // d pl / d mu1 = xp_0
    if (lane == 5 + p + q) g = carry_vp;       // d pl / d V1 = vp_0
#pragma unroll
    for (int k = 0; k < MAXPQ; k++) {
        if (c.u && k < p && lane == 1 + k) g = red[4 + k];
        if (c.v && k < q && lane == 2 + p + k) g = red[4 + MAXPQ + k];
    }
    strip_sync();
    *g_out = g;
    return pl;
}

__global__ __launch_bounds__(64) void ldsr_pl_grad_kernel(PlGradParams prm) {
    const int lane = threadIdx.x;
    const int P = 6 + prm.S.p + prm.S.q;
    double *const st = prm.S.strip + plg_wave_strip((int)blockIdx.x, prm.S.T);
    for (int cell = blockIdx.x; cell < prm.S.n_cells; cell += gridDim.x) {
        const CellView c = cell_view(prm.S, cell);
        const double xv = lane < P ? prm.theta[plg_row_at(cell, lane, P)] : 0.0;
        double f, g = 0.0;
        if (prm.grad) f = pl_eval<true>(c, st, prm.lambda, xv, lane, &g);
        else f = pl_eval<false>(c, st, prm.lambda, xv, lane, nullptr);
        if (lane == 0) prm.pl[plg_row_at(cell, 0, 1)] = f;
        if (prm.grad && lane < P) prm.grad[plg_row_at(cell, lane, P)] = g;
    }
}

// f = -pl
struct NegPlObjective {
    CellView c;
    double *strip;
    double lambda;
    template <bool GRAD>
    __device__ __forceinline__ double eval(double x, int lane, double *g) const {
        double gp = 0.0;
        const double f = -pl_eval<GRAD>(c, strip, lambda, x, lane, GRAD ? &gp : nullptr);
        if (GRAD) *g = -gp;
        return f;
    }
};

// The optimiser (bfgs_impl.h) on -pl.
__global__ __launch_bounds__(64) void ldsr_bfgs_update_kernel(BfgsParams prm) {
    const int lane = threadIdx.x;
    const int P = 6 + prm.S.p + prm.S.q;
    const bool mine = lane < P;
    const double lo = mine ? prm.lb[lane] : 0.0, hi = mine ? prm.ub[lane] : 0.0;
    double *const st = prm.S.strip + plg_wave_strip((int)blockIdx.x, prm.S.T);
    for (int cell = blockIdx.x; cell < prm.S.n_cells; cell += gridDim.x) {
        const NegPlObjective obj{cell_view(prm.S, cell), st, prm.lambda};
        bfgs_cell(obj, prm, cell, P, lane, mine, lo, hi);
    }
}

hipError_t launch_pl_grad(const PlGradParams &prm, hipStream_t stream) {
    if (prm.S.n_cells <= 0) return hipSuccess;
    hipLaunchKernelGGL(ldsr_pl_grad_kernel, dim3((unsigned)plg_waves(prm.S.n_cells)), dim3(64), 0, stream, prm);
    return hipGetLastError();
}

hipError_t launch_bfgs_update(const BfgsParams &prm, hipStream_t stream) {
    if (prm.S.n_cells <= 0) return hipSuccess;
    hipLaunchKernelGGL(ldsr_bfgs_update_kernel, dim3((unsigned)plg_waves(prm.S.n_cells)), dim3(64), 0, stream, prm);
    return hipGetLastError();
}
