// bfgs.hip -- the L-BFGS learner on the device (LDS_BFGS, the reference's R/LDS_GA.R:155-184; the
// optimiser is this project's own specification, INTEGRATION.md "The bound-constrained L-BFGS").
//
// The objective is ssqTrain (R/LDS_GA.R:143-147) over propagate (src/EM.cpp:295-356):
//     x_1 = mu1,  x_{t+1} = A x_t + B u_t,  Y_t = C x_t + D v_t,  r_t = y_t - Y_t (0 where y_t is not
//     finite),  f = sum r_t^2,
// and its exact gradient comes from the adjoint recursion lam_t = -2 C r_t + A lam_{t+1} (lam_{T+1} = 0):
//     df/dC = -2 sum r_t x_t, df/dD_k = -2 sum r_t v_tk, df/dmu1 = lam_1,
//     df/dA = sum_{t<T} lam_{t+1} x_t, df/dB_k = sum_{t<T} lam_{t+1} u_tk, nothing for Q, R, V1.
//
// One wave per (series, restart) cell, one wave per workgroup: restarts stop after very different
// numbers of iterations, and a lone wave gives its LDS back the moment it is done.  In the vector
// algebra lane i owns variable i (P = 6 + p + q <= 38); the coefficients the time passes need come out
// of those lanes by v_readlane and stay in scalar registers.  In the forward pass lane l owns step
// 64 k + l of chunk k, and x over a chunk is the inclusive scan AffineScan of plgrad_lanes.h (DPP row
// shifts and broadcasts, one fma by a power of A per round).  The backward pass is the same scan run
// from the other end: it walks the chunks downwards with the lanes mirrored (lane l owns step
// 64 k + 63 - l), so lam_{t+1} is the lane below.  It needs x_t and r_t again: the forward pass leaves
// them in the wave's strip, 2 T doubles of LDS (T <= BFGS_LDS_MAX_T) or of a device workspace.
// The sums are wave reductions (the halving form of em_scan_impl.h).
//
// Every product-sum is an explicit fma and contraction is off, so the forward pass gives the same f
// with and without the gradient.
#include "bfgs.h"
#include "bfgs_impl.h"        // the optimiser; plgrad_lanes.h: cell_view, theta_lanes, AffineScan, wave_sum1

#pragma clang fp contract(off)

#define MAXPQ LDSR_MAXPQ

// f at the theta whose variable i sits in lane i (xv); with GRAD also the gradient, variable i in lane i
// (0 in the lanes beyond P).  Both results are the same in every lane resp. wave-uniform.
// strip: the wave's [2 T], x_t then r_t (GRAD only).
template <bool GRAD>
__device__ __forceinline__ double ssq_eval(const CellView &c, double *strip, double xv, int lane, double *g_out) {
    const int T = c.T, p = c.p, q = c.q;
    const ThetaLanes th = theta_lanes(c, xv);
    const double A = th.co.A, C = th.co.C, mu1 = th.mu1;
    const AffineScan scan(A, lane);

    double red[2 + MAXPQ];          // f, sum r x, sum r v_k
#pragma unroll
    for (int k = 0; k < 2 + MAXPQ; k++) red[k] = 0.0;
    double carry = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool in = t < T;
        double e = 0.0, dv = 0.0, yt = NAN;
        double vt[MAXPQ];
#pragma unroll
        for (int k = 0; k < MAXPQ; k++) vt[k] = 0.0;
        if (in) {
            if (t == 0) {
                e = mu1;
            } else if (c.u) {
                const double *ut = c.u + (size_t)(t - 1) * p;
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < p) e = fma(th.Bk[k], ut[k], e);
            }
            if (c.v) {
                const double *vr = c.v + (size_t)t * q;
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < q) {
                        vt[k] = vr[k];
                        dv = fma(th.Dk[k], vt[k], dv);
                    }
            }
            yt = c.y[t];
        }
        if (lane == 0) e = fma(A, carry, e);
        double x = scan.run(e);
        carry = readlane_d(x, 63);
        const bool obs = in && isfinite(yt);
        const double r = obs ? yt - fma(C, x, dv) : 0.0;
        red[0] = fma(r, r, red[0]);
        if (GRAD) {
            if (in) {
                strip[t] = x;
                strip[T + t] = r;
            }
            if (obs) {
                red[1] = fma(r, x, red[1]);
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < q) red[2 + k] = fma(r, vt[k], red[2 + k]);
            }
        }
    }
    if (!GRAD) return wave_sum1(red[0]);
    wave_sum_n<2 + MAXPQ>(red);
    const double f = red[0];
    double g = 0.0;
    if (lane == 1 + p) g = -2.0 * red[1];
    if (c.v) {
#pragma unroll
        for (int k = 0; k < MAXPQ; k++)
            if (k < q && lane == 2 + p + k) g = -2.0 * red[2 + k];
    }

    // the strip is written by one lane and read by another
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    double rb[1 + MAXPQ];           // sum lam_{t+1} x_t, sum lam_{t+1} u_tk
#pragma unroll
    for (int k = 0; k < 1 + MAXPQ; k++) rb[k] = 0.0;
    const double m2C = -2.0 * C;
    carry = 0.0;                    // lam_{T+1}
    for (int t0 = ((T - 1) >> 6) << 6; t0 >= 0; t0 -= 64) {
        const int t = t0 + 63 - lane;
        const bool in = t < T;
        double xt = 0.0, r = 0.0;
        if (in) {
            xt = strip[t];
            r = strip[T + t];
        }
        double e = m2C * r;
        if (lane == 0) e = fma(A, carry, e);
        const double lam = scan.run(e);
        const double lam_next = dppd<DPP_WAVE_SHR1, 0xF>(carry, lam);     // lam_{t+1}: the lane below, or the chunk above
        carry = readlane_d(lam, 63);
        if (t < T - 1) {
            rb[0] = fma(lam_next, xt, rb[0]);
            if (c.u) {
                const double *ut = c.u + (size_t)t * p;
#pragma unroll
                for (int k = 0; k < MAXPQ; k++)
                    if (k < p) rb[1 + k] = fma(lam_next, ut[k], rb[1 + k]);
            }
        }
    }
    wave_sum_n<1 + MAXPQ>(rb);
    if (lane == 0) g = rb[0];
    if (c.u) {
#pragma unroll
        for (int k = 0; k < MAXPQ; k++)
            if (k < p && lane == 1 + k) g = rb[1 + k];
    }
    if (lane == 4 + p + q) g = carry;      // lam_1
    // the next forward pass overwrites the strip other lanes have just read
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    *g_out = g;
    return f;
}

// the wave's strip: its [2 T] of the workspace, or of LDS where the launch has no workspace
__device__ __forceinline__ double *ssq_strip(const CellSeries &S, double *lds_strip) {
    return S.strip ? S.strip + (size_t)blockIdx.x * 2 * S.T : lds_strip;
}

__global__ __launch_bounds__(64) void ldsr_ssq_grad_kernel(SsqParams prm) {
    extern __shared__ double lds_strip[];
    const int lane = threadIdx.x;
    const int P = 6 + prm.S.p + prm.S.q;
    double *const strip = ssq_strip(prm.S, lds_strip);
    for (int cell = blockIdx.x; cell < prm.S.n_cells; cell += gridDim.x) {
        const CellView c = cell_view(prm.S, cell);
        const double xv = lane < P ? prm.theta[plg_row_at(cell, lane, P)] : 0.0;
        double f, g = 0.0;
        if (prm.grad) f = ssq_eval<true>(c, strip, xv, lane, &g);
        else f = ssq_eval<false>(c, strip, xv, lane, nullptr);
        if (lane == 0) prm.ssq[cell] = f;
        if (prm.grad && lane < P) prm.grad[plg_row_at(cell, lane, P)] = g;
    }
}

struct SsqObjective {
    CellView c;
    double *strip;
    template <bool GRAD>
    __device__ __forceinline__ double eval(double x, int lane, double *g) const {
        return ssq_eval<GRAD>(c, strip, x, lane, g);
    }
};

// The optimiser (bfgs_impl.h) on ssqTrain.
__global__ __launch_bounds__(64) void ldsr_bfgs_kernel(BfgsParams prm) {
    extern __shared__ double lds_strip[];
    const int lane = threadIdx.x;
    const int P = 6 + prm.S.p + prm.S.q;
    const bool mine = lane < P;
    const double lo = mine ? prm.lb[lane] : 0.0, hi = mine ? prm.ub[lane] : 0.0;
    double *const strip = ssq_strip(prm.S, lds_strip);
    for (int cell = blockIdx.x; cell < prm.S.n_cells; cell += gridDim.x) {
        const SsqObjective obj{cell_view(prm.S, cell), strip};
        bfgs_cell(obj, prm, cell, P, lane, mine, lo, hi);
    }
}

// One wave per series: the first largest (select_max) or first smallest finite value of its cells.
__global__ __launch_bounds__(64) void ldsr_bfgs_select_kernel(BfgsSelectParams prm) {
    const int s = blockIdx.x, lane = threadIdx.x, P = prm.P;
    const int c0 = prm.cell_offsets[s], c1 = prm.cell_offsets[s + 1];
    double bv = 0.0;
    int bi = -1;
    for (int cc = c0 + lane; cc < c1; cc += 64) {
        const double f = prm.value[cc];
        if (isfinite(f) && (bi < 0 || (prm.select_max ? f > bv : f < bv))) { bv = f; bi = cc; }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (oi >= 0 && (bi < 0 || (prm.select_max ? ov > bv : ov < bv) || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        prm.winner[s] = bi;
        prm.value_w[s] = bi >= 0 ? bv : NAN;
    }
    if (lane < P) prm.theta_w[(size_t)s * P + lane] = bi >= 0 ? prm.par[(size_t)bi * P + lane] : NAN;
}

int bfgs_waves(int n_cells, int T) {
    // in LDS mode the hardware hands out cells as waves retire; the workspace mode bounds its strip
    return T <= BFGS_LDS_MAX_T ? n_cells : (n_cells < 2048 ? n_cells : 2048);
}

static size_t bfgs_lds_bytes(int T) { return T <= BFGS_LDS_MAX_T ? sizeof(double) * 2 * (size_t)T : 0; }

hipError_t launch_ssq_grad(const SsqParams &prm, hipStream_t stream) {
    if (prm.S.n_cells <= 0) return hipSuccess;
    hipLaunchKernelGGL(ldsr_ssq_grad_kernel, dim3((unsigned)bfgs_waves(prm.S.n_cells, prm.S.T)), dim3(64),
                       prm.grad ? bfgs_lds_bytes(prm.S.T) : 0, stream, prm);
    return hipGetLastError();
}

hipError_t launch_bfgs(const BfgsParams &prm, hipStream_t stream) {
    if (prm.S.n_cells <= 0) return hipSuccess;
    hipLaunchKernelGGL(ldsr_bfgs_kernel, dim3((unsigned)bfgs_waves(prm.S.n_cells, prm.S.T)), dim3(64),
                       bfgs_lds_bytes(prm.S.T), stream, prm);
    return hipGetLastError();
}

hipError_t launch_bfgs_select(const BfgsSelectParams &prm, hipStream_t stream) {
    hipLaunchKernelGGL(ldsr_bfgs_select_kernel, dim3((unsigned)prm.n_series), dim3(64), 0, stream, prm);
    return hipGetLastError();
}
