// simulate.hip -- stochastic replicates of a fitted LDS model (one_LDS_rep / LDS_rep, the
// reference's R/stochastics.R:18-63):
//     x_1 ~ N(0, V1),  x_{t+1} = A x_t + B u_t + q_t,  y_t = C x_t + D v_t + r_t,
//     simQ_t = exp(y_t + mu)  (or y_t + mu),  q_t ~ N(0, Q), r_t ~ N(0, R).
//
// One wave per (model, replicate); lane l handles step t = 64 k + l of chunk k.  Every lane forms
// its own increment e_t = B u_{t-1} + q_{t-1} (e_0 = x_1) and observation offset D v_t + r_t,
// then x over the chunk is an inclusive affine scan x_l = A x_{l-1} + e_l by DPP row shifts and
// broadcasts (A is the same in every lane, so each round is one fma by a power of A); the chunk's
// entry state is lane 63 of the previous chunk.  Uniform reads, input reads and the three output
// rows of a chunk are 512-byte coalesced.
//
// Normals follow R's default normal.kind = "Inversion" (nmath snorm.c): two uniforms u1, u2 ->
// p = ((int)(2^27 u1) + u2) / 2^27 -> qnorm(p) (AS 241).  The uniforms come from the caller in R's
// consumption order (R-stream mode: the result equals set.seed(k); LDS_rep(...)) or from SplitMix64
// of (seed, model, replicate, position) (counter mode: a pure function of the arguments, whatever
// the launch geometry or the split of replicates over calls).  Both modes index the uniforms of a
// replicate by the same positions: [x_1] [q_1 .. q_T] [r_1 .. r_T], two per draw, and a draw R
// does not make (zero, NaN, negative or infinite variance) takes no position (sim_draws).
//
// The scan multiplies by A^1 .. A^32: for |A| beyond ~1e9 these overflow where the serial
// recursion would only have grown without bound; fitted models have |A| < 1.
#include "plgrad_lanes.h"     // AffineScan; em_scan_impl.h: readlane_d
#include "ldsr_kernels.h"

#include <stdint.h>

#pragma clang fp contract(fast)       // (this unit's sums of products stay contracted: plgrad_lanes.h turns that off)

// SplitMix64 finaliser of ldsr_amd/synth.py (_splitmix64): the increment, then the mix.
__device__ __forceinline__ uint64_t sim_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// qnorm(p, 0, 1) of R (nmath qnorm.c, Wichura's AS 241 PPND16) for p in [2^-81, 1 - 2^-54]:
// r = sqrt(-log(min(p, 1 - p))) < 8, so the three branches below are all there is.
__device__ __forceinline__ double sim_qnorm(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r +
                        45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
                      133.14166789178437745) * r + 3.387132872796366608) /
               (((((((r * 5226.495278852545925 + 28729.085735721942674) * r + 39307.89580009271061) * r +
                    21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
                 42.313330701600911252) * r + 1.0);
    }
    double r = sqrt(-log(q > 0 ? 0.5 - p + 0.5 : p));
    double val;
    if (r <= 5.0) {
        r += -1.6;
        val = (((((((r * 7.7454501427834140764e-4 + 0.0227238449892691845833) * r + 0.24178072517745061177) * r +
                   1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
                4.6303378461565452959) * r + 1.42343711074968357734) /
              (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r +
                   0.14810397642748007459) * r + 0.68976733498510000455) * r + 1.6763848301838038494) * r +
                2.05319162663775882187) * r + 1.0);
    } else {
        r += -5.0;
        val = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r +
                   0.026532189526576123093) * r + 0.29656057182850489123) * r + 1.7848265399172913358) * r +
                5.4637849111641143699) * r + 6.6579046435011037772) /
              (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
                   7.868691311456132591e-4) * r + 0.0148753612908506148525) * r + 0.13692988092273580531) * r +
                0.59983220655588793769) * r + 1.0);
    }
    return q < 0.0 ? -val : val;
}

// norm_rand() from the two uniforms at positions i, i + 1 of the replicate's sequence
struct SimUniforms {
    const double *rs;     // R-stream mode: the replicate's first uniform
    uint64_t key;         // counter mode: SplitMix64 key of (seed, stream)
    __device__ __forceinline__ double at(long long i) const {
        if (rs) return rs[i];
        const uint64_t z = sim_splitmix64(key + (uint64_t)i * 0x9E3779B97F4A7C15ull);
        return ((double)(z >> 11) + 0.5) * 0x1p-53;      // open interval (0, 1)
    }
    __device__ __forceinline__ double norm(long long i) const {
        const double u1 = at(i), u2 = at(i + 1);
        return sim_qnorm(((double)(int)(134217728.0 * u1) + u2) * 0x1p-27);
    }
};

__global__ __launch_bounds__(256, 4) void ldsr_simulate_kernel(SimParams prm) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= (long long)prm.n_models * prm.num_reps) return;
    const int m = (int)(wid / prm.num_reps), rep = (int)(wid - (long long)m * prm.num_reps);
    const int T = prm.T, p = prm.p, q = prm.q;
    const double *th = prm.theta + (size_t)m * (6 + p + q);
    const double A = th[0], C = th[1 + p];
    double fixV, fixQ, fixR;
    const int dV = sim_draws(th[5 + p + q], &fixV), dQ = sim_draws(th[2 + p + q], &fixQ),
              dR = sim_draws(th[3 + p + q], &fixR);
    const double sV = sqrt(th[5 + p + q]), sQ = sqrt(th[2 + p + q]), sR = sqrt(th[3 + p + q]);
    const long long oQ = 2 * dV, oR = oQ + 2LL * T * dQ;      // positions of q_1 and r_1
    const double mu = prm.mu ? prm.mu[m] : 0.0;
    const double *B = th + 1, *D = th + 2 + p;
    const double *u = prm.u ? prm.u + (size_t)m * prm.u_stride : nullptr;
    const double *v = prm.v ? prm.v + (size_t)m * prm.v_stride : nullptr;

    SimUniforms U;
    if (prm.uniforms) {
        U.rs = prm.uniforms + prm.draw_off[m] + (long long)rep * (oR + 2LL * T * dR);
        U.key = 0;
    } else {
        U.rs = nullptr;
        const uint64_t stream = ((uint64_t)m << 32) + (uint64_t)(prm.first_rep + rep);
        U.key = sim_splitmix64(prm.seed ^ sim_splitmix64(stream));
    }

    const AffineScan scan(A, lane);

    const size_t out0 = ((size_t)m * prm.num_reps + rep) * (size_t)T;
    double carry = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        double e = 0.0, w = 0.0;
        if (t < T) {
            // increment into x_t: x_1 itself at t = 0, else B u_{t-1} + q_{t-1}
            double bu = 0.0, dv = 0.0;
            if (t > 0 && u) {
                const double *ut = u + (size_t)(t - 1) * p;
                for (int k = 0; k < p; k++) bu = fma(B[k], ut[k], bu);
            }
            if (v) {
                const double *vt = v + (size_t)t * q;
                for (int k = 0; k < q; k++) dv = fma(D[k], vt[k], dv);
            }
            const bool first = t == 0;
            const int dx = first ? dV : dQ;
            const double noise = dx ? (first ? sV : sQ) * U.norm(first ? 0 : oQ + 2LL * (t - 1))
                                    : (first ? fixV : fixQ);
            e = bu + noise;
            w = dv + (dR ? sR * U.norm(oR + 2LL * t) : fixR);
        }
        if (lane == 0) e = fma(A, carry, e);
        // inclusive scan x_l = A x_{l-1} + e_l over the 64 lanes
        const double x = scan.run(e);
        carry = readlane_d(x, 63);
        if (t < T) {
            const double y = C * x + w;
            if (prm.simX) prm.simX[out0 + t] = x;
            if (prm.simY) prm.simY[out0 + t] = y;
            if (prm.simQ) prm.simQ[out0 + t] = prm.exp_trans ? exp(y + mu) : y + mu;
        }
    }
}

hipError_t launch_simulate(const SimParams &prm, hipStream_t stream) {
    const long long waves = (long long)prm.n_models * prm.num_reps;
    if (waves <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    hipLaunchKernelGGL(ldsr_simulate_kernel, dim3(blocks), dim3(256), 0, stream, prm);
    return hipGetLastError();
}
