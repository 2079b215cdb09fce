// api_simulate.hip -- the stochastic replicates' entries of the C ABI.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "host_runtime.h"
#include "ldsr_kernels.h"

namespace ldsr_host {

// ---- stochastic replicates (simulate.hip) ----------------------------------------------------------
static int sim_check(int n_models, int T, int p, int q, const double *theta, int num_reps, int first_rep) {
    if (n_models < 1) return fail(LDSR_EINVAL, "n_models must be >= 1");
    if (T < 1) return fail(LDSR_EINVAL, "T must be >= 1");
    if (p < 1 || q < 1) return fail(LDSR_EINVAL, "p and q must be >= 1 (use 1 with u/v = NULL for an absent input)");
    if (num_reps < 1) return fail(LDSR_EINVAL, "num_reps must be >= 1");
    if (first_rep < 0) return fail(LDSR_EINVAL, "first_rep must be >= 0");
    if (!theta) return fail(LDSR_EINVAL, "theta must not be NULL");
    return LDSR_OK;
}

static SimParams sim_params(int n_models, int T, int p, int q, const double *u, const double *v,
                            int shared_uv, const double *theta, const double *mu, int num_reps,
                            int first_rep, int exp_trans, unsigned long long seed, const double *uniforms,
                            const long long *draw_off, double *simX, double *simY, double *simQ) {
    SimParams s;
    s.n_models = n_models; s.T = T; s.p = p; s.q = q; s.num_reps = num_reps;
    s.first_rep = first_rep; s.exp_trans = exp_trans ? 1 : 0;
    s.u = u; s.v = v;
    s.u_stride = shared_uv ? 0 : (long long)T * p;
    s.v_stride = shared_uv ? 0 : (long long)T * q;
    s.theta = theta; s.mu = mu; s.seed = seed;
    s.uniforms = uniforms; s.draw_off = draw_off;
    s.simX = simX; s.simY = simY; s.simQ = simQ;
    return s;
}

extern "C" long long ldsr_simulate_draw_count(int n_models, int T, int p, int q, const double *theta,
                                              int num_reps, long long *offsets) {
    const int rc = sim_check(n_models, T, p, q, theta, num_reps, 0);
    if (rc) return -rc;
    long long total = 0;
    for (int m = 0; m < n_models; m++) {
        if (offsets) offsets[m] = total;
        total += (long long)num_reps * sim_draws_per_rep(theta + (size_t)m * (6 + p + q), p, q, T);
    }
    if (offsets) offsets[n_models] = total;
    return total;
}

extern "C" int ldsr_simulate_batch(int device, int n_models, int T, int p, int q, const double *u,
                                   const double *v, int shared_uv, const double *theta, const double *mu,
                                   int num_reps, int first_rep, int exp_trans, unsigned long long seed,
                                   const double *uniforms, double *simX, double *simY, double *simQ) {
    int rc = sim_check(n_models, T, p, q, theta, num_reps, first_rep);
    if (rc) return rc;
    std::vector<long long> off((size_t)n_models + 1);
    const long long n_unif = ldsr_simulate_draw_count(n_models, T, p, q, theta, num_reps, off.data());
    const int P = 6 + p + q;
    const size_t nuv = shared_uv ? 1 : (size_t)n_models;
    const size_t n_out = (size_t)n_models * num_reps * T;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    Carver c;
    const size_t o_th = c.take(sizeof(double) * (size_t)n_models * P);
    const size_t o_mu = c.take(mu ? sizeof(double) * (size_t)n_models : 0);
    const size_t o_off = c.take(uniforms ? sizeof(long long) * (size_t)n_models : 0);
    const size_t o_u = c.take(u ? sizeof(double) * nuv * T * p : 0);
    const size_t o_v = c.take(v ? sizeof(double) * nuv * T * q : 0);
    const size_t o_un = c.take(uniforms ? sizeof(double) * (size_t)n_unif : 0);
    const size_t in_bytes = c.o;
    const size_t o_X = c.take(simX ? sizeof(double) * n_out : 0);
    const size_t o_Y = c.take(simY ? sizeof(double) * n_out : 0);
    const size_t o_Q = c.take(simQ ? sizeof(double) * n_out : 0);
    rc = arena_reserve(A, c, in_bytes, "ldsr_simulate_batch");
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    memcpy(pin + o_th, theta, sizeof(double) * (size_t)n_models * P);
    if (mu) memcpy(pin + o_mu, mu, sizeof(double) * (size_t)n_models);
    if (uniforms) memcpy(pin + o_off, off.data(), sizeof(long long) * (size_t)n_models);
    if (u) memcpy(pin + o_u, u, sizeof(double) * nuv * T * p);
    if (v) memcpy(pin + o_v, v, sizeof(double) * nuv * T * q);
    if (uniforms) memcpy(pin + o_un, uniforms, sizeof(double) * (size_t)n_unif);
    HIPCHK(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, A->stream));
    const SimParams sp = sim_params(
        n_models, T, p, q, u ? (const double *)(dev + o_u) : nullptr, v ? (const double *)(dev + o_v) : nullptr,
        shared_uv, (const double *)(dev + o_th), mu ? (const double *)(dev + o_mu) : nullptr, num_reps,
        first_rep, exp_trans, seed, uniforms ? (const double *)(dev + o_un) : nullptr,
        uniforms ? (const long long *)(dev + o_off) : nullptr, simX ? (double *)(dev + o_X) : nullptr,
        simY ? (double *)(dev + o_Y) : nullptr, simQ ? (double *)(dev + o_Q) : nullptr);
    HIPCHK(launch_simulate(sp, A->stream));
    if (simX) HIPCHK(hipMemcpyAsync(simX, dev + o_X, sizeof(double) * n_out, hipMemcpyDeviceToHost, A->stream));
    if (simY) HIPCHK(hipMemcpyAsync(simY, dev + o_Y, sizeof(double) * n_out, hipMemcpyDeviceToHost, A->stream));
    if (simQ) HIPCHK(hipMemcpyAsync(simQ, dev + o_Q, sizeof(double) * n_out, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    return LDSR_OK;
}

extern "C" int ldsr_simulate_batch_device(int device, void *stream_, int n_models, int T, int p, int q,
                                          const double *d_u, const double *d_v, int shared_uv,
                                          const double *d_theta, const double *d_mu, int num_reps,
                                          int first_rep, int exp_trans, unsigned long long seed,
                                          const double *d_uniforms, const long long *d_offsets,
                                          double *d_simX, double *d_simY, double *d_simQ) {
    const int rc = sim_check(n_models, T, p, q, d_theta, num_reps, first_rep);
    if (rc) return rc;
    if (d_uniforms && !d_offsets) return fail(LDSR_EINVAL, "R-stream mode needs d_offsets");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_simulate(sim_params(n_models, T, p, q, d_u, d_v, shared_uv, d_theta, d_mu, num_reps, first_rep,
                                      exp_trans, seed, d_uniforms, d_offsets, d_simX, d_simY, d_simQ),
                           (hipStream_t)stream_));
    return LDSR_OK;
}

}  // namespace ldsr_host
