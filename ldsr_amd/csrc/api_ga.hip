// api_ga.hip -- the island GA's entry of the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#include "host_series.h"
#include "ga.h"

namespace ldsr_host {

// ---- LDS_GA: the island genetic algorithm (ga.hip) ------------------------------------------------
// The series are uploaded and prepared once, the fitness launch's tables are built once; a generation
// is then smoother_enqueue (scalar-only, reading the current population buffer) + launch_ga_breed, and
// nothing in that loop touches host memory.  Generations go out LDSR_GA_CHUNK at a time; between chunks
// the problems' states come back (a few bytes each) to see whether every problem has stopped.
extern "C" int ldsr_ga_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                             const double *v, int shared_uv, const double *lb, const double *ub, double lambda,
                             int num_islands, int pop_per_island, int maxiter, int run,
                             unsigned long long seed, const double *suggestions, int n_suggestions,
                             double *theta_best, double *pl_best, int *n_gen, double *trace,
                             double *population, double *fitness) {
    const int K = num_islands, n = pop_per_island;
    if (K < 1) return fail(LDSR_EINVAL, "num_islands must be >= 1");
    if (n < 2 || n > LDSR_GA_MAX_POP) return fail(LDSR_EINVAL, "pop_per_island must be in 2 .. 1024");
    if (maxiter < 1) return fail(LDSR_EINVAL, "maxiter must be >= 1");
    if (run < 1) return fail(LDSR_EINVAL, "run must be >= 1");
    if (n_series < 1 || n_series > 65535) return fail(LDSR_EINVAL, "n_series must be in 1 .. 65535");
    if ((long long)n_series * K * n > (long long)std::numeric_limits<int>::max() / 64)
        return fail(LDSR_EINVAL, "n_series * num_islands * pop_per_island is too large");
    std::vector<int> off((size_t)n_series + 1);
    for (int s = 0; s <= n_series; s++) off[(size_t)s] = s * K * n;
    int rc = check_common(n_series, T, p, q, y, off.data());
    if (rc) return rc;
    const int P = 6 + p + q;
    rc = check_box(lb, ub, P, "gene");
    if (rc) return rc;
    if (!std::isfinite(lambda)) return fail(LDSR_EINVAL, "lambda must be finite");
    if (n_suggestions < 0 || n_suggestions > n)
        return fail(LDSR_EINVAL, "n_suggestions must be in 0 .. pop_per_island");
    if (n_suggestions > 0 && !suggestions) return fail(LDSR_EINVAL, "suggestions must not be NULL");
    if (!theta_best || !pl_best || !n_gen) return fail(LDSR_EINVAL, "theta_best, pl_best and n_gen must not be NULL");

    const int n_cells = n_series * K * n;
    IntrScope intr_scope;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    const int PP = ldsr_pad_dim(p), QQ = ldsr_pad_dim(q);
    const WsLayout L = ws_layout(n_series, T, PP, QQ, shared_uv, n_cells, LDSR_ALGO_SCAN, 1);
    SeriesUpload U{n_series, T, p, q, y, u, v, shared_uv};
    // The scan kernel whitens the inputs by Svv / Tuu and has no answer for a series where one of them is
    // singular (fewer observations than columns of v, say), but Kalman_smoother does not need them: the
    // cells of such a series take the serial smoother, whatever else shares the call.  series_prep finds
    // those series, so the strip they need is known only after it: one more pass in that rare case.
    const bool all_serial = !smoother_is_scan(T, PP, QQ, L, 0);
    const size_t cells_per_problem = (size_t)K * n;
    std::vector<char> singular((size_t)n_series, 0);
    int n_sing = 0;
    size_t o_lb = 0, o_ub = 0, o_sg = 0, in_bytes = 0, o_st = 0, o_bt = 0, o_tr = 0, out_bytes = 0, o_pop0 = 0,
           o_pop1 = 0, o_fit = 0, o_lik = 0, o_cst = 0, o_soc = 0, o_X = 0, o_V = 0, o_ws = 0;
    const size_t pop_bytes = sizeof(double) * (size_t)n_cells * P;
    char *dev = nullptr, *pin = nullptr;
    for (int pass = 0;; pass++) {
        const size_t strip_cells = all_serial ? (size_t)n_cells : (size_t)n_sing * cells_per_problem;
        Carver c;
        U.carve(c);
        o_lb = c.take(sizeof(double) * (size_t)P);
        o_ub = c.take(sizeof(double) * (size_t)P);
        o_sg = c.take(sizeof(double) * (size_t)n_series * n_suggestions * P);
        in_bytes = c.o;
        o_st = c.take(sizeof(GaState) * 2 * (size_t)n_series);      // both parities
        o_bt = c.take(sizeof(double) * (size_t)n_series * P);
        o_tr = c.take(sizeof(double) * (size_t)n_series * maxiter);
        out_bytes = c.o - o_st;
        o_pop0 = c.take(pop_bytes);
        o_pop1 = c.take(pop_bytes);
        o_fit = c.take(sizeof(double) * (size_t)n_cells);
        o_lik = c.take(sizeof(double) * (size_t)n_cells);
        o_cst = c.take(sizeof(int) * (size_t)n_cells);
        o_soc = c.take(sizeof(int) * (size_t)n_cells);
        o_X = c.take(sizeof(double) * strip_cells * T);
        o_V = c.take(sizeof(double) * strip_cells * T);
        o_ws = c.take(L.total);
        const size_t sc_bytes = align256(2 * sizeof(int) * (size_t)n_series);      // (n_obs, status) of every series
        rc = arena_reserve(A, c, in_bytes + align256(out_bytes) + sc_bytes, "ldsr_ga_batch");
        if (rc) return rc;
        dev = A->dev; pin = A->pin;
        U.stage(A);
        memcpy(pin + o_lb, lb, sizeof(double) * (size_t)P);
        memcpy(pin + o_ub, ub, sizeof(double) * (size_t)P);
        if (n_suggestions) memcpy(pin + o_sg, suggestions, sizeof(double) * (size_t)n_series * n_suggestions * P);
        HIPCHK(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, A->stream));
        HIPCHK(U.prep(device, A->stream, dev + o_ws, &L));
        if (all_serial || pass == 1) break;
        static_assert(offsetof(SeriesConst, status) == sizeof(int), "the copy below takes n_obs and status");
        int *h_sc = (int *)(pin + in_bytes + align256(out_bytes));
        HIPCHK(hipMemcpy2DAsync(h_sc, 2 * sizeof(int), U.ps.ws + L.sc, sizeof(SeriesConst), 2 * sizeof(int),
                                (size_t)n_series, hipMemcpyDeviceToHost, A->stream));
        HIPCHK(wait_stream(A->stream));
        for (int s = 0; s < n_series; s++)
            if (h_sc[2 * s + 1] != 0) { singular[(size_t)s] = 1; n_sing++; }
        if (n_sing == 0) break;
    }
    std::vector<int> soc((size_t)n_cells);
    for (int cc = 0; cc < n_cells; cc++) soc[(size_t)cc] = cc / (K * n);
    SmootherTables tb;
    rc = smoother_tables(U.ps, n_cells, soc.data(), 0, (int *)(dev + o_soc), &tb, &singular);
    if (rc) return rc;
    if (n_sing) {       // (the serial smoother's cell -> series map, which the scan launch's table replaces)
        rc = stage_h2d_async(device, A->stream, dev + o_soc, soc.data(), sizeof(int) * (size_t)n_cells);
        if (rc) return rc;
    }
    // (pen: only the scalars leave the kernel, and the strip X / V stands in for Y / J)
    FitOut fo;
    fo.X = fo.Y = (double *)(dev + o_X); fo.V = fo.J = (double *)(dev + o_V);
    fo.lik = (double *)(dev + o_lik); fo.pen = (double *)(dev + o_fit); fo.status = (int *)(dev + o_cst);
    const int *d_soc = (const int *)(dev + o_soc);
    // one generation's fitness: the scan launch (or the serial one) over all cells, then the singular series
    auto enqueue_fitness = [&](const double *d_pop) -> int {
        int r = smoother_enqueue(U.ps, n_cells, tb, d_soc, d_pop, 0, 0, lambda, fo);
        for (int s = 0, j = 0; s < n_series && !r && n_sing; s++) {
            if (!singular[(size_t)s]) continue;
            const size_t c0 = (size_t)s * cells_per_problem, t0 = (size_t)j++ * cells_per_problem * T;
            FitOut f = fo;
            f.X = f.Y = fo.X + t0; f.V = f.J = fo.V + t0;
            f.lik += c0; f.pen += c0; f.status += c0;
            r = smoother_enqueue(U.ps, (int)cells_per_problem, SmootherTables(), d_soc + c0, d_pop + c0 * P, 0, 0, lambda, f);
        }
        return r;
    };

    GaParams gp;
    memset(&gp, 0, sizeof(gp));
    gp.n_series = n_series; gp.K = K; gp.n = n; gp.P = P;
    gp.maxiter = maxiter; gp.run = run;
    gp.n_elite = std::max(1, (LDSR_GA_ELITE_PCT * n + 50) / 100);
    gp.n_migr = std::max(1, LDSR_GA_MIGRATION_PCT * n / 100);
    gp.migration_interval = LDSR_GA_MIGRATION_INTERVAL;
    gp.n_sugg = n_suggestions;
    gp.pcrossover = LDSR_GA_PCROSSOVER;
    gp.pmutation = LDSR_GA_PMUTATION;
    gp.seed = seed;
    gp.lb = (const double *)(dev + o_lb);
    gp.ub = (const double *)(dev + o_ub);
    gp.sugg = n_suggestions ? (const double *)(dev + o_sg) : nullptr;
    gp.pop[0] = (double *)(dev + o_pop0);
    gp.pop[1] = (double *)(dev + o_pop1);
    gp.fit = (const double *)(dev + o_fit);
    gp.state[0] = (GaState *)(dev + o_st);
    gp.state[1] = gp.state[0] + n_series;
    gp.best_theta = (double *)(dev + o_bt);
    gp.trace = (double *)(dev + o_tr);
    HIPCHK(launch_ga_init(gp, A->stream));

    char *pout = pin + in_bytes;
    const GaState *h_state = (const GaState *)pout;
    int g = 0;
    for (bool all_done = false; !all_done;) {
        const int g_end = (int)std::min((long long)maxiter, (long long)g + LDSR_GA_CHUNK);
        for (; g < g_end; g++) {
            rc = enqueue_fitness(gp.pop[g & 1]);
            if (rc) return rc;
            gp.g = g;
            HIPCHK(launch_ga_breed(gp, A->stream));
        }
        HIPCHK(hipMemcpyAsync(pout, dev + o_st, out_bytes, hipMemcpyDeviceToHost, A->stream));
        HIPCHK(wait_stream(A->stream));
        intr_poll();
        if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
        all_done = true;
        for (int s = 0; s < n_series; s++)
            if (!h_state[(size_t)(g & 1) * n_series + s].done) all_done = false;
    }
    // every problem is done: both population buffers hold its last evaluated generation, and the
    // fitness buffer that generation's values
    for (int s = 0; s < n_series; s++) {
        const GaState &st = h_state[(size_t)(g & 1) * n_series + s];
        pl_best[s] = st.best;
        n_gen[s] = st.n_gen;
    }
    memcpy(theta_best, pout + (o_bt - o_st), sizeof(double) * (size_t)n_series * P);
    if (trace) memcpy(trace, pout + (o_tr - o_st), sizeof(double) * (size_t)n_series * maxiter);
    if (population) HIPCHK(hipMemcpy(population, gp.pop[g & 1], pop_bytes, hipMemcpyDeviceToHost));
    if (fitness) HIPCHK(hipMemcpy(fitness, dev + o_fit, sizeof(double) * (size_t)n_cells, hipMemcpyDeviceToHost));
    return LDSR_OK;
}

}  // namespace ldsr_host
