// ga.hip -- the generation loop of the island genetic algorithm on the device (LDS_GA, the reference's
// R/LDS_GA.R:54-82; the algorithm is this project's own specification, INTEGRATION.md "The island GA").
//
// A generation is two launches: the smoother's scalar-only fitness pass over the current population
// buffer (api_ga.hip), then ldsr_ga_breed_kernel, one workgroup per island:
//   * problem-wide bookkeeping.  Every island's workgroup reduces all K n fitness values of its problem
//     and reaches the same verdict (improved / stall / done) from the state of parity g & 1; island 0
//     alone writes the state of parity (g + 1) & 1, the trace and the best gene vector.  Nothing a
//     workgroup reads is written in the same launch, so no cross-workgroup synchronisation is needed.
//   * a problem that is done copies its population forward unchanged: generations enqueued past the stop
//     are no-ops, and the fitness pass keeps rewriting the same values.
//   * ranks by counting in LDS (thread i counts who beats individual i: n broadcast reads), then one
//     thread per slot of the next population: elite, child (selection, crossover, mutation), or -- on a
//     migration generation -- the last m slots, which the PREVIOUS island's workgroup fills from its own
//     best m (a scatter into the other buffer: the slots a workgroup writes are disjoint from its
//     neighbour's).
//
// Every random number is uniform i of stream (island k, generation g) under seed + s, the SplitMix64
// construction of ldsr_amd/synth.py's uniform(); the index ranges are laid out below (GaDraws).
// The arithmetic on genes is kept uncontracted so that the host model of tests/ga_model.py reproduces
// it bit for bit.
#include "ga.h"

#include <stdint.h>

#pragma clang fp contract(off)

// SplitMix64 finaliser of ldsr_amd/synth.py (_splitmix64): the increment, then the mix.
__device__ __forceinline__ uint64_t ga_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// synth.uniform(seed + s, (k << 32) | (g + 1), .)[i]; generation "-1" (stream word k << 32) is the
// initial population.
struct GaUniforms {
    uint64_t key;
    __device__ GaUniforms(uint64_t seed, int s, int k, int g) {
        const uint64_t stream = ((uint64_t)k << 32) | (uint64_t)(uint32_t)(g + 1);
        key = ga_splitmix64((seed + (uint64_t)s) ^ ga_splitmix64(stream));
    }
    __device__ __forceinline__ double at(long long i) const {
        const uint64_t z = ga_splitmix64(key + (uint64_t)i * 0x9E3779B97F4A7C15ull);
        return (double)(z >> 11) * 0x1p-53;      // [0, 1)
    }
};

// Index ranges of a generation's stream (n individuals, P genes; pair j = selected (2j, 2j + 1)):
struct GaDraws {
    long long sel, cross, weight, mut, gene, value;
    __device__ GaDraws(int n, int P)
        : sel(0),                               // [n]     selection draw of selected individual i
          cross(n),                             // [n / 2] crossover decision of pair j
          weight(2LL * n),                      // [n P]   crossover weight of pair j, gene c at j P + c
          mut(2LL * n + (long long)n * P),      // [n]     mutation decision of child i
          gene(3LL * n + (long long)n * P),     // [n]     which gene
          value(4LL * n + (long long)n * P) {}  // [n]     its new value
};

__device__ __forceinline__ double ga_clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }
__device__ __forceinline__ double ga_in_box(double u, double lo, double hi) { return ga_clip(lo + u * (hi - lo), lo, hi); }

// Linear-rank selection: P(rank r) = (2 / n) (1 - (r - 1) / (n - 1)), r = 1 the best.  The cumulative
// is c_r = r (2 n - 1 - r) / (n (n - 1)); with w = u n (n - 1) the selected rank is the smallest r
// with w < r (2 n - 1 - r) (integers, exact in double): the root of the quadratic, then one step of
// fix-up by that exact comparison, so a rounding in the root cannot change the answer.  Returns r - 1.
__device__ __forceinline__ int ga_select_rank(double u, int n) {
    const double b = (double)(2 * n - 1);
    const double w = u * (double)(n * (n - 1));
    int r = (int)floor((b - sqrt(b * b - 4.0 * w)) * 0.5) + 1;
    r = min(max(r, 1), n - 1);
    if (r > 1 && w < (double)((r - 1) * (2 * n - r)))
        r--;
    else if (r < n - 1 && !(w < (double)(r * (2 * n - 1 - r))))
        r++;
    return r - 1;
}

__global__ __launch_bounds__(256) void ldsr_ga_init_kernel(GaParams prm) {
    const int k = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;
    const int n = prm.n, P = prm.P;
    double *pop = prm.pop[0] + ((size_t)s * prm.K + k) * n * P;
    const GaUniforms U(prm.seed, s, k, -1);
    const int n_sugg = k == 0 && prm.sugg ? prm.n_sugg : 0;
    for (int idx = tid; idx < n * P; idx += nt) {
        const int i = idx / P, c = idx - i * P;
        pop[idx] = i < n_sugg ? ga_clip(prm.sugg[((size_t)s * prm.n_sugg + i) * P + c], prm.lb[c], prm.ub[c])
                              : ga_in_box(U.at(idx), prm.lb[c], prm.ub[c]);
    }
    if (k != 0) return;
    if (tid == 0) {
        GaState st;
        st.best = -INFINITY; st.stall = 0; st.done = 0; st.n_gen = 0; st.pad_ = 0;
        prm.state[0][s] = st;
    }
    for (int c = tid; c < P; c += nt) prm.best_theta[(size_t)s * P + c] = NAN;
    for (int g = tid; g < prm.maxiter; g += nt) prm.trace[(size_t)s * prm.maxiter + g] = NAN;
}

// does (fj, j) rank ahead of (fi, i)?  Finite before non-finite, higher first, ties by lower index.
__device__ __forceinline__ bool ga_beats(double fj, int j, double fi, int i) {
    const bool fin_j = isfinite(fj), fin_i = isfinite(fi);
    if (fin_j != fin_i) return fin_j;
    if (fin_j && fj != fi) return fj > fi;
    return j < i;
}

__global__ __launch_bounds__(1024) void ldsr_ga_breed_kernel(GaParams prm) {
    __shared__ double s_f[1024];      // the island's fitness; before that, the reduction's values
    __shared__ int s_ord[1024];       // rank -> individual; before that, the reduction's indices
    const int k = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, nt = blockDim.x;     // nt: a power of two >= n
    const int K = prm.K, n = prm.n, P = prm.P, g = prm.g;
    const GaState st = prm.state[g & 1][s];
    const size_t isl = ((size_t)s * K + k) * n;
    const double *cur = prm.pop[g & 1] + isl * P;
    double *nxt = prm.pop[(g + 1) & 1] + isl * P;

    int done = st.done;               // (uniform over the workgroup, as everything up to the ranks)
    if (!done) {
        // step 3: the problem's best of this generation, lowest (island, index) on ties
        const double *pf = prm.fit + (size_t)s * K * n;
        double bv = -INFINITY;
        int bi = -1;
        for (int j = tid; j < K * n; j += nt) {
            const double f = pf[j];
            if (isfinite(f) && (bi < 0 || f > bv)) { bv = f; bi = j; }
        }
        s_f[tid] = bv;
        s_ord[tid] = bi;
        __syncthreads();
        for (int h = nt >> 1; h > 0; h >>= 1) {
            if (tid < h) {
                const double ov = s_f[tid + h];
                const int oi = s_ord[tid + h];
                const int mi = s_ord[tid];
                if (oi >= 0 && (mi < 0 || ov > s_f[tid] || (ov == s_f[tid] && oi < mi))) {
                    s_f[tid] = ov;
                    s_ord[tid] = oi;
                }
            }
            __syncthreads();
        }
        bv = s_f[0];
        bi = s_ord[0];
        __syncthreads();
        const bool improved = bi >= 0 && bv > st.best;
        GaState ns;
        ns.best = improved ? bv : st.best;
        ns.stall = improved ? 0 : st.stall + 1;
        ns.n_gen = g + 1;
        ns.done = (g + 1 >= prm.maxiter || ns.stall >= prm.run) ? 1 : 0;
        ns.pad_ = 0;
        done = ns.done;
        if (k == 0) {
            if (tid == 0) {
                prm.state[(g + 1) & 1][s] = ns;
                prm.trace[(size_t)s * prm.maxiter + g] = ns.best;
            }
            if (improved)
                for (int c = tid; c < P; c += nt)
                    prm.best_theta[(size_t)s * P + c] = prm.pop[g & 1][((size_t)s * K * n + bi) * P + c];
        }
    } else if (k == 0 && tid == 0) {
        prm.state[(g + 1) & 1][s] = st;
    }
    if (done) {     // stopped: the population moves on unchanged
        for (int idx = tid; idx < n * P; idx += nt) nxt[idx] = cur[idx];
        return;
    }

    // step 2: order the island
    if (tid < n) s_f[tid] = prm.fit[isl + tid];
    __syncthreads();
    if (tid < n) {
        const double fi = s_f[tid];
        int r = 0;
        for (int j = 0; j < n; j++) r += ga_beats(s_f[j], j, fi, tid) ? 1 : 0;
        s_ord[r] = tid;
    }
    __syncthreads();

    const int e = prm.n_elite, m = prm.n_migr;
    const bool migrate = K > 1 && (g + 1) % prm.migration_interval == 0;
    // step 8: this island's best m go to the last m slots of the next island's next population
    if (migrate && tid < m) {
        const double *src = cur + (size_t)s_ord[tid] * P;
        double *dst = prm.pop[(g + 1) & 1] + (((size_t)s * K + (k + 1) % K) * n + (n - m + tid)) * P;
        for (int c = 0; c < P; c++) dst[c] = src[c];
    }
    if (tid >= n || (migrate && tid >= n - m)) return;      // (those slots belong to the previous island)
    double *out = nxt + (size_t)tid * P;
    if (tid < e) {                                          // step 7: the elite, unchanged
        const double *src = cur + (size_t)s_ord[tid] * P;
        for (int c = 0; c < P; c++) out[c] = src[c];
        return;
    }
    // steps 4-6: child i of pair j
    const int i = tid - e, j = i >> 1;
    const GaUniforms U(prm.seed, s, k, g);
    const GaDraws D(n, P);
    const double *x1 = cur + (size_t)s_ord[ga_select_rank(U.at(D.sel + 2 * j), n)] * P;
    const double *x2 = cur + (size_t)s_ord[ga_select_rank(U.at(D.sel + 2 * j + 1), n)] * P;
    const bool crossed = U.at(D.cross + j) < prm.pcrossover;
    const bool second = (i & 1) != 0;
    const bool mutated = U.at(D.mut + i) < prm.pmutation;
    const int mgene = mutated ? min((int)(U.at(D.gene + i) * (double)P), P - 1) : -1;
    for (int c = 0; c < P; c++) {
        const double lo = prm.lb[c], hi = prm.ub[c];
        double x = second ? x2[c] : x1[c];
        if (crossed) {
            const double a = U.at(D.weight + (long long)j * P + c);
            const double wa = second ? 1.0 - a : a;         // weight of x1
            const double wb = second ? a : 1.0 - a;         // weight of x2
            x = ga_clip(wa * x1[c] + wb * x2[c], lo, hi);
        }
        if (c == mgene) x = ga_in_box(U.at(D.value + i), lo, hi);
        out[c] = x;
    }
}

hipError_t launch_ga_init(const GaParams &prm, hipStream_t stream) {
    hipLaunchKernelGGL(ldsr_ga_init_kernel, dim3((unsigned)prm.K, (unsigned)prm.n_series), dim3(256), 0, stream, prm);
    return hipGetLastError();
}

hipError_t launch_ga_breed(const GaParams &prm, hipStream_t stream) {
    unsigned nt = 64;
    while ((int)nt < prm.n) nt <<= 1;
    hipLaunchKernelGGL(ldsr_ga_breed_kernel, dim3((unsigned)prm.K, (unsigned)prm.n_series), dim3(nt), 0, stream, prm);
    return hipGetLastError();
}
