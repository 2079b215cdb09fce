// ga.h -- launch interface of the island genetic algorithm (ga.hip): LDS_GA, R/LDS_GA.R:54-82, by the
// specification in INTEGRATION.md ("The island GA").  Included by ga.hip and api_ga.hip only.
#pragma once
#include <hip/hip_runtime.h>

// Cell (s, k, i) = individual i of island k of problem s is cell (s K + k) n + i of the fitness launch:
// a population buffer is the fitness launch's theta array as it stands.
struct GaState {          // per problem, double-buffered by generation parity
    double best;          // best fitness so far (-inf: none yet)
    int stall;            // generations since it last improved
    int done;             // the stop rule has fired: every later generation is a no-op
    int n_gen;            // generations evaluated
    int pad_;
};

struct GaParams {
    int n_series, K, n, P;            // problems, islands per problem, individuals per island, genes
    int maxiter, run, g;              // g: the generation this launch works on
    int n_elite, n_migr, migration_interval, n_sugg;
    double pcrossover, pmutation;
    unsigned long long seed;
    const double *lb, *ub;            // [P]
    const double *sugg;               // [n_series][n_sugg][P] or null
    double *pop[2];                   // [n_series][K][n][P]: generation g lives in pop[g & 1]
    const double *fit;                // [n_series][K][n] fitness of pop[g & 1]
    GaState *state[2];                // [n_series]: generation g reads state[g & 1], writes state[(g + 1) & 1]
    double *best_theta;               // [n_series][P]
    double *trace;                    // [n_series][maxiter] best so far after each generation, NaN beyond n_gen
};

hipError_t launch_ga_init(const GaParams &prm, hipStream_t stream);     // generation 0's population and state
hipError_t launch_ga_breed(const GaParams &prm, hipStream_t stream);    // steps 2-8 of generation prm.g
