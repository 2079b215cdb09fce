// The host half of plgrad.h on its own: (1) the addressing the kernels of plgrad.hip use, walked over every
// (chunk, lane) of both lane-to-step mappings for T = 1 .. 200, 813 and 1639; (2) pl and its gradient evaluated
// serially in time with the per-step functions the kernels call, for the cases of a text file:
//     n_cases, then per case:  T p q has_u has_v lambda,  y [T],  u [T][p] (if has_u),  v [T][q] (if has_v),
//     theta [6+p+q]
// and printed as one line per case: pl and the 6+p+q gradient entries, %.17g.
// usage: plgrad_host CASES_FILE      (exit 0: every check passed)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plgrad.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static void walk_addressing(int T) {
    const size_t strip = plg_strip_doubles(T);
    const int n_chunks = plg_chunks(T);
    std::vector<int> fwd((size_t)T, 0), rev((size_t)T, 0);
    std::vector<char> hit(strip, 0);
    for (int ch = 0; ch < n_chunks; ch++)
        for (int lane = 0; lane < 64; lane++) {
            const int tf = plg_fwd_step(ch, lane), tr = plg_rev_step(ch, lane);
            CHECK(tf >= 0 && tr >= 0);
            if (tf < T) fwd[(size_t)tf]++;
            if (tr < T) rev[(size_t)tr]++;
            // the lane below in the forward mapping is the step before, in the mirrored mapping the step above
            if (lane > 0) CHECK(plg_fwd_step(ch, lane - 1) == tf - 1 && plg_rev_step(ch, lane - 1) == tr + 1);
            if (ch > 0 && lane == 0) CHECK(plg_fwd_step(ch - 1, 63) == tf - 1);
            if (ch + 1 < n_chunks && lane == 0) CHECK(plg_rev_step(ch + 1, 63) == tr + 1);
            for (int t : {tf, tr})
                if (t < T)
                    for (int k = 0; k < PLG_NSTRIP; k++) {
                        const size_t o = plg_strip_at(k, t, T);
                        CHECK(o < strip);
                        hit[o] = 1;
                    }
        }
    for (int t = 0; t < T; t++) CHECK(fwd[(size_t)t] == 1 && rev[(size_t)t] == 1);
    for (size_t o = 0; o < strip; o++) CHECK(hit[o]);     // the arrays tile the strip: no two share a double
    // the strips of a launch: wave w's ends where wave w + 1's begins, the last one where the reservation ends
    for (int n_cells : {1, 2, 100, PLG_MAX_WAVES - 1, PLG_MAX_WAVES, PLG_MAX_WAVES + 1, 50000}) {
        const int w = plg_waves(n_cells);
        CHECK(w >= 1 && w <= n_cells && w <= PLG_MAX_WAVES);
        CHECK((size_t)w * strip == plg_launch_strip_doubles(n_cells, T));
        CHECK(plg_wave_strip(w - 1, T) + strip == plg_launch_strip_doubles(n_cells, T));
        for (int i = 1; i < w; i += (w > 64 ? w / 7 : 1)) CHECK(plg_wave_strip(i, T) == plg_wave_strip(i - 1, T) + strip);
    }
    // the series and the rows: the extents are one past the largest address
    CHECK(plg_y_doubles(3, T) == (size_t)3 * T && plg_y_at(2, T - 1, T) + 1 == plg_y_doubles(3, T));
    CHECK(plg_uv_doubles(3, 0, T, 5) == (size_t)T * 5 && plg_uv_doubles(3, (long)T * 5, T, 5) == (size_t)3 * T * 5);
    CHECK(plg_rows_doubles(7, 11) == 77);
}

static void check_extents() {
    char block[4096];
    CellSeries S;
    S.n_cells = 3; S.T = 4; S.p = 1; S.q = 2;
    S.y = (const double *)block; S.u = nullptr; S.v = (const double *)(block + 256);
    S.u_stride = 0; S.v_stride = 0;
    S.series_of_cell = (const int *)(block + 512);
    S.strip = (double *)(block + 1024);
    const size_t strip_bytes = sizeof(double) * plg_launch_strip_doubles(3, 4);
    size_t have[5] = {256, 256, 256, 256, strip_bytes};
    PlgExtent e[PLG_MAX_EXTENTS];
    int n = plg_series_extents(S, 2, have, e);
    CHECK(n == 5 && plg_first_bad_extent(e, n, block, sizeof(block)) == -1);
    have[4] -= sizeof(double);
    n = plg_series_extents(S, 2, have, e);
    CHECK(plg_first_bad_extent(e, n, block, sizeof(block)) == 4);
    have[4] = strip_bytes;
    n = plg_series_extents(S, 2, have, e);
    CHECK(plg_first_bad_extent(e, n, block, 1024 + strip_bytes - 1) == 4);
    S.y = nullptr;
    n = plg_series_extents(S, 2, have, e);
    CHECK(plg_first_bad_extent(e, n, block, sizeof(block)) == 0);
}

struct Case {
    int T, p, q, has_u, has_v;
    double lambda;
    std::vector<double> y, u, v, theta;
};

// pl and d pl / d theta [P], the passes of plgrad.hip with the scans replaced by their serial recurrences
static double evaluate(const Case &c, std::vector<double> &g) {
    const int T = c.T, p = c.p, q = c.q, P = 6 + p + q;
    const double *th = c.theta.data();
    const PlgCoef co = plg_coef(th[0], th[1 + p], th[2 + p + q], th[3 + p + q]);
    const double mu1 = th[4 + p + q], V1 = th[5 + p + q], lambda = c.lambda;
    std::vector<double> strip(plg_strip_doubles(T));
    double *st = strip.data();
    const double *y = c.y.data() + plg_y_at(0, 0, T);
    const double *u = c.has_u ? c.u.data() : nullptr, *v = c.has_v ? c.v.data() : nullptr;

    double lik_terms = 0.0, Vp = V1, Xp = mu1;
    for (int t = 0; t < T; t++) {
        double bu = 0.0, dv = 0.0;
        if (u) for (int k = 0; k < p; k++) bu = fma(th[1 + k], u[plg_uv_at(0, 0, t, p, k)], bu);
        if (v) for (int k = 0; k < q; k++) dv = fma(th[2 + p + k], v[plg_uv_at(0, 0, t, q, k)], dv);
        const double yt = y[plg_y_at(0, t, T)];
        const bool obs = isfinite(yt);
        const double ymdv = obs ? yt - dv : 0.0;
        // (the composition with the identity exercises plg_mob_then's renormalisation)
        const double Vp_next = plg_mob_apply(plg_mob_then(plg_mob_identity(), plg_mob_step(co, obs)), Vp);
        double S, K, Vu;
        plg_var_step(co, Vp, obs, &S, &K, &Vu);
        const double Xp_next = plg_aff_apply(plg_aff_then(plg_aff_identity(), plg_mean_step(co, K, ymdv, bu)), Xp);
        const PlgFwd f = plg_fwd_step_values(co, Vp, Xp, obs, ymdv);
        lik_terms += f.lik_term;
        const PlgAff sm = plg_smooth_step(co, f.Vu, f.Xu, Vp_next, Xp_next, t == T - 1);
        st[plg_strip_at(PLG_J, t, T)] = sm.a;
        st[plg_strip_at(PLG_SRC, t, T)] = sm.b;
        st[plg_strip_at(PLG_BU, t, T)] = bu;
        st[plg_strip_at(PLG_VP, t, T)] = Vp;
        st[plg_strip_at(PLG_K, t, T)] = f.K;
        st[plg_strip_at(PLG_XP, t, T)] = Xp;
        st[plg_strip_at(PLG_D, t, T)] = f.d;
        Vp = Vp_next;
        Xp = Xp_next;
    }
    double ssq = 0.0, Xs_next = 0.0;
    for (int t = T - 1; t >= 0; t--) {
        const PlgAff sm = {st[plg_strip_at(PLG_J, t, T)], st[plg_strip_at(PLG_SRC, t, T)]};
        const double bu = st[plg_strip_at(PLG_BU, t, T)];
        const double Xs = plg_aff_apply(sm, Xs_next);
        const double e = plg_resid(co, Xs, Xs_next, bu, t == T - 1);
        ssq = fma(e, e, ssq);
        st[plg_strip_at(PLG_XS, t, T)] = Xs;
        st[plg_strip_at(PLG_EB, t, T)] = -2.0 * lambda * e;
        Xs_next = Xs;
    }
    const double pl = plg_value(lik_terms, ssq, lambda);

    double a = 0.0;
    for (int t = 0; t < T; t++) {
        const double eb = st[plg_strip_at(PLG_EB, t, T)];
        const double J_prev = t > 0 ? st[plg_strip_at(PLG_J, t - 1, T)] : 0.0;
        const double eb_prev = t > 0 ? st[plg_strip_at(PLG_EB, t - 1, T)] : 0.0;
        a = plg_aff_apply(plg_adj_xs_step(co, J_prev, eb_prev, eb), a);
        const bool last = t == T - 1;
        const double Xsn = last ? 0.0 : st[plg_strip_at(PLG_XS, t + 1, T)];
        const double Xpn = last ? 0.0 : st[plg_strip_at(PLG_XP, t + 1, T)];
        st[plg_strip_at(PLG_AB, t, T)] = a;
        st[plg_strip_at(PLG_JB, t, T)] = plg_adj_j(a, Xsn, Xpn, last);
    }

    g.assign((size_t)P, 0.0);
    double xp_next = 0.0, vp_next = 0.0;
    for (int t = T - 1; t >= 0; t--) {
        PlgBack b;
        b.obs = isfinite(y[plg_y_at(0, t, T)]); b.first = t == 0; b.last = t == T - 1;
        b.Vp = st[plg_strip_at(PLG_VP, t, T)];
        b.K = st[plg_strip_at(PLG_K, t, T)];
        b.Xp = st[plg_strip_at(PLG_XP, t, T)];
        b.d = st[plg_strip_at(PLG_D, t, T)];
        b.Xs = st[plg_strip_at(PLG_XS, t, T)];
        b.eb = st[plg_strip_at(PLG_EB, t, T)];
        b.a = st[plg_strip_at(PLG_AB, t, T)];
        b.Vp_next = 1.0; b.Jb = 0.0; b.back = 0.0; b.back_v = 0.0;
        if (!b.last) {
            b.Vp_next = st[plg_strip_at(PLG_VP, t + 1, T)];
            b.Jb = st[plg_strip_at(PLG_JB, t, T)];
        }
        if (!b.first) {
            const double J_prev = st[plg_strip_at(PLG_J, t - 1, T)];
            b.back = J_prev * st[plg_strip_at(PLG_AB, t - 1, T)];
            b.back_v = st[plg_strip_at(PLG_JB, t - 1, T)] * J_prev / b.Vp;
        }
        plg_back_derive(co, &b);
        const double xp = plg_aff_apply(plg_adj_xp_step(co, b), xp_next);
        const double xu = plg_adj_xu(co, b, xp_next);
        const double vp = plg_aff_apply(plg_adj_vp_step(co, b, xu), vp_next);
        const PlgContrib gc = plg_contrib(co, b, xu, plg_adj_vu(co, b, vp_next), xp_next, vp_next);
        g[0] += gc.gA; g[(size_t)(2 + p + q)] += gc.gQ; g[(size_t)(1 + p)] += gc.gC; g[(size_t)(3 + p + q)] += gc.gR;
        if (u) for (int k = 0; k < p; k++) g[(size_t)(1 + k)] = fma(gc.fB, u[plg_uv_at(0, 0, t, p, k)], g[(size_t)(1 + k)]);
        if (v) for (int k = 0; k < q; k++) g[(size_t)(2 + p + k)] = fma(gc.fD, v[plg_uv_at(0, 0, t, q, k)], g[(size_t)(2 + p + k)]);
        xp_next = xp;
        vp_next = vp;
    }
    g[(size_t)(4 + p + q)] = xp_next;
    g[(size_t)(5 + p + q)] = vp_next;
    return pl;
}

static void read_doubles(FILE *f, std::vector<double> &a, size_t n) {
    a.resize(n);
    for (size_t i = 0; i < n; i++) CHECK(fscanf(f, "%lf", &a[i]) == 1);
}

int main(int argc, char **argv) {
    for (int T = 1; T <= 200; T++) walk_addressing(T);
    walk_addressing(813);
    walk_addressing(1639);
    check_extents();
    if (argc < 2) return 0;
    FILE *f = fopen(argv[1], "r");
    CHECK(f);
    int n_cases = 0;
    CHECK(fscanf(f, "%d", &n_cases) == 1 && n_cases >= 0);
    for (int i = 0; i < n_cases; i++) {
        Case c;
        CHECK(fscanf(f, "%d %d %d %d %d %lf", &c.T, &c.p, &c.q, &c.has_u, &c.has_v, &c.lambda) == 6);
        CHECK(c.T >= 1 && c.p >= 1 && c.q >= 1 && c.p <= 16 && c.q <= 16);
        read_doubles(f, c.y, (size_t)c.T);
        if (c.has_u) read_doubles(f, c.u, (size_t)c.T * c.p);
        if (c.has_v) read_doubles(f, c.v, (size_t)c.T * c.q);
        read_doubles(f, c.theta, (size_t)(6 + c.p + c.q));
        std::vector<double> g;
        const double pl = evaluate(c, g);
        printf("%.17g", pl);
        for (double x : g) printf(" %.17g", x);
        printf("\n");
    }
    fclose(f);
    return 0;
}
