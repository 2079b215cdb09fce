// api_grid.hip -- the host-pointer EM entries of the C ABI: slices of the cell grid over the devices, the restart
// grid with its winners' fit, the group entry, and the restart selection rule.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "host_em.h"

namespace ldsr_host {

// ---- one contiguous slice of the cell grid on one device ---------------------------------------
// Phase 1 (slice_run): ONE pinned->device copy of [y | u | v | theta0], series_prep + EM kernel,
// ONE device->pinned copy of [theta | lik | n_iter | status].  Phase 2 (slice_fit_winners, the
// restart-grid entry only): gather the winners' theta and likelihood traces on the device, one
// smoother pass for them, one copy back.  The arena stays leased between the phases.
struct Slice {
    // inputs (host pointers already offset to the slice; `off` are local cell offsets)
    int device = 0, n_series = 0, T = 0, p = 0, q = 0, shared_uv = 0, niter = 0, algo = 0;
    int lead_steps = 0;      // data facts found in y (EmPlanIn): -1 fully observed, else the all-missing lead
    EmPlan plan;             // what the batch launch ran
    double tol = 0.0;
    const double *y = nullptr, *u = nullptr, *v = nullptr, *theta0 = nullptr;
    std::vector<int> off;
    // Striped cut (make_slices): the slice holds EVERY series of the call and, of series s, the
    // cells [g_lo[s], g_lo[s] + off[s+1] - off[s]) of the caller's arrays -- theta0 / theta / lik /
    // n_iter / status / liks are the caller's whole arrays, gathered and scattered per series.
    std::vector<int> g_lo;
    const int *plan_off = nullptr;      // the whole call's offsets (EmLaunch), several devices only
    int plan_ns = 0;
    // host outputs of phase 1 (liks optional: the full [n_cells][niter] trace, NaN padded)
    double *theta = nullptr, *lik = nullptr, *liks = nullptr;
    int *n_iter = nullptr, *status = nullptr;
    int max_winners = 0;        // > 0: reserve phase-2 buffers and keep the traces on the device
    // Fused restart path (the whole grid on this one slice): selection, winner gather and the
    // winners' fit are enqueued right behind the EM kernel and everything comes back with ONE
    // synchronisation; the per-cell arrays cross PCIe only if the caller asked for them.
    bool fuse = false, want_all = true;
    int *h_winner = nullptr, *h_nit_w = nullptr;
    double *h_theta_w = nullptr, *h_lik_w = nullptr, *h_liks_w = nullptr;
    double *h_X = nullptr, *h_Y = nullptr, *h_V = nullptr, *h_J = nullptr;
    bool fused_done = false;
    // state
    ArenaLease lease;
    int n_cells = 0, PP = 0, QQ = 0, P = 0;
    bool trace_on_device = false;
    WsLayout L;
    size_t wsb = 0;
    size_t d_in = 0, d_y = 0, d_u = 0, d_v = 0, d_th0 = 0, d_off = 0, in_bytes = 0;      // device offsets
    size_t d_out = 0, d_theta = 0, d_lik = 0, d_nit = 0, d_st = 0, out_bytes = 0;
    size_t d_liks = 0, d_ws = 0;
    size_t d_w = 0, w_bytes = 0;          // phase-2 device block
    size_t p_in = 0, p_out = 0, p_w = 0;  // pinned offsets
};

static size_t liks_trace_cap_bytes() {
    const char *e = getenv("LDSR_LIKS_TRACE_MAX_BYTES");
    if (e && *e) return (size_t)strtoull(e, nullptr, 10);
    return (size_t)8 << 30;
}

// phase-2 block layout for n winners (offsets relative to its start)
struct WinLayout {
    size_t cell, ser, theta, liks, X, Y, V, J, lik, st, theta0, blk, lik_w, nit_w, total;
    size_t out_begin, out_bytes;    // [cell | theta | liks | X | Y | V | J | lik | lik_w | nit_w] is copied back
};
static WinLayout win_layout(int n, int P, int T, int niter) {
    WinLayout W;
    Carver c(true);         // (a layout inside one buffer of the slice's block)
    W.ser = c.take(sizeof(int) * n);
    W.theta0 = c.take(sizeof(double) * n * P);
    W.st = c.take(sizeof(int) * n);
    W.blk = c.take(sizeof(int) * 3 * n);
    W.out_begin = c.o;
    W.cell = c.take(sizeof(int) * n);        // winners' cell indices (uploaded, or selected on the device)
    W.theta = c.take(sizeof(double) * n * P);
    W.liks = c.take(sizeof(double) * (size_t)n * niter);
    W.X = c.take(sizeof(double) * (size_t)n * T);
    W.Y = c.take(sizeof(double) * (size_t)n * T);
    W.V = c.take(sizeof(double) * (size_t)n * T);
    W.J = c.take(sizeof(double) * (size_t)n * T);
    W.lik = c.take(sizeof(double) * n);
    W.lik_w = c.take(sizeof(double) * n);
    W.nit_w = c.take(sizeof(int) * n);
    W.out_bytes = c.o - W.out_begin;
    W.total = c.o;
    return W;
}

// the winners' fit of a slice: one pass at the n thetas of its phase-2 block dw, on the series phase 1 prepared in ws
static int slice_fit(const Slice &S, char *ws, char *dw, const WinLayout &W, int n, const int *series_of_cell,
                     const int *d_tab_prebuilt = nullptr) {
    const PreparedSeries PS{S.device, S.lease.a->stream, S.T, S.p, S.q, S.PP, S.QQ, S.shared_uv, S.u != nullptr,
                            S.v != nullptr, ws, &S.L};
    const FitOut F{(double *)(dw + W.X), (double *)(dw + W.Y), (double *)(dw + W.V), (double *)(dw + W.J),
                   (double *)(dw + W.lik), nullptr, (int *)(dw + W.st)};
    return launch_smoother(PS, n, series_of_cell, (const double *)(dw + W.theta), 1, 0, 0.0, F, (int *)(dw + W.ser),
                           d_tab_prebuilt);
}

// per-cell results of the slice (pinned block `pout`) -> the caller's arrays, series by series
static void slice_scatter(const Slice &S, const char *pout) {
    const int P = S.P;
    for (int s = 0; s < S.n_series; s++) {
        const size_t lo = (size_t)S.off[(size_t)s], nc = (size_t)S.off[(size_t)s + 1] - lo, g = (size_t)S.g_lo[(size_t)s];
        if (!nc) continue;
        memcpy(S.theta + g * P, pout + (S.d_theta - S.d_out) + sizeof(double) * lo * P, sizeof(double) * nc * P);
        memcpy(S.lik + g, pout + (S.d_lik - S.d_out) + sizeof(double) * lo, sizeof(double) * nc);
        memcpy(S.n_iter + g, pout + (S.d_nit - S.d_out) + sizeof(int) * lo, sizeof(int) * nc);
        memcpy(S.status + g, pout + (S.d_st - S.d_out) + sizeof(int) * lo, sizeof(int) * nc);
    }
}

// the EM launch of a slice on its arena: the prepared inputs, the per-cell outputs and the workspace
static EmLaunch slice_launch(const Slice &S) {
    const Arena *A = S.lease.a;
    EmLaunch E;
    E.device = S.device; E.stream = A->stream;
    E.n_series = S.n_series; E.T = S.T; E.p = S.p; E.q = S.q; E.shared_uv = S.shared_uv;
    E.y = (const double *)(A->dev + S.d_y);
    E.u = S.u ? (const double *)(A->dev + S.d_u) : nullptr;
    E.v = S.v ? (const double *)(A->dev + S.d_v) : nullptr;
    E.niter = S.niter; E.tol = S.tol;
    E.theta = (double *)(A->dev + S.d_theta); E.lik = (double *)(A->dev + S.d_lik);
    E.n_iter = (int *)(A->dev + S.d_nit); E.status = (int *)(A->dev + S.d_st);
    E.workspace = A->dev + S.d_ws; E.workspace_bytes = S.wsb;
    E.lead_steps = S.lead_steps;
    return E;
}

static int slice_run(Slice &S) {
    S.n_cells = S.off[S.n_series];
    S.P = 6 + S.p + S.q;
    S.PP = ldsr_pad_dim(S.p);
    S.QQ = ldsr_pad_dim(S.q);
    if (S.n_cells == 0) return LDSR_OK;
    const int T = S.T, P = S.P, n = S.n_cells;
    const size_t nuv = S.shared_uv ? 1 : (size_t)S.n_series;
    int rc = arena_acquire(S.device, &S.lease.a);
    if (rc) return rc;
    Arena *A = S.lease.a;

    Carver c;
    S.d_in = c.o;
    S.d_y = c.take(sizeof(double) * (size_t)S.n_series * T);
    S.d_u = c.take(S.u ? sizeof(double) * nuv * T * S.p : 0);
    S.d_v = c.take(S.v ? sizeof(double) * nuv * T * S.q : 0);
    S.d_th0 = c.take(sizeof(double) * (size_t)n * P);
    S.d_off = c.take(sizeof(int) * ((size_t)S.n_series + 1));
    S.in_bytes = c.o - S.d_in;
    S.d_out = c.o;
    S.d_theta = c.take(sizeof(double) * (size_t)n * P);
    S.d_lik = c.take(sizeof(double) * (size_t)n);
    S.d_nit = c.take(sizeof(int) * (size_t)n);
    S.d_st = c.take(sizeof(int) * (size_t)n);
    S.out_bytes = c.o - S.d_out;
    const size_t trace_bytes = sizeof(double) * (size_t)n * S.niter;
    S.trace_on_device = S.liks != nullptr || (S.max_winners > 0 && trace_bytes <= liks_trace_cap_bytes());
    S.d_liks = c.take(S.trace_on_device ? trace_bytes : 0);
    S.wsb = ldsr_em_workspace_bytes(S.n_series, T, S.p, S.q, n, S.algo);
    if (!S.wsb) return fail(LDSR_EINVAL, "unsupported (T, p, q, algo) combination");
    S.d_ws = c.take(S.wsb);
    const WinLayout W = win_layout(std::max(S.max_winners, 1), P, T, S.niter);
    S.d_w = c.take(S.max_winners > 0 ? W.total : 0);
    S.w_bytes = S.max_winners > 0 ? W.total : 0;
    // pinned: inputs, outputs, phase-2 block (same relative layouts as on the device)
    S.p_in = 0;
    S.p_out = align256(S.in_bytes);
    S.p_w = S.p_out + align256(S.out_bytes);
    const size_t pin_total = S.p_w + S.w_bytes;
    rc = arena_reserve(A, c, pin_total, "the EM slice (ldsr_em_batch / _multi / ldsr_em_restart_grid / _groups)");
    if (rc) return rc;

    // stage inputs
    char *pin = A->pin + S.p_in;
    memcpy(pin + (S.d_y - S.d_in), S.y, sizeof(double) * (size_t)S.n_series * T);
    {
        bool all_obs = true;
        const size_t ny = (size_t)S.n_series * T;
        for (size_t i = 0; i < ny && all_obs; i++) all_obs = std::isfinite(S.y[i]);
        // all-missing lead common to every series (the pair family's closed form)
        int lead = T;
        for (int s = 0; s < S.n_series && lead > 0; s++) {
            int t = 0;
            while (t < lead && !std::isfinite(S.y[(size_t)s * T + t])) t++;
            lead = std::min(lead, t);
        }
        S.lead_steps = all_obs ? -1 : lead;
    }
    if (S.u) memcpy(pin + (S.d_u - S.d_in), S.u, sizeof(double) * nuv * T * S.p);
    if (S.v) memcpy(pin + (S.d_v - S.d_in), S.v, sizeof(double) * nuv * T * S.q);
    for (int s = 0; s < S.n_series; s++)      // this slice's cells of every series
        memcpy(pin + (S.d_th0 - S.d_in) + sizeof(double) * (size_t)S.off[(size_t)s] * P,
               S.theta0 + (size_t)S.g_lo[(size_t)s] * P,
               sizeof(double) * (size_t)(S.off[(size_t)s + 1] - S.off[(size_t)s]) * P);
    memcpy(pin + (S.d_off - S.d_in), S.off.data(), sizeof(int) * ((size_t)S.n_series + 1));
    HIPCHK(hipMemcpyAsync(A->dev + S.d_in, pin, S.in_bytes, hipMemcpyHostToDevice, A->stream));

    EmLaunch E = slice_launch(S);
    E.cell_offsets = S.off.data();
    E.theta0 = (const double *)(A->dev + S.d_th0);
    E.algo = S.algo;
    E.liks = S.trace_on_device ? (double *)(A->dev + S.d_liks) : nullptr;
    E.liks_nanfill = S.liks != nullptr;
    E.abort_flag = intr_flag_for_kernels();
    E.plan_off = S.plan_off; E.plan_ns = S.plan_ns;
    rc = em_batch_device_impl(E);
    if (rc) return rc;
    S.plan = E.plan;
    S.L = E.layout;         // (phase 2 reuses the prepared series and the scan kernel's image)
    char *pout = A->pin + S.p_out;
    if (S.fuse && S.trace_on_device) {
        // selection, winner extraction and the winners' fit behind the EM kernel, one sync
        const int ns = S.n_series;
        char *dw = A->dev + S.d_w, *pw = A->pin + S.p_w;
        SelectParams sel;
        sel.n_series = ns; sel.P = P; sel.c_index = 1 + S.p;
        sel.off = (const int *)(A->dev + S.d_off);
        sel.theta = (const double *)(A->dev + S.d_theta);
        sel.lik = (const double *)(A->dev + S.d_lik);
        sel.winner = (int *)(dw + W.cell);
        HIPCHK(launch_select_winners(sel, A->stream));
        GatherParams gp;
        gp.n_w = ns; gp.P = P; gp.niter = S.niter;
        gp.cell = (const int *)(dw + W.cell);
        gp.theta = sel.theta;
        gp.theta0 = (const double *)(A->dev + S.d_th0);
        gp.n_iter = (const int *)(A->dev + S.d_nit);
        gp.liks = (const double *)(A->dev + S.d_liks);
        gp.theta_w = (double *)(dw + W.theta);
        gp.theta0_w = (double *)(dw + W.theta0);
        gp.liks_w = (double *)(dw + W.liks);
        gp.lik = sel.lik;
        gp.lik_w = (double *)(dw + W.lik_w);
        gp.n_iter_w = (int *)(dw + W.nit_w);
        gp.blk = (int *)(dw + W.blk);
        HIPCHK(launch_gather_winners(gp, A->stream));
        const bool want_fit = S.h_X || S.h_Y || S.h_V || S.h_J;
        if (want_fit) {
            std::vector<int> soc((size_t)ns);
            for (int i = 0; i < ns; i++) soc[(size_t)i] = i;
            char *ws = A->dev + S.d_ws;
            rc = slice_fit(S, ws, dw, W, ns, soc.data(), (const int *)(dw + W.blk));
            if (rc) return rc;
        }
        if (S.want_all)
            HIPCHK(hipMemcpyAsync(pout, A->dev + S.d_out, S.out_bytes, hipMemcpyDeviceToHost, A->stream));
        HIPCHK(hipMemcpyAsync(pw + W.out_begin, dw + W.out_begin, W.out_bytes, hipMemcpyDeviceToHost,
                              A->stream));
        HIPCHK(wait_stream(A->stream));
        if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
        if (S.want_all) slice_scatter(S, pout);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        memcpy(S.h_winner, pw + W.cell, sizeof(int) * ns);
        memcpy(S.h_theta_w, pw + W.theta, sizeof(double) * (size_t)ns * P);
        memcpy(S.h_lik_w, pw + W.lik_w, sizeof(double) * ns);
        memcpy(S.h_nit_w, pw + W.nit_w, sizeof(int) * ns);
        if (S.h_liks_w) memcpy(S.h_liks_w, pw + W.liks, sizeof(double) * (size_t)ns * S.niter);
        double *rows[4] = {S.h_X, S.h_Y, S.h_V, S.h_J};
        const size_t roff[4] = {W.X, W.Y, W.V, W.J};
        for (int k = 0; k < 4; k++) {
            if (!rows[k]) continue;
            memcpy(rows[k], pw + roff[k], sizeof(double) * (size_t)ns * T);
            for (int i = 0; i < ns; i++)      // series without a winner: the fit kernel skipped them
                if (S.h_winner[i] < 0)
                    for (int t = 0; t < T; t++) rows[k][(size_t)i * T + t] = nan;
        }
        S.fused_done = true;
        return LDSR_OK;
    }
    HIPCHK(hipMemcpyAsync(pout, A->dev + S.d_out, S.out_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(wait_stream(A->stream));
    slice_scatter(S, pout);
    if (S.liks)     // the full trace goes straight to the caller's (pageable) array, series by series
        for (int s = 0; s < S.n_series; s++) {
            const size_t nc = (size_t)(S.off[(size_t)s + 1] - S.off[(size_t)s]);
            if (nc)
                HIPCHK(hipMemcpy(S.liks + (size_t)S.g_lo[(size_t)s] * S.niter,
                                 A->dev + S.d_liks + sizeof(double) * (size_t)S.off[(size_t)s] * S.niter,
                                 sizeof(double) * nc * S.niter, hipMemcpyDeviceToHost));
        }
    return LDSR_OK;
}

// Phase 2.  w_series / w_cell: local series index and local cell index of each winner of this
// slice; outputs are rows [i] of the given host arrays (any of liks_w .. J may be NULL).
static int slice_fit_winners(Slice &S, int n_w, const int *w_series, const int *w_cell,
                             double *liks_w, double *X, double *Y, double *V, double *J) {
    if (n_w == 0) return LDSR_OK;
    Arena *A = S.lease.a;
    const int T = S.T, P = S.P, niter = S.niter;
    HIPCHK(hipSetDevice(S.device));
    const WinLayout W = win_layout(std::max(S.max_winners, 1), P, T, niter);
    char *dw = A->dev + S.d_w, *pw = A->pin + S.p_w;
    memcpy(pw + W.cell, w_cell, sizeof(int) * n_w);
    memcpy(pw + W.ser, w_series, sizeof(int) * n_w);
    HIPCHK(hipMemcpyAsync(dw + W.cell, pw + W.cell, sizeof(int) * n_w, hipMemcpyHostToDevice, A->stream));
    HIPCHK(hipMemcpyAsync(dw + W.ser, pw + W.ser, sizeof(int) * n_w, hipMemcpyHostToDevice, A->stream));
    GatherParams gp;
    gp.n_w = n_w; gp.P = P; gp.niter = niter;
    gp.cell = (const int *)(dw + W.cell);
    gp.theta = (const double *)(A->dev + S.d_theta);
    gp.theta0 = (const double *)(A->dev + S.d_th0);
    gp.n_iter = (const int *)(A->dev + S.d_nit);
    gp.liks = S.trace_on_device ? (const double *)(A->dev + S.d_liks) : nullptr;
    gp.theta_w = (double *)(dw + W.theta);
    gp.theta0_w = (double *)(dw + W.theta0);
    gp.liks_w = (double *)(dw + W.liks);
    gp.lik = nullptr; gp.lik_w = nullptr; gp.n_iter_w = nullptr; gp.blk = nullptr;
    HIPCHK(launch_gather_winners(gp, A->stream));
    char *ws = A->dev + S.d_ws;
    if (!S.trace_on_device && liks_w) {
        // the per-cell traces were too large to keep: re-run the winners alone (one cell per
        // series; a cell's result does not depend on its position in the grid) with a trace
        std::vector<int> sel_off((size_t)S.n_series + 1, 0);
        for (int i = 0; i < n_w; i++) sel_off[(size_t)w_series[i] + 1] = 1;
        for (int s = 0; s < S.n_series; s++) sel_off[(size_t)s + 1] += sel_off[(size_t)s];
        for (int i = 1; i < n_w; i++)
            if (w_series[i] <= w_series[i - 1]) return fail(LDSR_EINVAL, "internal: winners must be sorted by series");
        EmLaunch E = slice_launch(S);
        E.cell_offsets = sel_off.data();
        E.theta0 = (const double *)(dw + W.theta0);
        E.algo = S.plan.algo;           // the kernel of the batch run, whatever AUTO would pick for a few cells
        E.lead_force = S.plan.lead;
        E.liks = (double *)(dw + W.liks);
        int rc = em_batch_device_impl(E);
        if (rc) return rc;
    }
    // the winners' fit: one smoother pass at theta_w on the prepared series
    if (X || Y || V || J) {
        std::vector<int> soc(w_series, w_series + n_w);
        int rc = slice_fit(S, ws, dw, W, n_w, soc.data());
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(pw + W.out_begin, dw + W.out_begin, W.out_bytes, hipMemcpyDeviceToHost,
                          A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    for (int i = 0; i < n_w; i++) {
        if (liks_w) memcpy(liks_w + (size_t)i * niter, pw + W.liks + sizeof(double) * (size_t)i * niter, sizeof(double) * niter);
        const size_t row = sizeof(double) * (size_t)i * T;
        if (X) memcpy(X + (size_t)i * T, pw + W.X + row, sizeof(double) * T);
        if (Y) memcpy(Y + (size_t)i * T, pw + W.Y + row, sizeof(double) * T);
        if (V) memcpy(V + (size_t)i * T, pw + W.V + row, sizeof(double) * T);
        if (J) memcpy(J + (size_t)i * T, pw + W.J + row, sizeof(double) * T);
    }
    return LDSR_OK;
}

// Cut the cell grid over the devices BY SERIES: device d gets the d-th of n_devices contiguous
// parts of EVERY series' restarts.  Series differ a lot in iterations to converge (config 5: 34 k
// to 130 k E-steps per series), so contiguous ranges of the flattened grid -- round 2's cut -- left
// the devices up to 1.32x apart at eight; the reference hands each restart to whichever worker is
// idle (R/LDS_reconstruction.R:46), and restarts of one series are statistically alike, so equal
// shares of every series are equal shares of the work (1.004 / 1.007 / 1.012 at 2 / 4 / 8 on the
// same grid; tests/test_shard_gloo.py pins the bound).  Every slice carries all series (<= 100 KB
// each) and the whole call's offsets for AUTO's plan.
static void make_slices(std::vector<Slice> &sl, int n_devices, const int *devices, int n_series,
                        int T, int p, int q, const double *y, const double *u, const double *v,
                        int shared_uv, const int *cell_offsets, const double *theta0, int niter,
                        double tol, int algo, double *theta, double *lik, int *n_iter,
                        int *status, double *liks) {
    sl.resize((size_t)n_devices);
    for (int d = 0; d < n_devices; d++) {
        Slice &S = sl[(size_t)d];
        S.device = devices[d];
        S.T = T; S.p = p; S.q = q; S.shared_uv = shared_uv; S.niter = niter; S.tol = tol; S.algo = algo;
        S.off.assign((size_t)n_series + 1, 0);
        S.g_lo.assign((size_t)n_series, 0);
        for (int s = 0; s < n_series; s++) {
            const long long a = cell_offsets[s], ns = cell_offsets[s + 1] - cell_offsets[s];
            // part (d + s) mod n_devices of series s: the remainders of restart counts the device count
            // does not divide rotate over the devices (ldsr_amd/shard.py rank_slice is the same rule)
            const long long k = (d + s) % n_devices;
            const int lo = (int)(a + ns * k / n_devices), hi = (int)(a + ns * (k + 1) / n_devices);
            S.g_lo[(size_t)s] = lo;
            S.off[(size_t)s + 1] = S.off[(size_t)s] + (hi - lo);
        }
        S.n_series = S.off[(size_t)n_series] > 0 ? n_series : 0;
        S.y = y; S.u = u; S.v = v;
        S.theta0 = theta0;
        S.theta = theta; S.lik = lik; S.n_iter = n_iter; S.status = status; S.liks = liks;
        if (n_devices > 1) { S.plan_off = cell_offsets; S.plan_ns = n_series; }
    }
}

// run phase 1 of every slice, one host thread per slice beyond the first
static int run_slices(std::vector<Slice> &sl) {
    const size_t n = sl.size();
    std::vector<int> rcs(n, LDSR_OK);
    std::vector<std::string> msgs(n);
    std::atomic<int> running{0};
    auto work = [&](size_t d, bool worker) {
        if (worker) mark_worker_thread();
        rcs[d] = slice_run(sl[d]);
        if (rcs[d]) msgs[d] = thread_error();      // thread-local message of this worker
        if (worker) running.fetch_sub(1);
    };
    std::vector<std::thread> pool;
    for (size_t d = 1; d < n; d++)
        if (sl[d].n_series > 0) {
            running.fetch_add(1);
            pool.emplace_back(work, d, true);
        }
    if (n > 0 && sl[0].n_series > 0) work(0, false);
    while (thread_polls() && running.load() > 0) {     // keep the interrupt callback alive while joining
        intr_poll();
        usleep(200);
    }
    for (auto &t : pool) t.join();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    for (size_t d = 0; d < n; d++)
        if (rcs[d]) return fail(rcs[d], "device " + std::to_string(sl[d].device) + ": " + msgs[d]);
    return LDSR_OK;
}

extern "C" int ldsr_em_batch_multi(int n_devices, const int *devices, int n_series, int T, int p,
                                   int q, const double *y, const double *u, const double *v,
                                   int shared_uv, const int *cell_offsets, const double *theta0,
                                   int niter, double tol, int algo, double *theta, double *lik,
                                   int *n_iter, int *status, double *liks) {
    if (n_devices < 1 || !devices) return fail(LDSR_EINVAL, "n_devices must be >= 1");
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    rc = check_em(niter, tol);
    if (rc) return rc;
    if (!theta0 || !theta || !lik || !n_iter || !status) return fail(LDSR_EINVAL, "NULL pointer");
    if (cell_offsets[n_series] == 0) return LDSR_OK;
    IntrScope intr;
    std::vector<Slice> sl;
    make_slices(sl, n_devices, devices, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta0,
                niter, tol, algo, theta, lik, n_iter, status, liks);
    return run_slices(sl);
}

extern "C" int ldsr_em_batch(int device, int n_series, int T, int p, int q, const double *y,
                             const double *u, const double *v, int shared_uv,
                             const int *cell_offsets, const double *theta0, int niter, double tol,
                             int algo, double *theta, double *lik, int *n_iter, int *status,
                             double *liks) {
    return ldsr_em_batch_multi(1, &device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets,
                               theta0, niter, tol, algo, theta, lik, n_iter, status, liks);
}

extern "C" int ldsr_em_restart_grid(int n_devices, const int *devices, int n_series, int T, int p,
                                    int q, const double *y, const double *u, const double *v,
                                    int shared_uv, const int *cell_offsets, const double *theta0,
                                    int niter, double tol, int algo, double *theta_all,
                                    double *lik_all, int *n_iter_all, int *status_all, int *winner,
                                    double *theta_w, double *lik_w, int *n_iter_w, double *liks_w,
                                    double *X, double *Y, double *V, double *J) {
    if (n_devices < 1 || !devices) return fail(LDSR_EINVAL, "n_devices must be >= 1");
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    rc = check_em(niter, tol);
    if (rc) return rc;
    if (!theta0 || !winner || !theta_w || !lik_w || !n_iter_w)
        return fail(LDSR_EINVAL, "theta0, winner, theta_w, lik_w and n_iter_w must not be NULL");
    const int n_cells = cell_offsets[n_series];
    const int P = 6 + p + q;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    IntrScope intr;
    if (n_devices > n_cells) n_devices = n_cells > 0 ? n_cells : 1;
    // One slice: selection and the winners' fit are fused behind the EM kernel on the device and
    // the per-cell arrays cross PCIe only if asked for.  Several slices: per-cell results come
    // back first (temporaries if the caller did not ask), the host selects, then phase 2 runs on
    // the slice that owns each winner.
    const bool want_all = theta_all || lik_all || n_iter_all || status_all;
    const bool fused = n_devices == 1 && n_cells > 0 &&
                       sizeof(double) * (size_t)n_cells * niter <= liks_trace_cap_bytes();
    std::vector<double> t_theta, t_lik;
    std::vector<int> t_nit, t_st;
    if (!fused || want_all) {
        if (!theta_all) { t_theta.resize((size_t)n_cells * P + 1); theta_all = t_theta.data(); }
        if (!lik_all) { t_lik.resize((size_t)n_cells + 1); lik_all = t_lik.data(); }
        if (!n_iter_all) { t_nit.resize((size_t)n_cells + 1); n_iter_all = t_nit.data(); }
        if (!status_all) { t_st.resize((size_t)n_cells + 1); status_all = t_st.data(); }
    }
    std::vector<Slice> sl;
    make_slices(sl, n_devices, devices, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta0,
                niter, tol, algo, theta_all, lik_all, n_iter_all, status_all, nullptr);
    for (Slice &S : sl) S.max_winners = S.n_series;
    if (fused) {
        Slice &S = sl[0];
        S.fuse = true;
        S.want_all = want_all;
        S.h_winner = winner; S.h_theta_w = theta_w; S.h_lik_w = lik_w; S.h_nit_w = n_iter_w;
        S.h_liks_w = liks_w; S.h_X = X; S.h_Y = Y; S.h_V = V; S.h_J = J;
    }
    if (n_cells > 0) {
        rc = run_slices(sl);
        if (rc) return rc;
        if (fused) {
            if (!sl[0].fused_done) return fail(LDSR_EINVAL, "internal: fused restart path did not run");
            return LDSR_OK;     // winner[] is already global (one slice: lo = 0)
        }
    }
    // selection (R/LDS_reconstruction.R:50-58), per series over its restarts
    for (int s = 0; s < n_series; s++) {
        const int a = cell_offsets[s], b = cell_offsets[s + 1];
        const int k = ldsr_select_restart(b - a, lik_all + a, theta_all + (size_t)a * P, p, q);
        winner[s] = k < 0 ? -1 : a + k;
        if (k < 0) {
            for (int j = 0; j < P; j++) theta_w[(size_t)s * P + j] = nan;
            lik_w[s] = nan;
            n_iter_w[s] = 0;
        } else {
            memcpy(theta_w + (size_t)s * P, theta_all + (size_t)(a + k) * P, sizeof(double) * P);
            lik_w[s] = lik_all[a + k];
            n_iter_w[s] = n_iter_all[a + k];
        }
        if (k < 0) {
            if (liks_w) for (int i = 0; i < niter; i++) liks_w[(size_t)s * niter + i] = nan;
            double *rows[4] = {X, Y, V, J};
            for (double *r : rows)
                if (r) for (int t = 0; t < T; t++) r[(size_t)s * T + t] = nan;
        }
    }
    if (!liks_w && !X && !Y && !V && !J) return LDSR_OK;
    // phase 2 on the slice that owns each winner
    for (size_t d = 0; d < sl.size(); d++) {
        Slice &S = sl[d];
        if (S.n_series == 0) continue;
        std::vector<int> ws_, wc_, gs_;
        for (int s = 0; s < S.n_series; s++) {
            const int lo = S.g_lo[(size_t)s], nc = S.off[(size_t)s + 1] - S.off[(size_t)s];
            if (winner[s] >= lo && winner[s] < lo + nc) {
                ws_.push_back(s);
                wc_.push_back(S.off[(size_t)s] + winner[s] - lo);
                gs_.push_back(s);
            }
        }
        const int n_w = (int)ws_.size();
        if (!n_w) continue;
        std::vector<double> b_liks, b_X, b_Y, b_V, b_J;
        if (liks_w) b_liks.resize((size_t)n_w * niter);
        if (X) b_X.resize((size_t)n_w * T);
        if (Y) b_Y.resize((size_t)n_w * T);
        if (V) b_V.resize((size_t)n_w * T);
        if (J) b_J.resize((size_t)n_w * T);
        rc = slice_fit_winners(S, n_w, ws_.data(), wc_.data(), liks_w ? b_liks.data() : nullptr,
                               X ? b_X.data() : nullptr, Y ? b_Y.data() : nullptr,
                               V ? b_V.data() : nullptr, J ? b_J.data() : nullptr);
        if (rc) return rc;
        for (int i = 0; i < n_w; i++) {
            const size_t s = (size_t)gs_[(size_t)i];
            if (liks_w) memcpy(liks_w + s * niter, b_liks.data() + (size_t)i * niter, sizeof(double) * niter);
            if (X) memcpy(X + s * T, b_X.data() + (size_t)i * T, sizeof(double) * T);
            if (Y) memcpy(Y + s * T, b_Y.data() + (size_t)i * T, sizeof(double) * T);
            if (V) memcpy(V + s * T, b_V.data() + (size_t)i * T, sizeof(double) * T);
            if (J) memcpy(J + s * T, b_J.data() + (size_t)i * T, sizeof(double) * T);
        }
    }
    return LDSR_OK;
}

extern "C" int ldsr_em_restart_groups(int n_devices, const int *devices, int n_groups,
                                      ldsr_group *groups, int niter, double tol, int algo) {
    if (n_devices < 1 || !devices) return fail(LDSR_EINVAL, "n_devices must be >= 1");
    if (n_groups < 0 || (n_groups > 0 && !groups)) return fail(LDSR_EINVAL, "groups must not be NULL");
    std::vector<std::string> msgs((size_t)n_groups);
    IntrScope intr;
    std::atomic<int> running{0};
    auto work = [&](int g) {
        ldsr_group &G = groups[g];
        // rotate the device list so that concurrent groups start on different GPUs
        std::vector<int> devs((size_t)n_devices);
        for (int d = 0; d < n_devices; d++) devs[(size_t)d] = devices[(g + d) % n_devices];
        G.rc = ldsr_em_restart_grid(n_devices, devs.data(), G.n_series, G.T, G.p, G.q, G.y, G.u, G.v,
                                    G.shared_uv, G.cell_offsets, G.theta0, niter, tol, algo,
                                    G.theta_all, G.lik_all, G.n_iter_all, G.status_all, G.winner,
                                    G.theta_w, G.lik_w, G.n_iter_w, G.liks_w, G.X, G.Y, G.V, G.J);
        if (G.rc) msgs[(size_t)g] = thread_error();
    };
    // a bounded pool: at most 8 groups in flight (each holds one arena per device)
    const int n_workers = std::min(n_groups, 8);
    std::vector<std::thread> pool;
    for (int w = 0; w < n_workers; w++) {
        running.fetch_add(1);
        pool.emplace_back([&, w]() {
            mark_worker_thread();
            for (int g = w; g < n_groups; g += n_workers) work(g);
            running.fetch_sub(1);
        });
    }
    while (thread_polls() && running.load() > 0) {     // the caller's thread keeps the interrupt callback alive
        intr_poll();
        usleep(200);
    }
    for (auto &t : pool) t.join();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    for (int g = 0; g < n_groups; g++)
        if (groups[g].rc) return fail(groups[g].rc, "group " + std::to_string(g) + ": " + msgs[(size_t)g]);
    return LDSR_OK;
}

// R/LDS_reconstruction.R:50-58: best lik among models with C > 0 (NaN ignored); if no
// model has C > 0, which.max(liks).  First index on ties; -1 if nothing is selectable.
extern "C" int ldsr_select_restart(int n, const double *lik, const double *theta, int p, int q) {
    if (n <= 0 || !lik || !theta) return -1;
    const int P = 6 + p + q;
    bool any_pos = false;
    for (int i = 0; i < n; i++)
        if (theta[(size_t)i * P + 1 + p] > 0) { any_pos = true; break; }
    int best = -1;
    for (int i = 0; i < n; i++) {
        if (std::isnan(lik[i])) continue;
        if (any_pos && !(theta[(size_t)i * P + 1 + p] > 0)) continue;
        if (best < 0 || lik[i] > lik[best]) best = i;
    }
    return best;
}

}  // namespace ldsr_host
