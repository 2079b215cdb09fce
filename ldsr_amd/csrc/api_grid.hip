// api_grid.hip -- the host-pointer EM entries of the C ABI: slices of the cell grid over the devices, the restart
// grid with its winners' phase (one enqueue, one deliver, whoever selected), the group entry, and the restart
// selection rule.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "host_em.h"

namespace ldsr_host {

// The arguments of a host-pointer EM call, in the ABI's order; the entry fills it once and every slice refers to it.
// theta .. liks are the caller's whole per-cell arrays (liks optional: the full [n_cells][niter] trace, NaN padded);
// theta null (the restart grid on one slice only): nobody asked for them and they stay on the device.
struct GridCall {
    int n_series, T, p, q;
    const double *y, *u, *v;
    int shared_uv;
    const int *cell_offsets;
    const double *theta0;
    int niter;
    double tol;
    int algo;
    double *theta, *lik;
    int *n_iter, *status;
    double *liks;
    int P() const { return 6 + p + q; }
};

// the caller's winner outputs of the restart grid, one row per series (any of liks_w .. J may be NULL)
struct WinnerOut {
    int *winner;
    double *theta_w, *lik_w;
    int *n_iter_w;
    double *liks_w, *X, *Y, *V, *J;
    bool want_fit() const { return X || Y || V || J; }
};

// the winners' block of a slice for n rows (offsets relative to its start)
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

// ---- one slice of the cell grid on one device --------------------------------------------------
// slice_enqueue: ONE pinned->device copy of [y | u | v | theta0 | offsets], series_prep + EM kernel.  The per-cell
// block [theta | lik | n_iter | status] comes back in ONE device->pinned copy (slice_cells_enqueue, slice_scatter).
// The restart grid's winners' phase works on the same arena, which stays leased as long as the slice lives.
struct Slice {
    const GridCall *call = nullptr;
    int device = 0;
    // Striped cut (make_slices): the slice holds EVERY series of the call and, of series s, the cells
    // [g_lo[s], g_lo[s] + off[s+1] - off[s]) of the caller's arrays, gathered and scattered per series; `off` are
    // its local cell offsets.  n_series: the call's, or 0 for a slice without cells.
    int n_series = 0, n_cells = 0;
    std::vector<int> off, g_lo;
    const int *plan_off = nullptr;      // the whole call's offsets (EmLaunch), several devices only
    int plan_ns = 0;
    int max_winners = 0;        // > 0: reserve the winners' block and keep the traces on the device if they fit
    // state
    ArenaLease lease;
    int lead_steps = 0;         // data facts found in y (EmPlanIn)
    EmPlan plan;                // what the batch launch ran
    bool trace_on_device = false;
    WsLayout L;                 // (the winners' fit reuses the prepared series and the scan kernel's image)
    WinLayout W;
    size_t wsb = 0;
    size_t d_in = 0, d_y = 0, d_u = 0, d_v = 0, d_th0 = 0, d_off = 0, in_bytes = 0;      // device offsets
    size_t d_out = 0, d_theta = 0, d_lik = 0, d_nit = 0, d_st = 0, out_bytes = 0;
    size_t d_liks = 0, d_ws = 0, d_w = 0;
    size_t p_out = 0, p_w = 0;      // pinned offsets (the inputs are at 0)
};

static size_t liks_trace_cap_bytes() {
    const char *e = getenv("LDSR_LIKS_TRACE_MAX_BYTES");
    if (e && *e) return (size_t)strtoull(e, nullptr, 10);
    return (size_t)8 << 30;
}
static bool trace_fits(int n_cells, int niter) {
    return sizeof(double) * (size_t)n_cells * niter <= liks_trace_cap_bytes();
}

// the slice's block of its arena [inputs | per-cell outputs | trace | EM workspace | winners' block] and its
// pinned mirror [inputs | per-cell outputs | winners' block] (same relative layouts as on the device)
static int slice_layout(Slice &S) {
    const GridCall &G = *S.call;
    const int T = G.T, P = G.P(), n = S.n_cells;
    const size_t nuv = G.shared_uv ? 1 : (size_t)S.n_series;
    int rc = arena_acquire(S.device, &S.lease.a);
    if (rc) return rc;
    Carver c;
    S.d_in = c.o;
    S.d_y = c.take(sizeof(double) * (size_t)S.n_series * T);
    S.d_u = c.take(G.u ? sizeof(double) * nuv * T * G.p : 0);
    S.d_v = c.take(G.v ? sizeof(double) * nuv * T * G.q : 0);
    S.d_th0 = c.take(sizeof(double) * (size_t)n * P);
    S.d_off = c.take(sizeof(int) * ((size_t)S.n_series + 1));
    S.in_bytes = c.o - S.d_in;
    S.d_out = c.o;
    S.d_theta = c.take(sizeof(double) * (size_t)n * P);
    S.d_lik = c.take(sizeof(double) * (size_t)n);
    S.d_nit = c.take(sizeof(int) * (size_t)n);
    S.d_st = c.take(sizeof(int) * (size_t)n);
    S.out_bytes = c.o - S.d_out;
    S.trace_on_device = G.liks != nullptr || (S.max_winners > 0 && trace_fits(n, G.niter));
    S.d_liks = c.take(S.trace_on_device ? sizeof(double) * (size_t)n * G.niter : 0);
    S.wsb = ldsr_em_workspace_bytes(S.n_series, T, G.p, G.q, n, G.algo);
    if (!S.wsb) return fail(LDSR_EINVAL, "unsupported (T, p, q, algo) combination");
    S.d_ws = c.take(S.wsb);
    S.W = win_layout(std::max(S.max_winners, 1), P, T, G.niter);
    const size_t w_bytes = S.max_winners > 0 ? S.W.total : 0;
    S.d_w = c.take(w_bytes);
    S.p_out = align256(S.in_bytes);
    S.p_w = S.p_out + align256(S.out_bytes);
    return arena_reserve(S.lease.a, c, S.p_w + w_bytes,
                         "the EM slice (ldsr_em_batch / _multi / ldsr_em_restart_grid / _groups)");
}

// data facts of the series for the launch planner (EmPlanIn::lead_steps): -1 fully observed, else the all-missing
// lead common to every series (the pair family's closed form)
static int lead_steps(const double *y, int n_series, int T) {
    if (std::all_of(y, y + (size_t)n_series * T, [](double x) { return std::isfinite(x); })) return -1;
    int lead = T;
    for (int s = 0; s < n_series && lead > 0; s++) {
        int t = 0;
        while (t < lead && !std::isfinite(y[(size_t)s * T + t])) t++;
        lead = std::min(lead, t);
    }
    return lead;
}

// the inputs into the pinned block (and what the planner wants to know of y), then the one upload
static int slice_stage(Slice &S) {
    const GridCall &G = *S.call;
    const Arena *A = S.lease.a;
    const int T = G.T, P = G.P();
    const size_t nuv = G.shared_uv ? 1 : (size_t)S.n_series;
    char *pin = A->pin;
    memcpy(pin + (S.d_y - S.d_in), G.y, sizeof(double) * (size_t)S.n_series * T);
    S.lead_steps = lead_steps(G.y, S.n_series, T);
    if (G.u) memcpy(pin + (S.d_u - S.d_in), G.u, sizeof(double) * nuv * T * G.p);
    if (G.v) memcpy(pin + (S.d_v - S.d_in), G.v, sizeof(double) * nuv * T * G.q);
    for (int s = 0; s < S.n_series; s++)      // this slice's cells of every series
        memcpy(pin + (S.d_th0 - S.d_in) + sizeof(double) * (size_t)S.off[(size_t)s] * P,
               G.theta0 + (size_t)S.g_lo[(size_t)s] * P,
               sizeof(double) * (size_t)(S.off[(size_t)s + 1] - S.off[(size_t)s]) * P);
    memcpy(pin + (S.d_off - S.d_in), S.off.data(), sizeof(int) * ((size_t)S.n_series + 1));
    HIPCHK(hipMemcpyAsync(A->dev + S.d_in, pin, S.in_bytes, hipMemcpyHostToDevice, A->stream));
    return LDSR_OK;
}

// an EM launch of a slice on its arena: the uploaded series, the per-cell outputs and the workspace
static EmLaunch slice_launch(const Slice &S) {
    const GridCall &G = *S.call;
    const Arena *A = S.lease.a;
    EmLaunch E;
    E.device = S.device; E.stream = A->stream;
    E.n_series = S.n_series; E.T = G.T; E.p = G.p; E.q = G.q; E.shared_uv = G.shared_uv;
    E.y = (const double *)(A->dev + S.d_y);
    E.u = G.u ? (const double *)(A->dev + S.d_u) : nullptr;
    E.v = G.v ? (const double *)(A->dev + S.d_v) : nullptr;
    E.niter = G.niter; E.tol = G.tol;
    E.theta = (double *)(A->dev + S.d_theta); E.lik = (double *)(A->dev + S.d_lik);
    E.n_iter = (int *)(A->dev + S.d_nit); E.status = (int *)(A->dev + S.d_st);
    E.workspace = A->dev + S.d_ws; E.workspace_bytes = S.wsb;
    E.lead_steps = S.lead_steps;
    return E;
}

// the batch launch: every cell of the slice from its theta0
static int slice_em(Slice &S) {
    const GridCall &G = *S.call;
    const Arena *A = S.lease.a;
    EmLaunch E = slice_launch(S);
    E.cell_offsets = S.off.data();
    E.theta0 = (const double *)(A->dev + S.d_th0);
    E.algo = G.algo;
    E.liks = S.trace_on_device ? (double *)(A->dev + S.d_liks) : nullptr;
    E.liks_nanfill = G.liks != nullptr;
    E.abort_flag = intr_flag_for_kernels();
    E.plan_off = S.plan_off; E.plan_ns = S.plan_ns;
    const int rc = em_batch_device_impl(E);
    S.plan = E.plan;
    S.L = E.layout;
    return rc;
}

// everything up to the EM kernel, enqueued on the arena's stream; nothing waits
static int slice_enqueue(Slice &S) {
    int rc = slice_layout(S);
    if (!rc) rc = slice_stage(S);
    return rc ? rc : slice_em(S);
}

// per-cell results: the one copy to the pinned block, and from there (after the wait) to the caller's arrays,
// series by series
static hipError_t slice_cells_enqueue(const Slice &S) {
    const Arena *A = S.lease.a;
    return hipMemcpyAsync(A->pin + S.p_out, A->dev + S.d_out, S.out_bytes, hipMemcpyDeviceToHost, A->stream);
}
static void slice_scatter(const Slice &S) {
    const GridCall &G = *S.call;
    const char *pout = S.lease.a->pin + S.p_out;
    const int P = G.P();
    for (int s = 0; s < S.n_series; s++) {
        const size_t lo = (size_t)S.off[(size_t)s], nc = (size_t)S.off[(size_t)s + 1] - lo, g = (size_t)S.g_lo[(size_t)s];
        if (!nc) continue;
        memcpy(G.theta + g * P, pout + (S.d_theta - S.d_out) + sizeof(double) * lo * P, sizeof(double) * nc * P);
        memcpy(G.lik + g, pout + (S.d_lik - S.d_out) + sizeof(double) * lo, sizeof(double) * nc);
        memcpy(G.n_iter + g, pout + (S.d_nit - S.d_out) + sizeof(int) * lo, sizeof(int) * nc);
        memcpy(G.status + g, pout + (S.d_st - S.d_out) + sizeof(int) * lo, sizeof(int) * nc);
    }
}

// a slice of the batch entries, and of a restart grid whose selection is the host's: run, wait, hand the cells back
static int slice_run(Slice &S) {
    if (S.n_cells == 0) return LDSR_OK;
    const GridCall &G = *S.call;
    const int rc = slice_enqueue(S);
    if (rc) return rc;
    const Arena *A = S.lease.a;
    HIPCHK(slice_cells_enqueue(S));
    HIPCHK(wait_stream(A->stream));
    slice_scatter(S);
    for (int s = 0; G.liks && s < S.n_series; s++) {    // the full trace goes straight to the caller's (pageable) array
        const size_t lo = (size_t)S.off[(size_t)s], nc = (size_t)S.off[(size_t)s + 1] - lo;
        if (nc)
            HIPCHK(hipMemcpy(G.liks + (size_t)S.g_lo[(size_t)s] * G.niter, A->dev + S.d_liks + sizeof(double) * lo * G.niter,
                             sizeof(double) * nc * G.niter, hipMemcpyDeviceToHost));
    }
    return LDSR_OK;
}

// ---- the winners' phase of the restart grid ----------------------------------------------------
// winners_enqueue puts a slice's work for its winners on the stream behind the EM kernel and does not wait: the
// gather of their theta, lik, n_iter and trace into the winners' block (the kernel also writes the fit's block table,
// one winner per block), the re-run of the winners alone where the traces were too large to keep, the FIT smoother
// when any of X / Y / V / J is wanted, and the copy of the block to pinned memory.  Row i of the block is the winner
// of series rows[i] (ascending).  w_cell: its local cell index, uploaded with the series; null: the cells are in
// W.cell already (select_winners_kernel: row i = series i, -1 = none).
static int winners_enqueue(Slice &S, const std::vector<int> &rows, const int *w_cell, const WinnerOut &out) {
    const GridCall &G = *S.call;
    const Arena *A = S.lease.a;
    const WinLayout &W = S.W;
    const int n_w = (int)rows.size();
    char *dw = A->dev + S.d_w, *pw = A->pin + S.p_w;
    HIPCHK(hipSetDevice(S.device));
    if (w_cell) {
        memcpy(pw + W.cell, w_cell, sizeof(int) * n_w);
        memcpy(pw + W.ser, rows.data(), sizeof(int) * n_w);
        HIPCHK(hipMemcpyAsync(dw + W.cell, pw + W.cell, sizeof(int) * n_w, hipMemcpyHostToDevice, A->stream));
        HIPCHK(hipMemcpyAsync(dw + W.ser, pw + W.ser, sizeof(int) * n_w, hipMemcpyHostToDevice, A->stream));
    }
    GatherParams gp;
    gp.n_w = n_w; gp.P = G.P(); gp.niter = G.niter;
    gp.cell = (const int *)(dw + W.cell);
    gp.ser = w_cell ? (const int *)(dw + W.ser) : nullptr;
    gp.theta = (const double *)(A->dev + S.d_theta); gp.theta0 = (const double *)(A->dev + S.d_th0);
    gp.lik = (const double *)(A->dev + S.d_lik); gp.n_iter = (const int *)(A->dev + S.d_nit);
    gp.liks = S.trace_on_device ? (const double *)(A->dev + S.d_liks) : nullptr;
    gp.theta_w = (double *)(dw + W.theta); gp.theta0_w = (double *)(dw + W.theta0);
    gp.liks_w = (double *)(dw + W.liks);
    gp.lik_w = (double *)(dw + W.lik_w); gp.n_iter_w = (int *)(dw + W.nit_w);
    gp.blk = (int *)(dw + W.blk);
    HIPCHK(launch_gather_winners(gp, A->stream));
    if (!S.trace_on_device && out.liks_w) {
        // the per-cell traces were too large to keep: re-run the winners alone (one cell per
        // series; a cell's result does not depend on its position in the grid) with a trace
        std::vector<int> sel_off((size_t)S.n_series + 1, 0);
        for (int i = 0; i < n_w; i++) sel_off[(size_t)rows[(size_t)i] + 1] = 1;
        for (int s = 0; s < S.n_series; s++) sel_off[(size_t)s + 1] += sel_off[(size_t)s];
        if (sel_off[(size_t)S.n_series] != n_w || !std::is_sorted(rows.begin(), rows.end()))
            return fail(LDSR_EINVAL, "internal: winners must be sorted by series");
        EmLaunch E = slice_launch(S);
        E.cell_offsets = sel_off.data();
        E.theta0 = (const double *)(dw + W.theta0);
        E.algo = S.plan.algo;           // the kernel of the batch run, whatever AUTO would pick for a few cells
        E.lead_force = S.plan.lead;
        E.liks = (double *)(dw + W.liks);
        const int rc = em_batch_device_impl(E);
        if (rc) return rc;
    }
    if (out.want_fit()) {       // one smoother pass at theta_w on the series the batch launch prepared
        const PreparedSeries PS{S.device, A->stream, G.T, G.p, G.q, ldsr_pad_dim(G.p), ldsr_pad_dim(G.q), G.shared_uv,
                                G.u != nullptr, G.v != nullptr, A->dev + S.d_ws, &S.L};
        const FitOut F{(double *)(dw + W.X), (double *)(dw + W.Y), (double *)(dw + W.V), (double *)(dw + W.J),
                       (double *)(dw + W.lik), nullptr, (int *)(dw + W.st)};
        // (rows: the cell -> series map, uploaded to W.ser, of a shape only the serial smoother runs)
        const int rc = launch_smoother(PS, n_w, rows.data(), (const double *)(dw + W.theta), 1, 0, 0.0, F,
                                       (int *)(dw + W.ser), (const int *)(dw + W.blk));
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(pw + W.out_begin, dw + W.out_begin, W.out_bytes, hipMemcpyDeviceToHost, A->stream));
    return LDSR_OK;
}

// a series without a winner (R's which.max on all-NA gives integer(0)): -1, NaN rows, no iterations
static void fill_no_winner(const GridCall &G, const WinnerOut &out, int s) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out.winner[s] = -1;
    std::fill_n(out.theta_w + (size_t)s * G.P(), G.P(), nan);
    out.lik_w[s] = nan;
    out.n_iter_w[s] = 0;
    if (out.liks_w) std::fill_n(out.liks_w + (size_t)s * G.niter, G.niter, nan);
    for (double *r : {out.X, out.Y, out.V, out.J})
        if (r) std::fill_n(r + (size_t)s * G.T, G.T, nan);
}

// After the wait: row i of the pinned winners' block -> row rows[i] of the caller's arrays, the winner as a cell
// index of the whole call.  (Where the host selected, winner .. n_iter_w hold the same numbers already.)
static void winners_deliver(const Slice &S, const std::vector<int> &rows, const WinnerOut &out) {
    const GridCall &G = *S.call;
    const WinLayout &W = S.W;
    const char *pw = S.lease.a->pin + S.p_w;
    const int *cell = (const int *)(pw + W.cell);
    for (size_t i = 0; i < rows.size(); i++) {
        const size_t s = (size_t)rows[i];
        if (cell[i] < 0) {
            fill_no_winner(G, out, (int)s);
            continue;
        }
        auto row = [&](double *dst, size_t from, size_t len) {
            if (dst) memcpy(dst + s * len, pw + from + sizeof(double) * i * len, sizeof(double) * len);
        };
        out.winner[s] = S.g_lo[s] + cell[i] - S.off[s];
        out.lik_w[s] = ((const double *)(pw + W.lik_w))[i];
        out.n_iter_w[s] = ((const int *)(pw + W.nit_w))[i];
        row(out.theta_w, W.theta, (size_t)G.P());
        row(out.liks_w, W.liks, (size_t)G.niter);
        row(out.X, W.X, (size_t)G.T);
        row(out.Y, W.Y, (size_t)G.T);
        row(out.V, W.V, (size_t)G.T);
        row(out.J, W.J, (size_t)G.T);
    }
}

// The whole restart grid on one slice, its traces on the device: selection and the winners' phase go on the stream
// right behind the EM kernel and everything comes back with ONE wait; the per-cell arrays cross PCIe only if the
// caller asked for them.
static int slice_restart(Slice &S, const WinnerOut &out) {
    const GridCall &G = *S.call;
    int rc = slice_enqueue(S);
    if (rc) return rc;
    const Arena *A = S.lease.a;
    SelectParams sel;
    sel.n_series = S.n_series; sel.P = G.P(); sel.c_index = 1 + G.p;
    sel.off = (const int *)(A->dev + S.d_off);
    sel.theta = (const double *)(A->dev + S.d_theta); sel.lik = (const double *)(A->dev + S.d_lik);
    sel.winner = (int *)(A->dev + S.d_w + S.W.cell);
    HIPCHK(launch_select_winners(sel, A->stream));
    std::vector<int> rows((size_t)S.n_series);
    std::iota(rows.begin(), rows.end(), 0);
    rc = winners_enqueue(S, rows, nullptr, out);
    if (rc) return rc;
    if (G.theta) HIPCHK(slice_cells_enqueue(S));
    HIPCHK(wait_stream(A->stream));
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    if (G.theta) slice_scatter(S);
    winners_deliver(S, rows, out);
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
static void make_slices(std::vector<Slice> &sl, const GridCall &G, int n_devices, const int *devices) {
    const int n_series = G.n_series;
    sl.resize((size_t)n_devices);
    for (int d = 0; d < n_devices; d++) {
        Slice &S = sl[(size_t)d];
        S.call = &G;
        S.device = devices[d];
        S.off.assign((size_t)n_series + 1, 0);
        S.g_lo.assign((size_t)n_series, 0);
        for (int s = 0; s < n_series; s++) {
            const long long a = G.cell_offsets[s], ns = G.cell_offsets[s + 1] - G.cell_offsets[s];
            // part (d + s) mod n_devices of series s: the remainders of restart counts the device count
            // does not divide rotate over the devices (ldsr_amd/shard.py rank_slice is the same rule)
            const long long k = (d + s) % n_devices;
            const int lo = (int)(a + ns * k / n_devices), hi = (int)(a + ns * (k + 1) / n_devices);
            S.g_lo[(size_t)s] = lo;
            S.off[(size_t)s + 1] = S.off[(size_t)s] + (hi - lo);
        }
        S.n_cells = S.off[(size_t)n_series];
        S.n_series = S.n_cells > 0 ? n_series : 0;
        if (n_devices > 1) { S.plan_off = G.cell_offsets; S.plan_ns = n_series; }
    }
}

// Jobs 0 .. n-1 on n_threads threads, job i on thread i mod n_threads; inline0: thread 0 is the caller's own.
// The caller's thread keeps the interrupt callback alive until every worker is done, then joins; the first failed
// job is reported as "<noun> <ids[i]>: <its message>".
static int run_jobs(int n, int n_threads, bool inline0, const std::function<int(int)> &job, const char *noun,
                    const std::vector<int> &ids) {
    std::vector<int> rcs((size_t)std::max(n, 0), LDSR_OK);
    std::vector<std::string> msgs(rcs.size());
    std::atomic<int> running{0};
    auto work = [&](int w, bool worker) {
        if (worker) mark_worker_thread();
        for (int i = w; i < n; i += n_threads) {
            rcs[(size_t)i] = job(i);
            if (rcs[(size_t)i]) msgs[(size_t)i] = thread_error();      // thread-local message of this thread
        }
        if (worker) running.fetch_sub(1);
    };
    std::vector<std::thread> pool;
    for (int w = inline0 ? 1 : 0; w < n_threads; w++) {
        running.fetch_add(1);
        pool.emplace_back(work, w, true);
    }
    if (inline0 && n_threads > 0) work(0, false);
    while (thread_polls() && running.load() > 0) {
        intr_poll();
        usleep(200);
    }
    for (auto &t : pool) t.join();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    for (int i = 0; i < n; i++)
        if (rcs[(size_t)i])
            return fail(rcs[(size_t)i], noun + std::to_string(ids[(size_t)i]) + ": " + msgs[(size_t)i]);
    return LDSR_OK;
}

// every slice at once: slice 0 on the caller's thread, one worker per further slice that has cells
static int run_slices(std::vector<Slice> &sl, const std::function<int(Slice &)> &run) {
    std::vector<Slice *> live;
    std::vector<int> devs;
    for (Slice &S : sl)
        if (&S == &sl[0] || S.n_cells > 0) { live.push_back(&S); devs.push_back(S.device); }
    const int n = (int)live.size();
    return run_jobs(n, n, true, [&](int i) { return run(*live[(size_t)i]); }, "device ", devs);
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
    const GridCall G{n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta0, niter, tol, algo,
                     theta, lik, n_iter, status, liks};
    std::vector<Slice> sl;
    make_slices(sl, G, n_devices, devices);
    return run_slices(sl, slice_run);
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
    const int n_cells = cell_offsets[n_series], P = 6 + p + q;
    IntrScope intr;
    if (n_devices > n_cells) n_devices = n_cells > 0 ? n_cells : 1;
    // One slice that can keep its traces selects on the device (slice_restart), and the per-cell arrays cross
    // PCIe only if asked for.  Anything else brings the per-cell results back first (to temporaries if the caller
    // did not ask) and selects here.  The winners' phase after the selection is the same.
    const bool want_all = theta_all || lik_all || n_iter_all || status_all;
    const bool select_on_device = n_devices == 1 && n_cells > 0 && trace_fits(n_cells, niter);
    std::vector<double> t_theta, t_lik;
    std::vector<int> t_nit, t_st;
    if (!select_on_device || want_all) {
        if (!theta_all) { t_theta.resize((size_t)n_cells * P + 1); theta_all = t_theta.data(); }
        if (!lik_all) { t_lik.resize((size_t)n_cells + 1); lik_all = t_lik.data(); }
        if (!n_iter_all) { t_nit.resize((size_t)n_cells + 1); n_iter_all = t_nit.data(); }
        if (!status_all) { t_st.resize((size_t)n_cells + 1); status_all = t_st.data(); }
    }
    const GridCall G{n_series, T, p, q, y, u, v, shared_uv, cell_offsets, theta0, niter, tol, algo,
                     theta_all, lik_all, n_iter_all, status_all, nullptr};
    const WinnerOut out{winner, theta_w, lik_w, n_iter_w, liks_w, X, Y, V, J};
    std::vector<Slice> sl;
    make_slices(sl, G, n_devices, devices);
    for (Slice &S : sl) S.max_winners = S.n_series;
    if (select_on_device) return run_slices(sl, [&](Slice &S) { return slice_restart(S, out); });
    if (n_cells > 0) {
        rc = run_slices(sl, slice_run);
        if (rc) return rc;
    }
    // selection (R/LDS_reconstruction.R:50-58), per series over its restarts, and what it read of the winner
    for (int s = 0; s < n_series; s++) {
        const int a = cell_offsets[s], b = cell_offsets[s + 1];
        const int k = ldsr_select_restart(b - a, lik_all + a, theta_all + (size_t)a * P, p, q);
        if (k < 0) {
            fill_no_winner(G, out, s);
            continue;
        }
        winner[s] = a + k;
        memcpy(theta_w + (size_t)s * P, theta_all + (size_t)(a + k) * P, sizeof(double) * P);
        lik_w[s] = lik_all[a + k];
        n_iter_w[s] = n_iter_all[a + k];
    }
    if (!liks_w && !out.want_fit()) return LDSR_OK;     // nothing more is wanted: no device work, no wait
    // the winners' phase on the slice that owns each winner, one slice after the other
    for (Slice &S : sl) {
        std::vector<int> rows, cells;
        for (int s = 0; s < S.n_series; s++) {
            const int lo = S.g_lo[(size_t)s], nc = S.off[(size_t)s + 1] - S.off[(size_t)s];
            if (winner[s] >= lo && winner[s] < lo + nc) {
                rows.push_back(s);
                cells.push_back(S.off[(size_t)s] + winner[s] - lo);
            }
        }
        if (rows.empty()) continue;
        rc = winners_enqueue(S, rows, cells.data(), out);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(S.lease.a->stream));
        winners_deliver(S, rows, out);
    }
    return LDSR_OK;
}

extern "C" int ldsr_em_restart_groups(int n_devices, const int *devices, int n_groups,
                                      ldsr_group *groups, int niter, double tol, int algo) {
    if (n_devices < 1 || !devices) return fail(LDSR_EINVAL, "n_devices must be >= 1");
    if (n_groups < 0 || (n_groups > 0 && !groups)) return fail(LDSR_EINVAL, "groups must not be NULL");
    IntrScope intr;
    auto work = [&](int g) {
        ldsr_group &G = groups[g];
        // rotate the device list so that concurrent groups start on different GPUs
        std::vector<int> devs((size_t)n_devices);
        for (int d = 0; d < n_devices; d++) devs[(size_t)d] = devices[(g + d) % n_devices];
        G.rc = ldsr_em_restart_grid(n_devices, devs.data(), G.n_series, G.T, G.p, G.q, G.y, G.u, G.v,
                                    G.shared_uv, G.cell_offsets, G.theta0, niter, tol, algo,
                                    G.theta_all, G.lik_all, G.n_iter_all, G.status_all, G.winner,
                                    G.theta_w, G.lik_w, G.n_iter_w, G.liks_w, G.X, G.Y, G.V, G.J);
        return G.rc;
    };
    // a bounded pool: at most 8 groups in flight (each holds one arena per device)
    std::vector<int> ids((size_t)n_groups);
    std::iota(ids.begin(), ids.end(), 0);
    return run_jobs(n_groups, std::min(n_groups, 8), false, work, "group ", ids);
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
