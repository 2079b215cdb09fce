// api_em.hip -- the EM side of the C ABI: which kernel a launch runs and its workspace layout, the plan and
// inventory queries, the device-pointer EM entries, and the smoother pass the other host units call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "host_em.h"
#include "em_pair_impl.h"      // (layout constants only: ws_layout)

namespace ldsr_host {

// ---- workspace layout (which kernel runs: em_plan.hip) ------------------------------------------
// compute units of a device (cached; a bad device id fails at hipSetDevice)
static int device_cu_count(int device) {
    if (device < 0) return 256;
    static std::mutex mu;
    static std::vector<int> cache;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)cache.size() <= device) cache.resize((size_t)device + 1, 0);
    if (!cache[(size_t)device]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
        cache[(size_t)device] = n;
    }
    return cache[(size_t)device];
}

// name of the EM kernel of the most recent launch per device (ldsr_last_em_kernel)
static std::mutex g_last_mu;
static std::vector<std::string> g_last_kernel;
static void remember_kernel(int device, const char *name) {
    std::lock_guard<std::mutex> lk(g_last_mu);
    if ((int)g_last_kernel.size() <= device) g_last_kernel.resize((size_t)device + 1);
    g_last_kernel[(size_t)device] = name;
}
extern "C" int ldsr_last_em_kernel(int device, char *buf, size_t len) {
    std::lock_guard<std::mutex> lk(g_last_mu);
    if (device < 0 || (int)g_last_kernel.size() <= device || g_last_kernel[(size_t)device].empty() || !buf || !len)
        return -1;
    snprintf(buf, len, "%s", g_last_kernel[(size_t)device].c_str());
    return 0;
}

WsLayout ws_layout(int n_series, int T, int PP, int QQ, int shared_uv, int n_cells,
                   int algo, int cpb) {
    WsLayout L;
    size_t o = 0;
    L.sc = o; o = align256(o + sizeof(SeriesConst) * (size_t)n_series);
    L.yp = o; o = align256(o + sizeof(double) * (size_t)n_series * T);
    L.yz = o; o = align256(o + sizeof(double) * (size_t)n_series * T);
    const size_t nuv = shared_uv ? 1 : (size_t)n_series;
    L.up = o; o = align256(o + sizeof(double) * nuv * T * PP);
    L.vp = o; o = align256(o + sizeof(double) * nuv * T * QQ);
    // chunk-transposed images for the scan kernel (also built for serial-kernel EM launches
    // whose shape the scan kernel supports: the winners' fit then runs on the scan kernel)
    em_scan_layout(T, PP, QQ, &L.img_L, &L.img_NL, &L.img_stride);
    L.img = o; o = align256(o + sizeof(double) * (size_t)L.img_stride * n_series);
    // room for the pair family's images whatever runs in the end (the launch decides: member,
    // chunk length, a closed-form lead): the largest 32-lane image, and u_t of a lead of up to T steps
    L.img2_stride = 0; L.img3_stride = 0;
    if (PP <= 8 && QQ <= 8 && algo != LDSR_ALGO_SERIAL) {
        // (wide inputs: the LEAD form's tail only, chunks of <= 16 steps)
        L.img2_stride = pair_image_doubles(PP <= 4 && QQ <= 4 ? 32 : 16, PP, QQ, 32);
        L.img3_stride = (long)(T + 32) * PP;
    }
    L.img2 = o; o = align256(o + sizeof(double) * (size_t)L.img2_stride * n_series);
    L.img3 = o; o = align256(o + sizeof(double) * (size_t)L.img3_stride * n_series);
    if (L.img_stride) cpb = std::min(cpb, em_scan_cells_per_block(T, PP, QQ));   // the winners' FIT launch
    if (PP <= 8 && QQ <= 8 && algo != LDSR_ALGO_SERIAL) cpb = std::min(cpb, 4);    // the pair family's smallest workgroup
    L.max_blocks = n_cells / cpb + n_series + 1;
    // (block table, then the device copy of the cell offsets for series_prep's cell ordering)
    L.blk = o; o = align256(o + sizeof(int) * (3 * (size_t)L.max_blocks + (size_t)n_series + 1));
    L.soc = o; o = align256(o + sizeof(int) * (size_t)(n_cells > 0 ? n_cells : 1));
    L.queue = o; o = align256(o + sizeof(int) * (size_t)n_series);
    // cell order of the pair kernel's steady form (two cells per wave, narrow inputs): position -> cell, and the keys
    const bool may_order = PP <= 4 && QQ <= 4 && algo != LDSR_ALGO_SERIAL;
    L.perm = o; o = align256(o + (may_order ? sizeof(int) * (size_t)(n_cells > 0 ? n_cells : 1) : 0));
    L.perm_key = o; o = align256(o + (may_order ? sizeof(int) * (size_t)(n_cells > 0 ? n_cells : 1) : 0));
    L.scratch_stride = ((long)n_cells + 63) / 64 * 64;
    L.scratch = o;
    if (algo == LDSR_ALGO_SERIAL) o = align256(o + sizeof(double) * 2 * (size_t)T * L.scratch_stride);
    L.total = o;
    return L;
}

extern "C" size_t ldsr_em_workspace_bytes(int n_series, int T, int p, int q, int n_cells,
                                          int algo) {
    if (n_series < 1 || n_cells < 0) return 0;
    EmPlanIn in;
    in.T = T; in.p = p; in.q = q; in.niter = 2; in.algo = algo;
    const EmPlan pl = em_plan(in);
    if (!pl.ok) return 0;
    // the layout for shared_uv = 0 is an upper bound for shared_uv = 1
    return ws_layout(n_series, T, pl.PP, pl.QQ, 0, n_cells, pl.algo_layout, pl.layout_cpb).total;
}

// what a launch that fills the device runs (lead_steps: -1 fully observed, 0 unknown, > 0 common lead)
extern "C" int ldsr_em_plan_lead(int T, int p, int q, int niter, double tol, int algo, int lead_steps,
                                 char *buf, size_t len) {
    EmPlanIn in;
    in.T = T; in.p = p; in.q = q; in.niter = niter; in.tol = tol; in.algo = algo; in.lead_steps = lead_steps;
    const EmPlan pl = em_plan(in);
    if (!pl.ok) return -1;
    if (buf && len) em_plan_kernel_name(pl, buf, len);
    return pl.algo;
}

extern "C" int ldsr_em_plan(int T, int p, int q, int niter, double tol, int algo, char *buf,
                            size_t len) {
    return ldsr_em_plan_lead(T, p, q, niter, tol, algo, 0, buf, len);
}

// the kernel one Kalman_smoother pass of this shape runs (launch_smoother): the FIT form of the scan
// kernel where its plan holds, else the serial smoother (returns LDSR_ALGO_SERIAL, empty name)
extern "C" int ldsr_smooth_plan(int T, int p, int q, char *buf, size_t len) {
    if (T < 2 || p < 1 || q < 1 || p > LDSR_MAXPQ || q > LDSR_MAXPQ) return -1;
    const int PP = ldsr_pad_dim(p), QQ = ldsr_pad_dim(q);
    if (buf && len) buf[0] = 0;
    if (!em_scan_supported(T, PP, QQ)) return LDSR_ALGO_SERIAL;
    if (buf && len) em_scan_kernel_name(T, PP, QQ, false, true, buf, len);
    return LDSR_ALGO_SCAN;
}

// names of every compiled instantiation of the scan and pair families, one per line; returns the
// length needed (including the terminating 0)
extern "C" size_t ldsr_kernel_inventory(char *buf, size_t len) {
    std::string s;
    em_kernel_inventory(s);
    if (buf && len) snprintf(buf, len, "%s", s.c_str());
    return s.size() + 1;
}

// series_prep's parameters for the prepared series and, with scan_img, the scan kernel's image (an EM
// launch of the pair family adds its images and the steady form's cell order)
PrepParams prep_params(int n_series, int T, int p, int q, int PP, int QQ, const double *d_y,
                       const double *d_u, const double *d_v, int shared_uv, char *ws,
                       const WsLayout &L, bool scan_img) {
    PrepParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.T = T; pp.p = p; pp.q = q; pp.PP = PP; pp.QQ = QQ; pp.shared_uv = shared_uv;
    pp.y = d_y; pp.u = d_u; pp.v = d_v;
    pp.yp = (double *)(ws + L.yp);
    pp.yz = (double *)(ws + L.yz);
    pp.up = (double *)(ws + L.up);
    pp.vp = (double *)(ws + L.vp);
    pp.sc = (SeriesConst *)(ws + L.sc);
    pp.queue = (int *)(ws + L.queue);
    pp.img = (L.img_stride && scan_img) ? (double *)(ws + L.img) : nullptr;
    pp.img_stride = L.img_stride;
    pp.L = L.img_L;
    pp.NL = L.img_NL;
    pp.n_series = n_series;
    return pp;
}

// A launch's blocks {series, first cell, n cells} (blocks never straddle a series) as the kernels read them: the
// table [series | first cell | n cells], each column n_blocks long
typedef std::array<int, 3> Block;
static std::vector<int> block_table(const std::vector<Block> &blocks) {
    const size_t n = blocks.size();
    std::vector<int> tab(3 * n);
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < 3; k++) tab[k * n + i] = blocks[i][k];
    return tab;
}

int em_batch_device_impl(EmLaunch &E) {
    const int n_series = E.n_series, T = E.T, p = E.p, q = E.q;
    const int *cell_offsets = E.cell_offsets;
    int rc = check_common(n_series, T, p, q, E.y, cell_offsets);
    if (rc) return rc;
    rc = check_em(E.niter, E.tol);
    if (rc) return rc;
    if (!E.theta0 || !E.theta || !E.lik || !E.n_iter || !E.status || !E.workspace)
        return fail(LDSR_EINVAL, "NULL output / workspace pointer");
    const int n_cells = cell_offsets[n_series];
    if (n_cells == 0) return LDSR_OK;
    EmPlanIn in;
    in.T = T; in.p = p; in.q = q; in.niter = E.niter; in.tol = E.tol; in.algo = E.algo;
    in.lead_steps = E.lead_steps; in.lead_force = E.lead_force; in.cus = device_cu_count(E.device);
    in.off = E.plan_off ? E.plan_off : cell_offsets;
    in.n_series = E.plan_off ? E.plan_ns : n_series;
    const EmPlan pl = E.plan = em_plan(in);
    if (!pl.ok) return fail(pl.err, pl.msg);
    const int PP = pl.PP, QQ = pl.QQ, cpb = pl.cpb;
    const WsLayout &L = E.layout = ws_layout(n_series, T, PP, QQ, E.shared_uv, n_cells, pl.algo_layout, pl.layout_cpb);
    if (E.workspace_bytes < L.total)
        return fail(LDSR_EINVAL, "workspace too small: need " + std::to_string(L.total) + " bytes");
    if (((size_t)E.workspace & 255) != 0) return fail(LDSR_EINVAL, "workspace must be 256-byte aligned");
    HIPCHK(hipSetDevice(E.device));
    char *ws = (char *)E.workspace;

    // block table.  Static schedule: (series, first cell, n cells of the block).  Work queue: (series, first
    // cell of the SERIES, n cells of the series) -- waves pull cells from the per-series queue.
    std::vector<Block> blocks;
    for (int s = 0; s < n_series; s++)
        for (int c = cell_offsets[s]; c < cell_offsets[s + 1]; c += cpb)
            blocks.push_back(pl.queue ? Block{s, cell_offsets[s], cell_offsets[s + 1] - cell_offsets[s]}
                                      : Block{s, c, std::min(cpb, cell_offsets[s + 1] - c)});
    const int n_blocks = (int)blocks.size();
    if (n_blocks > L.max_blocks) return fail(LDSR_EINVAL, "internal: block table overflow");
    std::vector<int> tab = block_table(blocks);
    int *d_tab = (int *)(ws + L.blk);
    const bool scan_img = E.fit_follows || !pl.cpw;
    PrepParams pp = prep_params(n_series, T, p, q, PP, QQ, E.y, E.u, E.v, E.shared_uv, ws, L, scan_img);
    if (pl.cpw) {       // the image of the member that runs (the room is for the largest)
        pp.img2 = L.img2_stride ? (double *)(ws + L.img2) : nullptr;
        pp.img2_stride = L.img2_stride;
        pp.L2 = pl.chunk;
        pp.NL2 = pl.lpc;
        pp.lead = pl.lead;
        pp.img3 = (pl.lead > 0 && L.img3_stride) ? (double *)(ws + L.img3) : nullptr;
        pp.img3_stride = L.img3_stride;
    }
    if (pl.steady_order) {     // (series_prep reads the cell offsets from the device copy behind the block table)
        tab.insert(tab.end(), cell_offsets, cell_offsets + n_series + 1);
        pp.perm = (int *)(ws + L.perm);
        pp.perm_key = (int *)(ws + L.perm_key);
        pp.cell_off = d_tab + 3 * n_blocks;
        pp.theta0 = E.theta0;
        pp.order_cpb = pl.queue ? 0 : cpb;
        pp.order_ntr = pl.chunk - 1;
    }
    rc = stage_h2d_async(E.device, E.stream, d_tab, tab.data(), sizeof(int) * tab.size());
    if (rc) return rc;
    HIPCHK(launch_series_prep(pp, n_series, E.stream));

    EmParams prm;
    prm.T = T; prm.p = p; prm.q = q; prm.has_u = E.u != nullptr; prm.has_v = E.v != nullptr;
    prm.niter = E.niter; prm.n_cells = n_cells; prm.tol = E.tol;
    prm.liks_nanfill = E.liks_nanfill;
    prm.abort = E.abort_flag;
    prm.yp = (const double *)(ws + L.yp);
    prm.yz = (const double *)(ws + L.yz);
    prm.up = (const double *)(ws + L.up);
    prm.vp = (const double *)(ws + L.vp);
    prm.u_stride = E.shared_uv ? 0 : (long)T * PP;
    prm.v_stride = E.shared_uv ? 0 : (long)T * QQ;
    prm.img = scan_img ? (const double *)(ws + L.img) : nullptr;
    prm.img_stride = L.img_stride;
    prm.img2 = pp.img2;
    prm.img2_stride = pp.img2_stride;
    prm.lead = pl.lead;
    prm.img3 = pp.img3;
    prm.img3_stride = pp.img3_stride;
    prm.fitX = prm.fitY = prm.fitV = prm.fitJ = prm.pen = nullptr;
    prm.lambda = 0.0;
    prm.stdlik = 1;
    prm.sc = (const SeriesConst *)(ws + L.sc);
    prm.blk_series = d_tab;
    prm.blk_cell0 = d_tab + n_blocks;
    prm.blk_ncell = d_tab + 2 * n_blocks;
    prm.theta0 = E.theta0;
    prm.theta = E.theta; prm.lik = E.lik; prm.liks = E.liks;
    prm.n_iter = E.n_iter; prm.status = E.status;
    prm.queue = (int *)(ws + L.queue);
    prm.perm = pl.steady_order ? (const int *)(ws + L.perm) : nullptr;
    prm.scratch = (double *)(ws + L.scratch);
    prm.scratch_stride = L.scratch_stride;
    int slot;
    HIPCHK(prof_begin(E.device, E.stream, &slot));
    char nm[160];
    em_plan_kernel_name(pl, nm, sizeof(nm));
    remember_kernel(E.device, nm);
    if (pl.cpw)
        HIPCHK(launch_em_pair(prm, PP, QQ, pl.lpc, n_blocks, pl.queue, E.stream));
    else if (pl.algo == LDSR_ALGO_SCAN)
        HIPCHK(launch_em_scan(prm, PP, QQ, n_blocks, pl.queue, false, E.stream));
    else
        HIPCHK(launch_em_serial(prm, PP, QQ, n_blocks, E.stream));
    HIPCHK(prof_end(E.stream, slot));
    return LDSR_OK;
}

extern "C" int ldsr_em_batch_device_lead(int device, void *stream_, int n_series, int T, int p, int q,
                                         const double *d_y, const double *d_u, const double *d_v,
                                         int shared_uv, const int *cell_offsets,
                                         const double *d_theta0, int niter, double tol, int algo,
                                         double *d_theta, double *d_lik, int *d_n_iter, int *d_status,
                                         double *d_liks, void *d_workspace, size_t workspace_bytes,
                                         int lead_steps) {
    EmLaunch E;
    E.device = device; E.stream = (hipStream_t)stream_;
    E.n_series = n_series; E.T = T; E.p = p; E.q = q; E.shared_uv = shared_uv;
    E.y = d_y; E.u = d_u; E.v = d_v; E.cell_offsets = cell_offsets; E.theta0 = d_theta0;
    E.niter = niter; E.tol = tol; E.algo = algo;
    E.theta = d_theta; E.lik = d_lik; E.n_iter = d_n_iter; E.status = d_status; E.liks = d_liks;
    E.workspace = d_workspace; E.workspace_bytes = workspace_bytes;
    E.lead_steps = lead_steps < 0 ? -1 : lead_steps;
    E.fit_follows = false;
    return em_batch_device_impl(E);
}

extern "C" int ldsr_em_batch_device(int device, void *stream_, int n_series, int T, int p, int q,
                                    const double *d_y, const double *d_u, const double *d_v,
                                    int shared_uv, const int *cell_offsets,
                                    const double *d_theta0, int niter, double tol, int algo,
                                    double *d_theta, double *d_lik, int *d_n_iter, int *d_status,
                                    double *d_liks, void *d_workspace, size_t workspace_bytes) {
    return ldsr_em_batch_device_lead(device, stream_, n_series, T, p, q, d_y, d_u, d_v, shared_uv,
                                     cell_offsets, d_theta0, niter, tol, algo, d_theta, d_lik, d_n_iter,
                                     d_status, d_liks, d_workspace, workspace_bytes, 0);
}

bool smoother_is_scan(int T, int PP, int QQ, const WsLayout &L, int mode) {
    return mode == 0 && L.img_stride && em_scan_supported(T, PP, QQ);
}

// The scan launch's block table (series, first cell, cells; blocks never straddle a series) into the
// workspace, or the serial kernel's cell -> series map into d_soc; both through the pinned staging ring.
int smoother_tables(const PreparedSeries &S, int n, const int *series_of_cell, int mode, int *d_soc,
                    SmootherTables *out, const std::vector<char> *skip_series) {
    out->scan = smoother_is_scan(S.T, S.PP, S.QQ, *S.L, mode);
    if (!out->scan) return stage_h2d_async(S.device, S.stream, d_soc, series_of_cell, sizeof(int) * (size_t)n);
    const int cpb = em_scan_cells_per_block(S.T, S.PP, S.QQ);
    std::vector<Block> blocks;
    for (int c = 0; c < n;) {
        if (skip_series && (*skip_series)[(size_t)series_of_cell[c]]) {      // (the caller runs these cells itself)
            c++;
            continue;
        }
        int e = c + 1;
        while (e < n && e - c < cpb && series_of_cell[e] == series_of_cell[c]) e++;
        blocks.push_back(Block{series_of_cell[c], c, e - c});
        c = e;
    }
    out->n_blocks = (int)blocks.size();
    if (out->n_blocks > S.L->max_blocks) return fail(LDSR_EINVAL, "internal: block table overflow (fit)");
    if (out->n_blocks == 0) return LDSR_OK;
    const std::vector<int> tab = block_table(blocks);
    int *d_ws_tab = (int *)(S.ws + S.L->blk);
    out->d_tab = d_ws_tab;
    return stage_h2d_async(S.device, S.stream, d_ws_tab, tab.data(), sizeof(int) * tab.size());
}

int smoother_enqueue(const PreparedSeries &S, int n, const SmootherTables &tb, const int *d_soc,
                     const double *d_theta, int stdlik, int mode, double lambda, const FitOut &out) {
    const bool scalar_only = out.pen != nullptr;
    if (tb.scan) {
        const int *d_tab = tb.d_tab;
        const int n_blocks = tb.n_blocks;
        if (n_blocks == 0) return LDSR_OK;
        EmParams prm;
        memset(&prm, 0, sizeof(prm));
        set_prepared_series(prm, S);
        prm.niter = 1; prm.n_cells = n; prm.tol = 0.0;
        prm.yz = (const double *)(S.ws + S.L->yz);
        prm.img = (const double *)(S.ws + S.L->img);
        prm.img_stride = S.L->img_stride;
        prm.blk_series = d_tab;
        prm.blk_cell0 = d_tab + n_blocks;
        prm.blk_ncell = d_tab + 2 * n_blocks;
        prm.queue = (int *)(S.ws + S.L->queue);
        prm.theta0 = d_theta;
        prm.lik = out.lik; prm.pen = out.pen; prm.status = out.status;
        prm.fitX = scalar_only ? nullptr : out.X; prm.fitY = scalar_only ? nullptr : out.Y;
        prm.fitV = scalar_only ? nullptr : out.V; prm.fitJ = scalar_only ? nullptr : out.J;
        prm.lambda = lambda;
        prm.stdlik = stdlik;
        HIPCHK(launch_em_scan(prm, S.PP, S.QQ, n_blocks, false, true, S.stream));
        return LDSR_OK;
    }
    SmoothParams sp;
    memset(&sp, 0, sizeof(sp));
    set_prepared_series(sp, S);
    sp.n_cells = n; sp.stdlik = stdlik; sp.mode = mode;
    sp.lambda = lambda;
    sp.series_of_cell = d_soc;
    sp.theta = d_theta;
    sp.X = out.X; sp.Y = out.Y; sp.V = out.V; sp.J = out.J;
    sp.lik = out.lik; sp.pen = out.pen; sp.status = out.status;
    sp.scalar_only = scalar_only;
    HIPCHK(launch_smooth(sp, S.PP, S.QQ, S.stream));
    return LDSR_OK;
}

// Both parts for a one-off pass.  d_tab_prebuilt: a block table [3][n], one block per cell, that the
// device filled itself (the restart grid's winners).
int launch_smoother(const PreparedSeries &S, int n, const int *series_of_cell, const double *d_theta,
                    int stdlik, int mode, double lambda, const FitOut &out, int *d_soc,
                    const int *d_tab_prebuilt) {
    SmootherTables tb;
    if (d_tab_prebuilt && smoother_is_scan(S.T, S.PP, S.QQ, *S.L, mode)) {
        tb.scan = true;         // (the caller's own table of n blocks, not the workspace's: no max_blocks to check)
        tb.d_tab = d_tab_prebuilt;
        tb.n_blocks = n;
    } else {
        const int rc = smoother_tables(S, n, series_of_cell, mode, d_soc, &tb);
        if (rc) return rc;
    }
    return smoother_enqueue(S, n, tb, d_soc, d_theta, stdlik, mode, lambda, out);
}

}  // namespace ldsr_host
