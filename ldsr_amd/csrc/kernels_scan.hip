// kernels_scan.hip -- launch plan of the parallel-in-time scan kernel (chunk length L, waves
// per cell W, LDS or global series image) and dispatch to the per-(L, W) translation units
// (em_members.h).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "em_members.h"
#include "em_scan_impl.h"
#include "em_pair_impl.h"
#include "ldsr_kernels.h"

static const size_t kLdsBytes = 160 * 1024;

// waves per block so that a CU holds ~8 waves given the LDS image of one series
static int scan_wpb(int L, int PP, int QQ) {
    const size_t lds = (size_t)scan_image_doubles(L, 1, PP, QQ) * sizeof(double);
    const int blocks_per_cu = (int)(kLdsBytes / lds);
    const int want = 8;
    int wpb = (want + blocks_per_cu - 1) / (blocks_per_cu > 0 ? blocks_per_cu : 1);
    if (wpb < 2) wpb = 2;
    if (L <= 16 && wpb < 4 && lds > 20 * 1024) wpb = 4;
    const int cap = 8;
    return wpb > cap ? cap : wpb;
}

// Smallest compiled chunk length (em_members.h) of the wave count W with T <= 64 W L.
// W = 1: every choice also has L (L-1) <= T.
// T > 2048: W = 2 (T <= 4096) or 4 (T <= 8192) waves per cell with half-stored chunks.
ScanPlan scan_plan(int T, int PP, int QQ) {
    ScanPlan p;
    if (PP > 8 || QQ > 8 || T < 2) return p;   // instantiated for padded widths up to 8
    if (T > 8192) return p;
    p.W = T <= 2048 ? 1 : T <= 4096 ? 2 : 4;
    for (const EmMember &m : kScanMembers)
        if (m.n == p.W && T <= 64 * p.W * m.L) { p.L = (p.W > 1 || T >= m.L * (m.L - 1)) ? m.L : 0; break; }
    if (!p.L) return p;
    // the image is read from global memory (raw buffer loads, L2 / L1 resident) when it does not
    // fit a CU's LDS (L >= 20 only: the short-chunk images always fit) and for every multi-wave
    // cell: one cell per workgroup would let an LDS image cap a CU at one or two cells, while the
    // global image leaves 4 (W = 2) or 2 (W = 4) cells per CU -- measured 1.5x faster at W = 2
    p.gimg = scan_uses_gimg(p.L, p.W, PP, QQ);
    if (!p.gimg && !scan_image_fits_lds(p.L, p.W, PP, QQ)) return p;
    p.cpb = p.W > 1 ? 1 : (p.gimg ? 4 : scan_wpb(p.L, PP, QQ));   // GIMG: two workgroups per CU by VGPRs
    p.ok = true;
    return p;
}

bool em_scan_supported(int T, int PP, int QQ) { return scan_plan(T, PP, QQ).ok; }
bool em_scan_global_image(int T, int PP, int QQ) { return scan_plan(T, PP, QQ).gimg; }
int em_scan_cells_per_block(int T, int PP, int QQ) { return scan_plan(T, PP, QQ).cpb; }
// shapes compiled with the work-queue schedule only: global-image and multi-wave kernels
bool em_scan_queue_only(int T, int PP, int QQ) {
    const ScanPlan p = scan_plan(T, PP, QQ);
    return p.gimg || p.W > 1;
}
void em_scan_layout(int T, int PP, int QQ, int *L, int *NL, long *img_doubles) {
    const ScanPlan p = scan_plan(T, PP, QQ);
    *L = p.L;
    *NL = 64 * p.W;
    *img_doubles = p.ok ? scan_image_doubles(p.L, p.W, PP, QQ) : 0;
}

void em_scan_kernel_name(int T, int PP, int QQ, bool queue, bool fit, char *buf, size_t len) {
    const ScanPlan p = scan_plan(T, PP, QQ);
    queue = !fit && (queue || p.gimg || p.W > 1);
    snprintf(buf, len, "em_scan_kernel<%d, %d, %d, %d, %s, %s, %s>", PP, QQ, p.L, p.W,
             queue ? "true" : "false", p.gimg ? "true" : "false", fit ? "true" : "false");
}

hipError_t launch_em_scan(const EmParams &prm, int PP, int QQ, int n_blocks, bool queue, bool fit,
                          hipStream_t stream) {
    const ScanPlan p = scan_plan(prm.T, PP, QQ);
    if (!p.ok) return hipErrorInvalidValue;
    queue = !fit && (queue || p.gimg || p.W > 1);
#define CASE_LW(Lv, Wv) \
    case Lv * 8 + Wv: return launch_em_scan_LW<Lv, Wv>(prm, PP, QQ, n_blocks, p.cpb, queue, p.gimg, fit, stream);
    switch (p.L * 8 + p.W) {
        LDSR_SCAN_MEMBERS(CASE_LW)
        default: return hipErrorInvalidValue;
    }
#undef CASE_LW
}

// ---- two / four cells per wave (em_pair_impl.h) --------------------------------------------------
// lpc = lanes per cell: 32 (two cells per wave, T <= 1024) or 16 (four, T <= 512).
// Smallest chunk length with L (L-1) <= T <= lpc L.  The kernel pays off only with two waves per
// SIMD: eight waves per workgroup (one workgroup fills a CU's LDS), i.e. the lpc-lane series image
// and eight strips must fit 160 KiB -- at lpc = 32: (1,2): every L; (1,4): L <= 29; (2,4), (4,2):
// L <= 27; (4,4): L <= 25.  Same-box A/B at 8192 cells: with 7 or 6 waves per CU (and the coarser
// workgroup count) it is 20-25 % SLOWER than the one-cell-per-wave kernel, with 8 it is 10-15 % faster.
PairPlan pair_plan(int T, int PP, int QQ, int lpc, bool lead_form) {
    PairPlan p;
    p.lpc = lpc;
    // Wide inputs (padded p or q = 8) exist as the two-cells-per-wave LEAD form only: the tail of a
    // closed-form lead in chunks of <= 16 steps (the generic sweeps of long chunks do not fit the
    // registers of two waves per SIMD at q = 8; the lead itself never touches v_t).
    const bool wide = pair_wide(PP, QQ);
    if ((lpc != 32 && lpc != 16) || PP > 8 || QQ > 8 || T <= 64) return p;
    if (wide && !(lead_form && ((lpc == 32 && T <= 512) || (lpc == 16 && T <= 256)))) return p;
    if (lead_form && T > lpc * kPairLeadMaxL) return p;
    // every compiled chunk length (em_members.h: 3 to 32, four cells per wave from 5): the shortest one wastes no lanes
    // (lanes 0 .. rp-1 own L steps, the others L-1: needs 1 <= rp <= nl)
    for (const EmMember &m : kPairMembers) {
        const int L = m.L;
        if (m.n != lpc || T > lpc * L) continue;
        const int nl = (T + L - 1) / L, rp = T - nl * (L - 1);
        if (rp >= 1 && rp <= nl) { p.L = L; break; }
    }
    if (!p.L) return p;
    if (!pair_member_fits(p.L, lpc, PP, QQ)) return p;     // (wide: four waves per workgroup may have to do)
    p.wpb = 8;
    p.ok = true;
    return p;
}

// Waves per workgroup of the launch: a CU holds eight waves of these kernels (256 VGPRs each), as
// one workgroup of eight or -- where the LDS has room for two images and two sets of strips (and
// two copies of a lead's u_t) -- as two workgroups of four.  The finer grain fills the last round
// of a launch better: config 4 (10 240 cells = 320 eight-wave workgroups on 256 CUs: two rounds,
// the second on a quarter of the device) 4.56 -> 3.45 ms, config 5 (768 = three full rounds)
// 3.42 -> 3.29 ms; config 2's image allows one workgroup per CU only.  LDSR_PAIR_WPB=8 keeps
// eight (A/B hook).
int em_pair_waves_per_block(int T, int PP, int QQ, int lpc, int lead) {
    const PairPlan p = pair_plan(T, PP, QQ, lpc, lead > 0);
    if (!p.ok) return 0;
    static const int wpb_env = [] { const char *e = getenv("LDSR_PAIR_WPB"); return e ? atoi(e) : 0; }();
    if (wpb_env == 8) return 8;
    const int w = wpb_env == 2 ? 2 : 4;
    const size_t lds = ((size_t)pair_image_doubles(p.L, PP, QQ, lpc) + (size_t)w * pair_strip_doubles(p.L) +
                        (lead > 0 ? (size_t)pair_lead_doubles(lead, lpc, PP) : 0) +
                        (lead == 0 && pair_steady(p.L, lpc, PP, QQ) ? (size_t)pair_tri_doubles(PP, QQ, lpc) : 0)) * sizeof(double);
    // (the runtime keeps some LDS per workgroup for itself: leave 1 KiB per workgroup free)
    if ((8 / w) * (lds + 1024) <= kLdsBytes) return w;
    // (wide LEAD forms whose image, strips and lead leave no room for eight waves: ONE workgroup of four)
    const size_t lds8 = lds + (size_t)(8 - w) * pair_strip_doubles(p.L) * sizeof(double);
    return lds8 <= kLdsBytes ? 8 : w;
}

bool em_pair_supported(int T, int PP, int QQ, int lpc, bool lead_form) { return pair_plan(T, PP, QQ, lpc, lead_form).ok; }
int em_pair_cells_per_block(int T, int PP, int QQ, int lpc, int lead) { return (64 / lpc) * em_pair_waves_per_block(T, PP, QQ, lpc, lead); }
void em_pair_layout(int T, int PP, int QQ, int lpc, int *L, long *img_doubles, bool lead_form) {
    const PairPlan p = pair_plan(T, PP, QQ, lpc, lead_form);
    *L = p.L;
    *img_doubles = p.ok ? pair_image_doubles(p.L, PP, QQ, lpc) : 0;
}
void em_pair_kernel_name(int T, int PP, int QQ, int lpc, bool queue, char *buf, size_t len, bool lead) {
    const PairPlan p = pair_plan(T, PP, QQ, lpc, lead);
    snprintf(buf, len, "em_pair_kernel<%d, %d, %d, %d, %s, %s>", PP, QQ, p.L, lpc, queue ? "true" : "false", lead ? "true" : "false");
}

hipError_t launch_em_pair(const EmParams &prm, int PP, int QQ, int lpc, int n_blocks, bool queue,
                          hipStream_t stream) {
    PairPlan p = pair_plan(prm.T - prm.lead, PP, QQ, lpc, prm.lead > 0);     // (LEAD form: the tail's plan)
    if (!p.ok || !prm.img2 || (prm.lead > 0 && !prm.img3)) return hipErrorInvalidValue;
    p.wpb = em_pair_waves_per_block(prm.T - prm.lead, PP, QQ, lpc, prm.lead);
#define CASE_L(Lv, LPCv) \
    case Lv * 64 + LPCv: return launch_em_pair_L<Lv, LPCv>(prm, PP, QQ, n_blocks, p.wpb, queue, stream);
    switch (p.L * 64 + lpc) {
        LDSR_PAIR_MEMBERS(CASE_L)
        default: return hipErrorInvalidValue;
    }
#undef CASE_L
}


// ---- what is compiled ------------------------------------------------------------------------------
// Every instantiation of the scan and pair families this library holds, by the names rocprofv3 prints:
// the members of em_members.h in the variants scan_variant() / pair_variant() name -- the list the build
// and the launchers are made of and the predicates the launchers instantiate with.  tests/test_abi_and_host.py
// checks that this set equals the kernels in the built library's code objects AND what the launch plans can
// return over the supported domain -- nothing unreachable is compiled, nothing reachable is missing.
void em_kernel_inventory(std::string &out) {
    static const int widths[] = {1, 2, 4, 8};
    static const char *const tf[] = {"false", "true"};
    char buf[160];
    for (const EmMember &m : kScanMembers)
        for (int PP : widths)
            for (int QQ : widths)
                for (int v = 0; v < 8; v++) {
                    const bool q = v & 1, g = v & 2, f = v & 4;
                    if (!scan_variant(PP, QQ, m.L, m.n, q, g, f)) continue;
                    snprintf(buf, sizeof(buf), "em_scan_kernel<%d, %d, %d, %d, %s, %s, %s>\n", PP, QQ, m.L, m.n, tf[q], tf[g], tf[f]);
                    out += buf;
                }
    for (const EmMember &m : kPairMembers)
        for (int PP : widths)
            for (int QQ : widths)
                for (int v = 0; v < 4; v++) {
                    const bool q = v & 1, lead = v & 2;
                    if (!pair_variant(PP, QQ, m.L, m.n, q, lead)) continue;
                    snprintf(buf, sizeof(buf), "em_pair_kernel<%d, %d, %d, %d, %s, %s>\n", PP, QQ, m.L, m.n, tf[q], tf[lead]);
                    out += buf;
                }
}
