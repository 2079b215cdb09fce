// em_plan.hip -- which EM kernel a launch runs: AUTO's rules, the support checks of the explicit
// algorithms, the schedule and the kernel's name, in one place.  Host code only, no HIP calls: every
// EM launch (api_em.hip em_batch_device_impl) and the plan queries of the C ABI (ldsr_em_plan,
// ldsr_em_plan_lead, ldsr_em_workspace_bytes) ask em_plan(); the queries assume a launch that fills
// the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/ldsr_hip.h"
#include "ldsr_kernels.h"
#include "em_pair_impl.h"      // (layout constants only)

// ---- A/B switches (read once) -------------------------------------------------------------------
static bool env_is(const char *name, char c) { const char *e = getenv(name); return e && e[0] == c; }
// LDSR_PAIR=0 in the environment keeps AUTO off the two-cells-per-wave kernel (same-box A/B runs)
static bool pair_enabled() { static const bool on = !env_is("LDSR_PAIR", '0'); return on; }
// LDSR_LEAD=0 keeps AUTO off the closed-form lead of the pair family (same-box A/B runs)
static bool lead_enabled() { static const bool on = !env_is("LDSR_LEAD", '0'); return on; }
// LDSR_STEADY_ORDER=0: the steady form takes the cells in the caller's order (A/B runs)
static bool order_enabled() { static const bool on = !env_is("LDSR_STEADY_ORDER", '0'); return on; }
// LDSR_FORCE_FILL=1: AUTO treats every launch as large enough for the pair family (tests and the
// fuzzer exercise AUTO's choices with a handful of cells)
static bool force_fill() { static const bool on = env_is("LDSR_FORCE_FILL", '1'); return on; }

// ---- the rules ---------------------------------------------------------------------------------
// AUTO resolves to LDSR_ALGO_PAIR as the name of the several-cells-per-wave family (two or four
// cells per wave); which member -- or the scan kernel after all -- runs is decided per launch
// (em_plan: launch size, tol, fully observed or not).
static int resolve_algo(int algo, int T, int PP, int QQ) {
    if (algo != LDSR_ALGO_AUTO) return algo;
    if (pair_enabled() && (em_pair_supported(T, PP, QQ, 32) || em_pair_supported(T, PP, QQ, 16)))
        return LDSR_ALGO_PAIR;
    return em_scan_supported(T, PP, QQ) ? LDSR_ALGO_SCAN : LDSR_ALGO_SERIAL;
}

// cells per workgroup of the EM launch (the workspace's block table is sized for the scan
// kernel's value, the smallest of them, whenever its image is built)
static int cells_per_block(int algo, int T, int PP, int QQ, int lpc = 32, int lead = 0) {
    if (algo == LDSR_ALGO_PAIR || algo == LDSR_ALGO_QUAD) {
        const int c = em_pair_cells_per_block(T, PP, QQ, algo == LDSR_ALGO_QUAD ? 16 : lpc, lead);
        return c > 0 ? c : 16;
    }
    return algo == LDSR_ALGO_SCAN ? em_scan_cells_per_block(T, PP, QQ) : 64;
}

// scan kernel: cells converge at their own pace (tol > 0) -> per-series work queue
static bool scan_uses_queue(int T, int PP, int QQ, double tol) { return tol > 0.0 || em_scan_queue_only(T, PP, QQ); }

// AUTO with early stopping: the pair kernel couples two cells per wave and sixteen per workgroup
// (= per CU), so widely different iteration counts cost it more than they cost the scan kernel's
// four-cell workgroups.  Measured (converged runs, tol = 1e-5): fully observed series (cells stop
// after 28..63 iterations) pair +8..12 %; masked series (4..176, cfg5 up to 745 iterations) pair
// -2..-24 %.  So with tol > 0 AUTO takes the pair kernel only for series known to be fully observed
// (the host-pointer entries look; lead_steps = -1) -- short series are the exception: in the
// two-cells-per-wave kernel's four-wave workgroups (chunks of <= 13 steps) the coupling costs less
// than the shared per-wave work saves: T = 300 (2,2) +34 %, T = 400 (1,2) +11..33 %; from T = 500 on
// the scan kernel wins by 5..24 %.
static bool pair_pays_with_early_stopping(int T, int PP, int QQ) { return T <= 416 && em_pair_waves_per_block(T, PP, QQ, 32, 0) == 4; }

// Runs to convergence with wide-ish inputs (padded p + q >= 8), whatever the mask: since the scan kernel reads its
// image ahead (round 4) it beats the two-cells-per-wave kernel on long chunks (fully observed, T = 813 (3,3) 20 000
// cells 2.46 against 2.79 ms), and four cells per wave lose to two (fully observed, T = 260 (4,4) 20 000 cells 1.13
// against 0.97): tools/auto_regret.py, profiles/r04_auto_regret.txt.  No randomly masked (4,4) run to convergence
// has been measured.
static bool conv_wide(double tol, int PP, int QQ) { return tol > 0.0 && PP + QQ >= 8; }

// does the LEAD form at lp lanes per cell fit a CU's LDS: the tail's image, the strips and the lead's u_t
static bool lead_fits(int T, int tail, int PP, int QQ, int lp) {
    const bool wide = pair_wide(PP, QQ);
    int Lc = 0;
    long img = 0;
    em_pair_layout(tail, PP, QQ, lp, &Lc, &img, true);
    if (!img) return false;
    const size_t lds = ((size_t)img + (wide ? 4 : 8) * (size_t)pair_strip_doubles(Lc) +
                        (size_t)pair_lead_doubles(T - tail, lp, PP)) * sizeof(double);
    return lds <= 160 * 1024;
}

// four cells per wave for the tail of a lead: narrow inputs, tails of <= 256 steps (p = 3, 4 since the
// lead's second pass sums 5 + 2 p values instead of 7 + 4 p: they fit the 16-lane reduction now)
static bool lead_quad(int T, int tail, int PP, int QQ) {
    return PP <= 8 && QQ <= 8 && tail <= 256 && em_pair_supported(tail, PP, QQ, 16, true) && lead_fits(T, tail, PP, QQ, 16);
}

// p = 3, 4 have the two-cells-per-wave LEAD form only (7 + 4 p lead sums per step): on short series the
// four-cells-per-wave kernel over all T steps is quicker (tools/auto_regret.py, same box: T = 260 (4,4)
// 20 000 cells 1.86 ms against 1.29, to convergence 11.4 against 7.0; the Nakhon Phanom shape, T = 813
// with a lead of 733 steps, keeps it: 3.29 -> 2.50 ms)
static bool lead_short34(int T, int tail, int PP) { return PP > 2 && T - tail < 512; }

// A long all-missing lead common to every series (paleo-type data): the pair family's LEAD form handles
// it in closed form and sweeps only the tail -- [T - tail, T) with tail a multiple of 16 of at most 512
// steps (chunks of <= 16 steps: four cells per wave up to 256 steps, two beyond).  0: no closed-form lead.
static int lead_tail(int T, int PP, int QQ, int lead_steps) {
    if (!pair_enabled() || !lead_enabled() || lead_steps < 192 || PP > 8 || QQ > 8) return 0;
    const int tail = (std::max(T - lead_steps, 80) + 15) / 16 * 16;
    static const int max_tail = [] { const char *e = getenv("LDSR_LEAD_MAX_TAIL"); return e ? atoi(e) : 512; }();
    if (tail > max_tail || tail > 512 || T - tail < 128) return 0;
    // (with four cells per wave -- p = 3, 4 since round 3, launches of >= 3/4 of a round -- the lead pays on
    // short series too: em_plan checks lead_short34() before it falls back to two cells per wave)
    if (lead_short34(T, tail, PP) && !lead_quad(T, tail, PP, QQ)) return 0;
    if (lead_quad(T, tail, PP, QQ)) return tail;
    // (two cells per wave with padded p = 8 run ONE four-wave workgroup per CU and lose to the scan kernel:
    // T = 813 (7,7) 2048 cells 1.76 against 1.40 ms, 4096 cells 3.03 against 2.66, four per wave 1.89;
    // beyond T = 1024 the scan kernel's chunks are long and they win again)
    return ((PP < 8 || T > 1024) && lead_fits(T, tail, PP, QQ, 32)) ? tail : 0;
}

// ---- the plan ----------------------------------------------------------------------------------
EmPlan em_plan(const EmPlanIn &in) {
    EmPlan pl;
    auto fail = [&](const char *msg) { pl.err = LDSR_EINVAL; pl.msg = msg; return pl; };
    if (in.T < 2 || in.p < 1 || in.q < 1 || in.p > LDSR_MAXPQ || in.q > LDSR_MAXPQ || in.niter < 2 || !(in.tol >= 0.0))
        return fail("bad (T, p, q, niter, tol)");
    const int T = in.T, PP = ldsr_pad_dim(in.p), QQ = ldsr_pad_dim(in.q);
    const double tol = in.tol;
    pl.T = T; pl.PP = PP; pl.QQ = QQ;
    const bool was_auto = in.algo == LDSR_ALGO_AUTO;
    int &algo = pl.algo, &lpc = pl.lpc, &lead = pl.lead;     // (the plan's fields, worked on in place)
    algo = pl.algo_layout = resolve_algo(in.algo, T, PP, QQ);
    pl.layout_cpb = cells_per_block(algo, T, PP, QQ);

    // Is the launch large enough for the pair family to pay?  Counted in CUs' worth of cells (eight
    // waves) over the whole call (a slice of a multi-device call counts every slice's cells).
    auto fills = [&](int Te, int lp, bool lead_form = false) {
        if (!em_pair_supported(Te, PP, QQ, lp, lead_form)) return false;
        if (!in.off || force_fill()) return true;
        const int c = (64 / lp) * 8;          // a CU's eight waves
        long wgs = 0;
        for (int s = 0; s < in.n_series; s++) wgs += (in.off[s + 1] - in.off[s] + c - 1) / c;
        const long cus = in.cus;
        // Eight-wave workgroups (long chunks): >= 7/8 of the CUs.  Four-wave workgroups (short series,
        // two per CU): the shared per-wave work pays much earlier -- same box, T = 400 (1,2) / 200 (2,2) /
        // 300 (1,4), scan -> pair -> quad in ms: 1024 cells 0.47 -> 0.39 -> 0.54, 2048 0.50 -> 0.42 -> 0.57,
        // 3072 0.74 -> 0.62 -> 0.59, 4096 0.94 -> 0.68 -> 0.62 (tools/fill_ab.sh) -- two cells per wave from
        // 1/4 of the CUs (1024 cells), four from 3/8 (3072 cells).
        // (runs to convergence: only up to chunks of 13 steps -- beyond, the scan kernel with its read-ahead wins on
        // launches of this size: T = 600 (1,2) 2000 cells 0.284 against 0.313 ms, (2,4) 0.384 against 0.512)
        if (!lead_form && em_pair_waves_per_block(Te, PP, QQ, lp, 0) == 4 && (tol == 0.0 || Te <= 416))
            return wgs * 8 >= (lp == 16 ? 3 : 2) * cus;
        // the closed-form lead skips most of the work, so it pays from ~1536 cells (same box, scan ->
        // LEAD in ms, tools/lead_fill_ab.sh: T = 2000 (1,4) 1536 cells 1.94 -> 1.40, 3072 3.79 -> 1.47;
        // T = 4000 (2,2) 1536 cells 8.27 -> 2.47; T = 813 (3,3) 1536 0.92 -> 0.85, 3072 1.42 -> 1.27);
        // with early stopping only for long leads (2048 cells: T = 2000 2.81 -> 2.23, T = 813 2.85 -> 3.09)
        // from T = 1536 on the scan kernel's chunks are 28..32 steps long (and its image may live in global
        // memory): there the lead pays whatever the launch size -- 50 lone cells, niter = 200, scan -> LEAD in
        // ms: T = 2000 (1,4) 3.61 -> 2.44, (3,5) 17.1 -> 3.96, T = 4000 (2,2) 6.30 -> 4.95; at T = 1100..1300
        // it is a toss-up (1.40 -> 1.48, 1.81 -> 2.07, 2.17 -> 1.78)
        // (four cells per wave with p = 3, 4 or wide inputs -- possible since the lead's second pass sums
        // 5 + 2 p values -- pay from 3072 cells, with leads of 1024 steps and more from 6144: same box, two ->
        // four cells per wave in ms, T = 813 (3,3) 8192 cells 2.33 -> 1.55, 4096 1.24 -> 1.06, 3072 1.21 -> 1.03,
        // 2048 0.82 -> 0.98; (4,8) T = 1024 3072 cells 1.52 -> 1.26, 2048 1.06 -> 1.22; T = 2000 (3,4) 4096
        // cells 2.25 -> 2.64, 6144 4.33 -> 2.73)
        if (lead_form && lp == 16 && (PP > 2 || QQ > 4)) return wgs * (in.lead_steps >= 1024 ? 4 : 8) >= 3 * cus;
        if (lead_form && T >= 1536) return true;
        if (lead_form && (tol == 0.0 || in.lead_steps >= 1024))
            return wgs * (lp == 16 ? 16 : 8) >= 3 * cus;
        return wgs * 8 >= 7 * cus;
    };

    lpc = algo == LDSR_ALGO_QUAD ? 16 : 32;
    const int tail = was_auto && algo != LDSR_ALGO_SERIAL ? lead_tail(T, PP, QQ, in.lead_steps) : 0;
    if (tail && lead_quad(T, tail, PP, QQ) && fills(tail, 16, true)) { lead = T - tail; lpc = 16; algo = LDSR_ALGO_QUAD; }
    else if (tail && (PP < 8 || T > 1024) && !lead_short34(T, tail, PP) && fills(tail, 32, true)) { lead = T - tail; lpc = 32; algo = LDSR_ALGO_PAIR; }
    if (in.lead_force > 0 && (algo == LDSR_ALGO_PAIR || algo == LDSR_ALGO_QUAD)) lead = in.lead_force;
    const int Te = pl.Te = T - lead;    // steps the sweeps of the pair family work on
    if (!lead && was_auto && algo == LDSR_ALGO_PAIR) {
        const bool masked_conv = tol > 0.0 && in.lead_steps >= 0;
        if (masked_conv && !pair_pays_with_early_stopping(T, PP, QQ)) algo = LDSR_ALGO_SCAN;
        else if (conv_wide(tol, PP, QQ) && T > 512 && em_scan_supported(T, PP, QQ)) algo = LDSR_ALGO_SCAN;
        // ... and only when its workgroups (one per CU: 16 cells at two cells per wave, 32 at four) fill
        // the device: 512 cells are 32 pair workgroups on 32 of 256 CUs but 128 scan workgroups on 128
        // of them (a quarter of the time).  Four cells per wave where they fit and fill, else two.  (Masked
        // series with early stopping reach this point only as short series: there four cells per wave win
        // once the launch is large -- tools/auto_regret.py, 20 000 cells: T = 150 (1,2) 2.96 -> 2.74 ms; at
        // 2000 cells two per wave stay ahead.  conv_wide keeps padded p + q >= 8 at two whatever the mask.)
        else if (!conv_wide(tol, PP, QQ) && fills(T, 16)) { lpc = 16; algo = LDSR_ALGO_QUAD; }
        else if (!fills(T, 32)) algo = em_scan_supported(T, PP, QQ) ? LDSR_ALGO_SCAN : LDSR_ALGO_SERIAL;
    }
    if (algo != LDSR_ALGO_SERIAL && algo != LDSR_ALGO_SCAN && algo != LDSR_ALGO_PAIR && algo != LDSR_ALGO_QUAD)
        return fail("unknown algo");
    if (algo == LDSR_ALGO_SCAN && !em_scan_supported(T, PP, QQ))
        return fail("LDSR_ALGO_SCAN needs T <= 8192 and p, q <= 8 (and T >= L (L - 1) for its chunk length)");
    if (algo == LDSR_ALGO_PAIR && !em_pair_supported(Te, PP, QQ, 32, lead > 0))
        return fail("LDSR_ALGO_PAIR needs 65 <= T <= 1024, p, q <= 4 and a series image that leaves room for eight waves per CU (ldsr_em_plan tells)");
    if (algo == LDSR_ALGO_QUAD && !em_pair_supported(Te, PP, QQ, 16, lead > 0))
        return fail("LDSR_ALGO_QUAD needs 65 <= T <= 512, p, q <= 4 (ldsr_em_plan tells)");

    const bool cpw = pl.cpw = algo == LDSR_ALGO_PAIR || algo == LDSR_ALGO_QUAD;     // the pair family's body
    long img = 0;
    if (cpw) em_pair_layout(Te, PP, QQ, lpc, &pl.chunk, &img, lead > 0);
    // block table: static schedule (serial kernel; scan and pair kernels with tol == 0: every cell runs
    // exactly niter iterations) or per-series work queue (tol > 0: a wave whose cell converges early
    // takes the next one instead of idling; members without a static-schedule variant -- wide LEAD forms)
    pl.queue = (algo == LDSR_ALGO_SCAN && scan_uses_queue(T, PP, QQ, tol)) ||
               (cpw && (tol > 0.0 || !pair_variant(PP, QQ, pl.chunk, lpc, false, lead > 0)));
    pl.cpb = cells_per_block(algo, cpw ? Te : T, PP, QQ, lpc, cpw ? lead : 0);
    // steady form of the two-cells-per-wave kernel (fully observed series, chunks of >= 24 steps):
    // series_prep orders every series' cells by predicted slowness (em_pair_impl.h em_pair_body_steady)
    pl.steady_order = cpw && lpc == 32 && lead == 0 && pair_steady(pl.chunk, 32, PP, QQ) && order_enabled();
    pl.ok = true;
    return pl;
}

void em_plan_kernel_name(const EmPlan &pl, char *buf, size_t len) {
    if (pl.cpw) em_pair_kernel_name(pl.Te, pl.PP, pl.QQ, pl.lpc, pl.queue, buf, len, pl.lead > 0);
    else if (pl.algo == LDSR_ALGO_SCAN) em_scan_kernel_name(pl.T, pl.PP, pl.QQ, pl.queue, false, buf, len);
    else em_serial_kernel_name(pl.T, pl.PP, pl.QQ, buf, len);
}
