// ldsr_api.hip -- the C ABI of include/ldsr_hip.h: argument checks, device arenas, workspace
// carving, block tables, launches, restart selection.  No numerics live here.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ldsr_hip.h"
#include "ldsr_kernels.h"
#include "em_pair_impl.h"      // (layout constants only)
#include "ga.h"
#include "bfgs.h"
#include "plgrad.h"
#include "source_hash.h"       // LDSR_SOURCE_HASH, written by the Makefile

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(LDSR_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

extern "C" const char *ldsr_last_error(void) { return g_err.c_str(); }
extern "C" const char *ldsr_version(void) { return "ldsr_hip 0.4.0 (gfx950) src " LDSR_SOURCE_HASH; }
extern "C" const char *ldsr_source_hash(void) { return LDSR_SOURCE_HASH; }

extern "C" int ldsr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- user interrupts ---------------------------------------------------------------------------
// One host-pinned flag for the whole library: kernels launched while a callback is registered
// poll it; only the thread that entered the library from outside (t_poll) runs the callback.
// The registration is ONE immutable record published through one atomic pointer (callback and
// argument as two atomics let a poller racing a re-registration call the old callback with the new
// argument); replaced records live until ldsr_shutdown.  An entering call announces itself (`active`)
// BEFORE it looks at the registration, and shutdown withdraws the registration BEFORE it looks at
// `active`: with sequentially consistent atomics either the call sees no registration and never
// touches the flag, or shutdown sees the call and leaves the flag alone.
struct IntrReg {
    int (*cb)(void *);
    void *arg;
};
static struct {
    std::mutex mu;                    // serialises registration and shutdown
    std::atomic<const IntrReg *> reg{nullptr};
    std::atomic<int *> flag{nullptr};  // pinned, portable
    std::atomic<int> active{0};       // external EM calls in flight
    std::vector<const IntrReg *> retired;
} g_intr;
static thread_local bool t_poll = false;     // this thread may run the callback
static thread_local bool t_worker = false;   // a library worker thread: never runs it

extern "C" int ldsr_set_interrupt_callback(int (*callback)(void *), void *arg) {
    std::lock_guard<std::mutex> lk(g_intr.mu);
    if (callback && !g_intr.flag.load()) {
        void *p = nullptr;
        HIPCHK(hipHostMalloc(&p, 64, hipHostMallocPortable | hipHostMallocMapped));
        *(int *)p = 0;
        g_intr.flag.store((int *)p);
    }
    const IntrReg *old = g_intr.reg.load();
    if (old && callback && old->cb == callback && old->arg == arg) return LDSR_OK;     // (the shim registers before every call)
    g_intr.reg.store(callback ? new IntrReg{callback, arg} : nullptr);
    if (old) g_intr.retired.push_back(old);
    return LDSR_OK;
}

static const int *intr_flag_for_kernels() { return g_intr.reg.load() ? g_intr.flag.load() : nullptr; }
static bool intr_raised() {
    int *f = g_intr.flag.load();
    return g_intr.reg.load() && f && *(volatile int *)f != 0;
}

// Run the callback (external caller thread only); raise the flag if it asks to stop.
static void intr_poll() {
    const IntrReg *r = g_intr.reg.load();
    int *f = g_intr.flag.load();
    if (!t_poll || !r || !f) return;
    if (*(volatile int *)f == 0 && r->cb(r->arg)) *(volatile int *)f = 1;
}

// RAII around an external EM entry: the outermost call on a non-worker thread becomes the poller
// and clears a stale flag when no other call is in flight.
struct IntrScope {
    bool owner = false;
    IntrScope() {
        if (t_worker || t_poll) return;
        const int before = g_intr.active.fetch_add(1);       // announce first ...
        if (!g_intr.reg.load()) {                             // ... then look (see above)
            g_intr.active.fetch_sub(1);
            return;
        }
        owner = true;
        t_poll = true;
        int *f = g_intr.flag.load();
        if (before == 0 && f) *(volatile int *)f = 0;
    }
    ~IntrScope() {
        if (!owner) return;
        // the last external call to leave clears the flag: a raised interrupt stops every call that
        // is in flight and is over once they have all returned
        int *f = g_intr.flag.load();
        if (g_intr.active.fetch_sub(1) == 1 && f) *(volatile int *)f = 0;
        t_poll = false;
    }
};

// Wait for a stream; the polling thread keeps the interrupt callback alive meanwhile.
static hipError_t wait_stream(hipStream_t stream) {
    if (!t_poll) return hipStreamSynchronize(stream);
    for (unsigned n = 0;; n++) {
        const hipError_t e = hipStreamQuery(stream);
        if (e != hipErrorNotReady) return e;
        if ((n & 15) == 15) intr_poll();
        usleep(50);
    }
}

// ---- optional kernel timer: HIP events around the EM kernel, on its launch stream ------------
// Slots are handed out under a mutex (ldsr_em_batch_multi / _groups call in from worker
// threads); an event pair belongs to the device it was created on.
struct ProfSlot {
    int device;
    hipEvent_t a, b;
};
static struct {
    std::mutex mu;
    bool on = false;
    std::vector<ProfSlot> ev;
    size_t used = 0;
} g_prof;

extern "C" void ldsr_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = on != 0;
    g_prof.used = 0;
}

extern "C" int ldsr_profile_collect(double *total_ms, int *n_launches) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    double tot = 0.0;
    for (size_t i = 0; i < g_prof.used; i++) {
        HIPCHK(hipEventSynchronize(g_prof.ev[i].b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, g_prof.ev[i].a, g_prof.ev[i].b));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (n_launches) *n_launches = (int)g_prof.used;
    g_prof.used = 0;
    return LDSR_OK;
}

// Records the start event and returns the slot (-1 when the timer is off).
static hipError_t prof_begin(int device, hipStream_t stream, int *slot) {
    *slot = -1;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (!g_prof.on) return hipSuccess;
    if (g_prof.used == g_prof.ev.size()) {
        ProfSlot s;
        s.device = device;
        hipError_t e = hipEventCreate(&s.a);
        if (e != hipSuccess) return e;
        e = hipEventCreate(&s.b);
        if (e != hipSuccess) return e;
        g_prof.ev.push_back(s);
    } else if (g_prof.ev[g_prof.used].device != device) {
        ProfSlot &s = g_prof.ev[g_prof.used];
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
        s.device = device;
        hipError_t e = hipEventCreate(&s.a);
        if (e != hipSuccess) return e;
        e = hipEventCreate(&s.b);
        if (e != hipSuccess) return e;
    }
    *slot = (int)g_prof.used++;
    return hipEventRecord(g_prof.ev[*slot].a, stream);
}

static hipError_t prof_end(hipStream_t stream, int slot) {
    if (slot < 0) return hipSuccess;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    return hipEventRecord(g_prof.ev[slot].b, stream);
}

// ---- pinned staging ring: small host tables that must reach the device asynchronously --------
// ldsr_em_batch_device promises to only enqueue work, so its block table cannot be copied from
// the caller's (or a function-local) pageable memory: it is written into a library-owned pinned
// slot, copied from there on the caller's stream, and the slot is recycled once its event has
// completed (normally long before the ring wraps around).
struct StageSlot {
    int device = -1;
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
};
static struct {
    std::mutex mu;
    StageSlot slot[16];
    unsigned next = 0;
} g_stage;

static int stage_h2d_async(int device, hipStream_t stream, void *dst, const void *src, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_stage.mu);
    StageSlot &s = g_stage.slot[g_stage.next++ % 16];
    if (s.pending) {
        HIPCHK(hipEventSynchronize(s.ev));
        s.pending = false;
    }
    if (s.device != device && s.ev) {       // events belong to a device
        (void)hipEventDestroy(s.ev);
        s.ev = nullptr;
    }
    if (!s.ev) HIPCHK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    s.device = device;
    if (s.cap < bytes) {
        if (s.host) (void)hipHostFree(s.host);
        s.host = nullptr;
        s.cap = 0;
        const size_t cap = std::max(align256(bytes) * 2, (size_t)16384);
        HIPCHK(hipHostMalloc(&s.host, cap, hipHostMallocDefault));
        s.cap = cap;
    }
    memcpy(s.host, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, s.host, bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(s.ev, stream));
    s.pending = true;
    return LDSR_OK;
}

// ---- device arenas of the host-pointer entry points -------------------------------------------
// One arena = one device block + one pinned host block (both grow-only) + one non-blocking
// stream.  A call leases a free arena of its device (or creates one), so concurrent callers never
// share buffers, and repeated calls of the same shape do no hipMalloc / hipFree at all.
struct Arena {
    int device = -1;
    hipStream_t stream = nullptr;
    char *dev = nullptr, *pin = nullptr;
    size_t dev_cap = 0, pin_cap = 0;
    bool busy = false;
};
static std::mutex g_arena_mu;
static std::vector<Arena *> g_arenas;

static int arena_acquire(int device, Arena **out) {
    HIPCHK(hipSetDevice(device));
    std::lock_guard<std::mutex> lk(g_arena_mu);
    for (Arena *a : g_arenas)
        if (a->device == device && !a->busy) {
            a->busy = true;
            *out = a;
            return LDSR_OK;
        }
    Arena *a = new Arena;
    a->device = device;
    hipError_t e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete a;
        return fail(LDSR_EHIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
    }
    a->busy = true;
    g_arenas.push_back(a);
    *out = a;
    return LDSR_OK;
}

static void arena_release(Arena *a) {
    if (!a) return;
    std::lock_guard<std::mutex> lk(g_arena_mu);
    a->busy = false;
}

struct ArenaLease {     // releases on scope exit
    Arena *a = nullptr;
    ~ArenaLease() { arena_release(a); }
};

static int arena_reserve(Arena *a, size_t dev_bytes, size_t pin_bytes) {
    if (dev_bytes > a->dev_cap) {
        HIPCHK(hipStreamSynchronize(a->stream));
        if (a->dev) (void)hipFree(a->dev);
        a->dev = nullptr;
        a->dev_cap = 0;
        const size_t cap = align256(dev_bytes + dev_bytes / 8);
        HIPCHK(hipMalloc((void **)&a->dev, cap));
        a->dev_cap = cap;
    }
    if (pin_bytes > a->pin_cap) {
        HIPCHK(hipStreamSynchronize(a->stream));
        if (a->pin) (void)hipHostFree(a->pin);
        a->pin = nullptr;
        a->pin_cap = 0;
        const size_t cap = align256(pin_bytes + pin_bytes / 8);
        HIPCHK(hipHostMalloc((void **)&a->pin, cap, hipHostMallocDefault));
        a->pin_cap = cap;
    }
    return LDSR_OK;
}

extern "C" void ldsr_shutdown(void) {
    {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        for (auto &p : g_prof.ev) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        g_prof.ev.clear();
        g_prof.used = 0;
    }
    {
        std::lock_guard<std::mutex> lk(g_stage.mu);
        for (StageSlot &s : g_stage.slot) {
            if (s.pending) (void)hipEventSynchronize(s.ev);
            if (s.ev) (void)hipEventDestroy(s.ev);
            if (s.host) (void)hipHostFree(s.host);
            s = StageSlot();
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_intr.mu);
        const IntrReg *cur = g_intr.reg.exchange(nullptr);     // withdraw first, then look at `active`
        if (g_intr.active.load() == 0) {
            if (g_intr.flag.load()) (void)hipHostFree(g_intr.flag.load());
            g_intr.flag.store(nullptr);
            for (const IntrReg *r : g_intr.retired) delete r;
            g_intr.retired.clear();
            delete cur;
        } else if (cur) {
            g_intr.retired.push_back(cur);      // calls in flight: the flag and the records stay
        }
    }
    std::lock_guard<std::mutex> lk(g_arena_mu);
    std::vector<Arena *> keep;
    for (Arena *a : g_arenas) {
        if (a->busy) {          // a call is still running on another thread: leave it alone
            keep.push_back(a);
            continue;
        }
        if (hipSetDevice(a->device) == hipSuccess) {
            (void)hipStreamSynchronize(a->stream);
            if (a->dev) (void)hipFree(a->dev);
            if (a->pin) (void)hipHostFree(a->pin);
            (void)hipStreamDestroy(a->stream);
        }
        delete a;
    }
    g_arenas.swap(keep);
}

// bump allocator over an arena block: first pass sizes, second pass hands out pointers
struct Carver {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t r = o;
        o = align256(o + (bytes ? bytes : 8));
        return r;
    }
};

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

struct WsLayout {
    size_t sc, yp, yz, up, vp, img, img2, img3, blk, soc, queue, perm, perm_key, scratch, total;
    long scratch_stride, img_stride;   // img_stride: doubles per series image (0 = no image)
    long img2_stride;                  // pair kernel's image (0 = none)
    long img3_stride;                  // ... and its lead image
    int max_blocks, img_L, img_NL;
};

static WsLayout ws_layout(int n_series, int T, int PP, int QQ, int shared_uv, int n_cells,
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

static int check_common(int n_series, int T, int p, int q, const double *y,
                        const int *cell_offsets) {
    if (n_series < 1) return fail(LDSR_EINVAL, "n_series must be >= 1");
    if (T < 2) return fail(LDSR_EINVAL, "T must be >= 2");
    if (p < 1 || q < 1) return fail(LDSR_EINVAL, "p and q must be >= 1 (use 1 with u/v = NULL for an absent input)");
    if (p > LDSR_MAXPQ || q > LDSR_MAXPQ)
        return fail(LDSR_EUNSUPPORTED, "p and q above 16 are not supported by this build");
    if (!y || !cell_offsets) return fail(LDSR_EINVAL, "y and cell_offsets must not be NULL");
    if (cell_offsets[0] != 0) return fail(LDSR_EINVAL, "cell_offsets[0] must be 0");
    for (int s = 0; s < n_series; s++)
        if (cell_offsets[s + 1] < cell_offsets[s])
            return fail(LDSR_EINVAL, "cell_offsets must be non-decreasing");
    return LDSR_OK;
}

static int check_em(int niter, double tol) {
    if (niter < 2) return fail(LDSR_EINVAL, "niter must be >= 2 (the reference reads lik[1], src/EM.cpp:256)");
    if (!(tol >= 0.0)) return fail(LDSR_EINVAL, "tol must be >= 0");
    return LDSR_OK;
}

static int check_box(const double *lb, const double *ub, int P, const char *noun) {
    if (!lb || !ub) return fail(LDSR_EINVAL, "lb and ub must not be NULL");
    for (int c = 0; c < P; c++) {
        if (!std::isfinite(lb[c]) || !std::isfinite(ub[c]) || !std::isfinite(ub[c] - lb[c]))
            return fail(LDSR_EINVAL, "lb and ub must be finite");
        if (lb[c] > ub[c]) return fail(LDSR_EINVAL, std::string("lb must be <= ub in every ") + noun);
    }
    return LDSR_OK;
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
static PrepParams prep_params(int n_series, int T, int p, int q, int PP, int QQ, const double *d_y,
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

// One EM launch on device data (cell_offsets: a host array).  em_batch_device_impl fills in the plan it
// chose and the workspace layout it carved.
struct EmLaunch {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_series = 0, T = 0, p = 0, q = 0, shared_uv = 0, niter = 0, algo = LDSR_ALGO_AUTO;
    double tol = 0.0;
    const double *y = nullptr, *u = nullptr, *v = nullptr, *theta0 = nullptr;
    const int *cell_offsets = nullptr;
    double *theta = nullptr, *lik = nullptr, *liks = nullptr;
    int *n_iter = nullptr, *status = nullptr;
    int liks_nanfill = 1;           // liks beyond a cell's n_iter set to NaN (the batch ABI; the restart grid reads n_iter)
    void *workspace = nullptr;
    size_t workspace_bytes = 0;
    const int *abort_flag = nullptr;
    int lead_steps = 0, lead_force = 0;     // EmPlanIn's data facts and forced lead
    const int *plan_off = nullptr;  // the whole call's offsets (plan_ns series; null: cell_offsets): AUTO's kernel,
    int plan_ns = 0;                // hence the rounding of the results, must not depend on how many devices share it
    bool fit_follows = true;        // the winners' FIT pass follows: series_prep builds the scan kernel's image even
                                    // behind a pair-family launch (the bare device entries skip it: 4096 values at config 2)
    EmPlan plan;                    // out
    WsLayout layout;                // out
};

static int em_batch_device_impl(EmLaunch &E) {
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

    // block table: blocks never straddle a series.  Static schedule: (series, first cell, n cells of
    // the block).  Work queue: (series, first cell of the SERIES, n cells of the series) -- waves pull
    // cells from the per-series queue.
    std::vector<int> tab, bc, bn;     // (tab: the series column, then the other two)
    for (int s = 0; s < n_series; s++)
        for (int c = cell_offsets[s]; c < cell_offsets[s + 1]; c += cpb) {
            tab.push_back(s);
            bc.push_back(pl.queue ? cell_offsets[s] : c);
            bn.push_back(pl.queue ? cell_offsets[s + 1] - cell_offsets[s] : std::min(cpb, cell_offsets[s + 1] - c));
        }
    const int n_blocks = (int)tab.size();
    if (n_blocks > L.max_blocks) return fail(LDSR_EINVAL, "internal: block table overflow");
    tab.insert(tab.end(), bc.begin(), bc.end());
    tab.insert(tab.end(), bn.begin(), bn.end());
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

// Series that series_prep has prepared in the workspace ws (layout *L); what reads them goes on `stream`
struct PreparedSeries {
    int device;
    hipStream_t stream;
    int T, p, q, PP, QQ, shared_uv;
    bool has_u, has_v;
    char *ws;
    const WsLayout *L;
};

// Where a smoother pass writes, on the device: rows [n][T] of X, Y, V, J and [n] of lik, pen, status.  pen set:
// only the scalars leave the kernel, and X and V are the serial smoother's filtered-state strip.
struct FitOut {
    double *X = nullptr, *Y = nullptr, *V = nullptr, *J = nullptr, *lik = nullptr, *pen = nullptr;
    int *status = nullptr;
};

// the prepared-series fields of a kernel's parameters (EmParams, SmoothParams)
template <class Params>
static void set_prepared_series(Params &prm, const PreparedSeries &S) {
    prm.T = S.T; prm.p = S.p; prm.q = S.q; prm.has_u = S.has_u; prm.has_v = S.has_v;
    prm.yp = (const double *)(S.ws + S.L->yp);
    prm.up = (const double *)(S.ws + S.L->up);
    prm.vp = (const double *)(S.ws + S.L->vp);
    prm.u_stride = S.shared_uv ? 0 : (long)S.T * S.PP; prm.v_stride = S.shared_uv ? 0 : (long)S.T * S.QQ;
    prm.sc = (const SeriesConst *)(S.ws + S.L->sc);
}

// One Kalman_smoother pass (src/EM.cpp:22-131) for n cells on prepared series: the FIT form of
// the scan kernel (one wave group per cell) whenever the shape is supported, else the serial
// one-thread-per-cell kernel.  mode: 0 smoother, 1 propagate (serial kernel only).
// It comes in two parts, so that a caller that runs the same cells again and again (the GA's fitness
// pass) pays the host work once: smoother_tables uploads what depends on the cell -> series map alone,
// smoother_enqueue launches and touches no host memory.
struct SmootherTables {
    bool scan = false;              // the scan kernel's FIT form runs
    const int *d_tab = nullptr;     // its block table [3][n_blocks] on the device
    int n_blocks = 0;
};

static bool smoother_is_scan(int T, int PP, int QQ, const WsLayout &L, int mode) {
    return mode == 0 && L.img_stride && em_scan_supported(T, PP, QQ);
}

// The scan launch's block table (series, first cell, cells; blocks never straddle a series) into the
// workspace, or the serial kernel's cell -> series map into d_soc; both through the pinned staging ring.
static int smoother_tables(const PreparedSeries &S, int n, const int *series_of_cell, int mode, int *d_soc,
                           SmootherTables *out, const std::vector<char> *skip_series = nullptr) {
    out->scan = smoother_is_scan(S.T, S.PP, S.QQ, *S.L, mode);
    if (!out->scan) return stage_h2d_async(S.device, S.stream, d_soc, series_of_cell, sizeof(int) * (size_t)n);
    const int cpb = em_scan_cells_per_block(S.T, S.PP, S.QQ);
    std::vector<int> tab, bc, bn;           // (tab: the series column, then the other two)
    for (int c = 0; c < n;) {
        if (skip_series && (*skip_series)[(size_t)series_of_cell[c]]) {      // (the caller runs these cells itself)
            c++;
            continue;
        }
        int e = c + 1;
        while (e < n && e - c < cpb && series_of_cell[e] == series_of_cell[c]) e++;
        tab.push_back(series_of_cell[c]);
        bc.push_back(c);
        bn.push_back(e - c);
        c = e;
    }
    out->n_blocks = (int)tab.size();
    if (out->n_blocks > S.L->max_blocks) return fail(LDSR_EINVAL, "internal: block table overflow (fit)");
    if (out->n_blocks == 0) return LDSR_OK;
    tab.insert(tab.end(), bc.begin(), bc.end());
    tab.insert(tab.end(), bn.begin(), bn.end());
    int *d_ws_tab = (int *)(S.ws + S.L->blk);
    out->d_tab = d_ws_tab;
    return stage_h2d_async(S.device, S.stream, d_ws_tab, tab.data(), sizeof(int) * tab.size());
}

static int smoother_enqueue(const PreparedSeries &S, int n, const SmootherTables &tb, const int *d_soc,
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
static int launch_smoother(const PreparedSeries &S, int n, const int *series_of_cell, const double *d_theta,
                           int stdlik, int mode, double lambda, const FitOut &out, int *d_soc,
                           const int *d_tab_prebuilt = nullptr) {
    SmootherTables tb;
    if (d_tab_prebuilt && smoother_is_scan(S.T, S.PP, S.QQ, *S.L, mode)) {
        tb.scan = true;
        tb.d_tab = d_tab_prebuilt;
        tb.n_blocks = n;
    } else {
        const int rc = smoother_tables(S, n, series_of_cell, mode, d_soc, &tb);
        if (rc) return rc;
    }
    return smoother_enqueue(S, n, tb, d_soc, d_theta, stdlik, mode, lambda, out);
}

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
    Carver c;
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
    const size_t dev_total = c.o;
    // pinned: inputs, outputs, phase-2 block (same relative layouts as on the device)
    S.p_in = 0;
    S.p_out = align256(S.in_bytes);
    S.p_w = S.p_out + align256(S.out_bytes);
    const size_t pin_total = S.p_w + S.w_bytes;
    rc = arena_reserve(A, dev_total, pin_total);
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
        if (worker) t_worker = true;
        rcs[d] = slice_run(sl[d]);
        if (rcs[d]) msgs[d] = g_err;      // thread-local message of this worker
        if (worker) running.fetch_sub(1);
    };
    std::vector<std::thread> pool;
    for (size_t d = 1; d < n; d++)
        if (sl[d].n_series > 0) {
            running.fetch_add(1);
            pool.emplace_back(work, d, true);
        }
    if (n > 0 && sl[0].n_series > 0) work(0, false);
    while (t_poll && running.load() > 0) {     // keep the interrupt callback alive while joining
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
        if (G.rc) msgs[(size_t)g] = g_err;
    };
    // a bounded pool: at most 8 groups in flight (each holds one arena per device)
    const int n_workers = std::min(n_groups, 8);
    std::vector<std::thread> pool;
    for (int w = 0; w < n_workers; w++) {
        running.fetch_add(1);
        pool.emplace_back([&, w]() {
            t_worker = true;
            for (int g = w; g < n_groups; g += n_workers) work(g);
            running.fetch_sub(1);
        });
    }
    while (t_poll && running.load() > 0) {     // the caller's thread keeps the interrupt callback alive
        intr_poll();
        usleep(200);
    }
    for (auto &t : pool) t.join();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    for (int g = 0; g < n_groups; g++)
        if (groups[g].rc) return fail(groups[g].rc, "group " + std::to_string(g) + ": " + msgs[(size_t)g]);
    return LDSR_OK;
}

// ---- what the host-pointer entries of the smoother, GA and BFGS families share ----------------
// The series of a call as they cross the ABI (u, v null: absent) and their part of its input block: carve() takes
// y | u | v and, given cell_offsets, the cell -> series map and the theta rows; stage() fills them in the pinned
// block and says where the caller's ONE copy of its whole input block puts them on the device.
struct SeriesUpload {
    int n_series, T, p, q;
    const double *y, *u, *v;
    int shared_uv;
    const int *cell_offsets = nullptr;
    const double *theta = nullptr;      // (null with cell_offsets: the rows are reserved and go up as they are)
    size_t o_y = 0, o_u = 0, o_v = 0, o_soc = 0, o_th = 0;
    const double *d_y = nullptr, *d_u = nullptr, *d_v = nullptr, *d_theta = nullptr;
    int *d_soc = nullptr, *h_soc = nullptr;     // (h_soc: the staged map, for the block tables)
    PreparedSeries ps;                          // prep(): the series as series_prep leaves them
    size_t uv_bytes(const double *a, int k) const { return a ? sizeof(double) * (shared_uv ? 1 : (size_t)n_series) * T * k : 0; }
    void carve(Carver &c, const int *offsets = nullptr, const double *theta_rows = nullptr) {
        cell_offsets = offsets; theta = theta_rows;
        o_y = c.take(sizeof(double) * (size_t)n_series * T);
        o_u = c.take(uv_bytes(u, p));
        o_v = c.take(uv_bytes(v, q));
        if (!offsets) return;
        o_soc = c.take(sizeof(int) * (size_t)offsets[n_series]);
        o_th = c.take(sizeof(double) * (size_t)offsets[n_series] * (6 + p + q));
    }
    void stage(const Arena *A) {
        memcpy(A->pin + o_y, y, sizeof(double) * (size_t)n_series * T);
        if (u) memcpy(A->pin + o_u, u, uv_bytes(u, p));
        if (v) memcpy(A->pin + o_v, v, uv_bytes(v, q));
        d_y = (const double *)(A->dev + o_y);
        d_u = u ? (const double *)(A->dev + o_u) : nullptr;
        d_v = v ? (const double *)(A->dev + o_v) : nullptr;
        if (!cell_offsets) return;
        h_soc = (int *)(A->pin + o_soc); d_soc = (int *)(A->dev + o_soc); d_theta = (const double *)(A->dev + o_th);
        for (int s = 0; s < n_series; s++)
            for (int cc = cell_offsets[s]; cc < cell_offsets[s + 1]; cc++) h_soc[cc] = s;
        if (theta) memcpy(A->pin + o_th, theta, sizeof(double) * (size_t)cell_offsets[n_series] * (6 + p + q));
    }
    // series_prep of the uploaded series into the workspace ws (layout *L)
    hipError_t prep(int device, hipStream_t stream, char *ws, const WsLayout *L) {
        ps = PreparedSeries{device, stream, T, p, q, ldsr_pad_dim(p), ldsr_pad_dim(q), shared_uv, u != nullptr, v != nullptr,
                            ws, L};
        return launch_series_prep(prep_params(n_series, T, p, q, ps.PP, ps.QQ, d_y, d_u, d_v, shared_uv, ws, *L, true),
                                  n_series, stream);
    }
};

// ---- smoother / propagate / mstep / penalized likelihood host entry points ---------------------
enum FitKind { FIT_SMOOTH, FIT_PROPAGATE, FIT_MSTEP, FIT_PENLIK };     // (PENLIK: only lik - lambda * ssq leaves the device)

// The arena block of one such call, uploaded and prepared (begin): [series | map | theta] go up in one copy;
// d.lik, d.pen, d.status and d_theta_out come back in one (small_out bytes, host() says where); the rows stay.
struct FitCall {
    ArenaLease lease;
    WsLayout L;
    SeriesUpload U;
    size_t n_cells, row_bytes, small_out;
    FitOut d;       // (d.pen: FIT_PENLIK only)
    double *d_theta_out;
    char *pout;     // (pinned: the small outputs)

    const char *host(const void *small) const { return pout + ((const char *)small - (const char *)d.lik); }
    // (the serial kernels use X / V as their filtered-state strip; only FIT_PENLIK writes no rows)
    int begin(FitKind kind, int device, const SeriesUpload &series, const int *cell_offsets, const double *theta,
              bool serial = false) {
        U = series;
        int rc = arena_acquire(device, &lease.a);
        if (rc) return rc;
        Arena *A = lease.a;
        const int PP = ldsr_pad_dim(U.p), QQ = ldsr_pad_dim(U.q);
        n_cells = (size_t)cell_offsets[U.n_series]; row_bytes = sizeof(double) * n_cells * U.T;
        L = ws_layout(U.n_series, U.T, PP, QQ, U.shared_uv, (int)n_cells, LDSR_ALGO_SCAN, 1);
        const bool need_strip = kind == FIT_PROPAGATE || kind == FIT_MSTEP || serial || !em_scan_supported(U.T, PP, QQ);
        const size_t yj_bytes = kind == FIT_PENLIK ? 0 : row_bytes, xv_bytes = need_strip ? row_bytes : yj_bytes;
        Carver c;
        U.carve(c, cell_offsets, theta);
        const size_t in_bytes = c.o;
        const size_t o_lik = c.take(sizeof(double) * n_cells), o_pen = c.take(sizeof(double) * n_cells);
        const size_t o_st = c.take(sizeof(int) * n_cells), o_tho = c.take(sizeof(double) * n_cells * (6 + U.p + U.q));
        small_out = c.o - o_lik;
        const size_t o_X = c.take(xv_bytes), o_V = c.take(xv_bytes), o_Y = c.take(yj_bytes), o_J = c.take(yj_bytes);
        const size_t o_ws = c.take(L.total);
        rc = arena_reserve(A, c.o, in_bytes + align256(small_out));
        if (rc) return rc;
        char *dev = A->dev;
        pout = A->pin + in_bytes;
        d.X = (double *)(dev + o_X); d.Y = (double *)(dev + o_Y); d.V = (double *)(dev + o_V); d.J = (double *)(dev + o_J);
        d.lik = (double *)(dev + o_lik); d.status = (int *)(dev + o_st); d_theta_out = (double *)(dev + o_tho);
        d.pen = kind == FIT_PENLIK ? (double *)(dev + o_pen) : nullptr;
        U.stage(A);
        HIPCHK(hipMemcpyAsync(dev, A->pin, in_bytes, hipMemcpyHostToDevice, A->stream));
        HIPCHK(U.prep(device, A->stream, dev + o_ws, &L));
        return LDSR_OK;
    }
};

// Mstep (src/EM.cpp:139-229): the fit arrives from the caller, its X, V, J rows go straight into the device arrays
static int run_mstep(int device, const SeriesUpload &U, const int *cell_offsets, const double *X, const double *V,
                     const double *J, double *theta_out, int *status) {
    int rc = check_common(U.n_series, U.T, U.p, U.q, U.y, cell_offsets);
    if (rc || cell_offsets[U.n_series] == 0) return rc;
    if (!X || !V || !J || !theta_out) return fail(LDSR_EINVAL, "mstep needs X, V, J and theta");
    FitCall F;
    rc = F.begin(FIT_MSTEP, device, U, cell_offsets, nullptr);
    if (rc) return rc;
    SmoothParams sp;
    memset(&sp, 0, sizeof(sp));
    set_prepared_series(sp, F.U.ps);
    sp.n_cells = (int)F.n_cells; sp.series_of_cell = F.U.d_soc;
    sp.X = F.d.X; sp.V = F.d.V; sp.J = F.d.J; sp.status = F.d.status; sp.theta_out = F.d_theta_out;
    HIPCHK(hipMemcpyAsync(sp.X, X, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(sp.V, V, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(sp.J, J, F.row_bytes, hipMemcpyHostToDevice, F.U.ps.stream));
    HIPCHK(launch_mstep(sp, F.U.ps.PP, F.U.ps.QQ, F.U.ps.stream));
    HIPCHK(hipMemcpyAsync(F.pout, F.d.lik, F.small_out, hipMemcpyDeviceToHost, F.U.ps.stream));
    HIPCHK(hipStreamSynchronize(F.U.ps.stream));
    memcpy(theta_out, F.host(F.d_theta_out), sizeof(double) * F.n_cells * (6 + U.p + U.q));
    if (status) memcpy(status, F.host(F.d.status), sizeof(int) * F.n_cells);
    return LDSR_OK;
}

// host: the caller's arrays, null where a row is not wanted (lik: for FIT_PENLIK the penalised likelihood).
// The scan kernel whitens the inputs by Svv / Tuu and flags a series where one of them is singular (fewer
// observations than columns of v, say) instead of answering, but Kalman_smoother needs neither: the cells of
// such a series then go through the serial smoother (serial: this call is that second pass), in a call of
// their own, so that a cell's result does not depend on what shares the call (LDS_GA does the same).
static int run_fit_kernel(FitKind kind, int device, const SeriesUpload &U, const int *cell_offsets,
                          const double *theta, int stdlik, double lambda, const FitOut &host, bool serial = false) {
    int rc = check_common(U.n_series, U.T, U.p, U.q, U.y, cell_offsets);
    if (rc || cell_offsets[U.n_series] == 0) return rc;
    if (!theta || !host.lik) return fail(LDSR_EINVAL, "theta and lik must not be NULL");
    const int mode = kind == FIT_PROPAGATE ? 1 : 0;
    std::vector<int> redo;      // the series the scan kernel flagged
    {
        FitCall F;
        rc = F.begin(kind, device, U, cell_offsets, theta, serial);
        if (rc) return rc;
        const FitOut &d = F.d;
        const bool scan = !serial && smoother_is_scan(U.T, F.U.ps.PP, F.U.ps.QQ, F.L, mode);
        rc = serial ? smoother_enqueue(F.U.ps, (int)F.n_cells, SmootherTables(), F.U.d_soc, F.U.d_theta, stdlik, mode,
                                       lambda, d)
                    : launch_smoother(F.U.ps, (int)F.n_cells, F.U.h_soc, F.U.d_theta, stdlik, mode, lambda, d, F.U.d_soc);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(F.pout, d.lik, F.small_out, hipMemcpyDeviceToHost, F.U.ps.stream));
        HIPCHK(hipStreamSynchronize(F.U.ps.stream));
        memcpy(host.lik, F.host(d.pen ? d.pen : d.lik), sizeof(double) * F.n_cells);
        const int *st = (const int *)F.host(d.status);
        for (int s = 0; s < U.n_series && scan; s++)        // (singular is a fact of the series: its first cell tells)
            if (cell_offsets[s + 1] > cell_offsets[s] && st[cell_offsets[s]] == LDSR_CELL_SINGULAR) redo.push_back(s);
        if (!d.pen) {
            if (host.X) HIPCHK(hipMemcpy(host.X, d.X, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.Y) HIPCHK(hipMemcpy(host.Y, d.Y, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.V) HIPCHK(hipMemcpy(host.V, d.V, F.row_bytes, hipMemcpyDeviceToHost));
            if (host.J) HIPCHK(hipMemcpy(host.J, d.J, F.row_bytes, hipMemcpyDeviceToHost));
        }
    }
    for (int s : redo) {
        const size_t c0 = (size_t)cell_offsets[s], uv = U.shared_uv ? 0 : (size_t)s * U.T;
        const int off1[2] = {0, cell_offsets[s + 1] - cell_offsets[s]};
        auto rows = [&](double *a) { return a ? a + c0 * U.T : nullptr; };
        rc = run_fit_kernel(kind, device,
                            SeriesUpload{1, U.T, U.p, U.q, U.y + (size_t)s * U.T, U.u ? U.u + uv * U.p : nullptr,
                                         U.v ? U.v + uv * U.q : nullptr, U.shared_uv},
                            off1, theta + c0 * (6 + U.p + U.q), stdlik, lambda,
                            FitOut{rows(host.X), rows(host.Y), rows(host.V), rows(host.J), host.lik + c0}, true);
        if (rc) return rc;
    }
    return LDSR_OK;
}

extern "C" int ldsr_smooth_batch(int device, int n_series, int T, int p, int q, const double *y,
                                 const double *u, const double *v, int shared_uv,
                                 const int *cell_offsets, const double *theta, int stdlik,
                                 double *X, double *Y, double *V, double *J, double *lik) {
    return run_fit_kernel(FIT_SMOOTH, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, stdlik, 0.0, FitOut{X, Y, V, J, lik});
}

extern "C" int ldsr_propagate_batch(int device, int n_series, int T, int p, int q, const double *y,
                                    const double *u, const double *v, int shared_uv,
                                    const int *cell_offsets, const double *theta, int stdlik,
                                    double *X, double *Y, double *V, double *lik) {
    return run_fit_kernel(FIT_PROPAGATE, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, stdlik, 0.0, FitOut{X, Y, V, nullptr, lik});
}

extern "C" int ldsr_penalized_lik_batch(int device, int n_series, int T, int p, int q,
                                        const double *y, const double *u, const double *v,
                                        int shared_uv, const int *cell_offsets, const double *theta,
                                        double lambda, double *pl) {
    return run_fit_kernel(FIT_PENLIK, device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets,
                          theta, 0, lambda, FitOut{nullptr, nullptr, nullptr, nullptr, pl});
}

extern "C" int ldsr_mstep_batch(int device, int n_series, int T, int p, int q, const double *y,
                                const double *u, const double *v, int shared_uv,
                                const int *cell_offsets, const double *X, const double *V,
                                const double *J, double *theta, int *status) {
    return run_mstep(device, SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, X, V, J, theta,
                     status);
}

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
        rc = arena_reserve(A, c.o, in_bytes + align256(out_bytes) + sc_bytes);
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

// ---- LDS_BFGS: ssqTrain, its gradient and the L-BFGS learner (bfgs.hip) ----------------------------
// Both entries upload the raw series (the kernels read the ABI's time-major u, v as they are and find the
// missing y_t themselves), the cell -> series map and the cells' thetas: a SeriesUpload with its cells.
static SsqSeries ssq_series(const SeriesUpload &U, double *d_strip) {
    SsqSeries S;
    S.n_cells = U.cell_offsets[U.n_series]; S.T = U.T; S.p = U.p; S.q = U.q;
    S.y = U.d_y; S.u = U.d_u; S.v = U.d_v;
    S.u_stride = U.shared_uv ? 0 : (long)U.T * U.p; S.v_stride = U.shared_uv ? 0 : (long)U.T * U.q;
    S.series_of_cell = U.d_soc; S.strip = d_strip;
    return S;
}
static size_t ssq_strip_bytes(int n_cells, int T) {
    return T <= BFGS_LDS_MAX_T ? 0 : sizeof(double) * 2 * (size_t)T * (size_t)bfgs_waves(n_cells, T);
}

// ---- LDS_BFGS_with_update: the penalised likelihood and its gradient (plgrad.hip) -----------------------
static size_t plg_strip_bytes(int n_cells, int T) {
    return n_cells > 0 ? sizeof(double) * plg_launch_strip_doubles(n_cells, T) : 0;
}
// the series side of a launch from the block's offsets (what U.stage() hands out as d_y, d_u, d_v, d_soc)
static PlgSeries plg_series(const SeriesUpload &U, char *dev, size_t o_strip) {
    PlgSeries S;
    S.n_cells = U.cell_offsets[U.n_series]; S.T = U.T; S.p = U.p; S.q = U.q;
    S.y = (const double *)(dev + U.o_y);
    S.u = U.u ? (const double *)(dev + U.o_u) : nullptr;
    S.v = U.v ? (const double *)(dev + U.o_v) : nullptr;
    S.u_stride = U.shared_uv ? 0 : (long)U.T * U.p; S.v_stride = U.shared_uv ? 0 : (long)U.T * U.q;
    S.series_of_cell = (const int *)(dev + U.o_soc);
    S.strip = (double *)(dev + o_strip);
    return S;
}
// bytes the block reserves for y, u, v, series_of_cell and the strip (SeriesUpload::carve)
struct PlgSeriesHave { size_t b[5]; };
static PlgSeriesHave plg_series_have(const SeriesUpload &U, size_t strip_bytes) {
    return PlgSeriesHave{{sizeof(double) * (size_t)U.n_series * U.T, U.uv_bytes(U.u, U.p), U.uv_bytes(U.v, U.q),
                          sizeof(int) * (size_t)U.cell_offsets[U.n_series], strip_bytes}};
}
// The pre-launch check: every extent inside what was reserved for it and inside the call's block, no required
// pointer null -- else LDSR_EINTERNAL with the field's name, and the caller does not launch.
static int refuse_bad_extent(const char *kernel, const PlgExtent *e, int n, const char *dev, size_t block_bytes) {
    const int bad = plg_first_bad_extent(e, n, dev, block_bytes);
    if (bad < 0) return LDSR_OK;
    const PlgExtent &x = e[bad];
    if (!x.ptr) return fail(LDSR_EINTERNAL, std::string("internal: ") + kernel + " not launched: " + x.name + " is NULL");
    return fail(LDSR_EINTERNAL, std::string("internal: ") + kernel + " not launched: the kernel touches " +
                std::to_string(x.need) + " bytes of " + x.name + ", " + std::to_string(x.have) + " are reserved at offset " +
                std::to_string((long long)((const char *)x.ptr - dev)) + " of a block of " + std::to_string(block_bytes));
}
static BfgsUpdateParams bfgs_update_params(const BfgsParams &bp, const PlgSeries &S, double lambda) {
    BfgsUpdateParams up;
    up.S = S;
    up.par0 = bp.par0; up.lb = bp.lb; up.ub = bp.ub;
    up.lambda = lambda;
    up.maxit = bp.maxit; up.lmm = bp.lmm; up.ftol = bp.ftol; up.pgtol = bp.pgtol;
    up.intr = bp.intr;
    up.par = bp.par; up.value = bp.value; up.n_iter = bp.n_iter; up.n_eval = bp.n_eval; up.status = bp.status;
    return up;
}
static int check_bfgs_update_extents(const BfgsUpdateParams &up, int n_series, const PlgSeriesHave &have, const char *dev,
                                     size_t block_bytes) {
    const int n_cells = up.S.n_cells, P = 6 + up.S.p + up.S.q;
    const size_t rows = sizeof(double) * (size_t)n_cells * P, vals = sizeof(double) * (size_t)n_cells;
    const size_t ints = sizeof(int) * (size_t)n_cells, box = sizeof(double) * (size_t)P;
    PlgExtent e[PLG_MAX_EXTENTS];
    int n = plg_series_extents(up.S, n_series, have.b, e);
    e[n++] = PlgExtent{"par0", up.par0, sizeof(double) * plg_rows_doubles(n_cells, P), rows, 1};
    e[n++] = PlgExtent{"lb", up.lb, sizeof(double) * plg_rows_doubles(1, P), box, 1};
    e[n++] = PlgExtent{"ub", up.ub, sizeof(double) * plg_rows_doubles(1, P), box, 1};
    e[n++] = PlgExtent{"par", up.par, sizeof(double) * plg_rows_doubles(n_cells, P), rows, 1};
    e[n++] = PlgExtent{"value", up.value, sizeof(double) * plg_rows_doubles(n_cells, 1), vals, 1};
    e[n++] = PlgExtent{"n_iter", up.n_iter, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    e[n++] = PlgExtent{"n_eval", up.n_eval, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    e[n++] = PlgExtent{"status", up.status, sizeof(int) * plg_rows_doubles(n_cells, 1), ints, 1};
    return refuse_bad_extent("ldsr_bfgs_update_kernel", e, n, dev, block_bytes);
}

extern "C" int ldsr_ssq_grad_batch(int device, int n_series, int T, int p, int q, const double *y,
                                   const double *u, const double *v, int shared_uv, const int *cell_offsets,
                                   const double *theta, double *ssq, double *grad) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    if (!theta || !ssq) return fail(LDSR_EINVAL, "theta and ssq must not be NULL");
    const int n_cells = cell_offsets[n_series];
    if (n_cells == 0) return LDSR_OK;
    const int P = 6 + p + q;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    SeriesUpload U{n_series, T, p, q, y, u, v, shared_uv};
    Carver c;
    U.carve(c, cell_offsets, theta);
    const size_t in_bytes = c.o;
    const size_t o_f = c.take(sizeof(double) * (size_t)n_cells);
    const size_t o_g = c.take(grad ? sizeof(double) * (size_t)n_cells * P : 0);
    const size_t out_bytes = c.o - o_f;
    const size_t strip_bytes = grad ? ssq_strip_bytes(n_cells, T) : 0;
    const size_t o_strip = c.take(strip_bytes);
    rc = arena_reserve(A, c.o, in_bytes + align256(out_bytes));
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    U.stage(A);
    HIPCHK(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, A->stream));
    SsqParams sp;
    sp.S = ssq_series(U, strip_bytes ? (double *)(dev + o_strip) : nullptr);
    sp.theta = U.d_theta;
    sp.ssq = (double *)(dev + o_f);
    sp.grad = grad ? (double *)(dev + o_g) : nullptr;
    HIPCHK(launch_ssq_grad(sp, A->stream));
    char *pout = pin + in_bytes;
    HIPCHK(hipMemcpyAsync(pout, dev + o_f, out_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    memcpy(ssq, pout, sizeof(double) * (size_t)n_cells);
    if (grad) memcpy(grad, pout + (o_g - o_f), sizeof(double) * (size_t)n_cells * P);
    return LDSR_OK;
}

// The block of ldsr_bfgs_batch / ldsr_bfgs_update_batch: [series | map | par0 | lb | ub | offsets] go up in one
// copy; then what the host always reads, the optional per-cell results, the winners' fit, the strip, the workspace.
struct BfgsCall {
    SeriesUpload U;
    bool update;
    int n_cells, P;
    WsLayout L;
    size_t nT, o_lb, o_ub, o_off, in_bytes, o_win, o_thw, o_vw, sel_bytes, o_par, o_val, o_nit, o_nev, o_st, cell_bytes,
           o_lik, o_X, o_Y, o_V, o_J, o_fst, fit_bytes, o_fsoc, o_fth, strip_bytes, o_strip, o_ws, total;
    BfgsCall(const SeriesUpload &series, const int *cell_offsets, const double *par0, bool update_)
        : U(series), update(update_) {
        const int n_series = U.n_series, T = U.T;
        n_cells = cell_offsets[n_series]; P = 6 + U.p + U.q;
        L = ws_layout(n_series, T, ldsr_pad_dim(U.p), ldsr_pad_dim(U.q), U.shared_uv, n_series, LDSR_ALGO_SCAN, 1);
        nT = (size_t)n_series * T;
        Carver c;
        U.carve(c, cell_offsets, par0);
        o_lb = c.take(sizeof(double) * (size_t)P);
        o_ub = c.take(sizeof(double) * (size_t)P);
        o_off = c.take(sizeof(int) * ((size_t)n_series + 1));
        in_bytes = c.o;
        o_win = c.take(sizeof(int) * (size_t)n_series);
        o_thw = c.take(sizeof(double) * (size_t)n_series * P);
        o_vw = c.take(sizeof(double) * (size_t)n_series);
        sel_bytes = c.o - o_win;
        o_par = c.take(sizeof(double) * (size_t)n_cells * P);
        o_val = c.take(sizeof(double) * (size_t)n_cells);
        o_nit = c.take(sizeof(int) * (size_t)n_cells);
        o_nev = c.take(sizeof(int) * (size_t)n_cells);
        o_st = c.take(sizeof(int) * (size_t)n_cells);
        cell_bytes = c.o - o_par;
        o_lik = c.take(sizeof(double) * (size_t)n_series);
        o_X = c.take(sizeof(double) * nT);
        o_Y = c.take(sizeof(double) * nT);
        o_V = c.take(sizeof(double) * nT);
        o_J = c.take(sizeof(double) * nT);
        o_fst = c.take(sizeof(int) * (size_t)n_series);
        fit_bytes = c.o - o_lik;
        o_fsoc = c.take(sizeof(int) * (size_t)n_series);
        o_fth = c.take(sizeof(double) * (size_t)n_series * P);
        strip_bytes = update ? plg_strip_bytes(n_cells, T) : ssq_strip_bytes(n_cells, T);
        o_strip = c.take(strip_bytes);
        o_ws = c.take(L.total);
        total = c.o;
    }
    // the pointers of the optimiser's launch (its scalars are the caller's); S: ssqTrain's series, after U.stage()
    BfgsParams params(char *dev) const {
        BfgsParams bp;
        memset(&bp, 0, sizeof(bp));
        bp.S = ssq_series(U, !update && strip_bytes ? (double *)(dev + o_strip) : nullptr);
        bp.par0 = (const double *)(dev + U.o_th);
        bp.lb = (const double *)(dev + o_lb);
        bp.ub = (const double *)(dev + o_ub);
        bp.par = (double *)(dev + o_par);
        bp.value = (double *)(dev + o_val);
        bp.n_iter = (int *)(dev + o_nit);
        bp.n_eval = (int *)(dev + o_nev);
        bp.status = (int *)(dev + o_st);
        return bp;
    }
    BfgsUpdateParams update_params(const BfgsParams &bp, char *dev, double lambda) const {
        return bfgs_update_params(bp, plg_series(U, dev, o_strip), lambda);
    }
    int check(const BfgsUpdateParams &up, size_t strip_have, const char *dev) const {
        return check_bfgs_update_extents(up, U.n_series, plg_series_have(U, strip_have), dev, total);
    }
};

// One launch runs every cell's optimisation from start to stop; a second picks the winners; the host then
// sees winner / theta_w / value_w, and the winners' fit is one pass of the existing propagate / FIT
// kernels on the prepared series.
// update: the objective is -pl at lambda (LDS_BFGS_with_update, plgrad.hip) instead of ssqTrain.
static int run_bfgs(bool update, double lambda, int device, int n_series, int T, int p, int q, const double *y,
                    const double *u, const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                    const double *lb, const double *ub, int maxit, int lmm, double factr, double pgtol,
                    int select_max, int fit_mode, double *par_all, double *value_all, int *n_iter_all,
                    int *n_eval_all, int *status_all, int *winner, double *theta_w, double *value_w, double *lik_w,
                    double *X, double *Y, double *V, double *J) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    const int P = 6 + p + q;
    rc = check_box(lb, ub, P, "variable");
    if (rc) return rc;
    if (!std::isfinite(lambda)) return fail(LDSR_EINVAL, "lambda must be finite");
    if (maxit < 1) return fail(LDSR_EINVAL, "maxit must be >= 1");
    if (lmm < 1 || lmm > BFGS_MAX_LMM) return fail(LDSR_EINVAL, "lmm must be in 1 .. 8");
    if (!(factr >= 0.0) || !std::isfinite(factr)) return fail(LDSR_EINVAL, "factr must be finite and >= 0");
    if (!(pgtol >= 0.0) || !std::isfinite(pgtol)) return fail(LDSR_EINVAL, "pgtol must be finite and >= 0");
    if (fit_mode != 0 && fit_mode != 1) return fail(LDSR_EINVAL, "fit_mode must be 0 (propagate) or 1 (Kalman_smoother)");
    if (!par0) return fail(LDSR_EINVAL, "par0 must not be NULL");
    if (!winner || !theta_w || !value_w) return fail(LDSR_EINVAL, "winner, theta_w and value_w must not be NULL");
    const int n_cells = cell_offsets[n_series];
    const bool want_fit = lik_w || X || Y || V || (J && fit_mode == 1);
    IntrScope intr_scope;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    BfgsCall B(SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, par0, update);
    SeriesUpload &U = B.U;
    const size_t nT = B.nT;
    const bool want_cells = par_all || value_all || n_iter_all || n_eval_all || status_all;
    rc = arena_reserve(A, B.total, B.in_bytes + align256(B.sel_bytes) + align256(std::max(B.cell_bytes, B.fit_bytes)));
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    U.stage(A);
    memcpy(pin + B.o_lb, lb, sizeof(double) * (size_t)P);
    memcpy(pin + B.o_ub, ub, sizeof(double) * (size_t)P);
    memcpy(pin + B.o_off, cell_offsets, sizeof(int) * ((size_t)n_series + 1));
    BfgsParams bp = B.params(dev);
    bp.maxit = maxit; bp.lmm = lmm;
    bp.ftol = factr * 0x1p-52; bp.pgtol = pgtol;
    bp.intr = intr_flag_for_kernels();
    const BfgsUpdateParams up = B.update_params(bp, dev, lambda);
    if (update && n_cells > 0) {        // (before anything is enqueued)
        rc = B.check(up, B.strip_bytes, dev);
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(dev, pin, B.in_bytes, hipMemcpyHostToDevice, A->stream));
    if (!update) {
        HIPCHK(launch_bfgs(bp, A->stream));
    } else if (n_cells > 0) {
        HIPCHK(launch_bfgs_update(up, A->stream));
    }
    BfgsSelectParams sl;
    sl.n_series = n_series; sl.P = P; sl.select_max = select_max;
    sl.cell_offsets = (const int *)(dev + B.o_off);
    sl.par = bp.par; sl.value = bp.value;
    sl.winner = (int *)(dev + B.o_win);
    sl.theta_w = (double *)(dev + B.o_thw);
    sl.value_w = (double *)(dev + B.o_vw);
    HIPCHK(launch_bfgs_select(sl, A->stream));
    char *psel = pin + B.in_bytes, *pbig = psel + align256(B.sel_bytes);
    HIPCHK(hipMemcpyAsync(psel, dev + B.o_win, B.sel_bytes, hipMemcpyDeviceToHost, A->stream));
    if (want_cells) HIPCHK(hipMemcpyAsync(pbig, dev + B.o_par, B.cell_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(wait_stream(A->stream));
    intr_poll();
    if (intr_raised()) return fail(LDSR_EINTERRUPTED, "interrupted by the caller's interrupt callback");
    memcpy(winner, psel, sizeof(int) * (size_t)n_series);
    memcpy(theta_w, psel + (B.o_thw - B.o_win), sizeof(double) * (size_t)n_series * P);
    memcpy(value_w, psel + (B.o_vw - B.o_win), sizeof(double) * (size_t)n_series);
    if (par_all) memcpy(par_all, pbig, sizeof(double) * (size_t)n_cells * P);
    if (value_all) memcpy(value_all, pbig + (B.o_val - B.o_par), sizeof(double) * (size_t)n_cells);
    if (n_iter_all) memcpy(n_iter_all, pbig + (B.o_nit - B.o_par), sizeof(int) * (size_t)n_cells);
    if (n_eval_all) memcpy(n_eval_all, pbig + (B.o_nev - B.o_par), sizeof(int) * (size_t)n_cells);
    if (status_all) memcpy(status_all, pbig + (B.o_st - B.o_par), sizeof(int) * (size_t)n_cells);
    if (!want_fit) return LDSR_OK;

    // the winners' fit: the series that have one, their thetas packed side by side
    std::vector<int> ws_series;
    std::vector<double> th((size_t)n_series * P);
    for (int s = 0; s < n_series; s++)
        if (winner[s] >= 0) {
            memcpy(&th[ws_series.size() * P], theta_w + (size_t)s * P, sizeof(double) * (size_t)P);
            ws_series.push_back(s);
        }
    const int n_w = (int)ws_series.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto fill = [&](double *a, size_t n) { if (a) std::fill(a, a + n, nan); };
    if (n_w < n_series) {
        fill(lik_w, (size_t)n_series); fill(X, nT); fill(Y, nT); fill(V, nT);
        if (fit_mode == 1) fill(J, nT);
    }
    if (n_w == 0) return LDSR_OK;
    HIPCHK(U.prep(device, A->stream, dev + B.o_ws, &B.L));
    rc = stage_h2d_async(device, A->stream, dev + B.o_fth, th.data(), sizeof(double) * (size_t)n_w * P);
    if (rc) return rc;
    const FitOut fit{(double *)(dev + B.o_X), (double *)(dev + B.o_Y), (double *)(dev + B.o_V), (double *)(dev + B.o_J),
                     (double *)(dev + B.o_lik), nullptr, (int *)(dev + B.o_fst)};
    rc = launch_smoother(U.ps, n_w, ws_series.data(), (const double *)(dev + B.o_fth), 1, fit_mode == 0 ? 1 : 0, 0.0, fit,
                         (int *)(dev + B.o_fsoc));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pbig, dev + B.o_lik, B.fit_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(wait_stream(A->stream));
    for (int i = 0; i < n_w; i++) {
        const size_t s = (size_t)ws_series[(size_t)i], row = sizeof(double) * (size_t)i * T;
        if (lik_w) lik_w[s] = ((const double *)pbig)[i];
        if (X) memcpy(X + s * T, pbig + (B.o_X - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (Y) memcpy(Y + s * T, pbig + (B.o_Y - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (V) memcpy(V + s * T, pbig + (B.o_V - B.o_lik) + row, sizeof(double) * (size_t)T);
        if (J && fit_mode == 1) memcpy(J + s * T, pbig + (B.o_J - B.o_lik) + row, sizeof(double) * (size_t)T);
    }
    // A series the scan kernel flagged (singular Svv / Tuu) has a smoother all the same: its winner takes the
    // serial kernel in a call of its own, which is what ldsr_smooth_batch gives for that theta.
    const int *fst = (const int *)(pbig + (B.o_fst - B.o_lik));
    const int off1[2] = {0, 1};
    for (int i = 0; i < n_w && smoother_is_scan(T, U.ps.PP, U.ps.QQ, B.L, fit_mode == 0 ? 1 : 0); i++) {
        if (fst[i] != LDSR_CELL_SINGULAR) continue;
        const size_t s = (size_t)ws_series[(size_t)i], uv = shared_uv ? 0 : s * T;
        auto row = [&](double *a) { return a ? a + s * T : nullptr; };
        double lik1;
        rc = run_fit_kernel(FIT_SMOOTH, device,
                            SeriesUpload{1, T, p, q, y + s * T, u ? u + uv * p : nullptr, v ? v + uv * q : nullptr, shared_uv},
                            off1, theta_w + s * P, 1, 0.0, FitOut{row(X), row(Y), row(V), row(J), &lik1}, true);
        if (rc) return rc;
        if (lik_w) lik_w[s] = lik1;
    }
    return LDSR_OK;
}

extern "C" int ldsr_bfgs_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                               const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                               const double *lb, const double *ub, int maxit, int lmm, double factr,
                               double pgtol, int select_max, int fit_mode, double *par_all, double *value_all,
                               int *n_iter_all, int *n_eval_all, int *status_all, int *winner, double *theta_w,
                               double *value_w, double *lik_w, double *X, double *Y, double *V, double *J) {
    return run_bfgs(false, 0.0, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, par0, lb, ub, maxit, lmm,
                    factr, pgtol, select_max, fit_mode, par_all, value_all, n_iter_all, n_eval_all, status_all, winner,
                    theta_w, value_w, lik_w, X, Y, V, J);
}

extern "C" int ldsr_bfgs_update_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                                      const double *v, int shared_uv, const int *cell_offsets, const double *par0,
                                      const double *lb, const double *ub, double lambda, int maxit, int lmm,
                                      double factr, double pgtol, int select_max, double *par_all, double *value_all,
                                      int *n_iter_all, int *n_eval_all, int *status_all, int *winner, double *theta_w,
                                      double *value_w, double *lik_w, double *X, double *Y, double *V, double *J) {
    return run_bfgs(true, lambda, device, n_series, T, p, q, y, u, v, shared_uv, cell_offsets, par0, lb, ub, maxit, lmm,
                    factr, pgtol, select_max, 1, par_all, value_all, n_iter_all, n_eval_all, status_all, winner,
                    theta_w, value_w, lik_w, X, Y, V, J);
}

// The block of ldsr_pl_grad_batch: [series | map | theta] go up in one copy, [pl | grad] come back in one.
struct PlGradCall {
    SeriesUpload U;
    int n_cells, P;
    size_t in_bytes, o_f, o_g, g_bytes, out_bytes, o_strip, strip_bytes, total;
    PlGradCall(const SeriesUpload &series, const int *cell_offsets, const double *theta, bool grad) : U(series) {
        n_cells = cell_offsets[U.n_series]; P = 6 + U.p + U.q;
        Carver c;
        U.carve(c, cell_offsets, theta);
        in_bytes = c.o;
        o_f = c.take(sizeof(double) * (size_t)n_cells);
        g_bytes = grad ? sizeof(double) * (size_t)n_cells * P : 0;
        o_g = c.take(g_bytes);
        out_bytes = c.o - o_f;
        strip_bytes = plg_strip_bytes(n_cells, U.T);
        o_strip = c.take(strip_bytes);
        total = c.o;
    }
    PlGradParams params(char *dev, double lambda) const {
        PlGradParams pp;
        pp.S = plg_series(U, dev, o_strip);
        pp.theta = (const double *)(dev + U.o_th);
        pp.lambda = lambda;
        pp.pl = (double *)(dev + o_f);
        pp.grad = g_bytes ? (double *)(dev + o_g) : nullptr;
        return pp;
    }
    int check(const PlGradParams &pp, size_t strip_have, const char *dev) const {
        PlgExtent e[PLG_MAX_EXTENTS];
        int n = plg_series_extents(pp.S, U.n_series, plg_series_have(U, strip_have).b, e);
        e[n++] = PlgExtent{"theta", pp.theta, sizeof(double) * plg_rows_doubles(n_cells, P), sizeof(double) * (size_t)n_cells * P, 1};
        e[n++] = PlgExtent{"pl", pp.pl, sizeof(double) * plg_rows_doubles(n_cells, 1), sizeof(double) * (size_t)n_cells, 1};
        e[n++] = PlgExtent{"grad", pp.grad, sizeof(double) * plg_rows_doubles(n_cells, P), g_bytes, 0};
        return refuse_bad_extent("ldsr_pl_grad_kernel", e, n, dev, total);
    }
};

extern "C" int ldsr_pl_grad_batch(int device, int n_series, int T, int p, int q, const double *y, const double *u,
                                  const double *v, int shared_uv, const int *cell_offsets, const double *theta,
                                  double lambda, double *pl, double *grad) {
    int rc = check_common(n_series, T, p, q, y, cell_offsets);
    if (rc) return rc;
    if (!theta || !pl) return fail(LDSR_EINVAL, "theta and pl must not be NULL");
    if (!std::isfinite(lambda)) return fail(LDSR_EINVAL, "lambda must be finite");
    if (cell_offsets[n_series] == 0) return LDSR_OK;
    ArenaLease lease;
    rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Arena *A = lease.a;
    PlGradCall call(SeriesUpload{n_series, T, p, q, y, u, v, shared_uv}, cell_offsets, theta, grad != nullptr);
    rc = arena_reserve(A, call.total, call.in_bytes + align256(call.out_bytes));
    if (rc) return rc;
    char *dev = A->dev, *pin = A->pin;
    call.U.stage(A);
    const PlGradParams pp = call.params(dev, lambda);
    rc = call.check(pp, call.strip_bytes, dev);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dev, pin, call.in_bytes, hipMemcpyHostToDevice, A->stream));
    HIPCHK(launch_pl_grad(pp, A->stream));
    char *pout = pin + call.in_bytes;
    HIPCHK(hipMemcpyAsync(pout, dev + call.o_f, call.out_bytes, hipMemcpyDeviceToHost, A->stream));
    HIPCHK(hipStreamSynchronize(A->stream));
    memcpy(pl, pout, sizeof(double) * (size_t)call.n_cells);
    if (grad) memcpy(grad, pout + (call.o_g - call.o_f), sizeof(double) * (size_t)call.n_cells * call.P);
    return LDSR_OK;
}

extern "C" int ldsr_plg_extent_check(int kernel, int n_series, int T, int p, int q, int has_u, int has_v, int shared_uv,
                                     const int *cell_offsets, int with_grad, long strip_short, long out_shift) {
    static const double present = 0.0;      // (y, u, v: only whether they are null matters here)
    int rc = check_common(n_series, T, p, q, &present, cell_offsets);
    if (rc) return rc;
    if (cell_offsets[n_series] < 1) return fail(LDSR_EINVAL, "the check needs at least one cell");
    char *const dev = (char *)(uintptr_t)0x100000;      // never dereferenced
    PlGradCall call(SeriesUpload{n_series, T, p, q, &present, has_u ? &present : nullptr, has_v ? &present : nullptr,
                                 shared_uv}, cell_offsets, nullptr, kernel == 1 || with_grad != 0);
    const PlGradParams pp0 = call.params(dev, 1.0);
    const size_t strip_have = call.strip_bytes - (size_t)strip_short;
    if (kernel == 0) {
        PlGradParams pp = pp0;
        if (pp.grad) pp.grad = (double *)((char *)pp.grad + out_shift);
        return call.check(pp, strip_have, dev);
    }
    // ldsr_bfgs_update_batch's own block
    const BfgsCall B(call.U, cell_offsets, nullptr, true);
    BfgsParams bp = B.params(dev);
    bp.par = (double *)((char *)bp.par + out_shift);
    return B.check(B.update_params(bp, dev, 1.0), B.strip_bytes - (size_t)strip_short, dev);
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
    rc = arena_reserve(A, c.o, in_bytes);
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
