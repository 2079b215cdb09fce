// host_runtime.hip -- the process-wide state of the C ABI's host units and the only code that touches it: error
// slot, interrupt registration, kernel timer, pinned staging ring, device arenas; and the shared argument checks.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "host_runtime.h"
#include "ldsr_device.h"       // LDSR_MAXPQ
#include "source_hash.h"       // LDSR_SOURCE_HASH, written by the Makefile

namespace ldsr_host {

static thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

const std::string &thread_error() { return g_err; }

extern "C" const char *ldsr_last_error(void) { return g_err.c_str(); }
extern "C" const char *ldsr_version(void) { return "ldsr_hip 0.4.0 (gfx950) src " LDSR_SOURCE_HASH; }
extern "C" const char *ldsr_source_hash(void) { return LDSR_SOURCE_HASH; }

extern "C" int ldsr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

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

void mark_worker_thread() { t_worker = true; }
bool thread_polls() { return t_poll; }

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

const int *intr_flag_for_kernels() { return g_intr.reg.load() ? g_intr.flag.load() : nullptr; }
bool intr_raised() {
    int *f = g_intr.flag.load();
    return g_intr.reg.load() && f && *(volatile int *)f != 0;
}

// Run the callback (external caller thread only); raise the flag if it asks to stop.
void intr_poll() {
    const IntrReg *r = g_intr.reg.load();
    int *f = g_intr.flag.load();
    if (!t_poll || !r || !f) return;
    if (*(volatile int *)f == 0 && r->cb(r->arg)) *(volatile int *)f = 1;
}

IntrScope::IntrScope() {
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
IntrScope::~IntrScope() {
    if (!owner) return;
    // the last external call to leave clears the flag: a raised interrupt stops every call that
    // is in flight and is over once they have all returned
    int *f = g_intr.flag.load();
    if (g_intr.active.fetch_sub(1) == 1 && f) *(volatile int *)f = 0;
    t_poll = false;
}

// Wait for a stream; the polling thread keeps the interrupt callback alive meanwhile.
hipError_t wait_stream(hipStream_t stream) {
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
hipError_t prof_begin(int device, hipStream_t stream, int *slot) {
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

hipError_t prof_end(hipStream_t stream, int slot) {
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

int stage_h2d_async(int device, hipStream_t stream, void *dst, const void *src, size_t bytes) {
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

// ---- device arenas of the host-pointer entry points (struct Arena: host_runtime.h) -----------------
static std::mutex g_arena_mu;
static std::vector<Arena *> g_arenas;

int arena_acquire(int device, Arena **out) {
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

// ---- guard mode (host_runtime.h) ---------------------------------------------------------------------
bool arena_guard_on() {
    static const bool on = [] { const char *e = getenv("LDSR_ARENA_GUARD"); return e && e[0] == '1'; }();
    return on;
}

static std::mutex g_guard_mu;
static std::vector<std::string> g_guard_hits;      // violations since the last ldsr_arena_guard_report

static void guard_record(const std::string &msg) {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard_hits.push_back(msg);
}

// the end of a lease (or a second reserve inside one): wait for the arena's stream, read the block back, look at
// every band
static void guard_check(Arena *a) {
    if (a->bands.empty()) return;
    std::vector<GuardBand> bands;
    bands.swap(a->bands);
    const std::string entry = a->entry ? a->entry : "?";
    const size_t used = bands.back().end;
    std::vector<unsigned char> host(used);
    hipError_t e = hipSetDevice(a->device);
    if (e == hipSuccess) e = hipStreamSynchronize(a->stream);
    if (e == hipSuccess) e = hipMemcpy(host.data(), a->dev, used, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        guard_record(entry + ": the bands could not be read back: " + hipGetErrorString(e));
        return;
    }
    for (size_t i = 0; i < bands.size(); i++) {
        size_t n = 0, first = 0, last = 0;
        for (size_t o = bands[i].begin; o < bands[i].end; o++)
            if (host[o] != 0xFF) {
                if (!n++) first = o;
                last = o;
            }
        if (!n) continue;
        char where[64], msg[256];
        if (i + 1 == bands.size()) snprintf(where, sizeof(where), "tail band");
        else snprintf(where, sizeof(where), "band behind carve %zu", i);
        snprintf(msg, sizeof(msg), "%s: %s (arena offsets %zu..%zu): %zu byte(s) changed, first at band offset %zu, last at %zu",
                 entry.c_str(), where, bands[i].begin, bands[i].end, n, first - bands[i].begin, last - bands[i].begin);
        guard_record(msg);
    }
}

extern "C" int ldsr_arena_guard_report(char *buf, size_t len) {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    std::string s;
    for (const std::string &h : g_guard_hits) s += h + "\n";
    if (buf && len) snprintf(buf, len, "%s", s.c_str());
    const int n = (int)g_guard_hits.size();
    g_guard_hits.clear();
    return n;
}

void arena_release(Arena *a) {
    if (!a) return;
    guard_check(a);
    std::lock_guard<std::mutex> lk(g_arena_mu);
    a->busy = false;
}

static int arena_reserve(Arena *a, size_t dev_bytes, size_t pin_bytes);

int arena_reserve(Arena *a, const Carver &c, size_t pin_bytes, const char *entry) {
    if (!c.guard) return arena_reserve(a, c.o, pin_bytes);
    guard_check(a);
    const int rc = arena_reserve(a, c.o + kGuardTail, pin_bytes);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(a->dev, 0xFF, a->dev_cap, a->stream));
    if (a->pin_cap) memset(a->pin, 0xFF, a->pin_cap);
    a->bands = c.bands;
    a->bands.push_back(GuardBand{c.o, c.o + kGuardTail});
    a->entry = entry;
    return LDSR_OK;
}

// Test hook: one lease with two buffers, one byte of the band between them set from the host (no kernel runs, and
// only the arena's own memory is touched); the next report counts exactly that.
extern "C" int ldsr_arena_guard_selftest(int device) {
    if (!arena_guard_on()) return fail(LDSR_EINVAL, "LDSR_ARENA_GUARD=1 is not set: the arenas have no bands");
    ArenaLease lease;
    int rc = arena_acquire(device, &lease.a);
    if (rc) return rc;
    Carver c;
    c.take(1000);
    c.take(1000);
    rc = arena_reserve(lease.a, c, 0, "ldsr_arena_guard_selftest");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(lease.a->stream));
    HIPCHK(hipMemset(lease.a->dev + c.bands[0].begin + 3, 0, 1));
    return LDSR_OK;
}

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

int check_common(int n_series, int T, int p, int q, const double *y,
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

int check_em(int niter, double tol) {
    if (niter < 2) return fail(LDSR_EINVAL, "niter must be >= 2 (the reference reads lik[1], src/EM.cpp:256)");
    if (!(tol >= 0.0)) return fail(LDSR_EINVAL, "tol must be >= 0");
    return LDSR_OK;
}

int check_box(const double *lb, const double *ub, int P, const char *noun) {
    if (!lb || !ub) return fail(LDSR_EINVAL, "lb and ub must not be NULL");
    for (int c = 0; c < P; c++) {
        if (!std::isfinite(lb[c]) || !std::isfinite(ub[c]) || !std::isfinite(ub[c] - lb[c]))
            return fail(LDSR_EINVAL, "lb and ub must be finite");
        if (lb[c] > ub[c]) return fail(LDSR_EINVAL, std::string("lb must be <= ub in every ") + noun);
    }
    return LDSR_OK;
}

}  // namespace ldsr_host
