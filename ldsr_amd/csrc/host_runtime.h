// host_runtime.h -- what every host unit of the C ABI (api_*.hip) stands on, defined in host_runtime.hip: the
// calling thread's error slot, user interrupts, the kernel timer, the pinned staging ring, the device arenas
// and the argument checks.  The state behind them is private to host_runtime.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

#include "../../include/ldsr_hip.h"

namespace ldsr_host {

// the calling thread's error slot (ldsr_last_error): fail() fills it and returns `code`
int fail(int code, const std::string &msg);
const std::string &thread_error();      // what this thread's last fail() left there

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(LDSR_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- user interrupts ---------------------------------------------------------------------------
void mark_worker_thread();      // the calling thread is a library worker: it never runs the callback
bool thread_polls();            // the calling thread entered the library from outside and runs the callback
const int *intr_flag_for_kernels();
bool intr_raised();
void intr_poll();

// RAII around an external EM entry: the outermost call on a non-worker thread becomes the poller
// and clears a stale flag when no other call is in flight.
struct IntrScope {
    bool owner = false;
    IntrScope();
    ~IntrScope();
};

hipError_t wait_stream(hipStream_t stream);

// ---- optional kernel timer ---------------------------------------------------------------------
hipError_t prof_begin(int device, hipStream_t stream, int *slot);
hipError_t prof_end(hipStream_t stream, int slot);

// ---- pinned staging ring -----------------------------------------------------------------------
int stage_h2d_async(int device, hipStream_t stream, void *dst, const void *src, size_t bytes);

// ---- device arenas of the host-pointer entry points -------------------------------------------
// One arena = one device block + one pinned host block (both grow-only) + one non-blocking
// stream.  A call leases a free arena of its device (or creates one), so concurrent callers never
// share buffers, and repeated calls of the same shape do no hipMalloc / hipFree at all.
// Guard mode (LDSR_ARENA_GUARD=1 in the environment, read once; a debug mode, off by default): a Carver leaves a
// band behind every buffer, arena_reserve adds a tail band and fills the whole device block (and the pinned block,
// which the entries' one upload copies over the bands between their inputs) with 0xFF before the entry uploads
// anything, and the end of the lease synchronises the stream, reads the bands back and records every changed byte
// for ldsr_arena_guard_report.  Off: Carver::take returns the offsets it always did and no call path does more.
bool arena_guard_on();
constexpr size_t kGuardBand = 256;              // behind every buffer, on top of its alignment slack
constexpr size_t kGuardTail = 64 * 1024;        // behind the last one

struct GuardBand {
    size_t begin, end;      // arena offsets: [end of the buffer's bytes, start of the next buffer)
};

struct Arena {
    int device = -1;
    hipStream_t stream = nullptr;
    char *dev = nullptr, *pin = nullptr;
    size_t dev_cap = 0, pin_cap = 0;
    bool busy = false;
    // guard mode: the bands of the lease's reserve (the last one is the tail band) and the entry that carved them
    std::vector<GuardBand> bands;
    const char *entry = nullptr;
};

int arena_acquire(int device, Arena **out);
void arena_release(Arena *a);

struct ArenaLease {     // releases on scope exit
    Arena *a = nullptr;
    ~ArenaLease() { arena_release(a); }
};

// bump allocator over an arena block: first pass sizes, second pass hands out pointers.  sub: a layout inside one
// buffer of another Carver (the EM workspace, the restart grid's winners' block): never banded.
struct Carver {
    size_t o = 0;
    bool guard;
    std::vector<GuardBand> bands;       // (guard mode only)
    explicit Carver(bool sub = false) : guard(!sub && arena_guard_on()) {}
    size_t take(size_t bytes) {
        const size_t r = o, n = bytes ? bytes : 8;
        o = align256(o + n);
        if (guard) {
            o += kGuardBand;
            bands.push_back(GuardBand{r + n, o});
        }
        return r;
    }
};

// room for what `c` carved (guard mode: and its bands, checked when the lease ends under the name `entry`)
int arena_reserve(Arena *a, const Carver &c, size_t pin_bytes, const char *entry);

// ---- argument checks shared by the entries -----------------------------------------------------
int check_common(int n_series, int T, int p, int q, const double *y, const int *cell_offsets);
int check_em(int niter, double tol);
int check_box(const double *lb, const double *ub, int P, const char *noun);

}  // namespace ldsr_host
