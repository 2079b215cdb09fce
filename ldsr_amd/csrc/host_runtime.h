// host_runtime.h -- what every host unit of the C ABI (api_*.hip) stands on, defined in host_runtime.hip: the
// calling thread's error slot, user interrupts, the kernel timer, the pinned staging ring, the device arenas
// and the argument checks.  The state behind them is private to host_runtime.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

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
struct Arena {
    int device = -1;
    hipStream_t stream = nullptr;
    char *dev = nullptr, *pin = nullptr;
    size_t dev_cap = 0, pin_cap = 0;
    bool busy = false;
};

int arena_acquire(int device, Arena **out);
void arena_release(Arena *a);

struct ArenaLease {     // releases on scope exit
    Arena *a = nullptr;
    ~ArenaLease() { arena_release(a); }
};

int arena_reserve(Arena *a, size_t dev_bytes, size_t pin_bytes);

// bump allocator over an arena block: first pass sizes, second pass hands out pointers
struct Carver {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t r = o;
        o = align256(o + (bytes ? bytes : 8));
        return r;
    }
};

// ---- argument checks shared by the entries -----------------------------------------------------
int check_common(int n_series, int T, int p, int q, const double *y, const int *cell_offsets);
int check_em(int niter, double tol);
int check_box(const double *lb, const double *ub, int P, const char *noun);

}  // namespace ldsr_host
