// tgp_api.hip -- the C-ABI of libturbogp.so (see include/turbogp.h for the reference call
// sites each entry replaces).  Host orchestration only: buffers, copies, launch order, status.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "host_backend.hpp"
#include "host_lbfgsb.hpp"
#include "host_slice.hpp"
#include "tgp_internal.hpp"
#include "pairwise.hpp"
#include "warp_math.hpp"

using namespace tgp;

struct tgp_handle_s {
    Context c;
    tgp_host::HostGP *host = nullptr;   // tgp_create(TGP_DEVICE_HOST): this handle never touches HIP
    bool worker = false;                 // a pooled worker handle (tgp_workers_acquire): owned by the library, tgp_destroy refuses it
};

// ---- the device's pool of WORKER handles (round 5) -------------------------------------------------------------
// A worker is a handle on a private stream: what runs the concurrent starts of a hyper-parameter fit above the
// one-launch sizes, in C++ threads (tgp_fit_optimise) or in the host's threads (HipGPSurrogate drives tgp_fit_grad on
// them with SciPy).  Round 4 gave every factory / every caller handle three or four of its own and kept them alive:
// with two factories in a process that is the library's shared streams + 6-8 private ones on the runtime's hardware
// queues (4 by default, 8 asked for by turbo_amd/_lib.py), two streams share a queue, run one after the other, and a
// hyper-parameter fit took twice as long (N = 500: 11.6 -> 19.3 ms).  Now ONE pool per device serves every caller, one
// hyper-parameter fit at a time (the pool's mutex is held from acquire to release): at most MAX_WORKERS private
// streams per device whatever the number of factories.  The workers live until the last ordinary handle on the device
// is destroyed.
namespace {
constexpr int MAX_WORKERS = 4;
struct WorkerPool {
    std::mutex mu;                       // held from tgp_workers_acquire to tgp_workers_release
    std::atomic<std::thread::id> owner{std::thread::id()};   // ... by this thread (valid while held; read without the mutex by acquire / release)
    std::atomic<bool> held{false};
    std::vector<tgp_handle> workers;
    int users = 0;                       // ordinary (non-worker) GPU handles alive on the device
    std::mutex count_mu;                 // guards users / the workers' destruction against a concurrent create
};
WorkerPool g_pools[64];
}  // namespace

// ---- the library's START THREADS (round 6) ----------------------------------------------------------------------
// tgp_fit_lbfgsb runs the starts of a hyper-parameter fit side by side, a host thread each.  Round 5 created and joined
// those threads in every call: at the small sizes of the reference's everyday regime (N <= 128: a whole fit is 1-2 ms)
// creating three threads -- and the HIP runtime's per-thread set-up at each one's first call -- was a tenth of the call.
// Now up to MAX_WORKERS - 1 threads live for the process (detached, parked on a condition variable; the state is
// never destroyed, so nothing runs at exit), and a call hands them its shares: helper t runs fn(t), the caller fn(0).
// Only the holder of a device's worker pool dispatches (tgp_workers_acquire serialises the fits of a device), and the
// helpers are shared by all devices: a second device's fit waits at `busy` for the first one's shares to finish.
namespace {
struct StartThreads {
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::function<void(int)> fn;
    int pending = 0;              // shares handed out and not finished
    unsigned long long epoch = 0; // bumped per dispatch
    int want = 0;                 // shares 1 .. want of this epoch are the helpers'
    int taken = 0;
    int threads = 0;
    bool busy = false;
};
StartThreads &start_threads() {
    static StartThreads *st = new StartThreads();      // (leaked on purpose: parked detached threads must outlive every static)
    return *st;
}
void start_thread_main() {
    StartThreads &st = start_threads();
    unsigned long long seen = 0;
    std::unique_lock<std::mutex> lk(st.mu);
    for (;;) {
        st.cv_work.wait(lk, [&] { return st.epoch != seen && st.taken < st.want; });
        const int share = ++st.taken;
        if (st.taken == st.want) seen = st.epoch;      // (this epoch has no share left for this thread)
        std::function<void(int)> fn = st.fn;
        lk.unlock();
        fn(share);
        lk.lock();
        if (st.taken >= st.want) seen = st.epoch;
        if (--st.pending == 0) st.cv_done.notify_all();
    }
}
// fn(0) on the caller, fn(1) .. fn(T - 1) on the parked threads (created on demand); returns how many shares ran on
// helpers -- the caller runs the rest itself when threads could not be had
int run_on_start_threads(int T, const std::function<void(int)> &fn) {
    StartThreads &st = start_threads();
    int helpers = 0;
    {
        std::unique_lock<std::mutex> lk(st.mu);
        st.cv_done.wait(lk, [&] { return !st.busy; });
        while (st.threads < T - 1) {
            try {
                std::thread(start_thread_main).detach();
                ++st.threads;
            } catch (const std::system_error &) {
                break;
            }
        }
        helpers = std::min(T - 1, st.threads);
        if (helpers > 0) {
            st.busy = true;
            st.fn = fn;
            st.want = helpers; st.taken = 0; st.pending = helpers;
            ++st.epoch;
            st.cv_work.notify_all();
        }
    }
    fn(0);
    for (int t = helpers + 1; t < T; ++t) fn(t);
    if (helpers > 0) {
        std::unique_lock<std::mutex> lk(st.mu);
        st.cv_done.wait(lk, [&] { return st.pending == 0; });
        st.fn = nullptr;
        st.busy = false;
        st.cv_done.notify_all();
    }
    return helpers;
}
}  // namespace

// entries that only exist on the GPU
#define HOST_NA(name)                                                                                   \
    do {                                                                                                \
        if (h->host) {                                                                                  \
            h->host->err = name ": not available on the host backend (a TGP_DEVICE_HOST handle keeps a " \
                                "reloaded model queryable: fit, predict, acquisition; the rest needs the GPU)"; \
            return TGP_BAD_ARG;                                                                         \
        }                                                                                               \
    } while (0)

static thread_local std::string g_create_err;

namespace tgp {
int prof_mark(Context &c, hipStream_t s) {
    if (!c.profiling) return -1;
    if (c.ev_used == c.ev_pool.size()) {
        Ev e;
        if (e.create(hipEventDefault) != hipSuccess) { (void)hipGetLastError(); return -1; }
        c.ev_pool.push_back(std::move(e));
    }
    if (hipEventRecord(c.ev_pool[c.ev_used], s) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return (int)c.ev_used++;
}
void prof_seg(Context &c, int a, int b, int kind, double flops) {
    if (a >= 0 && b >= 0) c.segs.push_back(ProfSeg{a, b, kind, flops});
}
}  // namespace tgp

static void prof_collect(Context &c) {
    for (const auto &g : c.segs) {
        float ms = 0.f;
        if (hipEventSynchronize(c.ev_pool[g.b]) == hipSuccess &&
            hipEventElapsedTime(&ms, c.ev_pool[g.a], c.ev_pool[g.b]) == hipSuccess) {
            if (g.kind == 0) { c.trmm_ms += ms; c.trmm_launches++; c.trmm_flops += g.flops; }
            else if (g.kind == 2) { c.screen_ms += ms; }
            else { c.kstar_ms += ms; c.kstar_launches++; }
        } else {
            (void)hipGetLastError();
        }
    }
    c.segs.clear();
    c.ev_used = 0;
}

static int fail(Context &c, int code, const std::string &msg) {
    c.err = msg;
    return code;
}
static int hip_fail(Context &c, hipError_t e, const char *where) {
    c.err = std::string(where) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return TGP_HIP_ERROR;
}

// The front of a sweep a fit started on the device's third stream (tgp_set_overlap): EVERY entry that uses the
// handle's buffers first makes its own stream wait for it -- one hipStreamWaitEvent, and only when something is
// pending -- so that nothing a later call writes, frees or re-uses is still being read or written over there.
// ... and the front is DISCARDED: only tgp_sweep, which looks at c.pre.front before it joins, can use one -- whatever
// else is called between the fit and the sweep may have changed the candidates (in place, same pointer and count),
// the factor or the workspace.
static hipError_t pre_join(Context &c) {
    c.pre.front = false;
    if (!c.pre.pending) return hipSuccess;
    c.pre.pending = false;
    return hipStreamWaitEvent(c.stream, c.pre.ev, 0);
}

#define API_HIP(call, where)                                    \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return hip_fail(c, e_, where);    \
    } while (0)

// ---- polled completion of the short calls (doorbell.hpp) ----
// the doorbell of the polled call about to be launched on this handle, or a null one (TGP_POLL_US=0)
static Bell bell_next(Context &c) {
    Bell b{nullptr, 0, nullptr};
    if (tuning().poll_us > 0 && c.h_bell.dev()) { b.word = c.h_bell.dev(); b.seq = ++c.bell_seq; b.ticket = c.d_ticket; }
    return b;
}
// wait for that call: spin on the mapped word, after TGP_POLL_US (or without a bell) synchronise the stream
static int bell_wait(Context &c, const Bell &b, const char *where) {
    if (b.word) {
        const volatile unsigned long long *w = c.h_bell;
        const auto t0 = std::chrono::steady_clock::now();
        const auto limit = std::chrono::microseconds(tuning().poll_us);
        for (unsigned spin = 1;; ++spin) {
            if (*w == b.seq) {
                std::atomic_thread_fence(std::memory_order_acquire);
                return TGP_OK;
            }
            __builtin_ia32_pause();
            if ((spin & 255u) == 0 && std::chrono::steady_clock::now() - t0 > limit) break;
        }
    }
    API_HIP(hipStreamSynchronize(c.stream), where);
    return TGP_OK;
}
// device time of the polled call that just finished, from the kernels' own wall_clock64() stamps (100 MHz)
static double bell_ms(const Context &c) {
    const unsigned long long t0 = c.h_bell[1], t1 = c.h_bell[2];
    return t1 >= t0 ? (double)(t1 - t0) * 1e-5 : 0.0;
}

// ---- one call's clock and its one wait ----
// A polled call (live bell) records no event and is timed on the host clock, launch to doorbell -- a sweep -- or by the
// kernels' own stamps (device_ticks) -- a fit; any other call is bracketed by ev0 / ev1 on its stream and ends in a
// stream synchronisation.
struct CallClock {
    Bell bell{nullptr, 0, nullptr};
    std::chrono::steady_clock::time_point t0{};
    bool stopped = false;      // ev1 is out
    bool device_ticks = false; // a polled call reports bell_ms(): what last_fit_ms has always meant
};
static int call_begin(Context &c, CallClock &k) {
    if (!k.bell.word) API_HIP(hipEventRecord(c.ev0, c.stream), "hipEventRecord");
    else if (!k.device_ticks) k.t0 = std::chrono::steady_clock::now();
    return TGP_OK;
}
// optional: ev1 HERE, so that what the entry queues behind it (copies back to the caller) is not timed
static int call_stop(Context &c, CallClock &k) {
    if (!k.bell.word && !k.stopped) API_HIP(hipEventRecord(c.ev1, c.stream), "hipEventRecord");
    k.stopped = true;
    return TGP_OK;
}
// wait for the call and leave its time in last_ms (c.last_fit_ms / c.last_sweep_ms)
static int call_finish(Context &c, CallClock &k, double &last_ms, const char *where) {
    if (k.bell.word) {
        const int rc = bell_wait(c, k.bell, where);
        if (rc == TGP_OK)
            last_ms = k.device_ticks ? bell_ms(c) : std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - k.t0).count();
        return rc;
    }
    const int rc = call_stop(c, k);
    if (rc != TGP_OK) return rc;
    API_HIP(hipStreamSynchronize(c.stream), where);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c.ev0, c.ev1);
    last_ms = ms;
    return TGP_OK;
}

// No C++ exception may cross the C boundary: every entry is a function-try-block.
static int exception_status(tgp_handle h, const char *fn, const char *what, int code) {
    try {
        if (h) (h->host ? h->host->err : h->c.err) = std::string(fn) + ": " + what;
    } catch (...) {
    }
    return code;
}
#define TGP_CATCH_AS(fn)                                                                        \
    catch (const std::bad_alloc &) { return exception_status(h, fn, "out of host memory", TGP_NO_MEMORY); } \
    catch (const std::exception &ex_) { return exception_status(h, fn, ex_.what(), TGP_HIP_ERROR); }       \
    catch (...) { return exception_status(h, fn, "unknown C++ exception", TGP_HIP_ERROR); }
#define TGP_CATCH TGP_CATCH_AS(__func__)

// Growing a buffer of the handle: dev_mem.hpp's reserve() contract, with c.stream drained before the old block goes
// (sync = false: nothing on the device can be using it -- empty, or its streams known idle)
template <class B>
static int grow(Context &c, B &buf, size_t need, const char *what, bool sync = true) {
    const hipError_t e = buf.reserve(need, [&] {
        const hipError_t se = sync ? hipStreamSynchronize(c.stream) : hipSuccess;
        if (se != hipSuccess) what = "hipStreamSynchronize";
        return se;
    });
    return e == hipSuccess ? TGP_OK : hip_fail(c, e, what);
}
#define API_MEM(call) do { const int rc_ = (call); if (rc_ != TGP_OK) return rc_; } while (0)

// y normalisation (sklearn _gpr.py:272-282): mean, population std, exact-zero std -> 1
static void normalise_targets(const double *y, int64_t N, int normalize_y, std::vector<double> &yn,
                              double &mean, double &sd) {
    mean = 0.0; sd = 1.0;
    if (normalize_y) {
        long double s = 0.0L;
        for (int64_t i = 0; i < N; ++i) s += y[i];
        mean = (double)(s / (long double)N);
        long double v = 0.0L;
        for (int64_t i = 0; i < N; ++i) { const long double t = (long double)y[i] - mean; v += t * t; }
        sd = sqrt((double)(v / (long double)N));
        if (sd == 0.0) sd = 1.0;
        for (int64_t i = 0; i < N; ++i) yn[i] = (y[i] - mean) / sd;
    } else {
        for (int64_t i = 0; i < N; ++i) yn[i] = y[i];
    }
}

extern "C" {

const char *tgp_version(void) { return "turbogp 0.1 gfx950"; }

const char *tgp_last_error(tgp_handle h) { return h ? (h->host ? h->host->err.c_str() : h->c.err.c_str()) : g_create_err.c_str(); }

int tgp_create(int device, int dtype, tgp_handle *out) {
    if (!out) { g_create_err = "tgp_create: out is NULL"; return TGP_BAD_ARG; }
    *out = nullptr;
    if (dtype != TGP_F64 && dtype != TGP_F32 && dtype != TGP_F32X3 && dtype != TGP_F32H2) { g_create_err = "tgp_create: dtype must be TGP_F64, TGP_F32, TGP_F32X3 or TGP_F32H2"; return TGP_BAD_ARG; }
    if (device == TGP_DEVICE_HOST) {   // no HIP call on this path (always f64, whatever dtype says)
        tgp_handle hh = new (std::nothrow) tgp_handle_s();
        if (hh) hh->host = new (std::nothrow) tgp_host::HostGP();
        if (!hh || !hh->host) { delete hh; g_create_err = "tgp_create: out of host memory"; return TGP_NO_MEMORY; }
        *out = hh;
        return TGP_OK;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_err = std::string("tgp_create: no HIP device (") + hipGetErrorString(e) + ")";
        (void)hipGetLastError();
        return TGP_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { g_create_err = "tgp_create: device index out of range"; return TGP_BAD_ARG; }
    tgp_handle h = new (std::nothrow) tgp_handle_s();
    if (!h) { g_create_err = "tgp_create: out of host memory"; return TGP_HIP_ERROR; }
    Context &c = h->c;
    c.device = device;
    c.dtype = dtype;
    auto bail = [&](hipError_t er, const char *w) {
        g_create_err = std::string(w) + ": " + hipGetErrorString(er);
        (void)hipGetLastError();
        const bool had = c.stream != nullptr;
        delete h;   // (the owners give back what was created so far)
        if (had) device_streams_release(device);
        return (int)TGP_HIP_ERROR;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = device_streams(device, &c.stream, nullptr)) != hipSuccess) return bail(e, "hipStreamCreate");
    if ((e = c.ev0.create(hipEventDefault)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = c.ev1.create(hipEventDefault)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = c.pre.ev.create(hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = c.pre.ev_in.create(hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = c.d_scal.reserve(4 * sizeof(double))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = c.d_flag.reserve(sizeof(int))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = c.d_best.reserve(sizeof(double))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = c.d_besti.reserve(4 * sizeof(long long))) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemset(c.d_besti, 0, 4 * sizeof(long long))) != hipSuccess) return bail(e, "hipMemset");   // [1] = clamp counter, kept at zero between calls
    // the doorbell of the short calls: one cache line of coherent device-mapped host memory + ticket counters
    if ((e = c.h_bell.reserve(64)) != hipSuccess) return bail(e, "hipHostMalloc");
    memset(c.h_bell, 0, 64);
    if ((e = c.d_ticket.reserve(64)) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemset(c.d_ticket, 0, 64)) != hipSuccess) return bail(e, "hipMemset");
    {
        WorkerPool &wp = g_pools[device & 63];
        std::lock_guard<std::mutex> lk(wp.count_mu);
        ++wp.users;
    }
    *out = h;
    return TGP_OK;
}

static int destroy_handle(tgp_handle h);

int tgp_destroy(tgp_handle h) try {
    if (!h) return TGP_OK;
    if (h->host) { delete h->host; delete h; return TGP_OK; }
    if (h->worker) return fail(h->c, TGP_BAD_ARG, "tgp_destroy: a pooled worker handle belongs to the library (tgp_workers_acquire)");
    return destroy_handle(h);
} TGP_CATCH

static int destroy_handle(tgp_handle h) {
    Context &c = h->c;
    if (!h->worker) {   // the last ordinary handle on the device takes the worker pool with it
        WorkerPool &wp = g_pools[c.device & 63];
        std::vector<tgp_handle> doomed;
        {
            std::lock_guard<std::mutex> lk(wp.count_mu);
            if (--wp.users == 0) {
                std::lock_guard<std::mutex> lk2(wp.mu);
                doomed.swap(wp.workers);
            }
        }
        for (tgp_handle w : doomed) (void)destroy_handle(w);
    }
    (void)hipSetDevice(c.device);
    if (c.pre.pending && c.stream_pre) (void)hipStreamSynchronize(c.stream_pre);   // the front of a sweep nobody came for
    c.pre.pending = false;
    if (c.stream) (void)hipStreamSynchronize(c.stream);
    prof_collect(c);
    const int dev = c.device;
    const hipStream_t own = c.stream_own;
    delete h;   // every owner frees here: the device is selected and the streams are idle
    if (own) { (void)hipStreamSynchronize(own); (void)hipStreamDestroy(own); }
    device_streams_release(dev);
    return TGP_OK;
}

int tgp_set_private_stream(tgp_handle h, int on) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_set_private_stream");
    Context &c = h->c;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    if (on && !c.stream_own) {
        API_HIP(hipStreamCreateWithFlags(&c.stream_own, hipStreamNonBlocking), "hipStreamCreate");
        c.stream = c.stream_own;
    } else if (!on && c.stream_own) {
        hipStream_t shared = nullptr;
        hipError_t e = device_streams(c.device, &shared, nullptr);   // (takes a reference ...)
        if (e != hipSuccess) return hip_fail(c, e, "device_streams");
        device_streams_release(c.device);                            // (... which this handle already holds)
        (void)hipStreamDestroy(c.stream_own);
        c.stream_own = nullptr;
        c.stream = shared;
    }
    return TGP_OK;
} TGP_CATCH

// n worker handles of h's device (each on a private stream), the pool locked for the caller until tgp_workers_release
int tgp_workers_acquire(tgp_handle h, int n, tgp_handle *out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_workers_acquire");
    Context &c = h->c;
    if (!out || n < 1 || n > MAX_WORKERS) return fail(c, TGP_BAD_ARG, "tgp_workers_acquire: need out and 1 <= n <= 4");
    if (h->worker) return fail(c, TGP_BAD_ARG, "tgp_workers_acquire: a worker handle cannot borrow workers");
    WorkerPool &wp = g_pools[c.device & 63];
    if (wp.held.load(std::memory_order_acquire) && wp.owner.load(std::memory_order_acquire) == std::this_thread::get_id())
        return fail(c, TGP_BAD_ARG, "tgp_workers_acquire: this thread already holds the device's pool (release it first)");
    wp.mu.lock();
    while ((int)wp.workers.size() < n) {
        tgp_handle w = nullptr;
        int rc = tgp_create(c.device, TGP_F64, &w);
        if (rc == TGP_OK) {
            {   // (a worker is not a user of the device: the pool goes when the last ORDINARY handle does)
                std::lock_guard<std::mutex> lk(wp.count_mu);
                --wp.users;
            }
            w->worker = true;
            rc = tgp_set_private_stream(w, 1);
            if (rc != TGP_OK) (void)destroy_handle(w);
        }
        if (rc != TGP_OK) {
            wp.mu.unlock();
            return fail(c, rc, "tgp_workers_acquire: could not create a worker handle on a stream of its own");
        }
        wp.workers.push_back(w);
    }
    for (int i = 0; i < n; ++i) out[i] = wp.workers[(size_t)i];
    wp.owner.store(std::this_thread::get_id(), std::memory_order_release);
    wp.held.store(true, std::memory_order_release);
    return TGP_OK;
} TGP_CATCH

int tgp_workers_release(tgp_handle h) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_workers_release");
    WorkerPool &wp = g_pools[h->c.device & 63];
    // (only the thread that holds the pool reads `held` as true with its own id: the fields are written under the mutex)
    if (!wp.held.load(std::memory_order_acquire) || wp.owner.load(std::memory_order_acquire) != std::this_thread::get_id())
        return fail(h->c, TGP_BAD_ARG, "tgp_workers_release: the pool is not held by this thread");
    // a worker that grew to a large problem does not keep its four N^2 f64 buffers until the device's last handle goes
    // (2 GiB each at N = 8192, three workers): above 0.5 GiB they are given back here; the next large fit allocates
    // again (well under a millisecond against a fit of tens of milliseconds)
    for (tgp_handle w : wp.workers) {
        if (w->c.cap_Np > 4096) {
            (void)hipSetDevice(w->c.device);
            (void)hipStreamSynchronize(w->c.stream);
            w->c.fitted = false;
            static_cast<FitMem &>(w->c) = FitMem{};
            w->c.linv_extent = 0;
        }
    }
    wp.owner.store(std::thread::id(), std::memory_order_release);
    wp.held.store(false, std::memory_order_release);
    wp.mu.unlock();
    return TGP_OK;
} TGP_CATCH

// The next fits start the sweep of the RESIDENT candidate batch inside themselves (include/turbogp.h).
int tgp_set_overlap(tgp_handle h, int mode) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_set_overlap");
    Context &c = h->c;
    if (mode < 0 || mode > 2) return fail(c, TGP_BAD_ARG, "tgp_set_overlap: mode must be 0, 1 or 2");
    c.pre.mode = mode;
    return TGP_OK;
} TGP_CATCH

int tgp_stream_status(tgp_handle h, int *out3) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_stream_status");
    Context &c = h->c;
    if (!out3) return fail(c, TGP_BAD_ARG, "tgp_stream_status: out3 is NULL");
    device_stream_status(c.device, &out3[0], &out3[1]);
    out3[2] = runtime_hw_queues_env();
    return TGP_OK;
} TGP_CATCH

// the reference's host candidate draw (NumPy's global MT19937 stream, continued in C++: host_backend.hpp)
int tgp_mt19937_uniform_columns(uint32_t *key624, int32_t *pos, int64_t M, int64_t D, const double *lo, const double *hi,
                                double *out) {
    try {
        return tgp_host::mt19937_uniform_columns(key624, pos, M, D, lo, hi, out);
    } catch (const std::bad_alloc &) {
        return TGP_NO_MEMORY;
    } catch (...) {
        return TGP_HIP_ERROR;
    }
}

int64_t tgp_tuning(char *buf, int64_t cap) {
    try {
        const std::string t = tuning().dump();
        if (buf && cap > 0) {
            const size_t n = std::min<size_t>((size_t)cap - 1, t.size());
            memcpy(buf, t.data(), n);
            buf[n] = 0;
        }
        return (int64_t)t.size() + 1;
    } catch (...) {
        return -1;
    }
}

// pinned, device-mapped host memory for the small-problem path: the kernels read their inputs
// from it and write their scalars / small outputs to it, so a call needs no memcpy at all
static int ensure_pinned(Context &c, Pin<double> &buf, size_t bytes) {
    if (bytes <= buf.bytes()) return TGP_OK;
    return grow(c, buf, std::max<size_t>(bytes, 1u << 20), "hipHostMalloc");
}
static int ensure_pinned(Context &c, size_t in_bytes, size_t out_bytes) {
    API_MEM(ensure_pinned(c, c.h_pin_in, in_bytes));
    return ensure_pinned(c, c.h_pin_out, out_bytes);
}

static bool small_path_enabled() {
    return tuning().small != 0;   // A/B switch
}

static int ensure_workspace(Context &c);

// LML-gradient workspace of the blocked path (allocated on first use, grown with the fit)
static int ensure_grad_workspace(Context &c) {
    if (c.Np > c.g_cap_Np || c.Dp > c.g_cap_Dp) {
        c.g_cap_Np = c.g_cap_Dp = 0;   // (until both exist)
        const size_t nt = (size_t)(c.Np / 64);
        API_MEM(grow(c, c.d_gpart, nt * (nt + 1) / 2 * (size_t)(3 + c.Dp) * sizeof(double), "hipMalloc gpart"));
        API_MEM(grow(c, c.d_gout, (size_t)(3 + c.Dp) * sizeof(double), "hipMalloc gout"));
        c.g_cap_Np = c.Np; c.g_cap_Dp = c.Dp;
    }
    return TGP_OK;
}

// leave-one-out workspaces, grown with the fit like the gradient's: the vectors (tgp_loo), and for the gradient also
// A (Np, Np) and the pairwise pass's partials
static int ensure_loo_workspace(Context &c, bool grad) {
    if (c.Np > c.loov_cap_Np) {
        c.loov_cap_Np = 0;
        API_MEM(grow(c, c.d_loov, (loo_vec_doubles(c.Np) + 2) * sizeof(double), "hipMalloc LOO vectors"));
        c.loov_cap_Np = c.Np;
    }
    if (!grad) return TGP_OK;
    if (c.Np > c.looA_cap_Np) {
        c.looA_cap_Np = 0;
        API_MEM(grow(c, c.d_looA, (size_t)c.Np * c.Np * sizeof(double), "hipMalloc LOO A"));
        c.looA_cap_Np = c.Np;
    }
    return ensure_grad_workspace(c);
}
// where launch_loo_points leaves [L_LOO, bad count] when the caller has no device-mapped place for them
static double *loo_scal_dev(Context &c) { return c.d_loov + loo_vec_doubles(c.loov_cap_Np); }

// the fit state's device buffers for Np padded rows and D dimensions.  full: everything a fit needs; otherwise only what
// a handle that RECEIVES a factor needs to sweep with it (tgp_import_factor_dev: no K, no inverse workspaces -- 4 N^2
// doubles less); a later fit on such a handle allocates the rest
static int ensure_fit_buffers(Context &c, int64_t Np, int64_t D, bool full) {
    if (Np <= c.cap_Np && D <= c.cap_D && (c.cap_full || !full)) return TGP_OK;
    const int64_t Dp = ((D + 3) / 4) * 4;
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    static_cast<FitMem &>(c) = FitMem{};   // (cap_Np = 0 until the whole set exists; linv_ld = 0: contents unknown)
    const size_t nn = (size_t)Np * Np;
    API_MEM(grow(c, c.d_Xs, (size_t)Np * Dp * sizeof(double), "hipMalloc Xs", false));
    API_MEM(grow(c, c.d_ls, (size_t)D * sizeof(double), "hipMalloc ls", false));
    API_MEM(grow(c, c.d_Linv, nn * sizeof(double), "hipMalloc Linv", false));
    if (full) {
        API_MEM(grow(c, c.d_K, nn * sizeof(double), "hipMalloc K", false));
        API_MEM(grow(c, c.d_W, nn * sizeof(double), "hipMalloc W", false));
        API_MEM(grow(c, c.d_U, nn * sizeof(double), "hipMalloc U", false));
        API_MEM(grow(c, c.d_Dinv, (size_t)2 * (Np / NB) * NB * NB * sizeof(double), "hipMalloc Dinv", false));
        API_MEM(grow(c, c.d_Apan, (size_t)2 * (Np / NB) * NB * NB * sizeof(double), "hipMalloc Apan", false));
        API_MEM(grow(c, c.d_apart, ((size_t)(Np / 128) * Np + Np / 128) * sizeof(double), "hipMalloc alpha shares", false));
        API_MEM(grow(c, c.d_t1, (size_t)Np * sizeof(double), "hipMalloc t1", false));
        API_MEM(grow(c, c.d_t2, (size_t)Np * sizeof(double), "hipMalloc t2", false));
    }
    API_MEM(grow(c, c.d_yn, (size_t)Np * sizeof(double), "hipMalloc yn", false));
    API_MEM(grow(c, c.d_z, (size_t)Np * sizeof(double), "hipMalloc z", false));
    API_MEM(grow(c, c.d_alpha, (size_t)Np * sizeof(double), "hipMalloc alpha", false));
    if (c.dtype != TGP_F64) {
        API_MEM(grow(c, c.d_Xs32, (size_t)Np * Dp * sizeof(float), "hipMalloc Xs32", false));
        API_MEM(grow(c, c.d_Linv32, nn * sizeof(float), "hipMalloc Linv32", false));
    }
    if (c.dtype == TGP_F32X3 || c.dtype == TGP_F32H2) {
        API_MEM(grow(c, c.d_Linv16, (c.dtype == TGP_F32X3 ? 3 : 2) * nn * sizeof(unsigned short), "hipMalloc Linv16", false));
        API_MEM(grow(c, c.d_x2scal, 2 * sizeof(unsigned), "hipMalloc x2scal", false));
    }
    c.cap_Np = Np;
    c.cap_D = D;
    c.cap_full = full;
    return TGP_OK;
}

// ---- the fit entries: one argument list, one argument check, one completion (CallClock), one commit ----
struct FitArgs {
    const double *X; int64_t N, D; const double *y;
    int kernel; double constant; const double *ls; int64_t n_ls; double noise, jitter;
    int normalize_y;
};
struct FitOut { double *lml = nullptr, *y_mean = nullptr, *y_std = nullptr; };
// ... and what a fit's kernels hand back: sum(log(diag L)), yn . alpha, first failing pivot + 1 (0: none)
struct FitResult { double sumlog = 0.0, y_alpha = 0.0; int flag = 0; };

static int host_fit(tgp_handle h, const FitArgs &a, const FitOut &out) {
    return h->host->fit(a.X, a.N, a.D, a.y, a.kernel, a.constant, a.ls, a.n_ls, a.noise, a.jitter, a.normalize_y, out.lml, out.y_mean, out.y_std);
}
static int check_fit_args(Context &c, const FitArgs &a) {
    if (!a.X || !a.y || !a.ls) return fail(c, TGP_BAD_ARG, "tgp_fit: X, y and ls must not be NULL");
    if (a.N < 1 || a.D < 1) return fail(c, TGP_BAD_ARG, "tgp_fit: need N >= 1 and D >= 1");
    if (a.N > 65536 || a.D > 4096) return fail(c, TGP_BAD_ARG, "tgp_fit: N <= 65536 and D <= 4096 supported");
    if (a.n_ls != 1 && a.n_ls != a.D) return fail(c, TGP_BAD_ARG, "tgp_fit: n_ls must be 1 or D");
    if (a.kernel < TGP_RBF || a.kernel > TGP_MATERN52) return fail(c, TGP_BAD_ARG, "tgp_fit: unknown kernel");
    if (!(a.constant > 0.0) || !(a.noise >= 0.0) || !(a.jitter >= 0.0)) return fail(c, TGP_BAD_ARG, "tgp_fit: constant > 0, noise >= 0, jitter >= 0 required");
    for (int64_t d = 0; d < a.n_ls; ++d)
        if (!(a.ls[d] > 0.0)) return fail(c, TGP_BAD_ARG, "tgp_fit: length scales must be > 0");
    return TGP_OK;
}

// TGP_NOT_PD with the pivot's number (who: "" or "model t of the batch: ")
static int not_pd(Context &c, int pivot, int64_t N, const std::string &who = std::string()) {
    char buf[160];
    snprintf(buf, sizeof buf, "kernel matrix is not positive definite (pivot %d of %lld <= 0)", pivot, (long long)N);
    return fail(c, TGP_NOT_PD, who + buf);
}
// _gpr.py:609-611: -0.5 y.alpha - sum(log(diag L)) - n/2 log(2 pi)
static double lml_from(double sumlog, double y_alpha, int64_t N) {
    return -0.5 * y_alpha - sumlog - (double)N / 2.0 * log(2.0 * M_PI);
}

// the one-workgroup kernels' packed input: Nin = N rounded up to NB rows of X / length_scale (stride Dp), Nin targets, D length scales
static void pack_small_inputs(double *in, const double *X, int64_t N, int64_t D, int64_t Dp, const double *ls, const double *yn) {
    const int64_t Nin = ((N + NB - 1) / NB) * NB;
    memset(in, 0, (size_t)(Nin * Dp + Nin) * sizeof(double));
    for (int64_t i = 0; i < N; ++i)
        for (int64_t d = 0; d < D; ++d) in[(size_t)i * Dp + d] = X[(size_t)i * D + d] / ls[d];   // X / length_scale
    memcpy(in + Nin * Dp, yn, (size_t)N * sizeof(double));
    memcpy(in + Nin * Dp + Nin, ls, (size_t)D * sizeof(double));
}

// a fit's clock: polled (where the path can ring and TGP_POLL_US allows) it reports the kernels' own ticks
static CallClock fit_clock(Context &c, bool may_poll) {
    CallClock k;
    k.device_ticks = true;
    if (may_poll) k.bell = bell_next(c);
    return k;
}

// the host's copies of the inputs (tgp_fit_append's prefix test, tgp_export_state); nobody reads them while c.fitted is false
static void keep_training_set(Context &c, const FitArgs &a) {
    c.h_X.assign(a.X, a.X + (size_t)a.N * a.D);
    c.h_y.assign(a.y, a.y + (size_t)a.N);
}

// the handle ready for this fit: third stream joined, buffers, theta and geometry recorded, targets normalised into yn (Np, zero beyond N)
static int fit_begin(Context &c, const FitArgs &a, std::vector<double> &yn) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    c.pre.front = false;   // whatever an earlier fit started early belongs to a factor this one replaces
    const int64_t Np = ((a.N + NPAD - 1) / NPAD) * NPAD;
    const int64_t Dp = ((a.D + 3) / 4) * 4;
    API_MEM(ensure_fit_buffers(c, Np, a.D, true));
    if (a.D != c.D) { c.d_cand = nullptr; c.M = 0; c.d_winner = nullptr; }   // resident candidates / winner record belong to the old D
    c.N = a.N; c.D = a.D; c.Np = Np; c.Dp = Dp;
    c.imported = false; c.import_rows = 0;
    c.kernel = a.kernel; c.constant = a.constant; c.noise = a.noise; c.jitter = a.jitter;
    c.ls.assign((size_t)a.D, 0.0);
    for (int64_t d = 0; d < a.D; ++d) c.ls[d] = a.ls[a.n_ls == 1 ? 0 : d];
    yn.assign((size_t)Np, 0.0);
    normalise_targets(a.y, a.N, a.normalize_y, yn, c.y_mean, c.y_std);
    return TGP_OK;
}

// ---- small problems (N <= 128): one workgroup, one launch, no memcpy (small_kernels.hip) ----
// grad_mode: 1 / 2 = the LML gradient (iso / ARD) too
static int fit_small(Context &c, const FitArgs &a, const std::vector<double> &yn, int grad_mode, FitResult &r) {
    const int64_t N = a.N, Np = c.Np, Nin = ((N + NB - 1) / NB) * NB;
    API_MEM(ensure_pinned(c, (size_t)(Nin * c.Dp + Nin + a.D) * sizeof(double), (size_t)(8 + 3 * SMALL_GRAD_OUT_STRIDE) * sizeof(double)));
    pack_small_inputs(c.h_pin_in, a.X, N, a.D, c.Dp, c.ls.data(), yn.data());
    // Round 6: ONE launch (the gradient's workgroups run the fit themselves) and a polled completion -- no event
    // record, no stream synchronisation; TGP_SMALL_FUSED=0 / TGP_POLL_US=0 keep round 5's calls (the A/B switches).
    const bool fused = grad_mode && tuning().small_fused != 0;
    if (fused) API_MEM(grow(c, c.d_sfg, small_fit_grad_ws_bytes(), "hipMalloc small fit + gradient workspace"));
    CallClock clk = fit_clock(c, !grad_mode || fused);
    API_MEM(call_begin(c, clk));
    hipError_t le = fused ? launch_small_fit_grad(c, grad_mode == 2, c.h_pin_out.dev() + 8, clk.bell) : launch_small_fit(c, clk.bell);
    c.linv_extent = std::max<int64_t>(c.linv_ld == Np ? c.linv_extent : Np, Nin);   // until the kernel is known to have finished
    c.linv_ld = Np;
    if (le != hipSuccess) return hip_fail(c, le, "launch_small_fit");
    if (grad_mode && !fused) {   // (timed together with the fit: two more event records would cost a third of the call)
        le = launch_small_grad(c, grad_mode == 2, c.h_pin_out.dev() + 8);
        if (le != hipSuccess) return hip_fail(c, le, "launch_small_grad");
    }
    API_MEM(call_finish(c, clk, c.last_fit_ms, "fit sync"));
    r = FitResult{c.h_pin_out[0], c.h_pin_out[1], (int)c.h_pin_out[2]};
    if (r.flag == 0) {
        c.linv_extent = Nin;
        keep_training_set(c, a);
    }
    return TGP_OK;
}

// ---- the blocked fit (fit_kernels.hip) ----
// X / length_scale (kernels.py:1556 / 1711), padded rows zero.  Up to 64 MiB of inputs are
// staged in device-mapped host memory and fetched by the fit's first kernel; the scalars come
// back the same way: no memcpy, no memset in the call.  Beyond: xs_heap, for the H2D copies
static int stage_blocked_inputs(Context &c, const FitArgs &a, const std::vector<double> &yn, bool &staged, std::vector<double> &xs_heap) {
    const double *X = a.X;
    const int64_t N = a.N, D = a.D, Np = c.Np, Dp = c.Dp;
    const size_t n_in = (size_t)Np * Dp + (size_t)Np + (size_t)D;
    staged = n_in * sizeof(double) <= ((size_t)64 << 20);
    if (staged) {
        API_MEM(ensure_pinned(c, n_in * sizeof(double), (size_t)(8 + 3 + Dp + 2) * sizeof(double)));   // (+ 2: tgp_fit_loo_grad's [L_LOO, bad count])
        double *xs = c.h_pin_in;
        if (D == Dp) memset(xs + (size_t)N * Dp, 0, (size_t)(Np - N) * Dp * sizeof(double));   // (the rows are about to be overwritten whole)
        else memset(xs, 0, (size_t)Np * Dp * sizeof(double));
        memcpy(xs + (size_t)Np * Dp, yn.data(), (size_t)Np * sizeof(double));
        memcpy(xs + (size_t)Np * Dp + Np, c.ls.data(), (size_t)D * sizeof(double));
        // raw rows: the fit's first kernel divides by the length scales (same IEEE division, off the host's critical path)
        if (D == Dp) memcpy(xs, X, (size_t)N * D * sizeof(double));
        else
            for (int64_t i = 0; i < N; ++i) memcpy(xs + (size_t)i * Dp, X + (size_t)i * D, (size_t)D * sizeof(double));
    } else {
        xs_heap.assign((size_t)Np * Dp, 0.0);
        for (int64_t i = 0; i < N; ++i)
            for (int64_t d = 0; d < D; ++d) xs_heap[(size_t)i * Dp + d] = X[(size_t)i * D + d] / c.ls[d];
    }
    return TGP_OK;
}

// tgp_set_overlap: the front of the resident batch's sweep goes out with this fit (the general sweep's f64 / f32
// kernels on the shared streams only; the geometry it is issued for is recorded and checked again by tgp_sweep)
static int decide_overlap_front(Context &c, int grad_mode) {
    c.pre.issue = 0; c.pre.front = false;
    // (never for tgp_fit_grad: an evaluation of the hyper-parameter objective is followed by another evaluation,
    // not by a sweep)
    const int mode = grad_mode ? 0 : std::min(c.pre.mode, tuning().overlap);
    if (mode > 0 && c.d_cand && c.M > 0 && !c.stream_own && (c.dtype == TGP_F64 || c.dtype == TGP_F32) &&
        sweep_path(c, c.M) == SweepPath::General) {
        API_MEM(ensure_workspace(c));
        c.pre.issue = mode;
        c.pre.gen = c.fit_gen + 1;
        c.pre.cand = c.d_cand; c.pre.M = c.M; c.pre.Mpad = c.ws_Mpad; c.pre.launch_rows = c.launch_rows; c.pre.chunk = c.chunk;
    }
    return TGP_OK;
}

// grad_mode: 1 / 2 = the LML gradient (iso / ARD) is launched behind the fit, before the one synchronisation;
// + GRAD_LOO: the leave-one-out score and ITS gradient instead (tgp_fit_loo_grad)
constexpr int GRAD_LOO = 4;
static int fit_blocked(Context &c, const FitArgs &a, const std::vector<double> &yn, int grad_mode, FitResult &r) {
    const int64_t N = a.N, D = a.D, Np = c.Np, Dp = c.Dp;
    bool staged;
    std::vector<double> xs_heap;
    API_MEM(stage_blocked_inputs(c, a, yn, staged, xs_heap));
    // (round 6) a fit whose inputs and scalars travel through the mapped staging buffers is a POLLED call up to Np = 4096:
    // no event record, no stream synchronisation -- a one-wave kernel behind the chain rings the doorbell (launch_ring) and
    // the chain's first kernel leaves the start tick.  Not while the per-launch profiling of tgp_profile_enable is on
    // (bench.py's headline runs: they keep round 5's events), nor with TGP_POLL_US=0.
    CallClock clk = fit_clock(c, staged && !c.profiling && Np <= 4096);
    const Bell &bell = clk.bell;
    API_MEM(call_begin(c, clk));
    if (!staged) {
        API_HIP(hipMemcpyAsync(c.d_Xs, xs_heap.data(), (size_t)Np * Dp * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xs");
        API_HIP(hipMemcpyAsync(c.d_ls, c.ls.data(), (size_t)D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D ls");
        API_HIP(hipMemcpyAsync(c.d_yn, yn.data(), (size_t)Np * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D yn");
    }
    if (grad_mode & GRAD_LOO) API_MEM(ensure_loo_workspace(c, true));
    else if (grad_mode) API_MEM(ensure_grad_workspace(c));
    // Linv is zero above the diagonal whenever its leading dimension is known (nothing ever writes there) and
    // zero from row linv_extent on; this fit writes everything on and below the diagonal of its Nr rows and
    // skips the panels of pure padding: the zero fill is only needed when an older fit reached further down
    const int64_t Nr = ((N + NB - 1) / NB) * NB;
    const bool always_zero = tuning().linv_zero != 0;   // A/B
    const bool linv_clean = !always_zero && c.linv_ld == Np && c.linv_extent <= Nr;
    API_MEM(decide_overlap_front(c, grad_mode));
    struct PrivateFit {                // (ended on every way out of this function, i.e. after the fit's synchronisation)
        Context &c; bool counted;
        ~PrivateFit() { if (counted) { private_fit_end(c.device, c.bg_lease != nullptr); c.bg_lease = nullptr; } }
    } private_fit{c, c.stream_own != nullptr};
    if (private_fit.counted) c.bg_lease = private_fit_begin(c.device, tuning().bg_lease != 0);
    hipError_t le = launch_fit(c, staged ? c.h_pin_in.dev() : nullptr, staged ? c.h_pin_out.dev() : nullptr, !linv_clean,
                               bell.word ? bell.word + 1 : nullptr);
    const bool pre_issued = c.pre.issue != 0;
    c.pre.issue = 0;
    c.linv_extent = Nr; c.linv_ld = Np;
    if (le != hipSuccess) {
        // a launch that failed half way may have left work on the third stream without having recorded its event
        // (c.pre.pending is set at launch_fit's end): wait for it here, so that no later call frees or rewrites what
        // it still reads
        if (pre_issued && !c.pre.pending && c.stream_pre) (void)hipStreamSynchronize(c.stream_pre);
        return hip_fail(c, le, "launch_fit");
    }

    int flag = 0;
    double scal[2] = {0.0, 0.0};
    if (!staged) {
        API_HIP(hipMemcpyAsync(&flag, c.d_flag, sizeof(int), hipMemcpyDeviceToHost, c.stream), "D2H flag");
        API_HIP(hipMemcpyAsync(scal, c.d_scal, 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H scal");
    }
    API_MEM(call_stop(c, clk));   // (an event-timed call's ev1: behind the scalars' copies, in front of the gradient)
    if (grad_mode) {   // behind the fit, in front of the call's one synchronisation
        c.grad_staged = staged;
        c.grad_timed = !bell.word;
        double *gout = staged ? c.h_pin_out.dev() + 8 : c.d_gout;
        if (grad_mode & GRAD_LOO) le = launch_loo_grad(c, (grad_mode & 3) == 2, gout, staged ? gout + 3 + Dp : loo_scal_dev(c), c.grad_timed);
        else le = launch_lml_grad(c, grad_mode == 2, gout, c.grad_timed);
        if (le != hipSuccess) return hip_fail(c, le, (grad_mode & GRAD_LOO) ? "launch_loo_grad" : "launch_lml_grad");
    }
    if (bell.word) {
        le = launch_ring(c, bell);
        if (le != hipSuccess) return hip_fail(c, le, "launch_ring");
    }
    keep_training_set(c, a);   // while the GPU works
    API_MEM(call_finish(c, clk, c.last_fit_ms, "fit sync"));   // (a polled call's time is the whole call: the LML gradient of tgp_fit_grad included)
    r = staged ? FitResult{c.h_pin_out[0], c.h_pin_out[1], (int)c.h_pin_out[2]} : FitResult{scal[0], scal[1], flag};
    return TGP_OK;
}

// The one place a fit or an append becomes the handle's model: TGP_NOT_PD for a failed pivot, else the LML, the optional
// outputs, the fitted flag and the next fit generation.  (ONE step of fit_gen, where the small path took two: every reader
// -- linv16_gen, ts_gen, mes_gen, pre.gen, an exported factor's fit_gen against fit_gen_src -- asks only whether a stored
// generation EQUALS the current one, and pre.gen, formed ahead as fit_gen + 1, is set by the blocked path alone.)
static int fit_commit(Context &c, const FitArgs &a, double sumlog, double y_alpha, int flag, const FitOut &out) {
    if (flag != 0) return not_pd(c, flag - 1, a.N);
    c.sumlog = sumlog;
    c.lml = lml_from(sumlog, y_alpha, a.N);
    c.normalize_y = a.normalize_y ? 1 : 0;
    if (out.lml) *out.lml = c.lml;
    if (out.y_mean) *out.y_mean = c.y_mean;
    if (out.y_std) *out.y_std = c.y_std;
    c.fitted = true; ++c.fit_gen;
    return TGP_OK;
}

static int fit_impl(tgp_handle h, const FitArgs &a, const FitOut &out, bool allow_small, int grad_mode = 0) {
    if (!h) return TGP_BAD_ARG;
    Context &c = h->c;
    c.fitted = false;   // (before the checks: a rejected call leaves the handle un-fitted)
    API_MEM(check_fit_args(c, a));
    std::vector<double> yn;
    API_MEM(fit_begin(c, a, yn));
    c.small = allow_small && a.N <= 2 * NB && small_path_enabled();
    FitResult r;
    API_MEM(c.small ? fit_small(c, a, yn, grad_mode, r) : fit_blocked(c, a, yn, grad_mode, r));
    return fit_commit(c, a, r.sumlog, r.y_alpha, r.flag, out);
}

// tgp_fit for the entries that end in one (tgp_fit_append, tgp_import_state, tgp_hyper_sample): either backend
static int fit_entry(tgp_handle h, const FitArgs &a, const FitOut &out) try {
    if (h && h->host) return host_fit(h, a, out);
    return fit_impl(h, a, out, true);
} TGP_CATCH_AS("tgp_fit")

int tgp_fit(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
            double constant, const double *ls, int64_t n_ls, double noise, double jitter,
            int normalize_y, double *lml, double *y_mean, double *y_std) {
    return fit_entry(h, FitArgs{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y}, FitOut{lml, y_mean, y_std});
}

// the append's body: the resident fit is this one less its last row (tgp_fit_append has checked)
static int fit_append(Context &c, const FitArgs &a, const FitOut &out) {
    const double *X = a.X;
    const int64_t N = a.N, D = a.D;
    c.fitted = false;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t n_old = c.N, Np = c.Np, Dp = c.Dp;
    double mean = 0.0, sd = 1.0;
    std::vector<double> yn((size_t)Np, 0.0);
    normalise_targets(a.y, N, a.normalize_y, yn, mean, sd);
    std::vector<double> xrow((size_t)Dp, 0.0);
    for (int64_t d = 0; d < D; ++d) xrow[d] = X[(size_t)n_old * D + d] / c.ls[d];

    CallClock clk;
    API_MEM(call_begin(c, clk));
    API_HIP(hipMemcpyAsync(c.d_Xs + n_old * Dp, xrow.data(), (size_t)Dp * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D x row");
    API_HIP(hipMemcpyAsync(c.d_yn, yn.data(), (size_t)Np * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D yn");
    c.linv_extent = std::max<int64_t>(c.linv_extent, ((N + NB - 1) / NB) * NB);   // the appended row of Linv
    hipError_t le = launch_fit_append(c, (int)n_old);
    if (le != hipSuccess) return hip_fail(c, le, "launch_fit_append");
    int flag = 0;
    double scal[4] = {0.0, 0.0, 0.0, 0.0};
    API_HIP(hipMemcpyAsync(&flag, c.d_flag, sizeof(int), hipMemcpyDeviceToHost, c.stream), "D2H flag");
    API_HIP(hipMemcpyAsync(scal, c.d_scal, 4 * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H scal");
    API_MEM(call_finish(c, clk, c.last_fit_ms, "append sync"));
    if (flag == 0) {
        c.N = N;
        if (N > 2 * NB) c.small = false;      // grown out of the small-problem kernels' range
        c.y_mean = mean; c.y_std = sd;
        c.h_X.insert(c.h_X.end(), X + (size_t)n_old * D, X + (size_t)N * D);
        c.h_y.assign(a.y, a.y + (size_t)N);
    }
    return fit_commit(c, a, c.sumlog + scal[3], scal[1], flag, out);   // (scal[3]: log of the new pivot)
}

int tgp_fit_append(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                   double constant, const double *ls, int64_t n_ls, double noise, double jitter,
                   int normalize_y, double *lml, double *y_mean, double *y_std, int *appended) try {
    if (!h) return TGP_BAD_ARG;
    const FitArgs a{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y};
    const FitOut out{lml, y_mean, y_std};
    if (appended) *appended = 0;
    if (h->host) return fit_entry(h, a, out);
    Context &c = h->c;
    bool ok = c.fitted && X && y && ls && D == c.D && N == c.N + 1 && N <= c.Np &&
              kernel == c.kernel && constant == c.constant && noise == c.noise && jitter == c.jitter &&
              (normalize_y ? 1 : 0) == c.normalize_y && (n_ls == 1 || n_ls == D) &&
              (int64_t)c.h_X.size() == c.N * c.D;
    if (ok)
        for (int64_t d = 0; d < D && ok; ++d) ok = (c.ls[d] == ls[n_ls == 1 ? 0 : d]);
    if (ok) ok = memcmp(c.h_X.data(), X, (size_t)c.N * D * sizeof(double)) == 0;
    if (!ok) return fit_entry(h, a, out);
    const int rc = fit_append(c, a, out);
    if (rc == TGP_OK && appended) *appended = 1;
    return rc;
} TGP_CATCH

// 0.5 * trace((alpha alpha^T - K^-1) dK/dtheta) from the gradient kernels' sums [S_c, S_iso, S_diag, gd[0..D)]: _gpr.py:643-647
static void lml_grad_from_sums(const FitArgs &a, const double *sums, double *grad) {
    grad[0] = 0.5 * a.constant * sums[0];
    if (a.n_ls > 1) {
        for (int64_t d = 0; d < a.D; ++d) grad[1 + d] = a.constant * sums[3 + (size_t)d];
    } else {
        grad[1] = 0.5 * a.constant * sums[1];
    }
    grad[1 + a.n_ls] = 0.5 * a.noise * sums[2];
}

static int fit_grad_entry(tgp_handle h, const FitArgs &a, const FitOut &out, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_grad");
    Context &c = h->c;
    if (!grad) return fail(c, TGP_BAD_ARG, "tgp_fit_grad: grad is NULL");
    const bool ard = a.n_ls > 1;
    // small problems: fit and gradient as two one-workgroup launches, one synchronisation, no memcpy
    const bool small = a.N <= 2 * NB && ((a.D + 3) / 4) * 4 <= 64 && small_path_enabled();
    // (otherwise the gradient needs U = Linv^T and the N^2 workspaces of the blocked path; there too it is
    // launched behind the fit, in front of the call's one synchronisation)
    const int rc = fit_impl(h, a, out, small, ard ? 2 : 1);
    if (rc != TGP_OK) return rc;
    const int nout = ard ? 3 + (int)c.Dp : 3;
    if (small && c.small) {
        double sums[3 + 64];
        const double *sh = c.h_pin_out + 8;   // the shares of the block pairs, added in a fixed order
        const int nsh = a.N > NB ? 3 : 1;
        for (int i = 0; i < nout; ++i) {
            double s = sh[i];
            for (int g = 1; g < nsh; ++g) s += sh[g * SMALL_GRAD_OUT_STRIDE + i];
            sums[i] = s;
        }
        c.last_grad_ms[0] = c.last_grad_ms[1] = c.last_grad_ms[2] = 0.0;   // (inside last_fit_ms)
        lml_grad_from_sums(a, sums, grad);
        return TGP_OK;
    }
    std::vector<double> sums((size_t)(3 + c.Dp), 0.0);
    if (c.grad_staged) {
        memcpy(sums.data(), c.h_pin_out + 8, (size_t)nout * sizeof(double));
    } else {
        API_HIP(hipSetDevice(c.device), "hipSetDevice");
        API_HIP(hipMemcpy(sums.data(), c.d_gout, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost), "D2H grad");
    }
    for (int i = 0; i < 3; ++i) {
        float gms = 0.f;
        if (c.grad_timed) (void)hipEventElapsedTime(&gms, c.evg[i], c.evg[i + 1]);   // (a polled call records no stage events: its time is all in last_fit_ms)
        c.last_grad_ms[i] = gms;
    }
    lml_grad_from_sums(a, sums.data(), grad);
    return TGP_OK;
} TGP_CATCH_AS("tgp_fit_grad")

int tgp_fit_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                 double constant, const double *ls, int64_t n_ls, double noise, double jitter,
                 int normalize_y, double *lml, double *y_mean, double *y_std, double *grad) {
    return fit_grad_entry(h, FitArgs{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y}, FitOut{lml, y_mean, y_std}, grad);
}

// ---- leave-one-out cross-validation (include/turbogp.h; loo_kernels.hip) ----
static int loo_not_pd(Context &c, const char *fn, double bad) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s: %d diagonal entries of K^-1 are <= 0 or not finite", fn, (int)bad);
    return fail(c, TGP_NOT_PD, buf);
}

int tgp_loo(tgp_handle h, double *resid, double *sigma, double *lpd, double *loo) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->loo(resid, sigma, lpd, loo);
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_loo: no fitted model");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    API_MEM(ensure_loo_workspace(c, false));
    double *sd = loo_scal_dev(c);
    API_HIP(hipEventRecord(c.ev0, c.stream), "hipEventRecord");
    const hipError_t le = launch_loo_points(c, sd);
    if (le != hipSuccess) return hip_fail(c, le, "launch_loo_points");
    API_HIP(hipEventRecord(c.ev1, c.stream), "hipEventRecord");
    double scal[2] = {0.0, 0.0};
    const size_t nb = (size_t)c.N * sizeof(double);
    API_HIP(hipMemcpyAsync(scal, sd, sizeof scal, hipMemcpyDeviceToHost, c.stream), "D2H LOO scalars");
    if (resid) API_HIP(hipMemcpyAsync(resid, c.d_loov + c.Np, nb, hipMemcpyDeviceToHost, c.stream), "D2H resid");
    if (sigma) API_HIP(hipMemcpyAsync(sigma, c.d_loov + 2 * c.Np, nb, hipMemcpyDeviceToHost, c.stream), "D2H sigma");
    if (lpd) API_HIP(hipMemcpyAsync(lpd, c.d_loov + 3 * c.Np, nb, hipMemcpyDeviceToHost, c.stream), "D2H lpd");
    API_HIP(hipStreamSynchronize(c.stream), "loo sync");
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c.ev0, c.ev1);
    c.last_loo_ms = ms;
    if (scal[1] != 0.0) return loo_not_pd(c, "tgp_loo", scal[1]);
    if (loo) *loo = scal[0];
    return TGP_OK;
} TGP_CATCH

int tgp_fit_loo_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                     double constant, const double *ls, int64_t n_ls, double noise, double jitter,
                     int normalize_y, double *lml, double *y_mean, double *y_std, double *loo, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_loo_grad");
    Context &c = h->c;
    if (!grad) return fail(c, TGP_BAD_ARG, "tgp_fit_loo_grad: grad is NULL");
    const FitArgs a{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y};
    const bool ard = n_ls > 1;
    // the blocked route for every N: the gradient needs U = Linv^T and the N^2 workspaces only that route guarantees
    const int rc = fit_impl(h, a, FitOut{lml, y_mean, y_std}, false, (ard ? 2 : 1) | GRAD_LOO);
    if (rc != TGP_OK) return rc;
    const int nout = ard ? 3 + (int)c.Dp : 3;
    std::vector<double> sums((size_t)(3 + c.Dp), 0.0);
    double scal[2] = {0.0, 0.0};
    if (c.grad_staged) {
        memcpy(sums.data(), c.h_pin_out + 8, (size_t)nout * sizeof(double));
        memcpy(scal, c.h_pin_out + 8 + 3 + c.Dp, sizeof scal);
    } else {
        API_HIP(hipSetDevice(c.device), "hipSetDevice");
        API_HIP(hipMemcpy(sums.data(), c.d_gout, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost), "D2H grad");
        API_HIP(hipMemcpy(scal, loo_scal_dev(c), sizeof scal, hipMemcpyDeviceToHost), "D2H LOO scalars");
    }
    for (int i = 0; i < 3; ++i) {
        float gms = 0.f;
        if (c.grad_timed) (void)hipEventElapsedTime(&gms, c.evg[i], c.evg[i + 1]);
        c.last_grad_ms[i] = gms;   // [0]: K^-1, kappa, b, A and B = A A^T
    }
    if (scal[1] != 0.0) {
        c.fitted = false;
        return loo_not_pd(c, "tgp_fit_loo_grad", scal[1]);
    }
    if (loo) *loo = scal[0];
    lml_grad_from_sums(a, sums.data(), grad);
    if (noise == 0.0) grad[1 + n_ls] = 0.0;   // (exactly +0.0, whatever the sign of the trace)
    return TGP_OK;
} TGP_CATCH

// State blob: what defines the fitted model, not the factor (the factor is N^2 and is rebuilt in
// milliseconds; X, y and theta are N*(D+1) + D + 3 doubles).  Layout, all little-endian 8-byte
// words: magic "TGPSTAT1", N, D, kernel, normalize_y (int64) | constant, noise, jitter (f64) |
// ls[D] | X[N*D] | y[N].
static const char STATE_MAGIC[8] = {'T', 'G', 'P', 'S', 'T', 'A', 'T', '1'};

int tgp_export_state(tgp_handle h, void *buf, int64_t cap, int64_t *size) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->export_state(buf, cap, size);
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_export_state: no fitted model");
    if (c.imported) return fail(c, TGP_BAD_ARG, "tgp_export_state: this handle holds a factor it received (tgp_import_factor_dev), not the training set it was computed from");
    const int64_t words = 8 + c.D + c.N * c.D + c.N;
    const int64_t need = words * 8;
    if (size) *size = need;
    if (!buf) return size ? TGP_OK : fail(c, TGP_BAD_ARG, "tgp_export_state: buf and size both NULL");
    if (cap < need) return fail(c, TGP_BAD_ARG, "tgp_export_state: buffer too small");
    char *p = static_cast<char *>(buf);
    memcpy(p, STATE_MAGIC, 8); p += 8;
    const int64_t ints[4] = {c.N, c.D, (int64_t)c.kernel, (int64_t)c.normalize_y};
    memcpy(p, ints, sizeof ints); p += sizeof ints;
    const double reals[3] = {c.constant, c.noise, c.jitter};
    memcpy(p, reals, sizeof reals); p += sizeof reals;
    memcpy(p, c.ls.data(), (size_t)c.D * 8); p += c.D * 8;
    memcpy(p, c.h_X.data(), (size_t)c.N * c.D * 8); p += c.N * c.D * 8;
    memcpy(p, c.h_y.data(), (size_t)c.N * 8);
    return TGP_OK;
} TGP_CATCH

int tgp_import_state(tgp_handle h, const void *buf, int64_t size, double *lml) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->import_state(buf, size, lml);
    Context &c = h->c;
    if (!buf || size < 64) return fail(c, TGP_BAD_ARG, "tgp_import_state: blob too short");   // (tgp_fit below joins the third stream)
    const char *p = static_cast<const char *>(buf);
    if (memcmp(p, STATE_MAGIC, 8) != 0) return fail(c, TGP_BAD_ARG, "tgp_import_state: bad magic");
    int64_t ints[4];
    double reals[3];
    memcpy(ints, p + 8, sizeof ints);
    memcpy(reals, p + 40, sizeof reals);
    const int64_t N = ints[0], D = ints[1];
    if (N < 1 || D < 1 || N > 65536 || D > 4096) return fail(c, TGP_BAD_ARG, "tgp_import_state: bad shape");
    if (size != (8 + D + N * D + N) * 8) return fail(c, TGP_BAD_ARG, "tgp_import_state: size does not match the header");
    // the blob carries no alignment promise: copy out before use
    std::vector<double> ls((size_t)D), X((size_t)N * D), y((size_t)N);
    p += 64;
    memcpy(ls.data(), p, (size_t)D * 8); p += D * 8;
    memcpy(X.data(), p, (size_t)N * D * 8); p += N * D * 8;
    memcpy(y.data(), p, (size_t)N * 8);
    return fit_entry(h, FitArgs{X.data(), N, D, y.data(), (int)ints[2], reals[0], ls.data(), D, reals[1], reals[2], (int)ints[3]},
                     FitOut{lml, nullptr, nullptr});
} TGP_CATCH

// ---- handing a FACTOR over instead of recomputing it (round 6; SURVEY 8e's alternative: "fit on GPU0 + broadcast of L, alpha") ----
int tgp_export_factor_dev(tgp_handle h, tgp_factor *out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_export_factor_dev");
    Context &c = h->c;
    if (!out) return fail(c, TGP_BAD_ARG, "tgp_export_factor_dev: out is NULL");
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_export_factor_dev: no fitted model");
    memset(out, 0, sizeof *out);
    out->N = c.N; out->D = c.D; out->Np = c.Np; out->Dp = c.Dp; out->fit_gen = c.fit_gen;
    out->kernel = c.kernel; out->normalize_y = c.normalize_y; out->small_path = c.small ? 1 : 0;
    out->constant = c.constant; out->noise = c.noise; out->jitter = c.jitter;
    out->y_mean = c.y_mean; out->y_std = c.y_std; out->lml = c.lml; out->sumlog = c.sumlog;
    out->Xs = c.d_Xs; out->ls = c.d_ls; out->alpha = c.d_alpha; out->Linv = c.d_Linv;
    return TGP_OK;
} TGP_CATCH

int tgp_import_factor_dev(tgp_handle h, const tgp_factor *f, int64_t row0, int64_t rows) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_import_factor_dev");
    Context &c = h->c;
    if (!f || !f->Xs || !f->ls || !f->alpha || !f->Linv) return fail(c, TGP_BAD_ARG, "tgp_import_factor_dev: need a factor with Xs, ls, alpha and Linv");
    const int64_t N = f->N, D = f->D, Np = f->Np, Dp = f->Dp;
    if (N < 1 || N > 65536 || D < 1 || D > 4096 || Np != ((N + NPAD - 1) / NPAD) * NPAD || Dp != ((D + 3) / 4) * 4)
        return fail(c, TGP_BAD_ARG, "tgp_import_factor_dev: inconsistent shape (Np = N rounded up to 256, Dp = D rounded up to 4)");
    if (f->kernel < TGP_RBF || f->kernel > TGP_MATERN52) return fail(c, TGP_BAD_ARG, "tgp_import_factor_dev: unknown kernel");
    if (row0 < 0 || rows < 1 || row0 + rows > Np) return fail(c, TGP_BAD_ARG, "tgp_import_factor_dev: need 0 <= row0, 1 <= rows, row0 + rows <= Np");
    // the rows arrive top down, as a Cholesky finishes them: block 0 starts a new factor, every later block continues it
    if (row0 != 0 && !(c.import_rows == row0 && !c.fitted && c.imported && c.N == N && c.D == D && c.fit_gen_src == f->fit_gen))
        return fail(c, TGP_BAD_ARG, "tgp_import_factor_dev: rows must arrive in order, starting with row0 = 0, all from one fit");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    c.pre.front = false;
    if (row0 == 0) {
        c.fitted = false;
        const int arc = ensure_fit_buffers(c, Np, D, false);
        if (arc != TGP_OK) return arc;
        if (D != c.D) { c.d_cand = nullptr; c.M = 0; c.d_winner = nullptr; }
        c.N = N; c.D = D; c.Np = Np; c.Dp = Dp;
        c.kernel = f->kernel; c.constant = f->constant; c.noise = f->noise; c.jitter = f->jitter;
        c.normalize_y = f->normalize_y; c.y_mean = f->y_mean; c.y_std = f->y_std; c.lml = f->lml; c.sumlog = f->sumlog;
        c.small = f->small_path != 0 && N <= 2 * NB && small_path_enabled();
        c.imported = true; c.import_rows = 0; c.fit_gen_src = f->fit_gen;
        c.h_X.clear(); c.h_y.clear();
        c.ls.assign((size_t)D, 0.0);      // (the host's copy of the length scales: fetched below)
        API_HIP(hipMemcpyAsync(c.d_Xs, f->Xs, (size_t)Np * Dp * sizeof(double), hipMemcpyDefault, c.stream), "D2D Xs");
        API_HIP(hipMemcpyAsync(c.d_ls, f->ls, (size_t)D * sizeof(double), hipMemcpyDefault, c.stream), "D2D ls");
        API_HIP(hipMemcpyAsync(c.d_alpha, f->alpha, (size_t)Np * sizeof(double), hipMemcpyDefault, c.stream), "D2D alpha");
        API_HIP(hipMemcpyAsync(c.ls.data(), f->ls, (size_t)D * sizeof(double), hipMemcpyDefault, c.stream), "D2H ls");
        if (c.dtype != TGP_F64) {
            hipError_t le = launch_f64_to_f32(c, c.d_Xs, c.d_Xs32, (long)(Np * Dp));
            if (le != hipSuccess) return hip_fail(c, le, "f64 -> f32 Xs");
        }
        c.linv_ld = Np; c.linv_extent = Np;     // (whatever the giver's padding rows hold is copied as it is)
    }
    API_HIP(hipMemcpyAsync(c.d_Linv + row0 * Np, static_cast<const double *>(f->Linv) + row0 * Np, (size_t)(rows * Np) * sizeof(double),
                           hipMemcpyDefault, c.stream), "D2D Linv rows");
    if (c.dtype != TGP_F64) {
        hipError_t le = launch_f64_to_f32(c, c.d_Linv + row0 * Np, c.d_Linv32 + row0 * Np, (long)(rows * Np));
        if (le != hipSuccess) return hip_fail(c, le, "f64 -> f32 Linv rows");
    }
    c.import_rows = row0 + rows;
    if (c.import_rows == Np) {
        API_HIP(hipStreamSynchronize(c.stream), "import sync");
        c.fitted = true; ++c.fit_gen;
    }
    return TGP_OK;
} TGP_CATCH

int tgp_debug_read(tgp_handle h, int which, double *out) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->debug_read(which, out);
    Context &c = h->c;
    if (!out) return fail(c, TGP_BAD_ARG, "tgp_debug_read: out is NULL");
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_debug_read: no fitted model");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t N = c.N, Np = c.Np;
    if (which == TGP_BUF_ALPHA) {
        API_HIP(hipMemcpy(out, c.d_alpha, (size_t)N * sizeof(double), hipMemcpyDeviceToHost), "D2H alpha");
        return TGP_OK;
    }
    const double *src = which == TGP_BUF_LINV ? c.d_Linv : c.d_K;
    if (!src) return fail(c, TGP_BAD_ARG, "tgp_debug_read: this handle received its factor (tgp_import_factor_dev): it holds Linv and alpha, not L");
    if (which != TGP_BUF_K && which != TGP_BUF_L && which != TGP_BUF_LINV) return fail(c, TGP_BAD_ARG, "tgp_debug_read: unknown buffer");
    if (which == TGP_BUF_K) return fail(c, TGP_BAD_ARG, "tgp_debug_read: K is overwritten by L after the fit; read L");
    API_HIP(hipMemcpy2D(out, (size_t)N * sizeof(double), src, (size_t)Np * sizeof(double), (size_t)N * sizeof(double), (size_t)N, hipMemcpyDeviceToHost), "D2H matrix");
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = i + 1; j < N; ++j) out[i * N + j] = 0.0;
    return TGP_OK;
} TGP_CATCH

static int ensure_outputs(Context &c, bool mu, bool sg, bool aq) {
    if (c.M > c.out_cap) {
        API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
        static_cast<OutMem &>(c) = OutMem{};
        c.out_cap = c.M;
    }
    // every output buffer is sized for out_cap, whichever call creates it
    const size_t bytes = (size_t)std::max<int64_t>(c.out_cap, 1) * sizeof(double);
    if (mu) API_MEM(grow(c, c.d_mu, bytes, "hipMalloc mu", false));
    if (sg) API_MEM(grow(c, c.d_sigma, bytes, "hipMalloc sigma", false));
    if (aq) API_MEM(grow(c, c.d_acq, bytes, "hipMalloc acq", false));
    return TGP_OK;
}

// The owned candidate buffer, grown to `need` doubles (reserve()'s contract), the resident batch forgotten BEFORE the
// buffer it points into is released
static int grow_candidates(Context &c, int64_t need) {
    const size_t bytes = (size_t)need * sizeof(double);
    if (bytes <= c.d_cand_owned.bytes()) return TGP_OK;
    if (c.d_cand == c.d_cand_owned) { c.d_cand = nullptr; c.M = 0; }
    return grow(c, c.d_cand_owned, bytes, "hipMalloc candidates");
}

int tgp_set_candidates(tgp_handle h, const double *Xc, int64_t M) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->set_candidates(Xc, M);
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_set_candidates: fit first (D is taken from the model)");
    if (!Xc || M < 1) return fail(c, TGP_BAD_ARG, "tgp_set_candidates: need Xc and M >= 1");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t need = M * c.D;
    { const int grc = grow_candidates(c, need); if (grc != TGP_OK) return grc; }
    API_HIP(hipMemcpyAsync(c.d_cand_owned, Xc, (size_t)need * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D candidates");
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    c.d_cand = c.d_cand_owned;
    c.M = M;
    return TGP_OK;
} TGP_CATCH

// The reference-faithful HOST draw with only its sequential part on the host: NumPy's MT19937 stream is continued here
// (host_backend.cpp: the recurrence cannot be run in parallel), a column's 2 M words at a time into one of two pinned
// buffers, each copied to the device while the next is generated; the GPU forms the doubles and the (M, D) layout.
// C3's 262 144 x 32: NumPy 45-66 ms on the host, the library's all-host version 20-25 (page faults of a fresh 67 MB
// array included), this ~6.
int tgp_set_candidates_mt19937(tgp_handle h, uint32_t *key624, int32_t *pos, int64_t M_total, int64_t first_row, int64_t M,
                               const double *lo, const double *hi) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_set_candidates_mt19937");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_set_candidates_mt19937: fit first (D is taken from the model)");
    if (!key624 || !pos || !lo || !hi || M < 1 || first_row < 0 || first_row + M > M_total || *pos < 0 || *pos > 624)
        return fail(c, TGP_BAD_ARG, "tgp_set_candidates_mt19937: need key624, 0 <= pos <= 624, lo, hi and 1 <= rows, first_row + rows <= M_total");
    const int64_t D = c.D;
    std::vector<double> rng((size_t)(2 * D));
    for (int64_t d = 0; d < D; ++d) {
        rng[(size_t)d] = lo[d];
        rng[(size_t)(D + d)] = hi[d] - lo[d];          // NumPy's fscale = high - low
        if (!isfinite(rng[(size_t)(D + d)])) return fail(c, TGP_BAD_ARG, "tgp_set_candidates_mt19937: a range is not finite (NumPy raises OverflowError there)");
    }
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    // owned buffer: candidates (M D doubles) | lo, range (2 D) | the stream's words (2 M D of 4 bytes = M D doubles)
    const int64_t need = 2 * M * D + 2 * D;
    { const int grc = grow_candidates(c, need); if (grc != TGP_OK) return grc; }
    const size_t col_bytes = (size_t)(2 * M) * sizeof(uint32_t);
    API_MEM(grow(c, c.h_mt_words, 2 * col_bytes, "hipHostMalloc"));
    for (int b = 0; b < 2; ++b) API_HIP(c.ev_mt[b].create(hipEventDisableTiming), "hipEventCreate");
    double *d_lo = c.d_cand_owned + M * D, *d_range = d_lo + D;
    uint32_t *d_words = reinterpret_cast<uint32_t *>(d_range + D);
    if (c.d_cand == c.d_cand_owned) { c.d_cand = nullptr; c.M = 0; }     // (the resident batch is being overwritten)
    // the caller's RNG state moves only if the whole call succeeds
    uint32_t key[624];
    memcpy(key, key624, sizeof key);
    int32_t p = *pos;
    API_HIP(hipMemcpyAsync(d_lo, rng.data(), (size_t)(2 * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D lo, range");
    bool used[2] = {false, false};
    for (int64_t col = 0; col < D; ++col) {
        const int b = (int)(col & 1);
        uint32_t *buf = c.h_mt_words + (size_t)b * (size_t)(2 * M);
        if (used[b]) API_HIP(hipEventSynchronize(c.ev_mt[b]), "hipEventSynchronize");   // its last copy has left
        // a column consumes 2 M_total words of the stream; this handle's rows are [first_row, first_row + M) of it
        tgp_host::mt19937_skip(key, &p, 2 * first_row);
        tgp_host::mt19937_fill(key, &p, buf, 2 * M);
        tgp_host::mt19937_skip(key, &p, 2 * (M_total - first_row - M));
        API_HIP(hipMemcpyAsync(d_words + (size_t)col * (size_t)(2 * M), buf, col_bytes, hipMemcpyHostToDevice, c.stream), "H2D words");
        API_HIP(hipEventRecord(c.ev_mt[b], c.stream), "hipEventRecord");
        used[b] = true;
    }
    hipError_t le = launch_mt19937_columns(c, d_words, c.d_cand_owned, M, d_lo, d_range);
    if (le != hipSuccess) { (void)hipStreamSynchronize(c.stream); return hip_fail(c, le, "launch_mt19937_columns"); }
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    memcpy(key624, key, sizeof key);
    *pos = p;
    c.d_cand = c.d_cand_owned;
    c.M = M;
    return TGP_OK;
} TGP_CATCH

int tgp_gen_candidates(tgp_handle h, uint64_t seed, uint64_t first_candidate, int64_t M,
                       const double *lo, const double *hi) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_gen_candidates");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_gen_candidates: fit first (D is taken from the model)");
    if (!lo || !hi || M < 1) return fail(c, TGP_BAD_ARG, "tgp_gen_candidates: need lo, hi and M >= 1");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t need = M * c.D + 2 * c.D;      // candidates + the bounds behind them
    { const int grc = grow_candidates(c, need); if (grc != TGP_OK) return grc; }
    double *d_lo = c.d_cand_owned + M * c.D, *d_hi = d_lo + c.D;
    API_HIP(hipMemcpyAsync(d_lo, lo, (size_t)c.D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D lo");
    API_HIP(hipMemcpyAsync(d_hi, hi, (size_t)c.D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D hi");
    hipError_t le = launch_gen_candidates(c, c.d_cand_owned, M, seed, first_candidate, d_lo, d_hi);
    if (le != hipSuccess) return hip_fail(c, le, "launch_gen_candidates");
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    c.d_cand = c.d_cand_owned;
    c.M = M;
    return TGP_OK;
} TGP_CATCH

// A kernel reading or writing through a bad pointer faults the GPU: check a borrowed device
// pointer against what the HIP runtime knows (device memory, this GPU, `bytes` left in its
// allocation, 8-byte aligned) before any kernel sees it.
static int check_borrowed(Context &c, const void *p, size_t bytes, const char *who) {
    const std::string w(who);
    hipPointerAttribute_t at;
    hipError_t pe = hipPointerGetAttributes(&at, p);
    if (pe != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, TGP_BAD_ARG, w + ": not a pointer known to the HIP runtime");
    }
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)
        return fail(c, TGP_BAD_ARG, w + ": pointer is not device memory");
    if (at.type == hipMemoryTypeDevice && at.device != c.device)
        return fail(c, TGP_BAD_ARG, w + ": pointer lives on another GPU than this handle");
    hipDeviceptr_t base = nullptr;
    size_t span = 0;
    if (hipMemGetAddressRange(&base, &span, const_cast<void *>(p)) == hipSuccess) {
        const size_t off = (size_t)((const char *)p - (const char *)base);
        if (bytes > span - off) return fail(c, TGP_BAD_ARG, w + ": allocation is smaller than the bytes this call needs");
    } else {
        (void)hipGetLastError();
    }
    if (((uintptr_t)p & 7u) != 0) return fail(c, TGP_BAD_ARG, w + ": pointer must be 8-byte aligned");
    return TGP_OK;
}

// shared by the two LHS entries: D columns, bounds behind the batch in the candidate buffer
static int gen_lhs_into_owned(Context &c, uint64_t seed, uint64_t first, int64_t M, uint64_t n_total,
                              int64_t D, const double *lo, const double *hi, const char *who) {
    const std::string w(who);
    if (!lo || !hi || M < 1) return fail(c, TGP_BAD_ARG, w + ": need lo, hi and M >= 1");
    if (n_total < 1 || n_total > (1ull << 40) || first + (uint64_t)M > n_total)
        return fail(c, TGP_BAD_ARG, w + ": need first_sample + M <= n_total <= 2^40 (LHS sequence exhausted)");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");   // (after the argument checks, as in every other entry)
    const int64_t need = M * D + 2 * D;
    { const int grc = grow_candidates(c, need); if (grc != TGP_OK) return grc; }
    double *d_lo = c.d_cand_owned + M * D, *d_hi = d_lo + D;
    API_HIP(hipMemcpyAsync(d_lo, lo, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D lo");
    API_HIP(hipMemcpyAsync(d_hi, hi, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D hi");
    hipError_t le = launch_gen_lhs(c, c.d_cand_owned, M, D, seed, first, n_total, d_lo, d_hi);
    if (le != hipSuccess) return hip_fail(c, le, "launch_gen_lhs");
    return TGP_OK;
}

int tgp_gen_candidates_lhs(tgp_handle h, uint64_t seed, uint64_t first_sample, int64_t M,
                           uint64_t n_total, const double *lo, const double *hi) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_gen_candidates_lhs");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_gen_candidates_lhs: fit first (D is taken from the model)");
    int rc = gen_lhs_into_owned(c, seed, first_sample, M, n_total, c.D, lo, hi, "tgp_gen_candidates_lhs");
    if (rc != TGP_OK) return rc;
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    c.d_cand = c.d_cand_owned;
    c.M = M;
    return TGP_OK;
} TGP_CATCH

int tgp_lhs_design(tgp_handle h, uint64_t seed, uint64_t first_sample, int64_t M, uint64_t n_total,
                   int64_t D, const double *lo, const double *hi, double *out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_lhs_design");
    Context &c = h->c;
    if (!out || D < 1 || D > 4096) return fail(c, TGP_BAD_ARG, "tgp_lhs_design: need out and 1 <= D <= 4096");
    int rc = gen_lhs_into_owned(c, seed, first_sample, M, n_total, D, lo, hi, "tgp_lhs_design");
    if (rc != TGP_OK) return rc;
    API_HIP(hipMemcpyAsync(out, c.d_cand_owned, (size_t)(M * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H design");
    API_HIP(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    if (c.d_cand == c.d_cand_owned) { c.d_cand = nullptr; c.M = 0; }   // the owned batch was overwritten
    return TGP_OK;
} TGP_CATCH

int tgp_read_candidates(tgp_handle h, int64_t first, int64_t count, double *out) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->read_candidates(first, count, out);
    Context &c = h->c;
    if (!c.d_cand || !out || first < 0 || count < 1 || first + count > c.M)
        return fail(c, TGP_BAD_ARG, "tgp_read_candidates: bad range or no candidates");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    API_HIP(hipMemcpy(out, c.d_cand + first * c.D, (size_t)(count * c.D) * sizeof(double), hipMemcpyDeviceToHost), "D2H candidates");
    return TGP_OK;
} TGP_CATCH

int tgp_set_candidates_dev(tgp_handle h, const void *Xc_dev, int64_t M) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_set_candidates_dev");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_set_candidates_dev: fit first");
    if (!Xc_dev || M < 1) return fail(c, TGP_BAD_ARG, "tgp_set_candidates_dev: need a device pointer and M >= 1");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int rc = check_borrowed(c, Xc_dev, (size_t)M * (size_t)c.D * sizeof(double), "tgp_set_candidates_dev");
    if (rc != TGP_OK) return rc;
    c.d_cand = reinterpret_cast<const double *>(Xc_dev);
    c.M = M;
    return TGP_OK;
} TGP_CATCH

int tgp_set_winner_out(tgp_handle h, void *rec_dev, int64_t global_offset) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_set_winner_out");
    Context &c = h->c;
    if (!rec_dev) { c.d_winner = nullptr; c.winner_offset = 0; c.winner_recorded = false; return TGP_OK; }
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_set_winner_out: fit first (D is taken from the model)");
    if (global_offset < 0 || global_offset > ((int64_t)1 << 52)) return fail(c, TGP_BAD_ARG, "tgp_set_winner_out: global_offset must be in [0, 2^52]");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    const int rc = check_borrowed(c, rec_dev, (size_t)(c.D + 2) * sizeof(double), "tgp_set_winner_out");
    if (rc != TGP_OK) return rc;
    c.d_winner = reinterpret_cast<double *>(rec_dev);
    c.winner_offset = global_offset;
    c.winner_recorded = false;   // a new buffer holds no record yet: nothing for tgp_winner_wait to wait for
    return TGP_OK;
} TGP_CATCH

int tgp_winner_wait(tgp_handle h, void *stream) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_winner_wait");
    Context &c = h->c;
    if (!c.d_winner) return fail(c, TGP_BAD_ARG, "tgp_winner_wait: no winner record attached (tgp_set_winner_out)");
    if (!c.winner_recorded) return TGP_OK;      // nothing has packed a record into this buffer yet: nothing to wait for
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), c.ev_winner, 0), "hipStreamWaitEvent");
    return TGP_OK;
} TGP_CATCH

int tgp_get_candidate(tgp_handle h, int64_t idx, double *out_row) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->read_candidates(idx, 1, out_row);
    Context &c = h->c;
    if (!c.d_cand || !out_row || idx < 0 || idx >= c.M) return fail(c, TGP_BAD_ARG, "tgp_get_candidate: bad index or no candidates");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(hipMemcpy(out_row, c.d_cand + idx * c.D, (size_t)c.D * sizeof(double), hipMemcpyDeviceToHost), "D2H candidate");
    return TGP_OK;
} TGP_CATCH

// Sweep workspace: grow-only, so a loop that alternates batch sizes (plots, 1-point calls, the
// big sweep) does not re-allocate.  Leading dimensions are per call.
static int ensure_workspace(Context &c) {
    c.pre.front = false;   // whoever asks for the workspace is about to overwrite what a fit's early front left in it (tgp_sweep looks first)
    const size_t elt = c.dtype != TGP_F64 ? 4 : 8;
    const size_t kelt = c.dtype == TGP_F32X3 ? 6 : elt;   // bytes per element of the cross-kernel slab (three bf16 planes; two fp16 planes = 4)
    // chunk: a cross-kernel slab of about 256 MiB per launch, multiple of 1024.  Measured on the
    // four BASELINE configs (TGP_CHUNK sweeps, profiles/README.md): 128 MiB costs 1-5 % (twice
    // the launches, half the tiles per launch to balance), 512 MiB and more lose L2 locality.
    int64_t chunk = (int64_t)((256ull << 20) / ((size_t)c.Np * elt));   // (same candidates per launch for the three-plane slab: 384 MiB)
    chunk = std::max<int64_t>(1024, (chunk / 1024) * 1024);
    chunk = std::min<int64_t>(chunk, 65536);
    if (const long v = tuning_chunk_now(); v >= 1024) chunk = (v / 1024) * 1024;   // tuning knob (multiple of 1024), read at every call
    const int64_t mpad = ((c.M + 255) / 256) * 256;   // a multiple of every candidate-tile width in use
    if (mpad <= chunk) chunk = mpad;   // single group
    int rc;
    if ((rc = grow(c, c.d_Cs, (size_t)mpad * c.Dp * elt, "hipMalloc Cs")) != TGP_OK) return rc;
    // The cross-kernel slab.  f64 / f32: one launch pair (cross-kernel, contraction) covers several GROUPS of
    // `chunk` candidates; inside the contraction the tiles walk the slab group by group (sweep_tile()), so the
    // light tail of one group is filled by the heavy head of the next and the cross-kernel runs in fewer,
    // larger launches.  Measured on one box (C3, ms per step): 1 group per launch 36.4, 2: 35.1, 4: 35.0,
    // 8: 35.1, all 16: 35.4 (the slab then always comes back from HBM, never from the Infinity Cache);
    // C4 and C2 within 0.5 % whatever the grouping.  Default: TGP_SLAB_GB = 1 (four groups of 256 MiB).
    // The split-operand dtypes keep a launch per group (two slots).
    const bool per_group = c.dtype == TGP_F32X3 || c.dtype == TGP_F32H2;
    int64_t launch_rows = chunk;
    if (!per_group) {
        const double slab_gb = tuning().slab_gb;
        const int64_t cap = (int64_t)(slab_gb * 1073741824.0 / (double)((size_t)c.Np * kelt));
        const int64_t groups = std::max<int64_t>(1, std::min<int64_t>((mpad + chunk - 1) / chunk, cap / chunk));
        launch_rows = groups * chunk;
    }
    if ((rc = grow(c, c.d_Ks[0], (size_t)std::min<int64_t>(launch_rows, std::max<int64_t>(mpad, chunk)) * c.Np * kelt, "hipMalloc Ks")) != TGP_OK) return rc;
    if (per_group && (rc = grow(c, c.d_Ks[1], (size_t)chunk * c.Np * kelt, "hipMalloc Ks")) != TGP_OK) return rc;
    c.launch_rows = launch_rows;
    if ((rc = grow(c, c.d_part, (size_t)(c.Np / SW_BM) * mpad * sizeof(double), "hipMalloc part")) != TGP_OK) return rc;
    if ((rc = grow(c, c.d_mupart, (size_t)KS_JS * mpad * sizeof(double), "hipMalloc mupart")) != TGP_OK) return rc;
    c.chunk = chunk;
    c.ws_Mpad = mpad;
    const size_t nblk = (size_t)((c.M + NB - 1) / NB + 1);   // the small-problem sweep reduces 64 candidates per block
    if ((rc = grow(c, c.d_bval, nblk * sizeof(double), "hipMalloc bval")) != TGP_OK) return rc;
    return grow(c, c.d_bidx, nblk * sizeof(long long), "hipMalloc bidx");
}

// the small-problem sweep only needs the per-block arg-max partials
static int ensure_small_workspace(Context &c) {
    const size_t nblk = (size_t)((c.M + 31) / 32 + 1);   // (the one-launch sweep of N <= 512 reduces 32 candidates per workgroup)
    API_MEM(grow(c, c.d_bval, nblk * sizeof(double), "hipMalloc bval"));
    return grow(c, c.d_bidx, nblk * sizeof(long long), "hipMalloc bidx");
}

// One sweep of the resident candidates with the resident model, for every entry of the family: picks the kernel
// family, sees to its workspace, starts the call's clock in front of the first launch, launches, and records the winner
// event behind whatever packed the record.  The entry keeps its argument checks, its own buffers and what it copies back.
// TGP_ACQ_MES needs maxima that belong to the resident fit (tgp_mes_set_maxima / tgp_mes_draw); like a Thompson draw they
// are dropped by every later fit, append and import
static int mes_check(Context &c, int acq, const char *fn) {
    if (acq != TGP_ACQ_MES) return TGP_OK;
    if (c.mes_gen < 0 || c.mes_gen != c.fit_gen || c.mes_S < 1)
        return fail(c, TGP_BAD_ARG, std::string(fn) + ": TGP_ACQ_MES needs maxima for the resident fit (tgp_mes_set_maxima or tgp_mes_draw after the last fit)");
    return TGP_OK;
}

// the checks every entry that takes an acquisition makes, in the order they report.  acq_check: the acquisition is one of
// NONE .. acq_max (with its maxima, if it is MES) and sf a sign; acq_check_args: a fitted model and the entry's own check
// (`own`: its text when it failed, else null) in front of that.  An entry whose text for one of them differs reports that
// one itself (through `own`, or in front of acq_check).
static int acq_check(Context &c, const char *fn, int acq, int acq_max, double sf) {
    if (acq < TGP_ACQ_NONE || acq > acq_max) return fail(c, TGP_BAD_ARG, std::string(fn) + ": unknown acquisition");
    if (int mrc = mes_check(c, acq, fn); mrc != TGP_OK) return mrc;
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, std::string(fn) + ": sf must be +1 or -1");
    return TGP_OK;
}
static int acq_check_args(Context &c, const char *fn, const char *own, int acq, int acq_max, double sf) {
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, std::string(fn) + ": no fitted model");
    if (own) return fail(c, TGP_BAD_ARG, std::string(fn) + ": " + own);
    return acq_check(c, fn, acq, acq_max, sf);
}
// the box of a gradient-stage entry: D lower and upper bounds
static int box_check(Context &c, const char *fn, const double *lo, const double *hi) {
    for (int64_t d = 0; d < c.D; ++d)
        if (!(lo[d] <= hi[d])) return fail(c, TGP_BAD_ARG, std::string(fn) + ": need lo <= hi in every dimension");
    return TGP_OK;
}

// the winner record is packed: what tgp_winner_wait makes another stream (RCCL's) wait for -- a polled call
// returns without a stream synchronisation, so the ordering rests on this event
static int winner_mark(Context &c, const SweepCall &s) {
    if (!s.winner || s.acq == TGP_ACQ_NONE) return TGP_OK;
    API_HIP(c.ev_winner.create(hipEventDisableTiming), "hipEventCreate");
    API_HIP(hipEventRecord(c.ev_winner, c.stream), "hipEventRecord");
    c.winner_recorded = true;
    return TGP_OK;
}

static int run_sweep(Context &c, const SweepCall &call, CallClock &clk) {
    SweepCall s = call;
    if (s.acq == TGP_ACQ_MES) s.mes = MesArgs{c.d_mes, c.mes_S, c.noise * (c.y_std * c.y_std)};
    const SweepPath path = sweep_path(c, c.M);
    int rc = path == SweepPath::General ? ensure_workspace(c) : ensure_small_workspace(c);
    if (rc != TGP_OK) return rc;
    // the front a fit started (tgp_set_overlap) is used when it belongs to the resident fit, batch and workspace geometry
    const bool front = path == SweepPath::General && s.may_use_front && c.pre.gen == c.fit_gen && c.pre.cand == c.d_cand &&
                       c.pre.M == c.M && c.pre.Mpad == c.ws_Mpad && c.pre.launch_rows == c.launch_rows && c.pre.chunk == c.chunk;
    c.pre.front = false;   // one sweep per front: the slab it filled is overwritten from here on
    c.last_sweep_f64 = path != SweepPath::General || c.dtype == TGP_F64;   // (the one-workgroup / one-launch kernels only exist in f64)
    // (kg_grad_sweep_posterior sweeps query points in the resident batch's place and puts back what is set from here on
    // and in ensure_workspace: a field added here goes into its list)
    c.prune_state = -1;
    c.prune_lbset = c.prune_surv = 0;
    c.prune_screen = -1;
    c.prune_arith = 0;
    c.prune_spec = 0;
    if ((rc = call_begin(c, clk)) != TGP_OK) return rc;
    hipError_t le;
    if (path == SweepPath::OneLaunch) {
        le = launch_mid_sweep(c, s);
    } else if (path == SweepPath::OneWorkgroup) {
        le = launch_small_sweep(c, s);
        if (le == hipSuccess) le = launch_argmax_final(c, s);
    } else {
        le = launch_sweep(c, s, front);
    }
    if (le != hipSuccess) return hip_fail(c, le, "launch_sweep");
    return winner_mark(c, s);
}

// ---- the record [best value, best index, clamp count] of tgp_sweep and tgp_sweep_integrated ----
struct SweepRecord { double bv = 0.0; long long bi[2] = {0, 0}; };   // (the D2H copies' target: alive until the call's wait)
// behind the last kernel: nothing when it left the record in mapped host memory (zc), else two D2H copies and the counters'
// memset; ev1 of a clocked call (last_sweep_ms leaves the copies of the (M,) outputs out); those copies
static int sweep_queue_return(Context &c, bool zc, int acq, SweepRecord &r, CallClock *clk, double *mu, double *sigma, double *acq_out) {
    if (!zc) {
        if (acq != TGP_ACQ_NONE) API_HIP(hipMemcpyAsync(&r.bv, c.d_best, sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H best");
        API_HIP(hipMemcpyAsync(r.bi, c.d_besti, 2 * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H besti");
        API_HIP(hipMemsetAsync(c.d_besti, 0, 4 * sizeof(long long), c.stream), "memset counters");   // zero between calls
    }
    if (clk) API_MEM(call_stop(c, *clk));
    const size_t bytes = (size_t)c.M * sizeof(double);
    if (mu) API_HIP(hipMemcpyAsync(mu, c.d_mu, bytes, hipMemcpyDeviceToHost, c.stream), "D2H mu");
    if (sigma) API_HIP(hipMemcpyAsync(sigma, c.d_sigma, bytes, hipMemcpyDeviceToHost, c.stream), "D2H sigma");
    if (acq_out) API_HIP(hipMemcpyAsync(acq_out, c.d_acq, bytes, hipMemcpyDeviceToHost, c.stream), "D2H acq");
    return TGP_OK;
}
// after the call's wait: the record into the caller's optional outputs
static void sweep_read_record(Context &c, bool zc, int acq, SweepRecord &r, double *best_val, int64_t *best_idx, int64_t *n_clamped) {
    if (c.profiling) prof_collect(c);
    if (zc) { r.bv = c.h_pin_out[0]; r.bi[0] = (long long)c.h_pin_out[1]; r.bi[1] = (long long)c.h_pin_out[2]; }
    if (acq != TGP_ACQ_NONE) {
        if (best_val) *best_val = r.bv;
        if (best_idx) *best_idx = (r.bi[0] >= c.M) ? 0 : (int64_t)r.bi[0];
    }
    if (n_clamped) *n_clamped = (int64_t)r.bi[1];
}

int tgp_sweep(tgp_handle h, int acq, double sf, double incumbent, double param, double *mu,
              double *sigma, double *acq_out, double *best_val, int64_t *best_idx,
              int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->sweep(acq, sf, incumbent, param, mu, sigma, acq_out, best_val, best_idx, n_clamped);
    Context &c = h->c;
    if (int arc = acq_check_args(c, "tgp_sweep", (!c.d_cand || c.M < 1) ? "no candidates set" : nullptr, acq, TGP_ACQ_MES, sf); arc != TGP_OK) return arc;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    SweepCall s;
    s.acq = acq; s.sf = sf; s.incumbent = incumbent; s.param = param;
    s.may_use_front = c.pre.front;
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    int rc = ensure_outputs(c, mu != nullptr, sigma != nullptr, acq_out != nullptr);
    if (rc != TGP_OK) return rc;
    s.mu = mu ? c.d_mu : nullptr; s.sigma = sigma ? c.d_sigma : nullptr; s.acqv = acq_out ? c.d_acq : nullptr;
    s.winner = c.d_winner;
    // (the one question about the kernel family: only the one-workgroup / one-launch kernels can ring a doorbell, and
    // they always write the mapped record)
    const bool can_ring = sweep_path(c, c.M) != SweepPath::General;
    // every sweep's last kernel leaves [best value, best index, clamp count] in device-mapped host memory and
    // hands the counters back at zero: no D2H copy, no memset behind it (TGP_SWEEP_ZC=0: the copies, A/B)
    const bool zc = can_ring || tuning().sweep_zc != 0;
    if (zc && (rc = ensure_pinned(c, 0, 8 * sizeof(double))) != TGP_OK) return rc;
    s.res = zc ? c.h_pin_out.dev() : nullptr;
    // (round 6) the small-problem sweep that only returns its record -- the arg-max of a trial -- is a polled call: the
    // last kernel rings the doorbell, no event, no stream synchronisation (doorbell.hpp)
    if (can_ring && !mu && !sigma && !acq_out) s.bell = bell_next(c);
    CallClock clk{s.bell};
    if ((rc = run_sweep(c, s, clk)) != TGP_OK) return rc;
    SweepRecord rec;
    if ((rc = sweep_queue_return(c, zc, acq, rec, &clk, mu, sigma, acq_out)) != TGP_OK) return rc;
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "sweep sync")) != TGP_OK) return rc;
    sweep_read_record(c, zc, acq, rec, best_val, best_idx, n_clamped);
    return TGP_OK;
} TGP_CATCH

int tgp_acq_grad(tgp_handle h, const double *Xq, int64_t m, int acq, double sf, double incumbent,
                 double param, double *val, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_acq_grad");
    Context &c = h->c;
    const char *own = (!Xq || !val || !grad || m < 1 || m > 4096) ? "need Xq, val, grad and 1 <= m <= 4096" : nullptr;
    if (int arc = acq_check_args(c, "tgp_acq_grad", own, acq, TGP_ACQ_MES, sf); arc != TGP_OK) return arc;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    // Round 6: a POLLED call when the batch fits the pinned staging -- the points are read from, value + gradient
    // written to, device-mapped host memory, and the last workgroup rings the call's doorbell (doorbell.hpp): no
    // memcpy, no event, no stream synchronisation.  N <= 128 in ONE launch (a workgroup per point), above that the
    // four general kernels with value + gradient formed by the reduction's last workgroup.
    const int64_t D = c.D;
    const size_t zc_in = (size_t)(m * D) * sizeof(double), zc_out = (size_t)(8 + m + m * D) * sizeof(double);
    // (max-value entropy search lives in the general query kernels only: they serve every N)
    const bool small_q = small_refine_fits(c) && small_path_enabled() && tuning().small_query != 0 && acq != TGP_ACQ_MES;
    Bell bell{nullptr, 0, nullptr};
    if (zc_in <= ((size_t)1 << 20) && zc_out <= ((size_t)1 << 20)) bell = bell_next(c);
    if (bell.word) {
        int prc = ensure_pinned(c, zc_in, zc_out);
        if (prc != TGP_OK) return prc;
        memcpy(c.h_pin_in, Xq, zc_in);
        double *o_val = c.h_pin_out.dev() + 8, *o_grad = o_val + m;
        hipError_t le;
        if (small_q) {
            le = launch_small_query(c, c.h_pin_in.dev(), (int)m, acq, sf, incumbent, param, o_val, o_grad, bell);
        } else {
            API_MEM(grow(c, c.d_qws, query_ws(c, (int)m).bytes, "hipMalloc query workspace"));
            le = launch_query(c, c.h_pin_in.dev(), (int)m, acq, sf, incumbent, param, query_ws(c, (int)m).ws, o_val, o_grad, bell);   // (the layout of the copying path below, so both share d_qws)
        }
        if (le != hipSuccess) return hip_fail(c, le, "launch_query");
        int wrc = bell_wait(c, bell, "query sync");
        if (wrc != TGP_OK) return wrc;
        memcpy(val, c.h_pin_out + 8, (size_t)m * sizeof(double));
        memcpy(grad, c.h_pin_out + 8 + m, (size_t)(m * D) * sizeof(double));
        return TGP_OK;
    }
    API_MEM(grow(c, c.d_qws, query_ws(c, (int)m).bytes, "hipMalloc query workspace"));
    const QueryWs q = query_ws(c, (int)m);
    API_HIP(hipMemcpyAsync(q.Xq, Xq, (size_t)(m * c.D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    hipError_t le = launch_query(c, q.Xq, (int)m, acq, sf, incumbent, param, q.ws, q.val, q.grad);
    if (le != hipSuccess) return hip_fail(c, le, "launch_query");
    API_HIP(hipMemcpyAsync(val, q.val, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H val");
    API_HIP(hipMemcpyAsync(grad, q.grad, (size_t)(m * c.D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H grad");
    API_HIP(hipStreamSynchronize(c.stream), "query sync");
    return TGP_OK;
} TGP_CATCH

// ---- batch selection (include/turbogp.h): what tgp_sweep_batch and tgp_sweep_batch_mc share.  The first step IS a sweep
// (run_sweep) with the posterior kept on the device; every conditioned point then costs its O(N^2) front
// (w_j = K^-1 k*(z_j)), a one-workgroup small side and -- unless it is the last one and nothing after it is asked for --
// one O(M N D) pass over the candidates with the update and the next selection's arg-max (batch_kernels.hip).  Every step
// reads the previous winner from device memory: the host issues everything, then waits once.

// the checks both entries make, in the order they report; `own`: the failed check particular to the entry, or null
static int batch_check_args(Context &c, const char *fn, int64_t q, int64_t P, const double *Xp, const char *own, int acq,
                            double sf, const int64_t *idx_out, const double *val_out) {
    const std::string f = std::string(fn) + ": ";
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, f + "no fitted model");
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, f + "no candidates set");
    if (q < 1 || q > c.M) return fail(c, TGP_BAD_ARG, f + "need 1 <= q <= M");
    if (P < 0 || P + q > BT_MAXP) return fail(c, TGP_BAD_ARG, f + "need P >= 0 and P + q <= 64");
    if (P > 0 && !Xp) return fail(c, TGP_BAD_ARG, f + "Xp is NULL with P > 0");
    if (own) return fail(c, TGP_BAD_ARG, f + own);
    if (acq < TGP_ACQ_UCB || acq > TGP_ACQ_SIGMA) return fail(c, TGP_BAD_ARG, f + "acq must be UCB, PI, EI or SIGMA");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, f + "sf must be +1 or -1");
    if (!idx_out || !val_out) return fail(c, TGP_BAD_ARG, f + "idx_out and val_out are required");
    return TGP_OK;
}

// the call's buffers, carved.  mc: the Monte Carlo tail of d_bt (eps, fant and inc per simulation) in place of the greedy
// one (fant, e, one incumbent); n_acq: rows of acq_out the steps write (Monte Carlo)
static int batch_workspace(Context &c, int64_t J, bool mc, int64_t n_acq, BatchWs &ws) {
    constexpr int64_t NE = (int64_t)BT_MAXP * MC_MAXS;
    const int64_t D = c.D, Dp = c.Dp, Np = c.Np, M = c.M;
    ws = BatchWs{};
    ws.Mpad = ((M + 63) / 64) * 64;
    ws.nblk = (M + 255) / 256;
    ws.js = bt_pass_splits(c, M);
    const size_t n_bt = (size_t)(BT_MAXP * D + BT_MAXP * Dp + BT_MAXP * Np + 3 * Np + BT_MAXP * BT_MAXP + BT_MAXP +
                                 (mc ? 2 * NE + MC_MAXS : 2 * BT_MAXP + 8));
    const size_t n_btm = (size_t)(ws.Mpad * Dp + ws.js * ws.Mpad + 2 * M + ws.nblk + J * M + n_acq * M);
    const size_t n_bti = (size_t)(BT_MAXP + 2 + ws.nblk) * sizeof(long long) + (size_t)M;
    int rc;
    if ((rc = grow(c, c.d_bt, n_bt * sizeof(double), "hipMalloc batch state")) != TGP_OK) return rc;
    if ((rc = grow(c, c.d_btm, n_btm * sizeof(double), "hipMalloc batch arrays")) != TGP_OK) return rc;
    if ((rc = grow(c, c.d_bti, n_bti, "hipMalloc batch indices")) != TGP_OK) return rc;
    ws.Zraw = c.d_bt; ws.Zs = ws.Zraw + BT_MAXP * D; ws.Kz = ws.Zs + BT_MAXP * Dp; ws.hw = ws.Kz + BT_MAXP * Np;
    ws.v = ws.hw + Np; ws.w = ws.v + Np; ws.R = ws.w + Np; ws.selv = ws.R + BT_MAXP * BT_MAXP;
    if (mc) { ws.eps = ws.selv + BT_MAXP; ws.fant = ws.eps + NE; ws.inc = ws.fant + NE; }
    else { ws.fant = ws.selv + BT_MAXP; ws.e = ws.fant + BT_MAXP; ws.inc = ws.e + BT_MAXP; }
    ws.Cs = c.d_btm; ws.part = ws.Cs + ws.Mpad * Dp; ws.bmu = ws.part + ws.js * ws.Mpad; ws.bvar = ws.bmu + M;
    ws.bval = ws.bvar + M; ws.G = ws.bval + ws.nblk; ws.acqd = ws.G + J * M;
    ws.seli = c.d_bti; ws.clampw = ws.seli + BT_MAXP; ws.flagw = ws.clampw + 1; ws.bidx = ws.flagw + 1;
    ws.mask = reinterpret_cast<unsigned char *>(ws.bidx + ws.nblk);
    return TGP_OK;
}

// the first sweep: means and deviations left in c.d_mu / c.d_sigma (keep_acq: its acquisition vector in c.d_acq), its
// record in the mapped result buffer (read by the first selection on the device); the winner record of
// tgp_set_winner_out is not this call's to pack
static int batch_first_sweep(Context &c, int acq, double sf, double incumbent, double param, bool keep_acq,
                             size_t pin_in_bytes, size_t pin_out_bytes, CallClock &clk) {
    SweepCall first;
    first.acq = acq; first.sf = sf; first.incumbent = incumbent; first.param = param;
    first.may_use_front = c.pre.front;
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    int rc;
    if ((rc = ensure_outputs(c, true, true, keep_acq)) != TGP_OK) return rc;
    if ((rc = ensure_pinned(c, pin_in_bytes, pin_out_bytes)) != TGP_OK) return rc;
    first.mu = c.d_mu; first.sigma = c.d_sigma; first.res = c.h_pin_out.dev();
    if (keep_acq) first.acqv = c.d_acq;
    return run_sweep(c, first, clk);
}

// the J = P + q conditioned points in turn: selection k = j - P read from the first sweep's record or the previous
// step's arg-max, the strategy's condition(j), then its step(j, last, select, knext) -- skipped for the last point unless
// run_last (something after it is asked for)
extern "C++" template <typename Cond, typename Step>
static int batch_steps(Context &c, const BatchWs &ws, const BtSmall &s, int64_t P, int64_t q, bool run_last, Cond condition,
                       Step step) {
    const int64_t J = P + q;
    hipError_t le;
    for (int64_t j = 0; j < J; ++j) {
        if (j >= P) {   // selection k = j - P: the first sweep's winner, or the previous step's
            const int64_t k = j - P;
            le = launch_bt_point(c, (P == 0 && k == 0) ? c.h_pin_out.dev() : nullptr, s, (int)k, ws.Zraw + j * c.D, ws.mask);
            if (le != hipSuccess) return hip_fail(c, le, "launch_bt_point");
        }
        if ((le = condition((int)j)) != hipSuccess) return hip_fail(c, le, "batch condition");
        const bool last = j == J - 1;
        if (last && !run_last) break;
        const int64_t knext = j + 1 - P;              // the selection this step's update feeds, if any
        const bool select = !last && knext >= 0 && knext < q;
        if ((le = step((int)j, last, select, knext)) != hipSuccess) return hip_fail(c, le, "batch step");
    }
    return TGP_OK;
}

// after the wait: hi = [indices (64) | clamp count | flag] as copied back; the not-positive-definite report or idx_out
static int batch_finish(Context &c, const char *fn, const long long *hi, int64_t P, int64_t q, int64_t *idx_out) {
    const int flag = (int)(hi[BT_MAXP + 1] & 0xffffffff);
    if (flag != 0) {
        char buf[200];
        snprintf(buf, sizeof buf, "%s: the augmented kernel matrix is not positive definite (%s point %d)", fn,
                 flag - 1 < P ? "pending" : "selected", flag - 1 < P ? flag - 1 : (int)(flag - 1 - P));
        return fail(c, TGP_NOT_PD, buf);
    }
    for (int64_t k = 0; k < q; ++k) idx_out[k] = (int64_t)hi[k];
    return TGP_OK;
}

// Greedy batch selection with Kriging Believer / Constant Liar
int tgp_sweep_batch(tgp_handle h, int64_t q, int strategy, double lie, const double *Xp, int64_t P, int acq, double sf,
                    double incumbent, double param, int64_t *idx_out, double *val_out, double *x_out,
                    double *fantasy_out, double *mu_out, double *sigma_out, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_batch");
    Context &c = h->c;
    const char *own = (strategy != TGP_BATCH_KB && strategy != TGP_BATCH_CL) ? "unknown strategy"
                      : (strategy == TGP_BATCH_CL && !std::isfinite(lie))    ? "the lie must be finite"
                                                                             : nullptr;
    int rc;
    if ((rc = batch_check_args(c, "tgp_sweep_batch", q, P, Xp, own, acq, sf, idx_out, val_out)) != TGP_OK) return rc;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    const int64_t D = c.D, M = c.M, J = P + q;
    BatchWs ws;
    if ((rc = batch_workspace(c, J, false, 0, ws)) != TGP_OK) return rc;
    const BtSmall s{ws.R, ws.e, ws.fant, ws.inc, ws.selv, ws.seli, reinterpret_cast<int *>(ws.flagw)};
    CallClock clk;
    rc = batch_first_sweep(c, acq, sf, incumbent, param, false, (size_t)(P * D + 8) * sizeof(double), 8 * sizeof(double), clk);
    if (rc != TGP_OK) return rc;
    hipError_t le;

    // ---- the steps
    double *pin = c.h_pin_in;
    if (P > 0) memcpy(pin, Xp, (size_t)(P * D) * sizeof(double));
    pin[P * D] = incumbent;
    if (P > 0) API_HIP(hipMemcpyAsync(ws.Zraw, pin, (size_t)(P * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D pending");
    API_HIP(hipMemcpyAsync(ws.inc, pin + P * D, sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D incumbent");
    API_HIP(hipMemsetAsync(ws.w, 0, (size_t)c.Np * sizeof(double), c.stream), "memset w");
    API_HIP(hipMemsetAsync(ws.clampw, 0, 2 * sizeof(long long), c.stream), "memset counters");
    if ((le = launch_bt_prep(c, ws.Cs, ws.Mpad)) != hipSuccess) return hip_fail(c, le, "launch_bt_prep");
    if ((le = launch_bt_init(c, ws.bmu, ws.bvar, ws.mask)) != hipSuccess) return hip_fail(c, le, "launch_bt_init");
    const int kb = strategy == TGP_BATCH_KB;
    rc = batch_steps(c, ws, s, P, q, mu_out || sigma_out,
                     [&](int j) { return launch_bt_condition(c, ws, s, nullptr, j, kb, lie, sf); },
                     [&](int j, bool last, bool select, int64_t knext) {
                         return launch_bt_step(c, ws, s, j, last ? 0 : 1, select ? acq : TGP_ACQ_NONE, sf, param,
                                               last ? c.d_mu : nullptr, last ? c.d_sigma : nullptr, (int)knext);
                     });
    if (rc != TGP_OK) return rc;
    if ((rc = call_stop(c, clk)) != TGP_OK) return rc;

    // ---- one wait
    std::vector<double> hs((size_t)(BT_MAXP * D + 2 * BT_MAXP));   // [points (64 D) | sel_val (64) | fantasies (64)]
    std::vector<long long> hi((size_t)BT_MAXP + 2);
    API_HIP(hipMemcpyAsync(hs.data(), ws.Zraw, (size_t)(BT_MAXP * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H points");
    API_HIP(hipMemcpyAsync(hs.data() + BT_MAXP * D, ws.selv, (size_t)(2 * BT_MAXP) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H fantasies");
    API_HIP(hipMemcpyAsync(hi.data(), ws.seli, (size_t)(BT_MAXP + 2) * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H indices");
    const size_t bytes = (size_t)M * sizeof(double);
    if (mu_out) API_HIP(hipMemcpyAsync(mu_out, c.d_mu, bytes, hipMemcpyDeviceToHost, c.stream), "D2H mu");
    if (sigma_out) API_HIP(hipMemcpyAsync(sigma_out, c.d_sigma, bytes, hipMemcpyDeviceToHost, c.stream), "D2H sigma");
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "sweep_batch sync")) != TGP_OK) return rc;
    if ((rc = batch_finish(c, "tgp_sweep_batch", hi.data(), P, q, idx_out)) != TGP_OK) return rc;
    for (int64_t k = 0; k < q; ++k) {
        val_out[k] = hs[BT_MAXP * D + k];
        if (x_out) memcpy(x_out + k * D, hs.data() + (P + k) * D, (size_t)D * sizeof(double));
    }
    if (fantasy_out) memcpy(fantasy_out, hs.data() + BT_MAXP * D + BT_MAXP, (size_t)J * sizeof(double));
    if (n_clamped) *n_clamped = (int64_t)c.h_pin_out[2] + (int64_t)hi[BT_MAXP];
    return TGP_OK;
} TGP_CATCH

// The Monte Carlo strategy: the same schedule with S simulations of every point's outcome carried through the small side
// and the update (batch_kernels.hip)
int tgp_sweep_batch_mc(tgp_handle h, int64_t q, int64_t S, uint64_t seed, const double *eps_in, const double *Xp, int64_t P,
                       int acq, double sf, double incumbent, double param, int64_t *idx_out, double *val_out,
                       double *x_out, double *fantasy_out, double *eps_out, double *acq_out, double *sigma_out,
                       int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_batch_mc");
    Context &c = h->c;
    int rc;
    if ((rc = batch_check_args(c, "tgp_sweep_batch_mc", q, P, Xp, (S < 1 || S > MC_MAXS) ? "need 1 <= S <= 64" : nullptr, acq,
                               sf, idx_out, val_out)) != TGP_OK)
        return rc;
    const int64_t D = c.D, M = c.M, J = P + q;
    if (eps_in)
        for (int64_t i = 0; i < S * J; ++i)
            if (!std::isfinite(eps_in[i])) return fail(c, TGP_BAD_ARG, "tgp_sweep_batch_mc: eps_in must be finite");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    const bool first_acq = acq_out && P == 0;                      // the first sweep's vector is row 0 of acq_out
    const int64_t n_acq = acq_out ? (first_acq ? q - 1 : q) : 0;   // rows of acq_out the steps write
    BatchWs ws;
    if ((rc = batch_workspace(c, J, true, n_acq, ws)) != TGP_OK) return rc;
    McSmall s{};
    s.b = BtSmall{ws.R, nullptr, nullptr, nullptr, ws.selv, ws.seli, reinterpret_cast<int *>(ws.flagw)};
    s.eps = ws.eps; s.fant = ws.fant; s.inc = ws.inc; s.S = (int)S;
    constexpr int64_t NE = (int64_t)BT_MAXP * MC_MAXS;
    // result staging (pinned, so the copies back are not staged): [sweep record (8) | x (q D) | sel_val (64) | eps (J 64) |
    // fantasies (J 64) | indices, clamp count, flag (66)]
    const size_t n_pout = (size_t)(8 + q * D + BT_MAXP + 2 * J * MC_MAXS + BT_MAXP + 2);
    CallClock clk;
    rc = batch_first_sweep(c, acq, sf, incumbent, param, first_acq, (size_t)(P * D + NE + 8) * sizeof(double),
                           n_pout * sizeof(double), clk);
    if (rc != TGP_OK) return rc;
    hipError_t le;

    // ---- the steps
    double *pin = c.h_pin_in;
    if (P > 0) {
        memcpy(pin, Xp, (size_t)(P * D) * sizeof(double));
        API_HIP(hipMemcpyAsync(ws.Zraw, pin, (size_t)(P * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D pending");
    }
    if (eps_in) {   // (S, J) -> point-major (64, 64), zero elsewhere
        double *pe = pin + P * D;
        memset(pe, 0, (size_t)NE * sizeof(double));
        for (int64_t si = 0; si < S; ++si)
            for (int64_t j = 0; j < J; ++j) pe[j * MC_MAXS + si] = eps_in[si * J + j];
        API_HIP(hipMemcpyAsync(ws.eps, pe, (size_t)NE * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D eps");
    }
    API_HIP(hipMemsetAsync(ws.w, 0, (size_t)c.Np * sizeof(double), c.stream), "memset w");
    API_HIP(hipMemsetAsync(ws.clampw, 0, 2 * sizeof(long long), c.stream), "memset counters");
    if ((le = launch_mc_init(c, s, (int)J, eps_in == nullptr, (unsigned long long)seed, incumbent)) != hipSuccess)
        return hip_fail(c, le, "launch_mc_init");
    if ((le = launch_bt_prep(c, ws.Cs, ws.Mpad)) != hipSuccess) return hip_fail(c, le, "launch_bt_prep");
    if ((le = launch_bt_init(c, ws.bmu, ws.bvar, ws.mask)) != hipSuccess) return hip_fail(c, le, "launch_bt_init");
    rc = batch_steps(c, ws, s.b, P, q, sigma_out != nullptr,
                     [&](int j) { return launch_bt_condition(c, ws, s.b, &s, j, 0, 0.0, sf); },
                     [&](int j, bool last, bool select, int64_t knext) {
                         double *arow = (select && acq_out) ? ws.acqd + (knext - (first_acq ? 1 : 0)) * M : nullptr;
                         return launch_mc_step(c, ws, s, j, select ? acq : TGP_ACQ_NONE, sf, param, arow,
                                               last ? c.d_sigma : nullptr, (int)knext);
                     });
    if (rc != TGP_OK) return rc;
    if ((rc = call_stop(c, clk)) != TGP_OK) return rc;

    // ---- one wait: only what was asked for, and of eps / fantasies only the J rows in use (point-major: contiguous)
    double *h_x = c.h_pin_out + 8, *h_selv = h_x + q * D, *h_eps = h_selv + BT_MAXP, *h_fant = h_eps + J * MC_MAXS;
    long long *hi = reinterpret_cast<long long *>(h_fant + J * MC_MAXS);
    const size_t d8 = sizeof(double);
    if (x_out) API_HIP(hipMemcpyAsync(h_x, ws.Zraw + P * D, (size_t)(q * D) * d8, hipMemcpyDeviceToHost, c.stream), "D2H points");
    API_HIP(hipMemcpyAsync(h_selv, ws.selv, (size_t)q * d8, hipMemcpyDeviceToHost, c.stream), "D2H values");
    if (eps_out) API_HIP(hipMemcpyAsync(h_eps, ws.eps, (size_t)(J * MC_MAXS) * d8, hipMemcpyDeviceToHost, c.stream), "D2H eps");
    if (fantasy_out) API_HIP(hipMemcpyAsync(h_fant, ws.fant, (size_t)(J * MC_MAXS) * d8, hipMemcpyDeviceToHost, c.stream), "D2H fantasies");
    API_HIP(hipMemcpyAsync(hi, ws.seli, (size_t)(BT_MAXP + 2) * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H indices");
    const size_t bytes = (size_t)M * d8;
    if (first_acq) API_HIP(hipMemcpyAsync(acq_out, c.d_acq, bytes, hipMemcpyDeviceToHost, c.stream), "D2H acq");
    if (n_acq > 0)
        API_HIP(hipMemcpyAsync(acq_out + (first_acq ? M : 0), ws.acqd, (size_t)n_acq * bytes, hipMemcpyDeviceToHost, c.stream), "D2H acq");
    if (sigma_out) API_HIP(hipMemcpyAsync(sigma_out, c.d_sigma, bytes, hipMemcpyDeviceToHost, c.stream), "D2H sigma");
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "sweep_batch_mc sync")) != TGP_OK) return rc;
    if ((rc = batch_finish(c, "tgp_sweep_batch_mc", hi, P, q, idx_out)) != TGP_OK) return rc;
    for (int64_t k = 0; k < q; ++k) val_out[k] = h_selv[k];
    if (x_out) memcpy(x_out, h_x, (size_t)(q * D) * d8);
    if (first_acq)   // row 0 is the first sweep's vector: NaN -> -inf, the convention of the steps' rows
        for (int64_t x = 0; x < M; ++x)
            if (std::isnan(acq_out[x])) acq_out[x] = -INFINITY;
    for (int64_t si = 0; si < S; ++si)
        for (int64_t j = 0; j < J; ++j) {
            if (fantasy_out) fantasy_out[si * J + j] = h_fant[j * MC_MAXS + si];
            if (eps_out) eps_out[si * J + j] = h_eps[j * MC_MAXS + si];
        }
    if (n_clamped) *n_clamped = (int64_t)c.h_pin_out[2] + (int64_t)hi[BT_MAXP];
    return TGP_OK;
} TGP_CATCH

// ---- Thompson sampling (include/turbogp.h, ts_kernels.hip) ----
// d_ts: [omega (F Dp) | b (F) | W (Spad F) | V (Spad Np) | eps (S N) | priorX (N S) | R (S Np) | Z (S Np)], every
// part starting on a 32-byte boundary (V is read in 32-byte vectors)
static int64_t ts_al4(int64_t n) { return (n + 3) & ~(int64_t)3; }
static TsDraw ts_view(Context &c, double **priorX = nullptr, double **R = nullptr, double **Z = nullptr) {
    TsDraw t{};
    t.S = c.ts_S; t.F = c.ts_F;
    const int64_t Spad = ts_spad(t.S);
    double *p = c.d_ts;
    t.omega = p; p += ts_al4(t.F * c.Dp);
    t.b = p; p += ts_al4(t.F);
    t.W = p; p += ts_al4(Spad * t.F);
    t.V = p; p += ts_al4(Spad * c.Np);
    t.eps = p; p += ts_al4(t.S * c.N);
    if (priorX) *priorX = p;
    p += ts_al4(c.N * t.S);
    if (R) *R = p;
    p += ts_al4(t.S * c.Np);
    if (Z) *Z = p;
    return t;
}
static int64_t ts_doubles(const Context &c, int64_t S, int64_t F) {
    const int64_t Spad = ts_spad(S);
    return ts_al4(F * c.Dp) + ts_al4(F) + ts_al4(Spad * F) + ts_al4(Spad * c.Np) + ts_al4(S * c.N) + ts_al4(c.N * S) +
           2 * ts_al4(S * c.Np);
}
// tgp_ts_sweep's per-call region over the resident batch, carved from `base`:
// [Cs (Mpad Dp) | f (M S) | bval (S nblk) | sel_val (S) | sel_x (S D) | bidx (S nblk) | sel_idx (S) | mask (M bytes)]
struct TsSweepWs {
    double *Cs, *f, *bval, *selv, *selx;
    long long *bidx, *seli;
    unsigned char *mask;
    int64_t Mpad;
    size_t bytes;
};
static TsSweepWs ts_sweep_ws(const Context &c, double *base, int64_t S) {
    const int64_t M = c.M, D = c.D, nblk = (M + 255) / 256;
    TsSweepWs w{};
    w.Mpad = ((M + 63) / 64) * 64;
    w.Cs = base;
    w.f = w.Cs + ts_al4(w.Mpad * c.Dp);
    w.bval = w.f + ts_al4(M * S);
    w.selv = w.bval + ts_al4(S * nblk);
    w.selx = w.selv + ts_al4(S);
    w.bidx = reinterpret_cast<long long *>(w.selx + ts_al4(S * D));
    w.seli = w.bidx + S * nblk;
    w.mask = reinterpret_cast<unsigned char *>(w.seli + S);
    w.bytes = (size_t)(w.mask - reinterpret_cast<unsigned char *>(base)) + (size_t)M;
    return w;
}
static int ts_check_draw(Context &c, const char *fn) {
    if (!c.fitted) return fail(c, TGP_BAD_ARG, std::string(fn) + ": no fitted model");
    if (c.ts_gen < 0 || c.ts_gen != c.fit_gen)
        return fail(c, TGP_BAD_ARG, std::string(fn) + ": no draw for the resident fit (tgp_ts_draw after the last fit)");
    return TGP_OK;
}

int tgp_ts_draw(tgp_handle h, uint64_t seed, int64_t S, int64_t F) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ts_draw");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_BAD_ARG, "tgp_ts_draw: no fitted model");
    if (S < 1 || S > 64) return fail(c, TGP_BAD_ARG, "tgp_ts_draw: need 1 <= S <= 64");
    if (F < 64 || F > 16384 || F % 64 != 0) return fail(c, TGP_BAD_ARG, "tgp_ts_draw: F must be a multiple of 64 in [64, 16384]");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    c.ts_gen = -1;
    int rc = grow(c, c.d_ts, (size_t)ts_doubles(c, S, F) * sizeof(double), "hipMalloc Thompson draw");
    if (rc != TGP_OK) return rc;
    c.ts_S = S; c.ts_F = F;
    double *priorX, *R, *Z;
    const TsDraw t = ts_view(c, &priorX, &R, &Z);
    hipError_t le = launch_ts_draw(c, t, (unsigned long long)seed, priorX, R, Z);
    if (le != hipSuccess) return hip_fail(c, le, "launch_ts_draw");
    API_HIP(hipStreamSynchronize(c.stream), "ts_draw sync");
    c.ts_gen = c.fit_gen;
    return TGP_OK;
} TGP_CATCH

// one pass over the resident candidates, S arg-max reductions in device memory, one wait
int tgp_ts_sweep(tgp_handle h, double sf, int distinct, int64_t *idx_out, double *val_out, double *x_out, double *f_out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ts_sweep");
    Context &c = h->c;
    int rc = ts_check_draw(c, "tgp_ts_sweep");
    if (rc != TGP_OK) return rc;
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_ts_sweep: no candidates set");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, "tgp_ts_sweep: sf must be +1 or -1");
    if (distinct && c.ts_S > c.M) return fail(c, TGP_BAD_ARG, "tgp_ts_sweep: distinct needs S <= M");
    if (!idx_out || !val_out) return fail(c, TGP_BAD_ARG, "tgp_ts_sweep: idx_out and val_out are required");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const TsDraw t = ts_view(c);
    const int64_t S = t.S, M = c.M, D = c.D;
    if ((rc = grow(c, c.d_tsm, ts_sweep_ws(c, nullptr, S).bytes, "hipMalloc Thompson sweep")) != TGP_OK) return rc;
    const TsSweepWs ws = ts_sweep_ws(c, c.d_tsm, S);
    const int64_t Mpad = ws.Mpad;
    double *Cs = ws.Cs, *f = ws.f, *bval = ws.bval, *selv = ws.selv, *selx = ws.selx;
    long long *bidx = ws.bidx, *seli = ws.seli;
    unsigned char *mask = ws.mask;
    CallClock clk;
    if ((rc = call_begin(c, clk)) != TGP_OK) return rc;
    hipError_t le = launch_bt_prep(c, Cs, Mpad);
    if (le != hipSuccess) return hip_fail(c, le, "launch_bt_prep");
    if ((le = launch_ts_pass(c, t, Cs, M, true, f, c.y_mean, c.y_std)) != hipSuccess) return hip_fail(c, le, "launch_ts_pass");
    if ((le = launch_ts_select(c, t, f, sf, distinct ? 1 : 0, mask, bval, bidx, seli, selv, selx)) != hipSuccess)
        return hip_fail(c, le, "launch_ts_select");
    if ((rc = call_stop(c, clk)) != TGP_OK) return rc;
    std::vector<long long> hi((size_t)S);
    API_HIP(hipMemcpyAsync(hi.data(), seli, (size_t)S * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H indices");
    API_HIP(hipMemcpyAsync(val_out, selv, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H values");
    if (x_out) API_HIP(hipMemcpyAsync(x_out, selx, (size_t)(S * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H rows");
    if (f_out) API_HIP(hipMemcpyAsync(f_out, f, (size_t)(M * S) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H f");
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "ts_sweep sync")) != TGP_OK) return rc;
    for (int64_t s = 0; s < S; ++s) idx_out[s] = (int64_t)hi[s];
    return TGP_OK;
} TGP_CATCH

int tgp_ts_eval(tgp_handle h, const double *Xq, int64_t m, double *f_out, double *grad_out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ts_eval");
    Context &c = h->c;
    int rc = ts_check_draw(c, "tgp_ts_eval");
    if (rc != TGP_OK) return rc;
    if (!Xq || !f_out || m < 1 || m > 4096) return fail(c, TGP_BAD_ARG, "tgp_ts_eval: need Xq, f_out and 1 <= m <= 4096");
    if (ts_eval_lds_bytes(c, c.ts_S) > 65536) return fail(c, TGP_BAD_ARG, "tgp_ts_eval: S (1 + D) too large for one workgroup's LDS");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const TsDraw t = ts_view(c);
    const int64_t S = t.S, D = c.D;
    // [Xq (m D) | f (m S) | grad (m S D)] in the per-call region the sweep uses too
    const int64_t nd = ts_al4(m * D) + ts_al4(m * S) + m * S * D;
    if ((rc = grow(c, c.d_tsm, (size_t)nd * sizeof(double), "hipMalloc Thompson eval")) != TGP_OK) return rc;
    double *dX = c.d_tsm, *df = dX + ts_al4(m * D), *dg = df + ts_al4(m * S);
    API_HIP(hipMemcpyAsync(dX, Xq, (size_t)(m * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    hipError_t le = launch_ts_eval(c, t, dX, (int)m, df, grad_out ? dg : nullptr);
    if (le != hipSuccess) return hip_fail(c, le, "launch_ts_eval");
    API_HIP(hipMemcpyAsync(f_out, df, (size_t)(m * S) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H f");
    if (grad_out) API_HIP(hipMemcpyAsync(grad_out, dg, (size_t)(m * S * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H grad");
    API_HIP(hipStreamSynchronize(c.stream), "ts_eval sync");
    return TGP_OK;
} TGP_CATCH

int tgp_ts_read(tgp_handle h, double *omega, double *b, double *W, double *eps) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ts_read");
    Context &c = h->c;
    int rc = ts_check_draw(c, "tgp_ts_read");
    if (rc != TGP_OK) return rc;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const TsDraw t = ts_view(c);
    const size_t d8 = sizeof(double);
    if (omega) API_HIP(hipMemcpy2DAsync(omega, (size_t)c.D * d8, t.omega, (size_t)c.Dp * d8, (size_t)c.D * d8, (size_t)t.F,
                                        hipMemcpyDeviceToHost, c.stream), "D2H omega");
    if (b) API_HIP(hipMemcpyAsync(b, t.b, (size_t)t.F * d8, hipMemcpyDeviceToHost, c.stream), "D2H b");
    if (W) API_HIP(hipMemcpyAsync(W, t.W, (size_t)(t.S * t.F) * d8, hipMemcpyDeviceToHost, c.stream), "D2H W");
    if (eps) API_HIP(hipMemcpyAsync(eps, t.eps, (size_t)(t.S * c.N) * d8, hipMemcpyDeviceToHost, c.stream), "D2H eps");
    API_HIP(hipStreamSynchronize(c.stream), "ts_read sync");
    return TGP_OK;
} TGP_CATCH

// ---- max-value entropy search: the S maxima a TGP_ACQ_MES call averages over (include/turbogp.h) ----
static bool mes_values_ok(const double *ystar, int64_t S) {
    if (!ystar || S < 1 || S > MES_MAXS) return false;
    for (int64_t s = 0; s < S; ++s)
        if (!std::isfinite(ystar[s])) return false;
    return true;
}

int tgp_mes_set_maxima(tgp_handle h, const double *ystar, int64_t S) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->mes_set_maxima(ystar, S);
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_mes_set_maxima: no fitted model (the maxima belong to one fit)");
    if (!mes_values_ok(ystar, S)) return fail(c, TGP_BAD_ARG, "tgp_mes_set_maxima: need 1 <= S <= 64 finite values");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    c.mes_gen = -1;
    API_MEM(grow(c, c.d_mes, MES_MAXS * sizeof(double), "hipMalloc maxima", false));
    API_HIP(hipMemcpyAsync(c.d_mes, ystar, (size_t)S * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D maxima");
    API_HIP(hipStreamSynchronize(c.stream), "mes_set_maxima sync");
    c.mes_S = (int)S;
    c.mes_gen = c.fit_gen;
    return TGP_OK;
} TGP_CATCH

int tgp_mes_draw(tgp_handle h, uint64_t seed, int64_t S, int64_t F, double sf, double incumbent, double *ystar_out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_mes_draw");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_mes_draw: no fitted model");
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_mes_draw: no candidates set");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, "tgp_mes_draw: sf must be +1 or -1");
    c.mes_gen = -1;
    int rc = tgp_ts_draw(h, seed, S, F);      // (checks S and F)
    if (rc != TGP_OK) return rc;
    int64_t idx[MES_MAXS];
    double val[MES_MAXS];
    if ((rc = tgp_ts_sweep(h, sf, 0, idx, val, nullptr, nullptr)) != TGP_OK) return rc;
    for (int64_t s = 0; s < S; ++s)
        if (!std::isfinite(val[s])) return fail(c, TGP_BAD_ARG, "tgp_mes_draw: a sample path has no finite value over the candidates");
    // the sweep's winners are still where it left them on the device: the handle's maxima are formed from there
    API_MEM(grow(c, c.d_mes, MES_MAXS * sizeof(double), "hipMalloc maxima", false));
    hipError_t le = launch_mes_take(c, ts_sweep_ws(c, c.d_tsm, S).selv, (int)S, sf, incumbent, c.d_mes);
    if (le != hipSuccess) return hip_fail(c, le, "launch_mes_take");
    if (ystar_out) API_HIP(hipMemcpyAsync(ystar_out, c.d_mes, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H maxima");
    API_HIP(hipStreamSynchronize(c.stream), "mes_draw sync");
    c.mes_S = (int)S;
    c.mes_gen = c.fit_gen;
    return TGP_OK;
} TGP_CATCH

// ---- the joint posterior over m query points (include/turbogp.h; cov_kernels.hip) ----
// what both entries check, in the order they report; host handles are served before this
static int cov_check(Context &c, const char *fn, const double *Xq, int64_t m, const void *out) {
    const std::string f = std::string(fn) + ": ";
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, f + "no fitted model");
    if (!Xq || !out || m < 1 || m > 4096) return fail(c, TGP_BAD_ARG, f + "need Xq, the output and 1 <= m <= 4096");
    for (int64_t e = 0; e < m * c.D; ++e)
        if (!std::isfinite(Xq[e])) return fail(c, TGP_BAD_ARG, f + "Xq must be finite");
    return TGP_OK;
}

// the workspace (allocated on first use and kept, as the query workspace is) with Xq copied in
static int cov_begin(Context &c, const double *Xq, int64_t m, int64_t S, CovWs &w) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t nd = cov_ws_doubles(c, m, S, &w);
    int rc = grow(c, c.d_cov, (size_t)nd * sizeof(double), "hipMalloc joint posterior workspace");
    if (rc != TGP_OK) return rc;
    API_HIP(hipMemcpyAsync(c.d_cov + w.o_Xq, Xq, (size_t)(m * c.D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    return TGP_OK;
}

// the kernels' device time between the call's two events (the copies are outside): tgp_last_timings slot 15
static void cov_time(Context &c) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c.ev0, c.ev1);
    c.last_cov_ms = ms;
}

int tgp_predict_cov(tgp_handle h, const double *Xq, int64_t m, int latent, double *mu_out, double *cov_out,
                    int64_t *n_negative_diag) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->predict_cov(Xq, m, latent, mu_out, cov_out, n_negative_diag);
    Context &c = h->c;
    int rc = cov_check(c, "tgp_predict_cov", Xq, m, cov_out);
    if (rc != TGP_OK) return rc;
    CovWs w;
    if ((rc = cov_begin(c, Xq, m, 0, w)) != TGP_OK) return rc;
    API_HIP(hipEventRecord(c.ev0, c.stream), "hipEventRecord");
    hipError_t le = launch_cov_posterior(c, c.d_cov, w, latent, 0.0, false);
    if (le != hipSuccess) return hip_fail(c, le, "launch_cov_posterior");
    API_HIP(hipEventRecord(c.ev1, c.stream), "hipEventRecord");
    const size_t d8 = sizeof(double);
    long long neg = 0;
    API_HIP(hipMemcpy2DAsync(cov_out, (size_t)m * d8, c.d_cov + w.o_G, (size_t)w.mpad * d8, (size_t)m * d8, (size_t)m,
                             hipMemcpyDeviceToHost, c.stream), "D2H cov");
    if (mu_out) API_HIP(hipMemcpyAsync(mu_out, c.d_cov + w.o_mu, (size_t)m * d8, hipMemcpyDeviceToHost, c.stream), "D2H mu");
    API_HIP(hipMemcpyAsync(&neg, c.d_cov + w.o_cnt, sizeof neg, hipMemcpyDeviceToHost, c.stream), "D2H count");
    API_HIP(hipStreamSynchronize(c.stream), "predict_cov sync");
    cov_time(c);
    if (n_negative_diag) *n_negative_diag = (int64_t)neg;
    return TGP_OK;
} TGP_CATCH

int tgp_sample_joint(tgp_handle h, const double *Xq, int64_t m, int64_t S, int latent, double nugget, uint64_t seed,
                     const double *eps_in, double *y_out, double *eps_out, double *mu_out) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return h->host->sample_joint(Xq, m, S, latent, nugget, eps_in, y_out, eps_out, mu_out);
    Context &c = h->c;
    int rc = cov_check(c, "tgp_sample_joint", Xq, m, y_out);
    if (rc != TGP_OK) return rc;
    if (S < 1 || S > 4096) return fail(c, TGP_BAD_ARG, "tgp_sample_joint: need 1 <= S <= 4096");
    if (!(nugget >= 0.0) || !std::isfinite(nugget)) return fail(c, TGP_BAD_ARG, "tgp_sample_joint: nugget must be finite and >= 0");
    if (eps_in)
        for (int64_t e = 0; e < S * m; ++e)
            if (!std::isfinite(eps_in[e])) return fail(c, TGP_BAD_ARG, "tgp_sample_joint: eps_in must be finite");
    CovWs w;
    if ((rc = cov_begin(c, Xq, m, S, w)) != TGP_OK) return rc;
    const size_t d8 = sizeof(double);
    API_HIP(hipEventRecord(c.ev0, c.stream), "hipEventRecord");
    hipError_t le = launch_cov_posterior(c, c.d_cov, w, latent, nugget, true);
    if (le != hipSuccess) return hip_fail(c, le, "launch_cov_posterior");
    // (the given normals land where Ks was: behind the kernels that read it, in stream order)
    if (eps_in) API_HIP(hipMemcpyAsync(c.d_cov + w.o_Ein, eps_in, (size_t)(S * m) * d8, hipMemcpyHostToDevice, c.stream), "H2D eps");
    le = launch_cov_sample(c, c.d_cov, w, eps_in == nullptr, (unsigned long long)seed);
    if (le != hipSuccess) return hip_fail(c, le, "launch_cov_sample");
    API_HIP(hipEventRecord(c.ev1, c.stream), "hipEventRecord");
    long long cnt[2] = {0, 0};
    API_HIP(hipMemcpyAsync(cnt, c.d_cov + w.o_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.stream), "D2H flag");
    API_HIP(hipMemcpy2DAsync(y_out, (size_t)m * d8, c.d_cov + w.o_Y, (size_t)w.mpad * d8, (size_t)m * d8, (size_t)S,
                             hipMemcpyDeviceToHost, c.stream), "D2H samples");
    if (eps_out) API_HIP(hipMemcpy2DAsync(eps_out, (size_t)m * d8, c.d_cov + w.o_E, (size_t)w.mpad * d8, (size_t)m * d8, (size_t)S,
                                          hipMemcpyDeviceToHost, c.stream), "D2H eps");
    if (mu_out) API_HIP(hipMemcpyAsync(mu_out, c.d_cov + w.o_mu, (size_t)m * d8, hipMemcpyDeviceToHost, c.stream), "D2H mu");
    API_HIP(hipStreamSynchronize(c.stream), "sample_joint sync");
    cov_time(c);
    const int flag = (int)(cnt[1] & 0xFFFFFFFFll);
    if (flag != 0) {
        char buf[200];
        snprintf(buf, sizeof buf, "tgp_sample_joint: joint covariance is not positive definite (pivot %d of %lld): raise the nugget", flag - 1, (long long)m);
        return fail(c, TGP_NOT_PD, buf);
    }
    return TGP_OK;
} TGP_CATCH

int tgp_sweep_topk(tgp_handle h, int acq, double sf, double incumbent, double param, int64_t k,
                   double *vals, int64_t *idxs, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_topk");
    Context &c = h->c;
    const char *own = (!c.d_cand || c.M < 1) ? "no candidates set"
                      : (acq <= TGP_ACQ_NONE || acq > TGP_ACQ_MES) ? "needs an acquisition" : nullptr;
    if (int arc = acq_check_args(c, "tgp_sweep_topk", own, acq, TGP_ACQ_MES, sf); arc != TGP_OK) return arc;
    if (k < 1 || k > 64 || !vals || !idxs) return fail(c, TGP_BAD_ARG, "tgp_sweep_topk: need 1 <= k <= 64, vals and idxs");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    int rc = ensure_outputs(c, false, false, true);           // the (M,) acquisition vector stays on the device
    if (rc != TGP_OK) return rc;
    const int64_t nb = (c.M + 4095) / 4096;
    const size_t ents = (size_t)(2 * nb * k);
    if ((rc = grow(c, c.d_topv, ents * sizeof(double), "hipMalloc topk values")) != TGP_OK) return rc;
    if ((rc = grow(c, c.d_topi, ents * sizeof(long long), "hipMalloc topk indices")) != TGP_OK) return rc;
    // (round 6) small and one-launch models: a polled call -- the top-k's final pass leaves values, indices and the clamp
    // count in mapped host memory, hands the counters back at zero and rings; no D2H copy, memset, event or synchronisation.
    // (The one question about the kernel family: that final pass is only wired up behind the two f64 families.)
    CallClock clk;
    if (sweep_path(c, c.M) != SweepPath::General) {
        clk.bell = bell_next(c);
        if (clk.bell.word && (rc = ensure_pinned(c, 0, (size_t)(8 + 2 * k + 1) * sizeof(double))) != TGP_OK) return rc;
    }
    const bool polled = clk.bell.word != nullptr;
    SweepCall s;      // (no record, no bell: the top-k pass behind it ends the call)
    s.acq = acq; s.sf = sf; s.incumbent = incumbent; s.param = param;
    s.acqv = c.d_acq;
    s.winner = c.d_winner;
    if ((rc = run_sweep(c, s, clk)) != TGP_OK) return rc;
    long off = 0;
    hipError_t le = launch_topk(c, c.d_acq, (long)c.M, (int)k, c.d_topv, c.d_topi, &off, polled ? c.h_pin_out.dev() + 8 : nullptr, clk.bell);
    if (le != hipSuccess) return hip_fail(c, le, "launch_topk");
    long long hi[64], bi[2] = {0, 0};
    if (!polled) {
        API_HIP(hipMemcpyAsync(vals, c.d_topv + off, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H topk values");
        API_HIP(hipMemcpyAsync(hi, c.d_topi + off, (size_t)k * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H topk indices");
        API_HIP(hipMemcpyAsync(bi, c.d_besti, 2 * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H besti");
        API_HIP(hipMemsetAsync(c.d_besti, 0, 4 * sizeof(long long), c.stream), "memset counters");
    }
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "topk sync")) != TGP_OK) return rc;
    if (c.profiling) prof_collect(c);
    if (polled) {
        const double *rec = c.h_pin_out + 8;
        for (int64_t i = 0; i < k; ++i) { vals[i] = rec[i]; idxs[i] = (int64_t)rec[k + i]; }     // (-1: fewer than k candidates)
        if (n_clamped) *n_clamped = (int64_t)rec[2 * k];
        return TGP_OK;
    }
    for (int64_t i = 0; i < k; ++i) idxs[i] = (hi[i] == 0x7fffffffffffffffLL) ? -1 : (int64_t)hi[i];   // -1: fewer than k candidates
    if (n_clamped) *n_clamped = (int64_t)bi[1];
    return TGP_OK;
} TGP_CATCH

}  // extern "C"
#include "api_optimise.hpp"
extern "C" {

int tgp_acq_refine(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi,
                   int acq, double sf, double incumbent, double param, int64_t max_iter,
                   double *x_out, double *val_out, int64_t *status_out, int64_t *iterations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_acq_refine");
    Context &c = h->c;
    const RefineArgs a{X0, R, lo, hi, acq, sf, incumbent, param, max_iter};
    const RefineOut out{x_out, val_out, status_out, iterations};
    if (int rc = check_refine_args(c, "tgp_acq_refine", a, out, TGP_ACQ_SIGMA); rc != TGP_OK) return rc;
    return acq_refine(c, a, out);
} TGP_CATCH

int tgp_acq_lbfgsb(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi,
                   int acq, double sf, double incumbent, double param, int64_t max_iter,
                   double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_acq_lbfgsb");
    Context &c = h->c;
    const RefineArgs a{X0, R, lo, hi, acq, sf, incumbent, param, max_iter};
    const RefineOut out{x_out, val_out, status_out, evaluations};
    if (int rc = check_refine_args(c, "tgp_acq_lbfgsb", a, out, TGP_ACQ_MES); rc != TGP_OK) return rc;
    return acq_lbfgsb_lockstep(h, a, out, [&](const double *Xq, int64_t m, double *val, double *grad) {
        return tgp_acq_grad(h, Xq, m, a.acq, a.sf, a.incumbent, a.param, val, grad);
    });
} TGP_CATCH

int tgp_fit_lbfgsb(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                   const double *theta0, int64_t S, int64_t n_ls, const double *log_lo, const double *log_hi,
                   double jitter, int normalize_y, int64_t max_iter, double *theta_out, double *f_out,
                   int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_lbfgsb");
    Context &c = h->c;
    const HyperOptArgs a{X, N, D, y, kernel, theta0, S, n_ls, log_lo, log_hi, jitter, normalize_y, max_iter};
    const HyperOptOut out{theta_out, f_out, status_out, evaluations};
    if (int rc = check_optimise_args(c, "tgp_fit_lbfgsb", a, out); rc != TGP_OK) return rc;
    return fit_lbfgsb(h, a, out);
} TGP_CATCH

int tgp_fit_optimise(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                     const double *theta0, int64_t S, int64_t n_ls, const double *log_lo, const double *log_hi,
                     double jitter, int normalize_y, int64_t max_iter, double *theta_out, double *f_out,
                     int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_optimise");
    Context &c = h->c;
    const HyperOptArgs a{X, N, D, y, kernel, theta0, S, n_ls, log_lo, log_hi, jitter, normalize_y, max_iter};
    const HyperOptOut out{theta_out, f_out, status_out, evaluations};
    if (int rc = check_optimise_args(c, "tgp_fit_optimise", a, out); rc != TGP_OK) return rc;
    return fit_optimise(h, a, out);
} TGP_CATCH

}  // extern "C"
#include "api_warp.hpp"
extern "C" {

// ---- learned input warping (include/turbogp.h; api_warp.hpp, warp_kernels.hip) -------------------------------------
int tgp_fit_input_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                       double constant, const double *ls, int64_t n_ls, double noise, double jitter,
                       int normalize_y, double *lml, double *y_mean, double *y_std, double *grad, double *dX) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_input_grad");
    Context &c = h->c;
    if (!grad) return fail(c, TGP_BAD_ARG, "tgp_fit_input_grad: grad is NULL");
    return fit_input_grad(h, FitArgs{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y}, FitOut{lml, y_mean, y_std}, grad, dX, false);
} TGP_CATCH

int tgp_warp_points(tgp_handle h, const double *X, int64_t m, int64_t D, const double *lo, const double *hi, const double *a,
                    const double *b, double *w_out, double *dw_du, double *dw_da, double *dw_db) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return tgp_host::warp_points(h->host->err, X, m, D, lo, hi, a, b, w_out, dw_du, dw_da, dw_db);
    Context &c = h->c;
    if (!X || !w_out || m < 1) return fail(c, TGP_BAD_ARG, "tgp_warp_points: need X, w_out and m >= 1");
    const WarpBox w{D, lo, hi, a, b};
    if (int rc = check_warp_box(c, "tgp_warp_points", w); rc != TGP_OK) return rc;
    return warp_points_device(c, X, m, w, w_out, dw_du, dw_da, dw_db);
} TGP_CATCH

int tgp_warp_inverse(tgp_handle h, const double *W, int64_t m, int64_t D, const double *lo, const double *hi, const double *a,
                     const double *b, double *x_out) try {
    if (!h) return TGP_BAD_ARG;
    return tgp_host::warp_inverse(h->host ? h->host->err : h->c.err, W, m, D, lo, hi, a, b, x_out);
} TGP_CATCH

int tgp_warp_candidates(tgp_handle h, const double *lo, const double *hi, const double *a, const double *b) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_warp_candidates");
    Context &c = h->c;
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_warp_candidates: no resident candidates");
    const WarpBox w{c.D, lo, hi, a, b};
    if (int rc = check_warp_box(c, "tgp_warp_candidates", w); rc != TGP_OK) return rc;
    return warp_resident(c, w);
} TGP_CATCH

int tgp_warp_read_raw(tgp_handle h, int64_t first, int64_t count, double *out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_warp_read_raw");
    Context &c = h->c;
    if (!warp_in_force(c)) return fail(c, TGP_BAD_ARG, "tgp_warp_read_raw: the resident batch is not a warped one (tgp_warp_candidates)");
    if (!out || first < 0 || count < 1 || first + count > c.M) return fail(c, TGP_BAD_ARG, "tgp_warp_read_raw: bad range");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(hipMemcpy(out, c.d_wraw + first * c.D, (size_t)(count * c.D) * sizeof(double), hipMemcpyDeviceToHost), "D2H raw candidates");
    return TGP_OK;
} TGP_CATCH

int tgp_fit_warp_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                      double constant, const double *ls, int64_t n_ls, double noise, double jitter, int normalize_y,
                      const double *lo, const double *hi, const double *a, const double *b,
                      double *lml, double *y_mean, double *y_std, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_warp_grad");
    Context &c = h->c;
    if (!grad) return fail(c, TGP_BAD_ARG, "tgp_fit_warp_grad: grad is NULL");
    return fit_warp_grad(h, FitArgs{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y}, WarpBox{D, lo, hi, a, b},
                         FitOut{lml, y_mean, y_std}, grad);
} TGP_CATCH

int tgp_fit_warp_lbfgsb(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                        const double *lo, const double *hi, const double *theta0, int64_t S, int64_t n_ls,
                        const double *log_lo, const double *log_hi, double prior_sigma, double jitter, int normalize_y,
                        int64_t max_iter, double *theta_out, double *f_out, int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_fit_warp_lbfgsb");
    Context &c = h->c;
    const HyperOptArgs a{X, N, D, y, kernel, theta0, S, n_ls, log_lo, log_hi, jitter, normalize_y, max_iter};
    const HyperOptOut out{theta_out, f_out, status_out, evaluations};
    if (int rc = check_optimise_args(c, "tgp_fit_warp_lbfgsb", a, out); rc != TGP_OK) return rc;
    bool ok = lo && hi && prior_sigma >= 0.0 && isfinite(prior_sigma);
    for (int64_t d = 0; ok && d < D; ++d) ok = warp_params_ok(lo[d], hi[d], 1.0, 1.0);
    for (int64_t i = 2 + n_ls; ok && i < 2 + n_ls + 2 * D; ++i) ok = log_lo[i] <= log_hi[i] && isfinite(log_lo[i]) && isfinite(log_hi[i]);
    for (int64_t s = 0; ok && s < S; ++s)      // (check_optimise_args knows 2 + n_ls entries; a NaN warp start is not left to the clip)
        for (int64_t i = 2 + n_ls; ok && i < 2 + n_ls + 2 * D; ++i) ok = isfinite(theta0[s * (2 + n_ls + 2 * D) + i]);
    if (!ok) return fail(c, TGP_BAD_ARG, "tgp_fit_warp_lbfgsb: need lo, hi with hi > lo (finite), prior_sigma >= 0, finite bounds lo <= hi for the 2 D warp entries and finite warp entries in theta0");
    return warp_optimise_streams(h, a, WarpOptArgs{lo, hi, prior_sigma}, out);
} TGP_CATCH

// ---- marginalised hyper-parameters: the slice sampler and the integrated sweep ------------------------------------
int tgp_hyper_sample(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel, const double *theta0,
                     int64_t n_ls, const double *log_lo, const double *log_hi, double jitter, int normalize_y, int64_t S,
                     int64_t burn, int64_t thin, const double *width, uint64_t seed, double *theta_out, double *lml_out,
                     int64_t *evaluations, int64_t *not_pd) try {
    if (!h) return TGP_BAD_ARG;
    // every evaluation is the handle's own tgp_fit, taken for its LML: whichever fit path N selects, or the host backend
    auto fit = [&](double constant, const double *ls, double noise, double *lml) {
        return fit_entry(h, FitArgs{X, N, D, y, kernel, constant, ls, n_ls, noise, jitter, normalize_y}, FitOut{lml, nullptr, nullptr});
    };
    return hyper_sample(fit, h->host ? h->host->err : h->c.err, X, N, D, y, kernel, theta0, n_ls, log_lo, log_hi, jitter, S, burn,
                        thin, width, seed, theta_out, lml_out, evaluations, not_pd);
} TGP_CATCH

int tgp_sweep_integrated(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                         const double *thetas, int64_t S, int64_t n_ls, double jitter, int normalize_y, int acq, double sf,
                         double incumbent, double param, double *mu, double *sigma, double *acq_out, double *best_val,
                         int64_t *best_idx, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_integrated");
    Context &c = h->c;
    if (!X || !y || !thetas) return fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: X, y and thetas must not be NULL");
    if (S < 1 || S > 64) return fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: 1 <= S <= 64 samples");
    if (D < 1 || (n_ls != 1 && n_ls != D)) return fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: n_ls must be 1 or D");
    if (acq == TGP_ACQ_MES)
        return fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: TGP_ACQ_MES is not integrated (its maxima belong to one fit)");
    if (int arc = acq_check(c, "tgp_sweep_integrated", acq, TGP_ACQ_SIGMA, sf); arc != TGP_OK) return arc;
    if (!c.d_cand || c.M < 1 || c.D != D)
        return fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: no candidates set for this D (tgp_set_candidates* after a fit with the same D)");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    SweepCall acc;                        // the acquisition's parameters, for the accumulation and the final kernel
    acc.acq = acq; acc.sf = sf; acc.incumbent = incumbent; acc.param = param;
    bool swept = false;
    // a failure between the first sweep and the final kernel leaves the samples' clamp counts in the counter: hand it
    // back at zero, as every sweep does
    auto bail = [&](int rc) {
        if (swept) {
            (void)hipMemsetAsync(c.d_besti + 1, 0, sizeof(long long), c.stream);
            (void)hipStreamSynchronize(c.stream);
            (void)hipGetLastError();
        }
        return rc;
    };
    std::vector<double> ls((size_t)n_ls);
    const int64_t P = 2 + n_ls;
    for (int64_t k = 0; k < S; ++k) {
        double constant, noise;
        slice_unpack(thetas + k * P, n_ls, constant, ls.data(), noise);
        int rc = fit_impl(h, FitArgs{X, N, D, y, kernel, constant, ls.data(), n_ls, noise, jitter, normalize_y}, FitOut{}, true);
        if (rc != TGP_OK) {
            const std::string why = c.err;
            return bail(fail(c, rc, "tgp_sweep_integrated: sample " + std::to_string((long long)k) + ": " + why));
        }
        if (!c.d_cand || c.M < 1) return bail(fail(c, TGP_BAD_ARG, "tgp_sweep_integrated: the candidates were dropped"));
        {   // (a front this fit started under tgp_set_overlap is joined and not used: the sweep below wants outputs)
            const hipError_t e = pre_join(c);
            if (e != hipSuccess) return bail(hip_fail(c, e, "hipStreamWaitEvent"));
        }
        if ((rc = ensure_outputs(c, true, true, acq_out != nullptr)) != TGP_OK) return bail(rc);
        if (k == 0) {
            const size_t bytes = (size_t)c.M * sizeof(double);
            if ((rc = grow(c, c.d_int_a, bytes, "hipMalloc integrated acq")) != TGP_OK) return bail(rc);
            if ((rc = grow(c, c.d_int_mu, bytes, "hipMalloc integrated mu")) != TGP_OK) return bail(rc);
            if ((rc = grow(c, c.d_int_m2, bytes, "hipMalloc integrated m2")) != TGP_OK) return bail(rc);
        }
        // the unpruned predict-only sweep of this sample, in the handle's arithmetic: no record, no winner, no bell --
        // the clamp counter keeps adding up over the samples
        SweepCall s;
        s.mu = c.d_mu; s.sigma = c.d_sigma;
        CallClock clk;
        swept = true;
        if ((rc = run_sweep(c, s, clk)) != TGP_OK) return bail(rc);
        const hipError_t le = launch_integrate_accumulate(c, acc, (int)k);
        if (le != hipSuccess) return bail(hip_fail(c, le, "launch_integrate_accumulate"));
    }
    const bool zc = tuning().sweep_zc != 0;
    int rc;
    if (zc && (rc = ensure_pinned(c, 0, 8 * sizeof(double))) != TGP_OK) return bail(rc);
    acc.mu = mu ? c.d_mu.get() : nullptr; acc.sigma = sigma ? c.d_sigma.get() : nullptr; acc.acqv = acq_out ? c.d_acq.get() : nullptr;
    acc.winner = c.d_winner;
    acc.res = zc ? c.h_pin_out.dev() : nullptr;
    {
        const hipError_t le = launch_integrate_final(c, acc, (int)S);
        if (le != hipSuccess) return bail(hip_fail(c, le, "launch_integrate_final"));
    }
    if ((rc = winner_mark(c, acc)) != TGP_OK) return rc;
    // (the call keeps no clock: no ev1, one plain synchronisation)
    SweepRecord rec;
    if ((rc = sweep_queue_return(c, zc, acq, rec, nullptr, mu, sigma, acq_out)) != TGP_OK) return rc;
    API_HIP(hipStreamSynchronize(c.stream), "integrated sweep sync");
    sweep_read_record(c, zc, acq, rec, best_val, best_idx, n_clamped);
    return TGP_OK;
} TGP_CATCH

// ---- constrained and cost-aware acquisition (include/turbogp.h; weight_kernels.hip) -------------------------------
// the checks the three entries share, in the order they report; a side's index is named
static int weighted_check(tgp_handle h, const char *fn, const tgp_side *sides, int64_t K, int acq, double sf) {
    Context &c = h->c;
    const std::string f = std::string(fn) + ": ";
    if (K < 0 || K > WT_MAX_SIDES) return fail(c, TGP_BAD_ARG, f + "need 0 <= K <= 8 sides");
    if (K > 0 && !sides) return fail(c, TGP_BAD_ARG, f + "sides is NULL with K > 0");
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, f + "no fitted model");
    if (acq != TGP_ACQ_NONE && acq != TGP_ACQ_PI && acq != TGP_ACQ_EI)
        return fail(c, TGP_BAD_ARG, f + "the acquisition must be TGP_ACQ_EI, TGP_ACQ_PI or TGP_ACQ_NONE (a weight on a signed or entropy-valued acquisition has no meaning)");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, f + "sf must be +1 or -1");
    for (int64_t k = 0; k < K; ++k) {
        const std::string sk = f + "side " + std::to_string((long long)k) + ": ";
        const tgp_side &s = sides[k];
        if (!s.g) return fail(c, TGP_BAD_ARG, sk + "the handle is NULL");
        if (s.g->host) return fail(c, TGP_BAD_ARG, sk + "a TGP_DEVICE_HOST handle cannot be a side");
        if (s.g == h) return fail(c, TGP_BAD_ARG, sk + "the objective's own handle cannot be a side");
        for (int64_t j = 0; j < k; ++j)
            if (sides[j].g == s.g) return fail(c, TGP_BAD_ARG, sk + "the same handle as side " + std::to_string((long long)j));
        if (s.kind != TGP_SIDE_GE && s.kind != TGP_SIDE_LE && s.kind != TGP_SIDE_COST) return fail(c, TGP_BAD_ARG, sk + "unknown kind");
        if (!std::isfinite(s.level)) return fail(c, TGP_BAD_ARG, sk + "the level must be finite");
        if (s.kind == TGP_SIDE_COST && s.level != 0.0) return fail(c, TGP_BAD_ARG, sk + "a cost side's level must be 0");
        const Context &g = s.g->c;
        if (!g.fitted) return fail(c, TGP_NOT_FITTED, sk + "no fitted model");
        if (g.device != c.device) return fail(c, TGP_BAD_ARG, sk + "the handle is on another device");
        if (g.D != c.D) return fail(c, TGP_BAD_ARG, sk + "D differs from the objective's");
    }
    return TGP_OK;
}

// a side's stream is ordered in front of the objective's by an event (nothing to do where both use the device's shared
// main stream: one queue, in order)
static int weighted_join(Context &c, Context &g, Ev &ev) {
    if (g.stream == c.stream) return TGP_OK;
    API_HIP(ev.create(hipEventDisableTiming), "hipEventCreate");
    API_HIP(hipEventRecord(ev, g.stream), "hipEventRecord");
    API_HIP(hipStreamWaitEvent(c.stream, ev, 0), "hipStreamWaitEvent");
    return TGP_OK;
}

int tgp_sweep_weighted(tgp_handle h, const tgp_side *sides, int64_t K, int acq, double sf, double incumbent, double param,
                       double *mu, double *sigma, double *acq_out, double *logw_out, double *value_out, double *side_mu,
                       double *side_sigma, double *best_val, int64_t *best_idx, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_weighted");
    Context &c = h->c;
    if (int rc = weighted_check(h, "tgp_sweep_weighted", sides, K, acq, sf); rc != TGP_OK) return rc;
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_sweep_weighted: no candidates set");
    if (warp_in_force(c))
        return fail(c, TGP_BAD_ARG, "tgp_sweep_weighted: the resident batch is a warped one (tgp_warp_candidates): each model would need its own warp");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t M = c.M, D = c.D;
    const size_t mb = (size_t)M * sizeof(double);
    int rc = ensure_outputs(c, true, true, true);
    if (rc != TGP_OK) return rc;
    API_MEM(grow(c, c.d_wt_logw, mb, "hipMalloc weighted logw"));
    API_MEM(grow(c, c.d_wt_val, mb, "hipMalloc weighted value"));
    if (side_mu && K > 0) API_MEM(grow(c, c.d_wt_smu, (size_t)K * mb, "hipMalloc weighted side mu"));
    if (side_sigma && K > 0) API_MEM(grow(c, c.d_wt_ssg, (size_t)K * mb, "hipMalloc weighted side sigma"));
    if (c.ev_wt.size() < (size_t)K) c.ev_wt.resize((size_t)K);
    // a failure between the first sweep and the final kernel leaves clamp counts in the counters of the handles swept so
    // far: they are handed back at zero, as every sweep does
    std::vector<Context *> swept;
    auto bail = [&](int code) {
        for (Context *g : swept) {
            (void)hipMemsetAsync(g->d_besti + 1, 0, sizeof(long long), g->stream);
            (void)hipStreamSynchronize(g->stream);
        }
        // (the accumulation behind every side's sweep has moved that side's count into the objective's counter)
        (void)hipMemsetAsync(c.d_besti + 1, 0, sizeof(long long), c.stream);
        (void)hipStreamSynchronize(c.stream);
        (void)hipGetLastError();
        return code;
    };
    auto side_fail = [&](int64_t k, int code, const Context &g) {
        const std::string why = g.err;
        return bail(fail(c, code, "tgp_sweep_weighted: side " + std::to_string((long long)k) + ": " + why));
    };
    for (int64_t k = 0; k < K; ++k) {
        Context &g = sides[k].g->c;
        // the side's batch becomes its OWN device-to-device copy of the objective's rows -- what tgp_set_candidates with
        // those rows leaves: a front is dropped, a borrowed buffer is released (never written), a warped batch is gone
        if (const hipError_t e = pre_join(g); e != hipSuccess) { (void)hip_fail(g, e, "hipStreamWaitEvent"); return side_fail(k, TGP_HIP_ERROR, g); }
        if ((rc = grow_candidates(g, M * D)) != TGP_OK) return side_fail(k, rc, g);
        if (const hipError_t e = hipMemcpyAsync(g.d_cand_owned, c.d_cand, (size_t)(M * D) * sizeof(double), hipMemcpyDeviceToDevice, g.stream);
            e != hipSuccess) { (void)hip_fail(g, e, "D2D candidates"); return side_fail(k, TGP_HIP_ERROR, g); }
        g.d_cand = g.d_cand_owned;
        g.M = M;
        if ((rc = ensure_outputs(g, true, true, false)) != TGP_OK) return side_fail(k, rc, g);
        // its unpruned predict-only sweep, in its own arithmetic and on its own stream: no record, no winner, no bell
        SweepCall s;
        s.mu = g.d_mu; s.sigma = g.d_sigma;
        CallClock clk;
        swept.push_back(&g);
        if ((rc = run_sweep(g, s, clk)) != TGP_OK) return side_fail(k, rc, g);
        if ((rc = weighted_join(c, g, c.ev_wt[(size_t)k])) != TGP_OK) return bail(rc);
        const hipError_t le = launch_weight_accumulate(c, g, (int)k, sides[k].kind, sides[k].level, c.d_wt_logw,
                                                       side_mu ? c.d_wt_smu + k * M : nullptr, side_sigma ? c.d_wt_ssg + k * M : nullptr);
        if (le != hipSuccess) return bail(hip_fail(c, le, "launch_weight_accumulate"));
    }
    // the objective's unpruned predict-only sweep (the pruned sweep's bounds belong to the unweighted arg-max), the value
    // and the shared arg-max, record and winner record
    swept.push_back(&c);
    {
        SweepCall s;
        s.mu = c.d_mu; s.sigma = c.d_sigma;
        CallClock clk;
        if ((rc = run_sweep(c, s, clk)) != TGP_OK) return bail(rc);
    }
    SweepCall w;
    w.acq = acq; w.sf = sf; w.incumbent = incumbent; w.param = param;
    if (const hipError_t le = launch_weight_value(c, w, (int)K, c.d_wt_logw, c.d_wt_val); le != hipSuccess)
        return bail(hip_fail(c, le, "launch_weight_value"));
    SweepCall fin;
    fin.acq = TGP_ACQ_EI;                 // (any acquisition: the final kernel only asks whether there is one)
    fin.winner = c.d_winner;
    const bool zc = tuning().sweep_zc != 0;
    if (zc && (rc = ensure_pinned(c, 0, 8 * sizeof(double))) != TGP_OK) return bail(rc);
    fin.res = zc ? c.h_pin_out.dev() : nullptr;
    if (const hipError_t le = launch_argmax_of(c, fin, c.d_wt_val); le != hipSuccess) return bail(hip_fail(c, le, "launch_argmax_of"));
    if ((rc = winner_mark(c, fin)) != TGP_OK) return rc;
    SweepRecord rec;
    if ((rc = sweep_queue_return(c, zc, fin.acq, rec, nullptr, mu, sigma, acq_out)) != TGP_OK) return rc;
    if (logw_out) API_HIP(hipMemcpyAsync(logw_out, c.d_wt_logw, mb, hipMemcpyDeviceToHost, c.stream), "D2H logw");
    if (value_out) API_HIP(hipMemcpyAsync(value_out, c.d_wt_val, mb, hipMemcpyDeviceToHost, c.stream), "D2H value");
    if (side_mu && K > 0) API_HIP(hipMemcpyAsync(side_mu, c.d_wt_smu, (size_t)K * mb, hipMemcpyDeviceToHost, c.stream), "D2H side mu");
    if (side_sigma && K > 0) API_HIP(hipMemcpyAsync(side_sigma, c.d_wt_ssg, (size_t)K * mb, hipMemcpyDeviceToHost, c.stream), "D2H side sigma");
    API_HIP(hipStreamSynchronize(c.stream), "weighted sweep sync");     // the one wait: every side's stream is ordered in front of it
    sweep_read_record(c, zc, fin.acq, rec, best_val, best_idx, n_clamped);
    return TGP_OK;
} TGP_CATCH

static int kg_grad_sweep_posterior(Context &c, const double *d_Xq, int64_t m, double *d_mu, double *d_sigma);

// the VALUES of a model's posterior at the query points: its own unpruned predict-only sweep of them where that sweep runs
// in f64 (every f64 handle, and the one-workgroup / one-launch kernels of any handle), so that val is, for such handles,
// what tgp_sweep_weighted returns for the same rows; an f32 sweep is not used (the query sums' f64 posterior stands)
static bool weighted_sweep_is_f64(const Context &c, int64_t m) { return sweep_path(c, m) != SweepPath::General || c.dtype == TGP_F64; }

int tgp_weighted_grad(tgp_handle h, const tgp_side *sides, int64_t K, const double *Xq, int64_t m, int acq, double sf,
                      double incumbent, double param, double *val, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_weighted_grad");
    Context &c = h->c;
    if (int rc = weighted_check(h, "tgp_weighted_grad", sides, K, acq, sf); rc != TGP_OK) return rc;
    if (!Xq || !val || !grad || m < 1 || m > 4096) return fail(c, TGP_BAD_ARG, "tgp_weighted_grad: need Xq, val, grad and 1 <= m <= 4096");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t D = c.D;
    API_MEM(grow(c, c.d_wt_q, (size_t)(2 * m * D + m + 2 * (K + 1) * m) * sizeof(double), "hipMalloc weighted query"));
    API_MEM(grow(c, c.d_qws, query_ws(c, (int)m).bytes, "hipMalloc query workspace"));
    if (c.ev_wt.size() < (size_t)K) c.ev_wt.resize((size_t)K);
    double *d_Xq = c.d_wt_q, *d_val = d_Xq + m * D, *d_grad = d_val + m, *d_mu = d_grad + m * D, *d_sg = d_mu + (K + 1) * m;
    API_HIP(hipMemcpyAsync(d_Xq, Xq, (size_t)(m * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    bool in_marked = false;
    WtGrad w{};
    w.K = (int)K; w.m = (int)m; w.D = (int)D; w.acq = acq; w.sf = sf; w.incumbent = incumbent; w.param = param;
    w.val = d_val; w.grad = d_grad;
    // every model's sums [k.alpha, v.v, gm, gv] per point from the query kernels behind tgp_acq_grad, each on its handle's
    // stream and in its handle's workspace; the combination reads them all on the objective's
    {
        const QueryWs q = query_ws(c, (int)m);
        const hipError_t le = launch_query(c, d_Xq, (int)m, TGP_ACQ_NONE, sf, 0.0, 0.0, q.ws, nullptr, nullptr);
        if (le != hipSuccess) return hip_fail(c, le, "launch_query");
        const bool own = weighted_sweep_is_f64(c, m);
        if (own)
            if (int rc = kg_grad_sweep_posterior(c, d_Xq, m, d_mu, d_sg); rc != TGP_OK) return rc;
        w.mdl[0] = WtModel{q.red, c.d_ls, c.constant + c.noise, c.y_mean, c.y_std, 0.0, 0, own ? d_mu : nullptr, own ? d_sg : nullptr};
    }
    for (int64_t k = 0; k < K; ++k) {
        Context &g = sides[k].g->c;
        auto side_fail = [&](int code) {
            const std::string why = g.err;
            (void)hipStreamSynchronize(c.stream);
            (void)hipStreamSynchronize(g.stream);
            (void)hipGetLastError();
            return fail(c, code, "tgp_weighted_grad: side " + std::to_string((long long)k) + ": " + why);
        };
        if (const hipError_t e = pre_join(g); e != hipSuccess) { (void)hip_fail(g, e, "hipStreamWaitEvent"); return side_fail(TGP_HIP_ERROR); }
        if (const int rc = grow(g, g.d_qws, query_ws(g, (int)m).bytes, "hipMalloc query workspace"); rc != TGP_OK) return side_fail(rc);
        if (g.stream != c.stream) {          // the points are on the device before a private stream reads them
            if (!in_marked) {
                API_HIP(c.ev_wt_in.create(hipEventDisableTiming), "hipEventCreate");
                API_HIP(hipEventRecord(c.ev_wt_in, c.stream), "hipEventRecord");
                in_marked = true;
            }
            API_HIP(hipStreamWaitEvent(g.stream, c.ev_wt_in, 0), "hipStreamWaitEvent");
        }
        const QueryWs q = query_ws(g, (int)m);
        const hipError_t le = launch_query(g, d_Xq, (int)m, TGP_ACQ_NONE, sf, 0.0, 0.0, q.ws, nullptr, nullptr);
        if (le != hipSuccess) { (void)hip_fail(g, le, "launch_query"); return side_fail(TGP_HIP_ERROR); }
        const bool own = weighted_sweep_is_f64(g, m);
        if (own)
            if (const int rc = kg_grad_sweep_posterior(g, d_Xq, m, d_mu + (1 + k) * m, d_sg + (1 + k) * m); rc != TGP_OK) return side_fail(rc);
        if (const int rc = weighted_join(c, g, c.ev_wt[(size_t)k]); rc != TGP_OK) return rc;
        w.mdl[1 + k] = WtModel{q.red, g.d_ls, g.constant + g.noise, g.y_mean, g.y_std, sides[k].level, sides[k].kind,
                               own ? d_mu + (1 + k) * m : nullptr, own ? d_sg + (1 + k) * m : nullptr};
    }
    if (const hipError_t le = launch_weight_grad(c, w); le != hipSuccess) return hip_fail(c, le, "launch_weight_grad");
    API_HIP(hipMemcpyAsync(val, d_val, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H val");
    API_HIP(hipMemcpyAsync(grad, d_grad, (size_t)(m * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H grad");
    API_HIP(hipStreamSynchronize(c.stream), "weighted grad sync");
    return TGP_OK;
} TGP_CATCH

int tgp_weighted_lbfgsb(tgp_handle h, const tgp_side *sides, int64_t K, const double *X0, int64_t R, const double *lo,
                        const double *hi, int acq, double sf, double incumbent, double param, int64_t max_iter, double *x_out,
                        double *val_out, int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_weighted_lbfgsb");
    Context &c = h->c;
    const RefineArgs a{X0, R, lo, hi, acq, sf, incumbent, param, max_iter};
    const RefineOut out{x_out, val_out, status_out, evaluations};
    if (int rc = check_refine_args(c, "tgp_weighted_lbfgsb", a, out, TGP_ACQ_EI); rc != TGP_OK) return rc;
    if (int rc = weighted_check(h, "tgp_weighted_lbfgsb", sides, K, acq, sf); rc != TGP_OK) return rc;
    return acq_lbfgsb_lockstep(h, a, out, [&](const double *Xq, int64_t m, double *val, double *grad) {
        return tgp_weighted_grad(h, sides, K, Xq, m, a.acq, a.sf, a.incumbent, a.param, val, grad);
    });
} TGP_CATCH

}  // extern "C"
#include "api_ehvi.hpp"
extern "C" {

// ---- two-objective expected hypervolume improvement (include/turbogp.h; api_ehvi.hpp, ehvi_kernels.hip) ------------
int tgp_ehvi_set_front(tgp_handle h, const double *Y, int64_t n, double sf1, double sf2, const double *ref, int64_t *P_out,
                       double *front_out, double *hv_out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ehvi_set_front");
    return ehvi_set_front(h, Y, n, sf1, sf2, ref, P_out, front_out, hv_out);
} TGP_CATCH

int tgp_sweep_ehvi(tgp_handle h, tgp_handle g, double *mu, double *sigma, double *mu2, double *sigma2, double *ehvi_out,
                   double *best_val, int64_t *best_idx, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_ehvi");
    if (int rc = ehvi_check(h, g, "tgp_sweep_ehvi"); rc != TGP_OK) return rc;
    return ehvi_sweep(h, g, mu, sigma, mu2, sigma2, ehvi_out, best_val, best_idx, n_clamped);
} TGP_CATCH

int tgp_ehvi_grad(tgp_handle h, tgp_handle g, const double *Xq, int64_t m, double *val, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ehvi_grad");
    if (int rc = ehvi_check(h, g, "tgp_ehvi_grad"); rc != TGP_OK) return rc;
    return ehvi_grad(h, g, Xq, m, val, grad);
} TGP_CATCH

int tgp_ehvi_lbfgsb(tgp_handle h, tgp_handle g, const double *X0, int64_t R, const double *lo, const double *hi,
                    int64_t max_iter, double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_ehvi_lbfgsb");
    Context &c = h->c;
    const RefineArgs a{X0, R, lo, hi, TGP_ACQ_EI, 1.0, 0.0, 0.0, max_iter};
    const RefineOut out{x_out, val_out, status_out, evaluations};
    if (int rc = check_refine_args(c, "tgp_ehvi_lbfgsb", a, out, TGP_ACQ_EI); rc != TGP_OK) return rc;
    if (int rc = ehvi_check(h, g, "tgp_ehvi_lbfgsb"); rc != TGP_OK) return rc;
    return acq_lbfgsb_lockstep(h, a, out, [&](const double *Xq, int64_t m, double *val, double *grad) {
        return ehvi_grad(h, g, Xq, m, val, grad);
    });
} TGP_CATCH

// ---- the knowledge gradient over the resident batch (include/turbogp.h; kg_kernels.hip) ----
// candidates per chunk of tgp_sweep_kg: a cross-kernel slab of about 512 MiB, a multiple of 1024, at most 16384
// (TGP_CHUNK replaces it, as it does the sweep's); a batch that fits one chunk takes what it needs, in whole 128-tiles.
// The chunk is what fills the chip: the cross-covariance launches (rows / 128) (Apad / 128) workgroups, and at 128 MiB
// (4096 rows at Np = 4096: 32 or 64 workgroups on 256 CUs) C3's call spent 39 ms in its own kernels whatever A was.
static int64_t kg_chunk_rows(const Context &c) {
    int64_t chunk = (int64_t)((512ull << 20) / ((size_t)c.Np * sizeof(double)));
    chunk = std::min<int64_t>(std::max<int64_t>(1024, (chunk / 1024) * 1024), 16384);
    if (const long v = tuning_chunk_now(); v >= 1024) chunk = (v / 1024) * 1024;
    const int64_t mpad = (c.M + 127) / 128 * 128;
    return std::min(chunk, mpad);
}

int tgp_kg_set_points(tgp_handle h, const double *Xa, int64_t A, double *mu_out) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_kg_set_points");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_kg_set_points: no fitted model (the points belong to one fit)");
    if (!Xa || A < 1 || A > 256) return fail(c, TGP_BAD_ARG, "tgp_kg_set_points: need Xa and 1 <= A <= 256 points");
    for (int64_t e = 0; e < A * c.D; ++e)
        if (!std::isfinite(Xa[e])) return fail(c, TGP_BAD_ARG, "tgp_kg_set_points: Xa must be finite");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    c.kg_gen = -1;
    KgPoints p;
    const int64_t nd = kg_points_doubles(c, A, &p);
    API_MEM(grow(c, c.d_kgp, (size_t)nd * sizeof(double), "hipMalloc knowledge-gradient points"));
    API_HIP(hipMemcpyAsync(c.d_kgp + p.o_Xa, Xa, (size_t)(A * c.D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xa");
    hipError_t le = launch_kg_points(c, c.d_kgp, p);
    if (le != hipSuccess) return hip_fail(c, le, "launch_kg_points");
    if (mu_out) API_HIP(hipMemcpyAsync(mu_out, c.d_kgp + p.o_mu, (size_t)A * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H mu");
    API_HIP(hipStreamSynchronize(c.stream), "kg_set_points sync");
    c.kg_A = (int)A;
    c.kg_gen = c.fit_gen;
    return TGP_OK;
} TGP_CATCH

int tgp_sweep_kg(tgp_handle h, double sf, double *kg_out, double *mu, double *sigma, double *cov_out, double *best_val,
                 int64_t *best_idx, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_sweep_kg");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_sweep_kg: no fitted model");
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_sweep_kg: no candidates set");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, "tgp_sweep_kg: sf must be +1 or -1");
    if (c.kg_gen < 0 || c.kg_gen != c.fit_gen || c.kg_A < 1)
        return fail(c, TGP_BAD_ARG, "tgp_sweep_kg: needs discretisation points for the resident fit (tgp_kg_set_points after the last fit)");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    int rc = ensure_outputs(c, true, true, true);
    if (rc != TGP_OK) return rc;
    KgPoints p;
    (void)kg_points_doubles(c, c.kg_A, &p);
    const int64_t rows = kg_chunk_rows(c);
    KgChunk k;
    const int64_t nd = kg_chunk_doubles(c, rows, p.Apad, &k);
    API_MEM(grow(c, c.d_kgw, (size_t)nd * sizeof(double), "hipMalloc knowledge-gradient workspace"));
    const size_t nchunks = (size_t)((c.M + rows - 1) / rows);
    while (c.ev_kg.size() < 2 * nchunks) {
        Ev e;
        API_HIP(e.create(hipEventDefault), "hipEventCreate");
        c.ev_kg.push_back(std::move(e));
    }
    // step 1: the unpruned predict-only sweep in the handle's arithmetic: no record, no winner, no bell; its clamp
    // count stays in the counter for the final kernel
    SweepCall s;
    s.mu = c.d_mu; s.sigma = c.d_sigma;
    CallClock clk;
    if ((rc = run_sweep(c, s, clk)) != TGP_OK) return rc;
    // a failure from here on hands the clamp counter back at zero, as every sweep does
    auto bail = [&](int code) {
        (void)hipMemsetAsync(c.d_besti + 1, 0, sizeof(long long), c.stream);
        (void)hipStreamSynchronize(c.stream);
        (void)hipGetLastError();
        return code;
    };
    // steps 2 and 3, chunk by chunk in f64: the cross-covariance, then the envelope into c.d_acq.  Where the sweep ran in
    // the handle's f32 arithmetic the mean is re-formed in f64 from the chunk's cross-kernel (one more pass over a slab
    // that is there anyway) and replaces the sweep's in c.d_mu: the f32 mean was the larger half of kg_out's error
    const bool remean = c.last_sweep_f64 == 0;
    const size_t d8 = sizeof(double);
    for (size_t ch = 0; ch < nchunks; ++ch) {
        const int64_t i0 = (int64_t)ch * rows;
        const int m = (int)std::min<int64_t>(rows, c.M - i0);
        hipError_t e = hipEventRecord(c.ev_kg[2 * ch], c.stream);
        if (e == hipSuccess) e = launch_kg_chunk(c, c.d_kgw, k, c.d_kgp, p, i0, m, sf, c.d_acq, remean);
        if (e == hipSuccess) e = hipEventRecord(c.ev_kg[2 * ch + 1], c.stream);
        if (e == hipSuccess && cov_out)
            e = hipMemcpy2DAsync(cov_out + i0 * c.kg_A, (size_t)c.kg_A * d8, c.d_kgw + k.o_C, (size_t)p.Apad * d8, (size_t)c.kg_A * d8,
                                 (size_t)m, hipMemcpyDeviceToHost, c.stream);
        if (e != hipSuccess) return bail(hip_fail(c, e, "launch_kg_chunk"));
    }
    // step 4: the shared arg-max, record and winner record
    SweepCall fin;
    fin.acq = TGP_ACQ_EI;                 // (any acquisition: the final kernel only asks whether there is one)
    fin.winner = c.d_winner;
    const bool zc = tuning().sweep_zc != 0;
    if (zc && (rc = ensure_pinned(c, 0, 8 * sizeof(double))) != TGP_OK) return bail(rc);
    fin.res = zc ? c.h_pin_out.dev() : nullptr;
    {
        const hipError_t le = launch_argmax_of(c, fin, c.d_acq);
        if (le != hipSuccess) return bail(hip_fail(c, le, "launch_argmax_of"));
    }
    if ((rc = winner_mark(c, fin)) != TGP_OK) return rc;
    SweepRecord rec;
    if ((rc = sweep_queue_return(c, zc, fin.acq, rec, nullptr, mu, sigma, kg_out)) != TGP_OK) return rc;
    API_HIP(hipStreamSynchronize(c.stream), "kg sweep sync");
    sweep_read_record(c, zc, fin.acq, rec, best_val, best_idx, n_clamped);
    double total = 0.0;
    for (size_t ch = 0; ch < nchunks; ++ch) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c.ev_kg[2 * ch], c.ev_kg[2 * ch + 1]) == hipSuccess) total += ms;
        else (void)hipGetLastError();
    }
    c.last_kg_ms = total;
    return TGP_OK;
} TGP_CATCH

// The posterior tgp_sweep_kg's lines are formed from, for the m query points in the workspace: its step 1 -- the
// predict-only sweep -- with the points standing in for the resident batch, so that a point's mu and sigma (and with
// them its value) are the bits tgp_sweep_kg returns for it.  The handle's candidates, its sweep geometry and what the
// last sweep reported are put back; the clamp counter is handed back at zero.
static int kg_grad_sweep_posterior(Context &c, const double *d_Xq, int64_t m, double *d_mu, double *d_sigma) {
    struct Kept {
        Context &c;
        const double *cand; int64_t M, chunk, launch_rows, ws_Mpad, lbset, surv, screen;
        int f64, state, arith, spec;
        explicit Kept(Context &c_) : c(c_), cand(c_.d_cand), M(c_.M), chunk(c_.chunk), launch_rows(c_.launch_rows), ws_Mpad(c_.ws_Mpad),
                                     lbset(c_.prune_lbset), surv(c_.prune_surv), screen(c_.prune_screen),
                                     f64(c_.last_sweep_f64), state(c_.prune_state), arith(c_.prune_arith), spec(c_.prune_spec) {}
        ~Kept() {
            c.d_cand = cand; c.M = M; c.chunk = chunk; c.launch_rows = launch_rows; c.ws_Mpad = ws_Mpad;
            c.prune_lbset = lbset; c.prune_surv = surv; c.prune_screen = screen;
            c.last_sweep_f64 = f64; c.prune_state = state; c.prune_arith = arith; c.prune_spec = spec;
        }
    } kept(c);
    c.d_cand = d_Xq; c.M = m;
    SweepCall s;
    s.mu = d_mu; s.sigma = d_sigma;
    CallClock clk;
    const int rc = run_sweep(c, s, clk);
    (void)hipMemsetAsync(c.d_besti, 0, 4 * sizeof(long long), c.stream);   // zero between calls, as every sweep leaves them
    return rc;
}

int tgp_kg_grad(tgp_handle h, const double *Xq, int64_t m, double sf, double *val, double *grad) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_kg_grad");
    Context &c = h->c;
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, "tgp_kg_grad: no fitted model");
    if (!Xq || !val || !grad || m < 1 || m > 4096) return fail(c, TGP_BAD_ARG, "tgp_kg_grad: need Xq, val, grad and 1 <= m <= 4096");
    if (sf != 1.0 && sf != -1.0) return fail(c, TGP_BAD_ARG, "tgp_kg_grad: sf must be +1 or -1");
    if (c.kg_gen < 0 || c.kg_gen != c.fit_gen || c.kg_A < 1)
        return fail(c, TGP_BAD_ARG, "tgp_kg_grad: needs discretisation points for the resident fit (tgp_kg_set_points after the last fit)");
    for (int64_t e = 0; e < m * c.D; ++e)
        if (!std::isfinite(Xq[e])) return fail(c, TGP_BAD_ARG, "tgp_kg_grad: Xq must be finite");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    KgPoints p;
    (void)kg_points_doubles(c, c.kg_A, &p);
    KgGradWs g;
    const int64_t nd = kg_grad_doubles(c, m, p.Apad, &g);
    API_MEM(grow(c, c.d_kgw, (size_t)nd * sizeof(double), "hipMalloc knowledge-gradient workspace"));
    while (c.ev_kg.size() < 2) {
        Ev e;
        API_HIP(e.create(hipEventDefault), "hipEventCreate");
        c.ev_kg.push_back(std::move(e));
    }
    double *ws = c.d_kgw;
    API_HIP(hipMemcpyAsync(ws + g.o_Xq, Xq, (size_t)(m * c.D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    // the lines' posterior: the sweep's own where the sweep of these points runs in f64 (the value is then tgp_sweep_kg's,
    // bit for bit); else formed in f64 from the query front's vectors -- never the f32 sweep's
    const bool sweep_f64 = sweep_path(c, m) != SweepPath::General || c.dtype == TGP_F64;
    if (sweep_f64)
        if (int rc = kg_grad_sweep_posterior(c, ws + g.o_Xq, m, ws + g.o_mu, ws + g.o_sigma); rc != TGP_OK) return rc;
    API_HIP(hipEventRecord(c.ev_kg[0], c.stream), "hipEventRecord");
    if (hipError_t le = launch_kg_grad(c, ws, g, c.d_kgp, p, (int)m, sf, !sweep_f64); le != hipSuccess) return hip_fail(c, le, "launch_kg_grad");
    API_HIP(hipEventRecord(c.ev_kg[1], c.stream), "hipEventRecord");
    API_HIP(hipMemcpyAsync(val, ws + g.o_val, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H val");
    API_HIP(hipMemcpyAsync(grad, ws + g.o_grad, (size_t)(m * c.D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H grad");
    API_HIP(hipStreamSynchronize(c.stream), "kg grad sync");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c.ev_kg[0], c.ev_kg[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    c.last_kg_ms = ms;
    return TGP_OK;
} TGP_CATCH

int tgp_kg_lbfgsb(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi, double sf, int64_t max_iter,
                  double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_kg_lbfgsb");
    Context &c = h->c;
    const RefineArgs a{X0, R, lo, hi, TGP_ACQ_NONE, sf, 0.0, 0.0, max_iter};
    const RefineOut out{x_out, val_out, status_out, evaluations};
    if (int rc = check_refine_args(c, "tgp_kg_lbfgsb", a, out, TGP_ACQ_MES); rc != TGP_OK) return rc;
    if (c.kg_gen < 0 || c.kg_gen != c.fit_gen || c.kg_A < 1)
        return fail(c, TGP_BAD_ARG, "tgp_kg_lbfgsb: needs discretisation points for the resident fit (tgp_kg_set_points after the last fit)");
    return acq_lbfgsb_lockstep(h, a, out, [&](const double *Xq, int64_t m, double *val, double *grad) {
        return tgp_kg_grad(h, Xq, m, sf, val, grad);
    });
} TGP_CATCH

int tgp_evaluate(tgp_handle h, const double *Xc, int64_t M, int acq, double sf, double incumbent,
                 double param, double *mu, double *sigma, double *acq_out, double *best_val,
                 int64_t *best_idx, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) {
        const int rc = h->host->set_candidates(Xc, M);
        return rc != TGP_OK ? rc : h->host->sweep(acq, sf, incumbent, param, mu, sigma, acq_out, best_val, best_idx, n_clamped);
    }
    Context &c = h->c;
    if (int arc = acq_check_args(c, "tgp_evaluate", (!Xc || M < 1) ? "need Xc and M >= 1" : nullptr, acq, TGP_ACQ_MES, sf); arc != TGP_OK) return arc;
    const size_t in_bytes = (size_t)M * (size_t)c.D * sizeof(double);
    // (the one question about the kernel family: only the one-workgroup / one-launch kernels write their outputs straight
    // into mapped host memory)
    const bool zero_copy = sweep_path(c, M) != SweepPath::General && in_bytes <= ((size_t)8 << 20) && M <= 262144;
    if (!zero_copy) {
        int rc = tgp_set_candidates(h, Xc, M);
        if (rc != TGP_OK) return rc;
        return tgp_sweep(h, acq, sf, incumbent, param, mu, sigma, acq_out, best_val, best_idx, n_clamped);
    }
    // Small (N <= 128) or mid-size (N <= 256) model, small batch (the plot path: turbo/plotting/trials.py:371,448,574-577; 1-point
    // calls of a foreign optimiser): candidates and results travel through pinned, device-mapped
    // host memory -- two launches, one synchronisation, no memcpy call.
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    if (in_bytes > c.h_pin_cand.bytes()) {
        if (c.d_cand == c.h_pin_cand.dev()) { c.d_cand = nullptr; c.M = 0; }   // (as grow_candidates: forgotten before its buffer goes)
        API_MEM(ensure_pinned(c, c.h_pin_cand, in_bytes));
    }
    int rc = ensure_pinned(c, 0, (size_t)(8 + 3 * M) * sizeof(double));
    if (rc != TGP_OK) return rc;
    memcpy(c.h_pin_cand, Xc, in_bytes);
    c.d_cand = c.h_pin_cand.dev();        // resident (in host memory the GPU can read) until replaced
    c.M = M;
    // (round 6) a polled call.  N <= 128: the record's kernel is a launch of its own behind the sweep, so when it rings every
    // mean / deviation / acquisition value the sweep wrote into mapped host memory is out.  The one-launch sweep of
    // 128 < N <= 256: every workgroup's output stores come from the wave that takes its ticket behind a system-scope
    // fence, and the last workgroup rings
    SweepCall s;
    s.acq = acq; s.sf = sf; s.incumbent = incumbent; s.param = param;
    double *o_mu = c.h_pin_out.dev() + 8, *o_sg = o_mu + M, *o_aq = o_sg + M;
    s.mu = mu ? o_mu : nullptr; s.sigma = sigma ? o_sg : nullptr; s.acqv = acq_out ? o_aq : nullptr;
    s.res = c.h_pin_out.dev();
    s.winner = c.d_winner;
    s.bell = bell_next(c);
    CallClock clk{s.bell};
    if ((rc = run_sweep(c, s, clk)) != TGP_OK) return rc;
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "evaluate sync")) != TGP_OK) return rc;
    const double *res = c.h_pin_out;
    if (mu) memcpy(mu, res + 8, (size_t)M * sizeof(double));
    if (sigma) memcpy(sigma, res + 8 + M, (size_t)M * sizeof(double));
    if (acq_out) memcpy(acq_out, res + 8 + 2 * M, (size_t)M * sizeof(double));
    if (acq != TGP_ACQ_NONE) {
        if (best_val) *best_val = res[0];
        if (best_idx) *best_idx = (int64_t)res[1];
    }
    if (n_clamped) *n_clamped = (int64_t)res[2];
    return TGP_OK;
} TGP_CATCH

int tgp_predict_batch(tgp_handle h, int64_t T, const int64_t *Ns, int64_t D, const double *const *Xs,
                      const double *const *ys, int kernel, const double *constants, const double *ls,
                      const double *noises, const double *jitters, int normalize_y, const double *Xc,
                      int64_t M, double *mu, double *sigma, double *lml, int64_t *n_clamped) try {
    if (!h) return TGP_BAD_ARG;
    HOST_NA("tgp_predict_batch");
    Context &c = h->c;
    if (!Ns || !Xs || !ys || !constants || !ls || !noises || !jitters || !Xc || !mu)
        return fail(c, TGP_BAD_ARG, "tgp_predict_batch: NULL argument");
    if (T < 1 || T > 4096 || D < 1 || D > 4096 || M < 1)
        return fail(c, TGP_BAD_ARG, "tgp_predict_batch: need 1 <= T <= 4096, 1 <= D <= 4096, M >= 1");
    if (kernel < TGP_RBF || kernel > TGP_MATERN52) return fail(c, TGP_BAD_ARG, "tgp_predict_batch: unknown kernel");
    int64_t nmax = 0;
    for (int64_t t = 0; t < T; ++t) {
        if (Ns[t] < 1 || Ns[t] > 4 * NB) return fail(c, TGP_BAD_ARG, "tgp_predict_batch: every model needs 1 <= N <= 256 (use tgp_fit + tgp_evaluate per model beyond that)");
        nmax = std::max(nmax, Ns[t]);
        if (!Xs[t] || !ys[t]) return fail(c, TGP_BAD_ARG, "tgp_predict_batch: NULL model data");
        if (!(constants[t] > 0.0) || !(noises[t] >= 0.0) || !(jitters[t] >= 0.0)) return fail(c, TGP_BAD_ARG, "tgp_predict_batch: constant > 0, noise >= 0, jitter >= 0 required");
        for (int64_t d = 0; d < D; ++d)
            if (!(ls[t * D + d] > 0.0)) return fail(c, TGP_BAD_ARG, "tgp_predict_batch: length scales must be > 0");
    }
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    // models of up to 128 points: the small-problem kernels (leading dimension 128); a batch with a larger model:
    // the one-workgroup fit and the one-launch sweep of 128 < N <= 256 for every model of it (leading dimension 256)
    const bool mid = nmax > 2 * NB;
    const int64_t Dp = ((D + 3) / 4) * 4, NPB = mid ? 4 * NB : 2 * NB;
    const int64_t in_stride = NPB * Dp + NPB + D + (D & 1);                 // doubles per model in the pinned input
    const size_t fa = small_fit_args_bytes(), sa = small_sweep_args_bytes();
    const size_t args_off = (size_t)(T * in_stride) * sizeof(double);
    const size_t in_bytes = args_off + (size_t)T * (fa + sa) + 64;
    int rc = ensure_pinned(c, in_bytes, (size_t)(3 * T + 8) * sizeof(double));
    if (rc != TGP_OK) return rc;
    // device: per-model workspaces | counters (4 T long long) | mu (T M) | sigma (T M) | candidates (M D)
    const int64_t wsd = mid ? mid_batch_ws_doubles(D, Dp) : small_batch_ws_doubles(D, Dp);
    const size_t dev_need = (size_t)(T * wsd + 4 * T + 2 * T * M + M * D) * sizeof(double);
    if ((rc = grow(c, c.d_batch, dev_need, "hipMalloc batch workspace")) != TGP_OK) return rc;
    double *d_ws = c.d_batch;
    long long *d_cnt = reinterpret_cast<long long *>(d_ws + T * wsd);
    double *d_mu = d_ws + T * wsd + 4 * T, *d_sg = d_mu + T * M, *d_xc = d_sg + T * M;

    char *pin = reinterpret_cast<char *>(c.h_pin_in.get());
    char *pin_dev = reinterpret_cast<char *>(c.h_pin_in.dev());
    void *fit_args = pin + args_off, *sweep_args = pin + args_off + (size_t)T * fa;
    std::vector<double> ymean((size_t)T), ystd((size_t)T), yn((size_t)NPB);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t N = Ns[t];
        std::fill(yn.begin(), yn.end(), 0.0);
        normalise_targets(ys[t], N, normalize_y, yn, ymean[(size_t)t], ystd[(size_t)t]);
        pack_small_inputs(c.h_pin_in + t * in_stride, Xs[t], N, D, Dp, ls + t * D, yn.data());
        (mid ? fill_mid_batch_args : fill_small_batch_args)(
            fit_args, sweep_args, t, c.h_pin_in.dev() + t * in_stride, d_ws + t * wsd, c.h_pin_out.dev() + 8 + 3 * t, d_cnt + 4 * t,
            d_xc, d_mu + t * M, sigma ? d_sg + t * M : nullptr, N, D, Dp, M, constants[t], noises[t], jitters[t],
            ymean[(size_t)t], ystd[(size_t)t]);
    }
    CallClock clk;
    if ((rc = call_begin(c, clk)) != TGP_OK) return rc;
    API_HIP(hipMemsetAsync(d_cnt, 0, (size_t)(4 * T) * sizeof(long long), c.stream), "memset counters");
    API_HIP(hipMemcpyAsync(d_xc, Xc, (size_t)(M * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D points");
    hipError_t le = mid ? launch_mid_batch(c, kernel, pin_dev + args_off, pin_dev + args_off + (size_t)T * fa, T, M)
                        : launch_small_batch(c, kernel, pin_dev + args_off, pin_dev + args_off + (size_t)T * fa, T, M, true, true);
    if (le != hipSuccess) return hip_fail(c, le, "launch_small_batch");
    std::vector<long long> cnt((size_t)(4 * T));
    API_HIP(hipMemcpyAsync(mu, d_mu, (size_t)(T * M) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H mu");
    if (sigma) API_HIP(hipMemcpyAsync(sigma, d_sg, (size_t)(T * M) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H sigma");
    API_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)(4 * T) * sizeof(long long), hipMemcpyDeviceToHost, c.stream), "D2H counters");
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "batch sync")) != TGP_OK) return rc;
    int64_t clamped = 0;
    for (int64_t t = 0; t < T; ++t) {
        const double *res = c.h_pin_out + 8 + 3 * t;
        if (res[2] != 0.0) return not_pd(c, (int)res[2] - 1, Ns[t], "model " + std::to_string((long long)t) + " of the batch: ");
        if (lml) lml[t] = lml_from(res[0], res[1], Ns[t]);
        clamped += (int64_t)cnt[(size_t)(4 * t + 1)];
    }
    if (n_clamped) *n_clamped = clamped;
    return TGP_OK;
} TGP_CATCH

int tgp_predict(tgp_handle h, const double *Xc, int64_t M, double *mu, double *sigma) try {
    return tgp_evaluate(h, Xc, M, TGP_ACQ_NONE, 1.0, 0.0, 0.0, mu, sigma, nullptr, nullptr, nullptr, nullptr);
} TGP_CATCH

int tgp_profile_enable(tgp_handle h, int on) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return TGP_OK;
    h->c.profiling = on != 0;
    return TGP_OK;
} TGP_CATCH

int tgp_profile_reset(tgp_handle h) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) return TGP_OK;
    Context &c = h->c;
    prof_collect(c);
    c.trmm_launches = c.kstar_launches = 0;
    c.trmm_ms = c.kstar_ms = c.screen_ms = 0.0;
    c.trmm_flops = 0.0;
    return TGP_OK;
} TGP_CATCH

int tgp_profile_read(tgp_handle h, int64_t *trmm_launches, double *trmm_ms, int64_t *kstar_launches,
                     double *kstar_ms, double *last_fit_ms, double *last_sweep_ms) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) {
        if (trmm_launches) *trmm_launches = 0;
        if (trmm_ms) *trmm_ms = 0.0;
        if (kstar_launches) *kstar_launches = 0;
        if (kstar_ms) *kstar_ms = 0.0;
        if (last_fit_ms) *last_fit_ms = h->host->last_fit_ms;
        if (last_sweep_ms) *last_sweep_ms = h->host->last_sweep_ms;
        return TGP_OK;
    }
    Context &c = h->c;
    prof_collect(c);
    if (trmm_launches) *trmm_launches = c.trmm_launches;
    if (trmm_ms) *trmm_ms = c.trmm_ms;
    if (kstar_launches) *kstar_launches = c.kstar_launches;
    if (kstar_ms) *kstar_ms = c.kstar_ms;
    if (last_fit_ms) *last_fit_ms = c.last_fit_ms;
    if (last_sweep_ms) *last_sweep_ms = c.last_sweep_ms;
    return TGP_OK;
} TGP_CATCH

int tgp_last_timings(tgp_handle h, double *out, int64_t n) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) {
        if (!out || n < 1) { h->host->err = "tgp_last_timings: need out and n >= 1"; return TGP_BAD_ARG; }
        for (int64_t i = 0; i < n; ++i) out[i] = i == 0 ? h->host->last_fit_ms : (i == 1 ? h->host->last_sweep_ms : (i == 6 ? 1.0 : (i == 12 || i == 16 ? -1.0 : 0.0)));   // [6]: the host backend is float64 throughout; [12], [16]: it never prunes
        return TGP_OK;
    }
    Context &c = h->c;
    if (!out || n < 1) return fail(c, TGP_BAD_ARG, "tgp_last_timings: need out and n >= 1");
    // [6] (round 6): 1 when the last sweep ran in float64 whatever the handle's dtype (the small-problem / one-launch
    // kernels), 0 when it ran in the handle's arithmetic, -1 before the first sweep
    // [7..11] (round 6, a debugging aid): phase stamps of the last POLLED small fit in microseconds from the kernel's start --
    // inputs staged, first kernel-matrix tile in LDS, first block factored, fit done, call done (0 when the call was not polled)
    // [12..14]: what the last tgp_sweep did about pruning (sweep_pruned): -1 not eligible, -2 gated off, 0 pruned, 1 fell
    // back to every candidate; the candidates of its lb set; its survivors
    // [16]: the survivors of that sweep's screen (prune_screen.hpp), -1 when the screen did not apply; [17]: profiled time of
    // the screen's launches since tgp_profile_reset (ms; apart from the cross-kernel's and the contraction's); [18]: that
    // screen's arithmetic, 0 none, 1 f32, 2 fp16 planes (TGP_SCREEN_ARITH)
    // [19]: device time of the last tgp_loo's three kernels (ms; the copies back left out)
    // [20]: device time of the last tgp_sweep_kg's own kernels (ms; cross-covariance + envelope, the copies left out)
    // [21]: the speculative round of the last tgp_sweep's pruned schedule (TGP_PRUNE_SPEC): 0 not tried, 1 hit (the runner-ups
    // covered every survivor: one exact round), 2 miss (the survivors' round ran as well)
    double v[22] = {c.last_fit_ms, c.last_sweep_ms, c.last_grad_ms[0], c.last_grad_ms[1], c.last_grad_ms[2], c.trmm_flops,
                    (double)c.last_sweep_f64, 0.0, 0.0, 0.0, 0.0, 0.0, (double)c.prune_state, (double)c.prune_lbset,
                    (double)c.prune_surv, c.last_cov_ms, (double)c.prune_screen, c.screen_ms, (double)c.prune_arith, c.last_loo_ms, c.last_kg_ms,
                    (double)c.prune_spec};
    if (c.h_bell && c.h_bell[1]) {
        const unsigned long long t0 = c.h_bell[1];
        const int src[5] = {3, 4, 5, 6, 2};
        for (int k = 0; k < 5; ++k) v[7 + k] = c.h_bell[src[k]] >= t0 ? (double)(c.h_bell[src[k]] - t0) * 1e-2 : 0.0;
    }
    for (int64_t i = 0; i < n; ++i) out[i] = i < 22 ? v[i] : 0.0;
    return TGP_OK;
} TGP_CATCH

int tgp_sweep_geometry(tgp_handle h, int64_t *chunk, int64_t *n_padded) try {
    if (!h) return TGP_BAD_ARG;
    if (h->host) { if (chunk) *chunk = 16; if (n_padded) *n_padded = h->host->N; return TGP_OK; }
    if (chunk) *chunk = h->c.chunk;
    if (n_padded) *n_padded = h->c.Np;
    return TGP_OK;
} TGP_CATCH

}  // extern "C"
