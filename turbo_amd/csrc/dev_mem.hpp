// dev_mem.hpp -- the owners of a handle's GPU memory, pinned host memory and events.  Each holds ONE resource, frees it
// in its destructor, cannot be copied, and releases what it held when it is move-assigned: a struct of them is released
// by assigning a fresh struct over it.  The allocator is the policy A -- HipMem below, seen by HIP sources only; the
// contracts are tested on the CPU over a counting malloc (tests/dev_mem_sanitizer_driver.cpp).
#pragma once
#include <stddef.h>
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#endif

namespace tgp {

// reserve(bytes, sync) -- the one way a buffer grows, the same for both buffer owners:
//   * large enough already: nothing happens (grow-only, never shrinks);
//   * else sync() runs first ("whatever may still use the block is idle"): if it fails the buffer is untouched;
//   * then the block is freed and the owner EMPTY (null, 0 bytes) before the allocation, so a failing allocation leaves
//     it empty -- never a stale size or a dangling pointer -- and a later reserve starts clean.
// Returns the failing step's error.  reserve(bytes): without a synchronisation.

template <class T, class A>
class DevBuf {   // one hipMalloc block
public:
    DevBuf() = default;
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T *() const { return p_; }   // the launchers read c.d_K as the pointer it was
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    void reset() { if (p_) A::dev_free(p_); p_ = nullptr; bytes_ = 0; }
    template <class Sync>
    typename A::err_t reserve(size_t bytes, Sync &&sync) {
        if (bytes <= bytes_) return A::ok;
        typename A::err_t e = sync();
        if (e != A::ok) return e;
        reset();
        void *p = nullptr;
        if ((e = A::dev_alloc(&p, bytes)) != A::ok) return e;
        p_ = static_cast<T *>(p); bytes_ = bytes;
        return A::ok;
    }
    typename A::err_t reserve(size_t bytes) { return reserve(bytes, [] { return A::ok; }); }

private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
};

template <class T, class A>
class PinBuf {   // one hipHostMalloc block and, when it is mapped, the device's view of it
public:
    explicit PinBuf(unsigned flags, bool mapped = true) : flags_(flags), mapped_(mapped) {}
    PinBuf &operator=(PinBuf &&o) noexcept {   // (the flags stay: they say what this owner allocates)
        if (this != &o) { reset(); h_ = o.h_; d_ = o.d_; bytes_ = o.bytes_; o.h_ = o.d_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~PinBuf() { reset(); }
    operator T *() const { return h_; }   // the host pointer
    T *get() const { return h_; }
    T *dev() const { return d_; }         // null when unmapped
    size_t bytes() const { return bytes_; }
    void reset() { if (h_) A::pin_free(h_); h_ = d_ = nullptr; bytes_ = 0; }
    template <class Sync>
    typename A::err_t reserve(size_t bytes, Sync &&sync) {
        if (bytes <= bytes_) return A::ok;
        typename A::err_t e = sync();
        if (e != A::ok) return e;
        reset();
        void *h = nullptr, *d = nullptr;
        if ((e = A::pin_alloc(&h, bytes, flags_)) != A::ok) return e;
        if (mapped_ && (e = A::pin_view(&d, h)) != A::ok) { A::pin_free(h); return e; }
        h_ = static_cast<T *>(h); d_ = static_cast<T *>(d); bytes_ = bytes;
        return A::ok;
    }
    typename A::err_t reserve(size_t bytes) { return reserve(bytes, [] { return A::ok; }); }

private:
    T *h_ = nullptr, *d_ = nullptr;
    size_t bytes_ = 0;
    const unsigned flags_;
    const bool mapped_;
};

template <class A>
class Event {   // one event, created on demand
public:
    using event_t = typename A::event_t;
    Event() = default;
    Event(Event &&o) noexcept : e_(o.e_) { o.e_ = event_t(); }   // (a std::vector of them grows)
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = event_t(); } return *this; }
    ~Event() { reset(); }
    operator event_t() const { return e_; }
    void reset() { if (e_ != event_t()) A::event_destroy(e_); e_ = event_t(); }
    typename A::err_t create(unsigned flags) { return e_ != event_t() ? A::ok : A::event_create(&e_, flags); }   // once

private:
    event_t e_ = event_t();
};

#if defined(__HIP__)
struct HipMem {   // the real policy (the only hipFree / hipHostFree / hipEventDestroy of the handle's state)
    using err_t = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t dev_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void dev_free(void *p) { (void)hipFree(p); }
    static hipError_t pin_alloc(void **h, size_t bytes, unsigned flags) { return hipHostMalloc(h, bytes, flags); }
    static hipError_t pin_view(void **d, void *h) { return hipHostGetDevicePointer(d, h, 0); }
    static void pin_free(void *h) { (void)hipHostFree(h); }
    using event_t = hipEvent_t;
    static hipError_t event_create(hipEvent_t *e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
    static void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
};
template <class T> using Dev = DevBuf<T, HipMem>;
template <class T> using Pin = PinBuf<T, HipMem>;
using Ev = Event<HipMem>;
#endif

}  // namespace tgp
