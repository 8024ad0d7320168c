// owned.hpp — the HIP resources of a context as objects that release themselves: device and pinned buffers, events,
// streams.  All are move-only (a move leaves the source empty) and free in their destructor, so nothing that holds one
// needs a list of what to release.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace rsreg {

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void *p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};

// Growable allocation; never shrinks, so steady-state calls allocate nothing.
template <typename Mem> struct OwnedBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) { release(); ptr = std::exchange(o.ptr, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~OwnedBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = Mem::alloc(&ptr, want);
        if (e == hipSuccess) cap = want;
        else ptr = nullptr;
        return e;
    }
    void release()
    {
        if (ptr) (void)Mem::free(ptr);
        ptr = nullptr, cap = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(ptr); }
};
struct DevBuf : OwnedBuf<DeviceMem> {};
struct PinnedBuf : OwnedBuf<PinnedMem> {};

// An event, created on demand (ensure) and read as a hipEvent_t wherever one is recorded or waited for
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { reset(); h = std::exchange(o.h, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming)
    {
        if (h) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    void reset() { if (h) (void)hipEventDestroy(h); h = nullptr; }
    operator hipEvent_t() const { return h; }
};

// A non-blocking stream of the context's own, created on demand.  Whoever destroys one has drained it first.
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept
    {
        if (this != &o) { reset(); h = std::exchange(o.h, nullptr); }
        return *this;
    }
    ~Stream() { reset(); }
    hipError_t ensure()
    {
        if (h) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
    void reset() { if (h) (void)hipStreamDestroy(h); h = nullptr; }
    operator hipStream_t() const { return h; }
};

// A stream with the events that belong to it, made together: complete afterwards, or empty and the error returned
template <size_t N> inline hipError_t ensure_lane(Stream &s, Event *const (&evs)[N])
{
    hipError_t e = s.ensure();
    for (size_t k = 0; k < N && e == hipSuccess; ++k) e = evs[k]->ensure();
    if (e != hipSuccess) {
        for (Event *ev : evs) ev->reset();
        s.reset();
    }
    return e;
}

}  // namespace rsreg
