// nm_own.h — what the host code owns from the HIP runtime, released on every way out of the scope (or the context) that holds it: device
// and pinned host memory, events and streams.  Every release of the library is in this file.  All of them can be moved and none copied,
// so a call that must leave all or nothing builds into locals, returns on an error, and moves them in.  Internal linkage: each file its copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace {

struct DeviceMem {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { hipHostFree(p); }
};

// n elements of T at p (null and 0 while empty); sizes are counts of T
template <class T, class Mem> struct Buf {
    T *p = nullptr;
    size_t n = 0;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; } // (what was held goes with o)
    ~Buf() { if (p) Mem::put(p); }
    // a fresh block of count elements (at least one: never null afterwards); a failure leaves what was held
    hipError_t alloc(size_t count)
    {
        void *q = nullptr;
        const hipError_t e = Mem::get(&q, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        if (p) Mem::put(p);
        p = (T *)q; n = count;
        return hipSuccess;
    }
    // grow only; the contents are not kept
    hipError_t reserve(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    // device memory only
    hipError_t zero(size_t count) { return hipMemset(p, 0, count * sizeof(T)); }
    hipError_t alloc_zeroed(size_t count)
    {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : zero(count);
    }
    hipError_t upload(const T *host, size_t count)
    {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t download(T *host, size_t count) const { return hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost); }
    operator T *() const { return p; }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinBuf = Buf<T, PinnedMem>;

template <class H, hipError_t (*destroy)(H)> struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
    Handle &operator=(Handle &&o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) destroy(h); }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&h, flags); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> { // (non-blocking: the contexts never meet on the null stream)
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};

} // namespace
