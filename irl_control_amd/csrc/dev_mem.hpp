// Owners of the host library's HIP resources: device buffers, pinned host blocks, events, streams.  Host code only (irlosc.hip; no kernel
// translation unit includes this).  An owner can be moved from but not copied or assigned, holds null while empty and releases what it
// holds when it is destroyed -- on the device current then (irlosc_destroy / irlosc_comm_destroy set it): a resource is stated once.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

namespace irlosc {

// Device buffer of T with the bytes it was allocated with; reads as a T* wherever one is expected.
template <typename T>
class DevBuf {
    T* p_ = nullptr;
    size_t bytes_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    ~DevBuf() { reset(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    // Frees and empties -- emptied whatever the free answers: no pointer is left behind.
    void reset() { if (p_) (void)hipFree((void*)p_); p_ = nullptr; bytes_ = 0; }
    // Allocate on first use: a new buffer of `bytes` (zeroed on `zero_on` when given) unless one is held already.  On failure the owner is
    // empty and the runtime's last error cleared: the caller decides what out of device memory means.
    hipError_t ensure(size_t bytes, hipStream_t zero_on = nullptr) {
        if (p_) return hipSuccess;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess && zero_on) e = hipMemsetAsync(q, 0, bytes, zero_on);
        if (e != hipSuccess) { (void)hipFree(q); (void)hipGetLastError(); return e; }
        p_ = (T*)q; bytes_ = bytes;
        return hipSuccess;
    }
    // Grow on demand, discarding the contents: at least `bytes` afterwards.  The old buffer goes first, so a failure leaves the owner empty.
    hipError_t reserve(size_t bytes) {
        if (bytes_ >= bytes) return hipSuccess;
        reset();
        return ensure(bytes);
    }
};

// Pinned host block, grown like a device buffer.
class PinnedBuf {
    void* p_ = nullptr;
    size_t bytes_ = 0;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    ~PinnedBuf() { reset(); }
    operator unsigned char*() const { return (unsigned char*)p_; }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; bytes_ = 0; }
    hipError_t reserve(size_t bytes) {
        if (bytes_ >= bytes) return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr; else bytes_ = bytes;
        return e;
    }
};

// Event, created by its first ensure().
class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    ~Event() { reset(); }
    operator hipEvent_t() const { return e_; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipError_t ensure(unsigned flags = hipEventDefault) {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
};

// Non-blocking stream, created by its first ensure().
class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    ~Stream() { reset(); }
    operator hipStream_t() const { return s_; }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    hipError_t ensure() {
        if (s_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
};

}  // namespace irlosc
