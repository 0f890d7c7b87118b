// dev_buf.h — owned device and pinned-host memory (DevBuf, PinnedBuf) and the two error macros they return through.  Shared by the
// kernels.hip translation unit (device_state.h includes it behind that unit's own definitions of the macros), temporal_session.hip and temporal_change.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <string>

#include "scene_internal.h"

#ifndef HIP_CHECK
#define HIP_CHECK(expr)                                                                                        \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            SetError(std::string(#expr) + ": " + hipGetErrorString(e_));                                       \
            return BHRT_ERR_HIP;                                                                               \
        }                                                                                                      \
    } while (0)
#endif
// the same for a call that returns a BHRT_* code (and has set the error text)
#ifndef BHRT_TRY
#define BHRT_TRY(expr)                                                                                         \
    do {                                                                                                       \
        const int rc_ = (expr);                                                                                \
        if (rc_) return rc_;                                                                                   \
    } while (0)
#endif

namespace bhrt {

// Device memory owned by its holder; grow-only.  n: capacity in elements.
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { Free(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { Free(); }
    // n >= want: nothing.  Otherwise the old memory is freed FIRST and the contents are not kept; a failed allocation leaves an empty buffer with
    // capacity 0, so the next call tries again.  (hipFree waits for the device: kernels of an earlier call may still read the old memory.)
    int Reserve(size_t want)
    {
        if (n >= want) return BHRT_OK;
        Free();
        HIP_CHECK(hipMalloc(&p, want * sizeof(T)));
        n = want;
        return BHRT_OK;
    }
    void Free()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    T *Release() // hands the memory to the caller
    {
        T *r = p;
        p = nullptr; n = 0;
        return r;
    }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};

// The pinned-host twin (one allocation, never regrown).
template <class T> struct PinnedBuf {
    T *p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int Alloc(size_t count, unsigned flags = hipHostMallocDefault)
    {
        HIP_CHECK(hipHostMalloc(&p, count * sizeof(T), flags));
        return BHRT_OK;
    }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};

} // namespace bhrt
