// orbfe_host.h -- the host scaffold every handle of liborbfe.so is built from: the device guard, "which device", the grow-only
// device / pinned buffers and the allocate-all / free-all pair of the fixed-size handles.  Host code only; include after
// orbfe_common.h.
#pragma once

#include <initializer_list>

#include "orbfe_common.h"

// Makes `d` the calling thread's device for the scope and puts the previous one back on every exit path.  Default-constructed
// it only restores (for code that switches between several devices itself).
struct DeviceGuard {
    int prev = -1, dev = -1;
    DeviceGuard()
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    explicit DeviceGuard(int d) : dev(d)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// The device a create function or a handle-less entry point runs on: *device < 0 means the calling thread's current device.
// ORBFE_ERR_NODEVICE (error text set, the runtime's sticky error cleared) when no device is visible, ORBFE_ERR_ARG when
// *device is past the last one.
static inline orbfe_status orb_resolve_device(int32_t *device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        orbfe_set_error("no HIP device visible; liborbfe has no CPU fallback");
        return ORBFE_ERR_NODEVICE;
    }
    int dev = *device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    if (dev >= ndev) {
        orbfe_set_error("device %d out of range (%d visible)", dev, ndev);
        return ORBFE_ERR_ARG;
    }
    *device = dev;
    return ORBFE_OK;
}

// device buffer that only grows (in steps of 256 bytes)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    size_t min_bytes = 0;  // the matcher's scratch blocks set 4: a zero-byte request still yields a pointer a kernel can take
    template <class T>
    T *as() const { return (T *)p; }
    hipError_t ensure(size_t need)
    {
        if (need < min_bytes) need = min_bytes;
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        need = (need + 255) & ~(size_t)255;
        hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// page-locked host buffer that only grows
struct PinBuf {
    void *p = nullptr;
    size_t bytes = 0;
    size_t min_bytes = 0;  // as DevBuf::min_bytes
    bool slack = false;    // the matcher's per-frame staging sets it: grow to need * 3 / 2, rounded up to 4 KiB
    template <class T>
    T *as() const { return (T *)p; }
    hipError_t ensure(size_t need)
    {
        if (need < min_bytes) need = min_bytes;
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        if (slack) need = (need * 3 / 2 + 4095) & ~(size_t)4095;
        hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// The fixed-size handles (orbfe_flow, orbfe_homography) allocate everything in create: a stream of their own plus a list of
// device blocks.  orb_alloc_all stops at the first failure; the caller then frees what there is with orb_free_all (its own
// list of the same pointers, also what destroy uses) and answers ORBFE_ERR_NOMEM.
struct OrbAlloc {
    void **p;
    size_t bytes;
};

inline bool orb_alloc_all(hipStream_t *stream, std::initializer_list<OrbAlloc> blocks)
{
    if (hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) return false;
    for (const OrbAlloc &a : blocks)
        if (hipMalloc(a.p, a.bytes) != hipSuccess) return false;
    return true;
}

inline void orb_free_all(hipStream_t stream, std::initializer_list<void *> blocks)
{
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
}
