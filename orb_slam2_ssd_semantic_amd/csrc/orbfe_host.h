// orbfe_host.h -- the host scaffold every handle of liborbfe.so is built from: the device guard, "which device", the grow-only
// device / pinned buffers, the allocate-all / free-all pair of the fixed-size handles with the head and tail of their create
// and the body of their destroy, and the runner of the known-answer entry points.  Host code only; include after
// orbfe_common.h.  csrc/orbfe_ransac.h builds the RANSAC solver handles on top of it.
#pragma once

#include <initializer_list>
#include <new>

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

// the allocation step of the device buffers, and the alignment of the pieces packed into one
static inline size_t orb_align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
        need = orb_align256(need);
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

// The fixed-size handles (orbfe_flow, orbfe_homography, orbfe_sim3, orbfe_pnp) allocate everything in create: a stream of
// their own plus a list of device blocks.  orb_alloc_all stops at the first failure; orb_create_finish then frees what there
// is through the handle's free function (orb_free_all over the same pointers, also what destroy uses) and answers
// ORBFE_ERR_NOMEM.
struct OrbAlloc {
    void **p;
    size_t bytes;
};

template <class T>
inline OrbAlloc orb_blk(T **p, size_t bytes) { return OrbAlloc{(void **)p, bytes}; }

inline bool orb_alloc_all(hipStream_t *stream, const OrbAlloc *blocks, size_t count)
{
    if (hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) return false;
    for (size_t i = 0; i < count; i++)
        if (hipMalloc(blocks[i].p, blocks[i].bytes) != hipSuccess) return false;
    return true;
}

inline bool orb_alloc_all(hipStream_t *stream, std::initializer_list<OrbAlloc> blocks) { return orb_alloc_all(stream, blocks.begin(), blocks.size()); }

inline void orb_free_all(hipStream_t stream, std::initializer_list<void *> blocks)
{
    for (void *p : blocks)
        if (p) (void)hipFree(p);
    if (stream) (void)hipStreamDestroy(stream);
}

// The head of create for the handles sized by (points, sets): the argument limits, the device, the handle itself with `device`
// and `max_sets` set.  The caller sets its DeviceGuard, allocates, and ends with orb_create_finish.
constexpr int32_t ORB_MAX_POINTS = 1 << 24, ORB_MAX_SETS = 1 << 20;

template <class H>
orbfe_status orb_create_begin(int32_t *device, int32_t max_points, int32_t max_sets, H **out, H **h)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    if (max_points < 1 || max_sets < 1 || max_points > ORB_MAX_POINTS || max_sets > ORB_MAX_SETS) return ORBFE_ERR_ARG;
    const orbfe_status rs = orb_resolve_device(device);
    if (rs != ORBFE_OK) return rs;
    *h = new (std::nothrow) H();
    if (!*h) return ORBFE_ERR_NOMEM;
    (*h)->device = *device;
    (*h)->max_sets = max_sets;
    return ORBFE_OK;
}

// The tail of create for any handle with `stream` and `last_stream`: ok is what orb_alloc_all answered, free_blocks the
// handle's free function (the one destroy uses: it skips the blocks that were never allocated).
template <class H>
orbfe_status orb_create_finish(bool ok, const char *name, H *h, void (*free_blocks)(H *), H **out)
{
    if (!ok) {
        (void)hipGetLastError();
        orbfe_set_error("%s: device allocation failed", name);
        free_blocks(h);
        delete h;
        return ORBFE_ERR_NOMEM;
    }
    h->last_stream = h->stream;
    *out = h;
    return ORBFE_OK;
}

// destroy: work of the last call may still run on the caller's stream (last_stream) or on the handle's own
template <class H>
void orb_destroy(H *h, void (*free_blocks)(H *))
{
    if (!h) return;
    DeviceGuard dg(h->device);
    (void)hipStreamSynchronize(h->last_stream);
    (void)hipStreamSynchronize(h->stream);
    free_blocks(h);
    delete h;
}

// A known-answer entry point (*_kat) on the caller's current device: in_b bytes of `in` go to the device, launch(d_in, d_out,
// d_ws) enqueues the kernel on the null stream (d_ws: ws_b bytes of workspace, nullptr for 0), out_b bytes come back.  A
// failed allocation answers ORBFE_ERR_NOMEM, any other runtime failure ORBFE_ERR_HIP, as create does: error text set, the
// runtime's sticky error cleared.
template <class Launch>
orbfe_status orb_kat_run(const char *name, const void *in, size_t in_b, void *out, size_t out_b, size_t ws_b, Launch launch)
{
    int32_t device = -1;
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    void *d_in = nullptr, *d_out = nullptr, *d_ws = nullptr;
    hipError_t e = hipMalloc(&d_in, in_b);
    if (e == hipSuccess) e = hipMalloc(&d_out, out_b);
    if (e == hipSuccess && ws_b) e = hipMalloc(&d_ws, ws_b);
    const bool nomem = e != hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(d_in, in, in_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch(d_in, d_out, d_ws);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost);
    for (void *p : {d_in, d_out, d_ws})
        if (p) (void)hipFree(p);
    if (e == hipSuccess) return ORBFE_OK;
    (void)hipGetLastError();
    orbfe_set_error("%s: %s", name, nomem ? "device allocation failed" : hipGetErrorString(e));
    return nomem ? ORBFE_ERR_NOMEM : ORBFE_ERR_HIP;
}
