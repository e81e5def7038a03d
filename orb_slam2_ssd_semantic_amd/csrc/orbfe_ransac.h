// orbfe_ransac.h -- what the RANSAC solver handles (orbfe_sim3, orbfe_pnp) share above orbfe_host.h: "one workgroup per set,
// iterate, with taps".  The common members of the handle, create / free / destroy, the tap binding at launch, the lazy tap
// allocation, the tap read-back, the round trip of the host form, and the two small functions both solvers restate from the
// reference (DUtils' RandomInt, the x86 double-to-int conversion).  What differs between the solvers comes in as sizes
// (RansacSizes) and as the handle's own blocks; nothing here knows which solver it serves.  Layout: DESIGN.md section 8i.
#pragma once

#include <math.h>

#include <vector>

#include "orbfe_host.h"

// DUtils::Random::RandomInt(0, size - 1) on a raw rand() value
__device__ inline int index_from_draw(int32_t r, int size) { return (int)(((double)(r & 0x7fffffff) / 2147483648.0) * (double)size); }

// what the x86-64 conversion (cvttsd2si) of the reference gives for a double: INT32_MIN outside int's range and for a NaN
static inline int32_t x86_double_to_int(double v) { return v > -2147483649.0 && v < 2147483648.0 ? (int32_t)v : INT32_MIN; }

struct RansacSizes {
    size_t set, state, result, iter;   // bytes of the solver's orbfe_*_set / _state / _result / _iter records
    int err_floats;                    // floats per point of the error tap
    int tap_sets, tap_iters;           // ORBFE_*_TAP_SETS, ORBFE_*_TAP_ITERS
};

// The members every solver handle has.  A solver derives from it, adds its own device arrays and names them in
//   std::vector<OrbAlloc> blocks(size_t np)   -- its own blocks with their sizes for np points, allocated first in create.
// max_points bounds what the solver's kernel is told (a Sim3 set, all PnP sets of a batch together: the solvers differ there).
struct RansacHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;
    int max_points = 0, max_sets = 0;
    int tap_cap = 0;         // sets the taps cover; 0 until ransac_set_tap_iteration allocates them
    int tap_sets = 0;        // sets of the last call the taps cover
    int tap_iteration = 0;   // the iteration whose errors the next call records
    int tap_launched = 0;    // ... and the one the last call recorded
    uint8_t *d_best_mask = nullptr, *d_mask = nullptr;
    int32_t *d_off = nullptr, *d_tap_info = nullptr;   // tap_info [tap_cap][2]: iterations run, points of the set
    void *d_set = nullptr, *d_state = nullptr, *d_result = nullptr;   // one record each: the host form's set
    void *d_tap_iter = nullptr;                                       // [tap_cap][tap_iters] iter records
    float *d_tap_err = nullptr;                                       // [tap_cap][max_points][err_floats]
    DevBuf draws;
};

template <class H>
void ransac_free(H *h)
{
    h->draws.release();
    for (const OrbAlloc &b : h->blocks(0))
        if (*b.p) (void)hipFree(*b.p);
    orb_free_all(h->stream, {h->d_best_mask, h->d_mask, h->d_off, h->d_set, h->d_state, h->d_result, h->d_tap_info, h->d_tap_iter, h->d_tap_err});
}

template <class H>
orbfe_status ransac_create(const char *name, const RansacSizes &z, int32_t device, int32_t max_points, int32_t max_sets, H **out)
{
    H *h = nullptr;
    const orbfe_status s = orb_create_begin(&device, max_points, max_sets, out, &h);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(device);
    h->max_points = max_points;
    const size_t np = (size_t)max_points;
    std::vector<OrbAlloc> all = h->blocks(np);
    all.insert(all.end(), {orb_blk(&h->d_best_mask, np), orb_blk(&h->d_mask, np), orb_blk(&h->d_off, 2 * sizeof(int32_t)),
                           orb_blk(&h->d_set, z.set), orb_blk(&h->d_state, z.state), orb_blk(&h->d_result, z.result)});
    return orb_create_finish(orb_alloc_all(&h->stream, all.data(), all.size()), name, h, ransac_free<H>, out);
}

// The taps of a launch over nsets sets on stream st, into the kernel's arguments, and what ransac_tap answers from afterwards.
template <class Args>
void ransac_bind_taps(RansacHandle *h, Args &a, int nsets, hipStream_t st)
{
    a.max_points = h->max_points;
    a.tap_iter = (decltype(a.tap_iter))h->d_tap_iter;
    a.tap_err = h->d_tap_err;
    a.tap_info = h->d_tap_info;
    a.tap_sets = nsets < h->tap_cap ? nsets : h->tap_cap;
    a.tap_iteration = h->tap_iteration;
    h->last_stream = st;
    h->tap_sets = a.tap_sets;
    h->tap_launched = a.tap_iteration;
}

inline orbfe_status ransac_set_tap_iteration(RansacHandle *h, const RansacSizes &z, const char *name, int32_t iteration)
{
    if (!h || iteration < 0) return ORBFE_ERR_ARG;
    if (!h->tap_cap) {   // the taps are test equipment: a handle that never asks for them neither holds nor writes them
        const size_t nt = (size_t)(h->max_sets < z.tap_sets ? h->max_sets : z.tap_sets), np = (size_t)h->max_points;
        DeviceGuard dg(h->device);
        if (hipMalloc((void **)&h->d_tap_info, nt * 2 * sizeof(int32_t)) != hipSuccess ||
            hipMalloc((void **)&h->d_tap_err, nt * np * z.err_floats * sizeof(float)) != hipSuccess ||
            hipMalloc(&h->d_tap_iter, nt * z.tap_iters * z.iter) != hipSuccess) {
            (void)hipGetLastError();
            for (void **p : {(void **)&h->d_tap_info, (void **)&h->d_tap_err, &h->d_tap_iter}) {
                if (*p) (void)hipFree(*p);
                *p = nullptr;
            }
            orbfe_set_error("%s: device allocation of the taps failed", name);
            return ORBFE_ERR_NOMEM;
        }
        h->tap_cap = (int)nt;
    }
    h->tap_iteration = iteration;
    return ORBFE_OK;
}

// A tap of set `set` of the last call, after it has finished: its iteration records (at most tap_iters), or the errors of the
// iteration that call recorded.  The caller has checked h, dst, count and the stage.
inline orbfe_status ransac_tap(RansacHandle *h, const RansacSizes &z, int32_t set, bool iterations, void *dst, size_t cap, int32_t *count)
{
    if (set < 0 || set >= h->tap_sets) return ORBFE_ERR_STATE;
    DeviceGuard dg(h->device);
    ORBFE_HIP(hipStreamSynchronize(h->last_stream));
    int32_t info[2];
    ORBFE_HIP(hipMemcpy(info, h->d_tap_info + 2 * (size_t)set, sizeof(info), hipMemcpyDeviceToHost));
    if (iterations) {
        const int32_t k = info[0] < z.tap_iters ? info[0] : z.tap_iters;
        if (cap < (size_t)k * z.iter) return ORBFE_ERR_CAP;
        if (k > 0) ORBFE_HIP(hipMemcpy(dst, (const char *)h->d_tap_iter + (size_t)set * z.tap_iters * z.iter, (size_t)k * z.iter, hipMemcpyDeviceToHost));
        *count = k;
        return ORBFE_OK;
    }
    if (h->tap_launched >= info[0]) return ORBFE_ERR_STATE;   // that iteration was not run
    const int32_t n = info[1];
    const size_t per = z.err_floats * sizeof(float);
    if (cap < (size_t)n * per) return ORBFE_ERR_CAP;
    if (n > 0) ORBFE_HIP(hipMemcpy(dst, h->d_tap_err + (size_t)set * h->max_points * z.err_floats, (size_t)n * per, hipMemcpyDeviceToHost));
    *count = n;
    return ORBFE_OK;
}

// The host form: one set of n points through the handle's own blocks and stream.  Up go off, set, state, nd draws, the
// solver's per-point arrays (`points`, in that order), best_mask; launch(h, a, 1, stream) runs with the common members of `a`
// pointing at the handle's blocks; down come state, result, best_mask, mask (if asked for); one synchronisation at the end.
struct RansacCopy {
    void *dst;
    const void *src;
    size_t bytes_per_point;
};

template <class H, class Args>
orbfe_status ransac_host_call(H *h, const RansacSizes &z, Args &a, orbfe_status (*launch)(H *, Args &, int, hipStream_t), int32_t n,
                              const void *set, void *state, const int32_t *draws, size_t nd, std::initializer_list<RansacCopy> points,
                              uint8_t *best_mask, void *result, uint8_t *mask)
{
    hipStream_t st = h->stream;
    ORBFE_HIP(h->draws.ensure((nd ? nd : 1) * sizeof(int32_t)));
    const int32_t off[2] = {0, n};
    ORBFE_HIP(hipMemcpyAsync(h->d_off, off, sizeof(off), hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_set, set, z.set, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_state, state, z.state, hipMemcpyHostToDevice, st));
    if (nd) ORBFE_HIP(hipMemcpyAsync(h->draws.p, draws, nd * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (n > 0) {
        for (const RansacCopy &c : points) ORBFE_HIP(hipMemcpyAsync(c.dst, c.src, (size_t)n * c.bytes_per_point, hipMemcpyHostToDevice, st));
        ORBFE_HIP(hipMemcpyAsync(h->d_best_mask, best_mask, (size_t)n, hipMemcpyHostToDevice, st));
    }
    a.off = h->d_off;
    a.sets = (decltype(a.sets))h->d_set;
    a.draws = h->draws.template as<int32_t>();
    a.state = (decltype(a.state))h->d_state;
    a.best_mask = h->d_best_mask;
    a.result = (decltype(a.result))h->d_result;
    a.mask = h->d_mask;
    const orbfe_status s = launch(h, a, 1, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(hipMemcpyAsync(state, h->d_state, z.state, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(result, h->d_result, z.result, hipMemcpyDeviceToHost, st));
    if (n > 0) {
        ORBFE_HIP(hipMemcpyAsync(best_mask, h->d_best_mask, (size_t)n, hipMemcpyDeviceToHost, st));
        if (mask) ORBFE_HIP(hipMemcpyAsync(mask, h->d_mask, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}
