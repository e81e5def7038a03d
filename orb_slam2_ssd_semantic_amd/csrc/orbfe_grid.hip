// orbfe_grid.hip -- the Frame grid index of the matcher handle (include/orbfe.h "Matcher"): orbfe_assign_grid*, orbfe_features_in_area*.
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"

// ---------------------------------------------------------------------------------------------------
// SURVEY 8(f).2  Frame grid index: AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea (src/Frame.cc:319-334, 465-531)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int grid_cell_of(float x, float y, float minx, float miny, float gwi, float ghi)
{
    const float rx = roundf(__fmul_rn(__fsub_rn(x, minx), gwi));  // :525 std::round(float)
    const float ry = roundf(__fmul_rn(__fsub_rn(y, miny), ghi));
    // the range is decided in float, as orbfe_assign_grid_host does: the reference converts first, and a NaN or a value that
    // no int holds becomes INT_MIN on the CPU (out of the grid), while the device's conversion gives 0 for a NaN (cell 0)
    if (!(rx >= 0.f && rx < (float)ORBFE_GRID_COLS && ry >= 0.f && ry < (float)ORBFE_GRID_ROWS)) return -1;
    return (int)rx * ORBFE_GRID_ROWS + (int)ry;
}

// one workgroup: histogram over the 3072 cells (LDS), scan, placement, then each cell's short list is put into
// ascending keypoint order (the reference push_backs in keypoint order)
// xs = floats between consecutive points (2 for packed (x, y), 7 for orbfe_keypoint records).  Batched form (d_n != null):
// workgroup f takes frame f of an extractor output block -- points at f * cap * xs, count d_n[f] -- and writes its own
// cell_off [GRID_NC + 1], cell_idx [cap] and n_in.
__global__ __launch_bounds__(1024) void k_assign_grid(const float *__restrict__ xy, int n, float minx, float miny, float gwi,
                                                      float ghi, uint32_t *__restrict__ cell_off,
                                                      uint32_t *__restrict__ cell_idx, int32_t *__restrict__ n_in, int xs,
                                                      int cap, const int32_t *__restrict__ d_n)
{
    __shared__ uint32_t s_cnt[GRID_NC], s_off[GRID_NC + 1];
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    if (d_n) {
        const int f = blockIdx.x;
        n = min(d_n[f], cap);
        xy += (int64_t)f * cap * xs;
        cell_off += (int64_t)f * (GRID_NC + 1);
        cell_idx += (int64_t)f * cap;
        n_in += f;
    }
    for (int c = tid; c < GRID_NC; c += 1024) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell_of(xy[(int64_t)xs * i], xy[(int64_t)xs * i + 1], minx, miny, gwi, ghi);
        if (c >= 0) atomicAdd(&s_cnt[c], 1u);
    }
    __syncthreads();
    // exclusive scan of 3072 counters: 3 per thread
    uint32_t loc[3], sum = 0;
    for (int k = 0; k < 3; ++k) { loc[k] = s_cnt[tid * 3 + k]; sum += loc[k]; }
    s_part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t v = tid >= d ? s_part[tid - d] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t base = s_part[tid] - sum;
    for (int k = 0; k < 3; ++k) { s_off[tid * 3 + k] = base; base += loc[k]; }
    if (tid == 1023) s_off[GRID_NC] = s_part[1023];
    __syncthreads();
    for (int c = tid; c <= GRID_NC; c += 1024) cell_off[c] = s_off[c];
    if (tid == 0) *n_in = (int32_t)s_off[GRID_NC];
    for (int c = tid; c < GRID_NC; c += 1024) s_cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell_of(xy[(int64_t)xs * i], xy[(int64_t)xs * i + 1], minx, miny, gwi, ghi);
        if (c >= 0) cell_idx[s_off[c] + atomicAdd(&s_cnt[c], 1u)] = (uint32_t)i;
    }
    __syncthreads();
    __threadfence_block();
    for (int c = tid; c < GRID_NC; c += 1024) {  // insertion sort of the (short) cell lists
        const uint32_t o = s_off[c], e = s_off[c + 1];
        for (uint32_t a = o + 1; a < e; ++a) {
            const uint32_t v = cell_idx[a];
            uint32_t bpos = a;
            while (bpos > o && cell_idx[bpos - 1] > v) { cell_idx[bpos] = cell_idx[bpos - 1]; --bpos; }
            cell_idx[bpos] = v;
        }
    }
}

// GetFeaturesInArea for query i; write == false only counts.  Returns the count.
__device__ int area_query(const float *__restrict__ xy, const int32_t *__restrict__ octave,
                          const uint32_t *__restrict__ cell_off, const uint32_t *__restrict__ cell_idx, float minx,
                          float miny, float gwi, float ghi, float x, float y, float r, int minL, int maxL,
                          uint32_t *out, bool write, int xs = 2, int os = 1)
{
    int nminx = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, minx), r), gwi));  // :470
    nminx = max(nminx, 0);
    if (nminx >= ORBFE_GRID_COLS) return 0;
    int nmaxx = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, minx), r), gwi));
    nmaxx = min(nmaxx, ORBFE_GRID_COLS - 1);
    if (nmaxx < 0) return 0;
    int nminy = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, miny), r), ghi));
    nminy = max(nminy, 0);
    if (nminy >= ORBFE_GRID_ROWS) return 0;
    int nmaxy = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, miny), r), ghi));
    nmaxy = min(nmaxy, ORBFE_GRID_ROWS - 1);
    if (nmaxy < 0) return 0;
    const bool check = (minL > 0) || (maxL >= 0);  // :486
    int cnt = 0;
    for (int ix = nminx; ix <= nmaxx; ++ix)
        for (int iy = nminy; iy <= nmaxy; ++iy) {
            const int c = ix * ORBFE_GRID_ROWS + iy;
            for (uint32_t j = cell_off[c]; j < cell_off[c + 1]; ++j) {
                const uint32_t k = cell_idx[j];
                if (check) {
                    const int o = octave[(size_t)os * k];
                    if (o < minL) continue;
                    if (maxL >= 0 && o > maxL) continue;
                }
                const float dx = __fsub_rn(xy[(size_t)xs * k], x), dy = __fsub_rn(xy[(size_t)xs * k + 1], y);
                if (fabsf(dx) < r && fabsf(dy) < r) {
                    if (write) out[cnt] = k;
                    ++cnt;
                }
            }
        }
    return cnt;
}

__global__ __launch_bounds__(256) void k_area_count(const float *xy, const int32_t *octave, const uint32_t *cell_off,
                                                    const uint32_t *cell_idx, float minx, float miny, float gwi,
                                                    float ghi, const float *qxyr, const int32_t *qlv, int nq,
                                                    uint32_t *cnt, int xs, int os)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    cnt[i] = (uint32_t)area_query(xy, octave, cell_off, cell_idx, minx, miny, gwi, ghi, qxyr[3 * i], qxyr[3 * i + 1],
                                  qxyr[3 * i + 2], qlv ? qlv[2 * i] : -1, qlv ? qlv[2 * i + 1] : -1, nullptr, false, xs, os);
}

// single-workgroup exclusive scan cnt[0..nq) -> off[0..nq]
__global__ __launch_bounds__(1024) void k_scan_u32(const uint32_t *__restrict__ cnt, int nq, uint32_t *__restrict__ off)
{
    __shared__ uint32_t s_part[1024];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nq; base += 1024) {
        const int i = base + tid;
        const uint32_t v = i < nq ? cnt[i] : 0u;
        s_part[tid] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint32_t t = tid >= d ? s_part[tid - d] : 0u;
            __syncthreads();
            s_part[tid] += t;
            __syncthreads();
        }
        if (i < nq) off[i] = s_carry + s_part[tid] - v;
        __syncthreads();
        if (tid == 1023) s_carry += s_part[1023];
        __syncthreads();
    }
    if (tid == 0) off[nq] = s_carry;
}

__global__ __launch_bounds__(256) void k_area_write(const float *xy, const int32_t *octave, const uint32_t *cell_off,
                                                    const uint32_t *cell_idx, float minx, float miny, float gwi,
                                                    float ghi, const float *qxyr, const int32_t *qlv, int nq,
                                                    const uint32_t *off, uint32_t *cand, uint32_t cap, int xs, int os)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq || off[nq] > cap) return;
    area_query(xy, octave, cell_off, cell_idx, minx, miny, gwi, ghi, qxyr[3 * i], qxyr[3 * i + 1], qxyr[3 * i + 2],
               qlv ? qlv[2 * i] : -1, qlv ? qlv[2 * i + 1] : -1, cand + off[i], true, xs, os);
}

void orbfe_internal_launch_scan_u32(const uint32_t *cnt, int nq, uint32_t *off, hipStream_t st)
{
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, st, cnt, nq, off);
}

extern "C" orbfe_status orbfe_features_in_area_device(orbfe_matcher *m, const orbfe_keypoint *d_kps,
                                                      const uint32_t *d_cell_off, const uint32_t *d_cell_idx, float minx,
                                                      float miny, float gw_inv, float gh_inv, const float *d_qxyr,
                                                      const int32_t *d_qlevels, int32_t nq, uint32_t *d_off,
                                                      uint32_t *d_cand, int32_t cap, void *stream)
{
    if (!m || nq < 0 || cap < 0 || !d_off || (nq > 0 && (!d_kps || !d_cell_off || !d_cell_idx || !d_qxyr || (cap > 0 && !d_cand)))) {
        orbfe_set_error("bad argument to orbfe_features_in_area_device");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[7].ensure((size_t)std::max(nq, 1) * 4));  // per-query counts
    const float *xy = (const float *)d_kps;                  // record = 7 floats: (x, y) first, octave sixth
    const int32_t *oct = (const int32_t *)d_kps + 5;
    static_assert(offsetof(orbfe_keypoint, octave) == 20 && sizeof(orbfe_keypoint) == 28, "keypoint record layout");
    if (nq > 0) {
        hipLaunchKernelGGL(k_area_count, dim3((nq + 255) / 256), dim3(256), 0, st, xy, oct, d_cell_off, d_cell_idx, minx, miny, gw_inv,
                           gh_inv, d_qxyr, d_qlevels, nq, m->b[7].as<uint32_t>(), 7, 7);
    }
    orbfe_internal_launch_scan_u32(m->b[7].as<const uint32_t>(), nq, d_off, st);
    if (nq > 0)
        hipLaunchKernelGGL(k_area_write, dim3((nq + 255) / 256), dim3(256), 0, st, xy, oct, d_cell_off, d_cell_idx, minx, miny, gw_inv,
                           gh_inv, d_qxyr, d_qlevels, nq, (const uint32_t *)d_off, d_cand, (uint32_t)cap, 7, 7);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_assign_grid(orbfe_matcher *m, const float *xy, int32_t n, float minx, float miny,
                                          float gw_inv, float gh_inv, uint32_t *cell_off, uint32_t *cell_idx,
                                          int32_t *n_in_grid)
{
    if (!m || n < 0 || !cell_off || (n > 0 && (!xy || !cell_idx))) {
        orbfe_set_error("bad argument to orbfe_assign_grid");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    ORBFE_HIP(m->b[0].ensure((size_t)n * 8));
    ORBFE_HIP(m->b[1].ensure((size_t)(GRID_NC + 1) * 4));
    ORBFE_HIP(m->b[2].ensure((size_t)n * 4));
    ORBFE_HIP(m->b[3].ensure(4));
    if (n > 0) ORBFE_HIP(hipMemcpyAsync(m->b[0].p, xy, (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_assign_grid, dim3(1), dim3(1024), 0, st, m->b[0].as<const float>(), n, minx, miny, gw_inv, gh_inv,
                       m->b[1].as<uint32_t>(), m->b[2].as<uint32_t>(), m->b[3].as<int32_t>(), 2, 0, (const int32_t *)nullptr);
    ORBFE_HIP(hipGetLastError());
    int32_t nin = 0;
    ORBFE_HIP(hipMemcpyAsync(cell_off, m->b[1].p, (size_t)(GRID_NC + 1) * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(&nin, m->b[3].p, 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    if (nin > 0) ORBFE_HIP(hipMemcpy(cell_idx, m->b[2].p, (size_t)nin * 4, hipMemcpyDeviceToHost));
    if (n_in_grid) *n_in_grid = nin;
    return ORBFE_OK;
}

// Host form of the same index (no device, no matcher handle): for callers that hold the keypoints but cannot reach the
// grid itself -- KeyFrame::mGrid is a protected member of the reference (include/KeyFrame.h:223), so the matcher shim
// rebuilds it from the public mvKeysUn.  Counting sort over the 3072 cells; per cell ascending keypoint index.
extern "C" orbfe_status orbfe_assign_grid_host(const float *xy, int32_t n, float minx, float miny, float gw_inv, float gh_inv,
                                               uint32_t *cell_off, uint32_t *cell_idx, int32_t *n_in_grid)
{
    if (n < 0 || !cell_off || (n > 0 && (!xy || !cell_idx))) {
        orbfe_set_error("bad argument to orbfe_assign_grid_host");
        return ORBFE_ERR_ARG;
    }
    auto cell = [&](int i) -> int {
        // src/Frame.cc:525-526: round() of a float product (no contraction: this file is built with -ffp-contract=off)
        const float fx = (xy[2 * (size_t)i] - minx) * gw_inv, fy = (xy[2 * (size_t)i + 1] - miny) * gh_inv;
        const float rx = roundf(fx), ry = roundf(fy);
        if (!(rx >= 0.f && rx < (float)ORBFE_GRID_COLS && ry >= 0.f && ry < (float)ORBFE_GRID_ROWS)) return -1;
        return (int)rx * ORBFE_GRID_ROWS + (int)ry;
    };
    for (int c = 0; c <= GRID_NC; ++c) cell_off[c] = 0u;
    for (int i = 0; i < n; ++i) {
        const int c = cell(i);
        if (c >= 0) cell_off[c + 1]++;
    }
    for (int c = 0; c < GRID_NC; ++c) cell_off[c + 1] += cell_off[c];
    std::vector<uint32_t> fill(cell_off, cell_off + GRID_NC);
    for (int i = 0; i < n; ++i) {
        const int c = cell(i);
        if (c >= 0) cell_idx[fill[(size_t)c]++] = (uint32_t)i;
    }
    if (n_in_grid) *n_in_grid = (int32_t)cell_off[GRID_NC];
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_assign_grid_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const int32_t *d_n,
                                                       int32_t cap, int32_t nframes, float minx, float miny, float gw_inv,
                                                       float gh_inv, uint32_t *d_cell_off, uint32_t *d_cell_idx,
                                                       int32_t *d_n_in_grid, void *stream)
{
    if (!m || nframes < 0 || cap < 0 || (nframes > 0 && (!d_kps || !d_n || !d_cell_off || !d_cell_idx || !d_n_in_grid))) {
        orbfe_set_error("bad argument to orbfe_assign_grid_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float), "keypoint record = 7 floats, (x, y) first");
    hipLaunchKernelGGL(k_assign_grid, dim3(nframes), dim3(1024), 0, (hipStream_t)stream, (const float *)d_kps, 0, minx, miny, gw_inv,
                       gh_inv, d_cell_off, d_cell_idx, d_n_in_grid, 7, cap, d_n);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_features_in_area(orbfe_matcher *m, const float *xy, const int32_t *octave, int32_t n,
                                               const uint32_t *cell_off, const uint32_t *cell_idx, float minx,
                                               float miny, float gw_inv, float gh_inv, const float *qxyr,
                                               const int32_t *qlevels, int32_t nq, uint32_t *off, uint32_t *cand,
                                               int32_t cap)
{
    if (!m || n < 0 || nq < 0 || cap < 0 || !cell_off || !off || (nq > 0 && !qxyr) || (n > 0 && (!xy || !octave || !cell_idx))) {
        orbfe_set_error("bad argument to orbfe_features_in_area");
        return ORBFE_ERR_ARG;
    }
    if (!orb_grid_csr_ok(cell_off, cell_idx, n, "n")) return ORBFE_ERR_ARG;
    const uint32_t nin = cell_off[GRID_NC];
    off[0] = 0;
    if (nq == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    const size_t sz[8] = {(size_t)n * 8, (size_t)n * 4, (size_t)(GRID_NC + 1) * 4, (size_t)nin * 4, (size_t)nq * 12,
                          (size_t)nq * 8, (size_t)(nq + 1) * 4, (size_t)nq * 4};
    for (int i = 0; i < 8; ++i) ORBFE_HIP(m->b[i].ensure(sz[i]));
    ORBFE_HIP(m->b[8].ensure((size_t)std::max(cap, 1) * 4));
    const void *src[6] = {xy, octave, cell_off, cell_idx, qxyr, qlevels};
    for (int i = 0; i < 6; ++i)
        if (src[i] && sz[i]) ORBFE_HIP(hipMemcpyAsync(m->b[i].p, src[i], sz[i], hipMemcpyHostToDevice, st));
    const int32_t *dql = qlevels ? m->b[5].as<const int32_t>() : nullptr;
    hipLaunchKernelGGL(k_area_count, dim3((nq + 255) / 256), dim3(256), 0, st, m->b[0].as<const float>(),
                       m->b[1].as<const int32_t>(), m->b[2].as<const uint32_t>(), m->b[3].as<const uint32_t>(), minx, miny,
                       gw_inv, gh_inv, m->b[4].as<const float>(), dql, nq, m->b[7].as<uint32_t>(), 2, 1);
    orbfe_internal_launch_scan_u32(m->b[7].as<const uint32_t>(), nq, m->b[6].as<uint32_t>(), st);
    hipLaunchKernelGGL(k_area_write, dim3((nq + 255) / 256), dim3(256), 0, st, m->b[0].as<const float>(),
                       m->b[1].as<const int32_t>(), m->b[2].as<const uint32_t>(), m->b[3].as<const uint32_t>(), minx, miny,
                       gw_inv, gh_inv, m->b[4].as<const float>(), dql, nq, m->b[6].as<const uint32_t>(),
                       m->b[8].as<uint32_t>(), (uint32_t)cap, 2, 1);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(off, m->b[6].p, (size_t)(nq + 1) * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    if (off[nq] > (uint32_t)cap) {
        orbfe_set_error("cap=%d too small for %u candidates", cap, off[nq]);
        return ORBFE_ERR_CAP;
    }
    if (off[nq] > 0) ORBFE_HIP(hipMemcpy(cand, m->b[8].p, (size_t)off[nq] * 4, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}
