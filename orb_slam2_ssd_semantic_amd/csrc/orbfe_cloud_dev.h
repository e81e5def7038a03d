// orbfe_cloud_dev.h -- what orbfe_cloud.hip and orbfe_objects.hip share: the handle, the per-pixel point of generatePointCloud +
// transformPointCloud, the ordered-compaction helpers, the scan and the pcl::VoxelGrid kernels with their driver.  Everything
// sits in an unnamed namespace: each translation unit gets its own copy.  Include after orbfe_common.h and orbfe_host.h.
#pragma once

#include <math.h>
#include <string.h>

#include "orbfe_common.h"
#include "orbfe_host.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int CL_T = 256;        // workgroup of every kernel but the scan
constexpr int CL_SCAN_T = 1024;
constexpr int CL_ROW = 1024;     // floats of a mean row staged at once
constexpr int CL_BOX_LIMIT = 1 << 20;

struct ClFrame {
    float fx, fy, cx, cy;
    double m[12];   // the upper three rows of T.inverse().matrix()
};

// rank of a kept lane among the kept lanes of its workgroup, the wave totals in sWave
__device__ inline int block_rank(bool keep, int *sWave)
{
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sWave[wv] = __popcll(bal);
    __syncthreads();
    int r = __popcll(bal & ((1ull << lane) - 1ull));
    for (int k = 0; k < wv; k++) r += sWave[k];
    return r;
}

__device__ inline int block_total(const int *sWave) { return (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]); }

__device__ inline bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// generatePointCloud + transformPointCloud for pixel (r, c) of depth d: the point as the organised cloud holds it (one that is not
// finite is left as it is)
__device__ inline void cloud_point(const ClFrame &f, int r, int c, float d, float *px, float *py, float *pz)
{
    float x = ((float)c - f.cx) * d / f.fx;
    float y = ((float)r - f.cy) * d / f.fy;
    float z = d;
    if (finite3(x, y, z)) {   // transformPointCloud leaves the others as they are
        const double xd = x, yd = y, zd = z;
        x = (float)(((f.m[0] * xd + f.m[1] * yd) + f.m[2] * zd) + f.m[3]);
        y = (float)(((f.m[4] * xd + f.m[5] * yd) + f.m[6] * zd) + f.m[7]);
        z = (float)(((f.m[8] * xd + f.m[9] * yd) + f.m[10] * zd) + f.m[11]);
    }
    *px = x;
    *py = y;
    *pz = z;
}

__device__ inline uint32_t cloud_rgba(const uint8_t *p) { return 0xff000000u | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0]; }

// in place: blk[i] = sum of blk[0 .. i), blk[n] = *total = the sum; seg_counts[s] = the sum over segment s of `seg` entries
__global__ __launch_bounds__(CL_SCAN_T) void k_cloud_scan(int *blk, int n, int seg, int nseg, int *seg_counts, int *total)
{
    __shared__ int sW[CL_SCAN_T / 64];
    __shared__ int sCarry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) sCarry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += CL_SCAN_T) {
        const int i = base + tid;
        const int v = i < n ? blk[i] : 0;
        int inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) sW[wv] = inc;
        __syncthreads();
        int before = sCarry;
        for (int k = 0; k < wv; k++) before += sW[k];
        if (i < n) blk[i] = before + inc - v;
        __syncthreads();
        if (tid == CL_SCAN_T - 1) sCarry = before + inc;
        __syncthreads();
    }
    if (tid == 0) {
        blk[n] = sCarry;
        *total = sCarry;
    }
    __syncthreads();
    if (seg_counts)
        for (int s = tid; s < nseg; s += CL_SCAN_T) seg_counts[s] = blk[(s + 1) * seg] - blk[s * seg];
}

// ---- pcl::VoxelGrid ------------------------------------------------------------------------------------------------------------
// floats as unsigned integers of the same order
__device__ inline unsigned f2ord(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float ord2f(unsigned o)
{
    const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// mm[0 .. 2] = min x, y, z; mm[3 .. 5] = max; mm[6] = finite points (getMinMax3D over them)
__global__ __launch_bounds__(CL_T) void k_cloud_minmax(const float4 *pts, int n, unsigned *mm)
{
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    int cnt = 0;
    for (int i = blockIdx.x * CL_T + threadIdx.x; i < n; i += gridDim.x * CL_T) {
        const float4 p = pts[i];
        if (!finite3(p.x, p.y, p.z)) continue;
        const unsigned o[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
        for (int k = 0; k < 3; k++) {
            lo[k] = min(lo[k], o[k]);
            hi[k] = max(hi[k], o[k]);
        }
        cnt++;
    }
    for (int s = 32; s > 0; s >>= 1) {
        for (int k = 0; k < 3; k++) {
            lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], s));
            hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], s));
        }
        cnt += __shfl_xor(cnt, s);
    }
    if ((threadIdx.x & 63) == 0 && cnt > 0) {
        for (int k = 0; k < 3; k++) {
            atomicMin(&mm[k], lo[k]);
            atomicMax(&mm[3 + k], hi[k]);
        }
        atomicAdd(&mm[6], (unsigned)cnt);
    }
}

struct ClGrid {
    float inv;
    float min_b[3];   // (float)min_b
    int mul[3];
};

// idx of every point; a point that is not finite gets the last key and sorts behind the finite ones
__global__ __launch_bounds__(CL_T) void k_cloud_keys(const float4 *pts, int n, ClGrid g, uint32_t *keys, uint32_t *vals)
{
    const int i = blockIdx.x * CL_T + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    uint32_t key = 0xffffffffu;
    if (finite3(p.x, p.y, p.z)) {
        const int i0 = (int)(floorf(p.x * g.inv) - g.min_b[0]);
        const int i1 = (int)(floorf(p.y * g.inv) - g.min_b[1]);
        const int i2 = (int)(floorf(p.z * g.inv) - g.min_b[2]);
        key = (uint32_t)(i0 * g.mul[0] + i1 * g.mul[1] + i2 * g.mul[2]);
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// the first sorted position of every voxel, in order (the compaction of k_cloud_generate)
template <int W>
__global__ __launch_bounds__(CL_T) void k_cloud_heads(const uint32_t *keys, int n, int *blk, int *starts)
{
    __shared__ int sWave[CL_T / 64];
    const int j = blockIdx.x * CL_T + threadIdx.x;
    const bool head = j < n && (j == 0 || keys[j] != keys[j - 1]);
    const int rank = block_rank(head, sWave);
    if (!W) {
        if (threadIdx.x == 0) blk[blockIdx.x] = block_total(sWave);
    } else if (head) {
        starts[blk[blockIdx.x] + rank] = j;
    }
}

// pcl::CentroidPoint per voxel: float sums in sorted order, a true division by (float)n
__global__ __launch_bounds__(CL_T) void k_cloud_centroids(const float4 *pts, const uint32_t *vals, const int *starts, int nv, int n, float4 *out)
{
    const int v = blockIdx.x * CL_T + threadIdx.x;
    if (v >= nv) return;
    const int a = starts[v], b = v + 1 < nv ? starts[v + 1] : n;
    float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;
    for (int j = a; j < b; j++) {
        const float4 p = pts[vals[j]];
        const uint32_t c = __float_as_uint(p.w);
        sx += p.x;
        sy += p.y;
        sz += p.z;
        sa += (float)(c >> 24);
        sr += (float)((c >> 16) & 255u);
        sg += (float)((c >> 8) & 255u);
        sb += (float)(c & 255u);
    }
    const float cnt = (float)(b - a);
    const uint32_t rgba = ((uint32_t)(sa / cnt) << 24) | ((uint32_t)(sr / cnt) << 16) | ((uint32_t)(sg / cnt) << 8) | (uint32_t)(sb / cnt);
    out[v] = make_float4(sx / cnt, sy / cnt, sz / cnt, __uint_as_float(rgba));
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + CL_T - 1) / CL_T); }

// (int64)v where C++ defines it
inline bool to_i64(float v, long long *out)
{
    if (!(v >= -9223372036854775808.0f && v < 9223372036854775808.0f)) return false;
    *out = (long long)v;
    return true;
}

// the device blocks one VoxelGrid pass works in: n entries each but blk (blocks_of(n) + 1), scal (1) and mm (8)
struct ClVoxScratch {
    uint32_t *keys, *keys2, *vals, *vals2;
    int *starts, *blk, *scal;
    unsigned *mm;
    DevBuf *sort;   // rocprim's scratch
};

// scan of blk[0 .. n) on st; the total comes back to the host (the stream is drained)
inline orbfe_status cloud_scan_blocks(int *blk, int *seg_counts, int *scal, int n, int seg, int nseg, int *total, hipStream_t st)
{
    k_cloud_scan<<<1, CL_SCAN_T, 0, st>>>(blk, n, seg, nseg, nseg ? seg_counts : nullptr, scal);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(total, scal, sizeof(int), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

// getMinMax3D over the finite points of pts[0 .. n): mn, mx and their number (the stream is drained)
inline orbfe_status cloud_minmax(unsigned *d_mm, const float4 *pts, int n, float *mn, float *mx, int *nfin, hipStream_t st)
{
    const unsigned mm0[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    unsigned mm[8];
    ORBFE_HIP(hipMemcpyAsync(d_mm, mm0, sizeof(mm0), hipMemcpyHostToDevice, st));
    const unsigned nb = blocks_of(n);
    k_cloud_minmax<<<nb < 1024 ? nb : 1024, CL_T, 0, st>>>(pts, n, d_mm);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    *nfin = (int)mm[6];
    for (int k = 0; k < 3; k++) mn[k] = ord2f(mm[k]), mx[k] = ord2f(mm[3 + k]);
    return ORBFE_OK;
}

// voxel_plan of the oracle: 0 = a grid, 1 = overflow
// voxel_plan of the oracle: 0 = a grid, 1 = overflow
static int cloud_grid(float leaf, const float *mn, const float *mx, ClGrid *g, long long *cells)
{
    const float inv = 1.0f / leaf;
    long long d[3], lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        if (!to_i64((mx[k] - mn[k]) * inv, &d[k]) || !to_i64(floorf(mn[k] * inv), &lo[k]) || !to_i64(floorf(mx[k] * inv), &hi[k])) return 1;
        d[k] += 1;
        if (lo[k] > INT32_MAX || lo[k] < -(long long)INT32_MAX || hi[k] > INT32_MAX || hi[k] < -(long long)INT32_MAX) return 1;
    }
    if ((__int128)d[0] * d[1] * d[2] > INT32_MAX) return 1;
    long long div[3];
    for (int k = 0; k < 3; k++) div[k] = hi[k] - lo[k] + 1;
    if ((__int128)div[0] * div[1] * div[2] > INT32_MAX) return 1;
    g->inv = inv;
    for (int k = 0; k < 3; k++) g->min_b[k] = (float)(int)lo[k];
    g->mul[0] = 1;
    g->mul[1] = (int)div[0];
    g->mul[2] = (int)(div[0] * div[1]);
    *cells = div[0] * div[1] * div[2];
    return 0;
}

// VoxelGrid over d_in[0 .. n) into d_out (cap records); copy_through: on overflow d_out receives the input (else the caller keeps d_in)
inline orbfe_status cloud_voxel_run(const ClVoxScratch &s, float leaf, const orbfe_cloud_point *d_in, int n, orbfe_cloud_point *d_out, int cap,
                                    bool copy_through, int *nv, int *overflow, hipStream_t st)
{
    *nv = 0;
    *overflow = 0;
    if (n == 0) return ORBFE_OK;
    float mn[3], mx[3];
    int nfin = 0;
    const orbfe_status ms = cloud_minmax(s.mm, (const float4 *)d_in, n, mn, mx, &nfin, st);
    if (ms != ORBFE_OK) return ms;
    if (nfin == 0) return ORBFE_OK;
    const unsigned nb = blocks_of(n);
    ClGrid g;
    long long cells = 0;
    if (cloud_grid(leaf, mn, mx, &g, &cells)) {
        *overflow = 1;
        *nv = n;
        if (!copy_through) return ORBFE_OK;
        if (n > cap) return ORBFE_ERR_CAP;
        ORBFE_HIP(hipMemcpyAsync(d_out, d_in, (size_t)n * 16, hipMemcpyDeviceToDevice, st));
        ORBFE_HIP(hipStreamSynchronize(st));
        return ORBFE_OK;
    }
    k_cloud_keys<<<nb, CL_T, 0, st>>>((const float4 *)d_in, n, g, s.keys, s.vals);
    ORBFE_HIP(hipGetLastError());
    unsigned bits = 32;   // the key of a point that is not finite is all ones
    if (nfin == n) {
        bits = 1;
        while (bits < 32 && (1LL << bits) < cells) bits++;
    }
    size_t tmp = 0;
    ORBFE_HIP(rocprim::radix_sort_pairs(nullptr, tmp, s.keys, s.keys2, s.vals, s.vals2, (size_t)n, 0u, bits, st));
    ORBFE_HIP(s.sort->ensure(tmp ? tmp : 256));
    ORBFE_HIP(rocprim::radix_sort_pairs(s.sort->p, tmp, s.keys, s.keys2, s.vals, s.vals2, (size_t)n, 0u, bits, st));
    const unsigned hb = blocks_of(nfin);
    k_cloud_heads<0><<<hb, CL_T, 0, st>>>(s.keys2, nfin, s.blk, s.starts);
    ORBFE_HIP(hipGetLastError());
    const orbfe_status ss = cloud_scan_blocks(s.blk, nullptr, s.scal, (int)hb, 0, 0, nv, st);
    if (ss != ORBFE_OK) return ss;
    if (*nv > cap) return ORBFE_ERR_CAP;
    k_cloud_heads<1><<<hb, CL_T, 0, st>>>(s.keys2, nfin, s.blk, s.starts);
    ORBFE_HIP(hipGetLastError());
    k_cloud_centroids<<<blocks_of(*nv), CL_T, 0, st>>>((const float4 *)d_in, s.vals2, s.starts, *nv, nfin, (float4 *)d_out);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

}  // namespace

struct ObjScratch;
void orbfe_objects_scratch_free(ObjScratch *s);   // orbfe_objects.hip

struct orbfe_cloud {
    int device = 0;
    hipStream_t stream = nullptr;
    float leaf = 0.f;
    int max_points = 0, max_frames = 0, w = 0, ht = 0;
    int nblk = 0;   // entries of d_blk less one
    int size = 0;
    orbfe_cloud_point *d_map = nullptr, *d_map2 = nullptr;
    uint32_t *d_keys = nullptr, *d_keys2 = nullptr, *d_vals = nullptr, *d_vals2 = nullptr;
    int *d_starts = nullptr, *d_blk = nullptr, *d_counts = nullptr, *d_scal = nullptr;   // d_scal[0]: a scan's total, [1]: the paint's running count
    unsigned *d_mm = nullptr;
    ClFrame *d_frames = nullptr;
    DevBuf sort, depth, bgr, box_counts;   // rocprim's scratch, the host form's planes, the paint's per-box counts
    PinBuf frames;                   // ClFrame [max_frames]
    ObjScratch *obj = nullptr;       // orbfe_objects.hip's blocks: none until one of its entry points is called
};
