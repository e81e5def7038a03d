// orbfe_cloud.hip -- the fork's dense coloured point-cloud map (reference src/pointcloudmapping.cc) on the GPU: the box paint,
// generatePointCloud + pcl::transformPointCloud + removeNaNFromPointCloud, the append and pcl::VoxelGrid.  Every step restates
// tests/cloud_oracle.py operation for operation (float where the C++ has float, double where it has double, no FMA, sums in
// the C++ order), so every record is bit-exact against it.  Layout: DESIGN.md section 8f.
//   k_cloud_generate<W>  one pixel per lane, blockIdx.y = keyframe.  W = 0 counts the surviving points of each workgroup, W = 1
//                        (after k_cloud_scan) writes them in order: wave ballot + popcount, wave totals through LDS, the
//                        workgroup's offset from the scan.  One 16-byte store per record.
//   k_cloud_scan         one workgroup: exclusive scan of the workgroup counts, the total, the per-keyframe counts.
//   k_cloud_paint        one workgroup per box, boxes of a frame one launch after the other.  Rows of the mean's window are
//                        staged in LDS and summed by lane 0 in the reference's order; the threshold test and the paint are
//                        parallel, the index list is compacted in order chunk by chunk.
//   k_cloud_minmax, k_cloud_keys, rocprim::radix_sort_pairs (stable), k_cloud_heads<W> (the same ordered compaction),
//   k_cloud_centroids    the VoxelGrid: one lane per voxel walks its points in sorted order.
#include <math.h>
#include <string.h>

#include <new>

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

// ---- generatePointCloud .. removeNaNFromPointCloud -----------------------------------------------------------------------------
struct ClGen {
    const char *depth;
    const uint8_t *bgr;
    size_t depth_stride, depth_fs, bgr_stride, bgr_fs;
    int w, npix;
    const ClFrame *frames;
    int *blk;   // W = 0: counts out; W = 1: exclusive offsets in
    float4 *out;
};

template <int W>
__global__ __launch_bounds__(CL_T) void k_cloud_generate(ClGen a)
{
    __shared__ int sWave[CL_T / 64];
    const int b = blockIdx.y, i = blockIdx.x * CL_T + threadIdx.x;
    bool keep = false;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < a.npix) {
        const int r = i / a.w, c = i - r * a.w;
        const ClFrame &f = a.frames[b];
        const float d = *(const float *)(a.depth + b * a.depth_fs + r * a.depth_stride + 4 * (size_t)c);
        float x = ((float)c - f.cx) * d / f.fx;
        float y = ((float)r - f.cy) * d / f.fy;
        float z = d;
        if (finite3(x, y, z)) {   // transformPointCloud leaves the others as they are
            const double xd = x, yd = y, zd = z;
            x = (float)(((f.m[0] * xd + f.m[1] * yd) + f.m[2] * zd) + f.m[3]);
            y = (float)(((f.m[4] * xd + f.m[5] * yd) + f.m[6] * zd) + f.m[7]);
            z = (float)(((f.m[8] * xd + f.m[9] * yd) + f.m[10] * zd) + f.m[11]);
        }
        keep = finite3(x, y, z);
        if (W && keep) {
            const uint8_t *p = a.bgr + b * a.bgr_fs + r * a.bgr_stride + 3 * (size_t)c;
            const uint32_t rgba = 0xff000000u | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
            rec = make_float4(x, y, z, __uint_as_float(rgba));
        }
    }
    const int rank = block_rank(keep, sWave);
    const size_t slot = (size_t)b * gridDim.x + blockIdx.x;
    if (!W) {
        if (threadIdx.x == 0) a.blk[slot] = block_total(sWave);
    } else if (keep) {
        a.out[a.blk[slot] + rank] = rec;
    }
}

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

// ---- draw_rect_with_depth_threshold --------------------------------------------------------------------------------------------
struct ClBox {
    int beg, W, H;
    uint8_t c[3];
};

struct ClPaint {
    const char *depth;
    uint8_t *bgr;
    size_t depth_stride, bgr_stride;
    int w;
    int *running;   // indices recorded by the boxes before this one
    int *counts;
    int *indices;
};

__device__ inline float depth_at(const ClPaint &a, int j)
{
    const int r = j / a.w, c = j - r * a.w;
    return *(const float *)(a.depth + r * a.depth_stride + 4 * (size_t)c);
}

__global__ __launch_bounds__(CL_T) void k_cloud_paint(ClPaint a, ClBox bx, int box)
{
    __shared__ float sRow[CL_ROW];
    __shared__ float sMean;
    __shared__ int sBase;
    __shared__ int sWave[CL_T / 64];
    const int tid = threadIdx.x;
    // 1. the mean depth of the inner window: lane 0 sums in row-major order
    float sum = 0.f;
    int count = 0;
    for (int k = (int)(bx.H * 0.3); (double)k < bx.H * 0.7; k++) {
        const int start = bx.beg + k * a.w;
        const int j0 = (int)((double)start + bx.W * 0.3), j1 = (int)((double)start + bx.W * 0.7);
        for (int c0 = j0; c0 < j1; c0 += CL_ROW) {
            const int m = min(CL_ROW, j1 - c0);
            for (int t = tid; t < m; t += CL_T) sRow[t] = depth_at(a, c0 + t);
            __syncthreads();
            if (tid == 0)
                for (int t = 0; t < m; t++) {
                    const float d = sRow[t];
                    if ((double)d < 0.5 || (double)d > 6) continue;
                    sum += d;
                    count++;
                }
            __syncthreads();
        }
    }
    if (tid == 0) {
        sMean = count > 0 ? sum / (float)count : 0.0f;
        sBase = *a.running;
    }
    __syncthreads();
    const float mean = sMean;
    const int base = sBase;
    // 2. the paint: every pixel of the box's rows on its own, the indices in order
    const int PW = bx.W - 2, PH = bx.H - 1;
    const long long E = PW > 0 && PH > 0 ? (long long)PW * PH : 0;
    int done = 0;
    for (long long e0 = 0; e0 < E; e0 += CL_T) {
        const long long e = e0 + tid;
        bool keep = false;
        int j = 0;
        if (e < E) {
            const int k = (int)(e / PW), jj = (int)(e - (long long)k * PW);
            j = bx.beg + k * a.w + jj;
            keep = (double)fabsf(depth_at(a, j) - mean) < 0.4;
        }
        const int rank = block_rank(keep, sWave);
        if (keep) {
            a.indices[base + done + rank] = j;
            const int r = j / a.w, c = j - r * a.w;
            uint8_t *p = a.bgr + r * a.bgr_stride + 3 * (size_t)c;
            p[0] = bx.c[0];
            p[1] = bx.c[1];
            p[2] = bx.c[2];
        }
        done += block_total(sWave);
        __syncthreads();   // sWave is rewritten by the next chunk
    }
    if (tid == 0) {
        a.counts[box] = done;
        *a.running = base + done;
    }
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

}  // namespace

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
};

static void cloud_free(orbfe_cloud *h)
{
    h->sort.release();
    h->depth.release();
    h->bgr.release();
    h->box_counts.release();
    h->frames.release();
    orb_free_all(h->stream, {h->d_map, h->d_map2, h->d_keys, h->d_keys2, h->d_vals, h->d_vals2, h->d_starts, h->d_blk, h->d_counts, h->d_scal,
                             h->d_mm, h->d_frames});
}

extern "C" orbfe_status orbfe_cloud_create(int32_t device, double resolution, int32_t max_points, int32_t max_frames, int32_t w, int32_t ht,
                                           orbfe_cloud **out)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    const float leaf = (float)resolution;
    if (!(leaf > 0.f) || !isfinite(leaf) || max_points < 1 || max_points > (1 << 30) || max_frames < 1 || w < 1 || ht < 1 ||
        (long long)max_frames * w * ht > (1LL << 30)) {
        orbfe_set_error("orbfe_cloud_create: resolution must be positive, max_points and max_frames * w * ht in [1, 2^30]");
        return ORBFE_ERR_ARG;
    }
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    orbfe_cloud *h = new (std::nothrow) orbfe_cloud();
    if (!h) return ORBFE_ERR_NOMEM;
    DeviceGuard dg(device);
    h->device = device;
    h->leaf = leaf;
    h->max_points = max_points;
    h->max_frames = max_frames;
    h->w = w;
    h->ht = ht;
    const size_t np = (size_t)max_points;
    h->nblk = (int)(blocks_of(max_points) > (size_t)max_frames * blocks_of((long long)w * ht) ? blocks_of(max_points)
                                                                                                : (size_t)max_frames * blocks_of((long long)w * ht));
    auto blk = [](auto **p, size_t bytes) { return OrbAlloc{(void **)p, bytes}; };
    bool ok = orb_alloc_all(&h->stream, {blk(&h->d_map, np * 16), blk(&h->d_map2, np * 16), blk(&h->d_keys, np * 4), blk(&h->d_keys2, np * 4),
                                          blk(&h->d_vals, np * 4), blk(&h->d_vals2, np * 4), blk(&h->d_starts, np * 4),
                                          blk(&h->d_blk, ((size_t)h->nblk + 1) * 4), blk(&h->d_counts, (size_t)max_frames * 4),
                                          blk(&h->d_scal, 16), blk(&h->d_mm, 32), blk(&h->d_frames, (size_t)max_frames * sizeof(ClFrame))});
    ok = ok && h->frames.ensure((size_t)max_frames * sizeof(ClFrame)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        orbfe_set_error("orbfe_cloud_create: device allocation failed");
        cloud_free(h);
        delete h;
        return ORBFE_ERR_NOMEM;
    }
    *out = h;
    return ORBFE_OK;
}

extern "C" void orbfe_cloud_destroy(orbfe_cloud *h)
{
    if (!h) return;
    DeviceGuard dg(h->device);
    (void)hipStreamSynchronize(h->stream);
    cloud_free(h);
    delete h;
}

extern "C" void *orbfe_cloud_get_stream(orbfe_cloud *h) { return h ? (void *)h->stream : nullptr; }
extern "C" int32_t orbfe_cloud_size(const orbfe_cloud *h) { return h ? h->size : 0; }
extern "C" const orbfe_cloud_point *orbfe_cloud_data_device(const orbfe_cloud *h) { return h ? h->d_map : nullptr; }

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// scan of d_blk[0 .. n) on st; the total comes back to the host (the stream is drained)
static orbfe_status cloud_scan(orbfe_cloud *h, int n, int seg, int nseg, int *total, hipStream_t st)
{
    k_cloud_scan<<<1, CL_SCAN_T, 0, st>>>(h->d_blk, n, seg, nseg, nseg ? h->d_counts : nullptr, h->d_scal);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(total, h->d_scal, sizeof(int), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

struct CloudPlanes {
    const float *d_depth;
    size_t depth_stride, depth_fs;
    const uint8_t *d_bgr;
    size_t bgr_stride, bgr_fs;
};

static orbfe_status cloud_check_planes(const orbfe_cloud *h, const CloudPlanes &p, int nframes, const float *intrinsics, const double *T,
                                       const char *who)
{
    if (nframes < 0 || nframes > h->max_frames) {
        orbfe_set_error("%s: %d frames outside [0, max_frames %d]", who, nframes, h->max_frames);
        return ORBFE_ERR_ARG;
    }
    if (nframes > 0 && (!p.d_depth || !p.d_bgr || !intrinsics || !T)) {
        orbfe_set_error("%s: a required pointer is NULL", who);
        return ORBFE_ERR_ARG;
    }
    if (nframes > 0 && (p.depth_stride < (size_t)h->w * 4 || (p.depth_stride & 3) || (p.depth_fs & 3) || p.bgr_stride < (size_t)h->w * 3 ||
                        (nframes > 1 && (p.depth_fs < p.depth_stride * h->ht || p.bgr_fs < p.bgr_stride * h->ht)))) {
        orbfe_set_error("%s: a stride is shorter than a row / a plane, or a depth stride is no multiple of 4", who);
        return ORBFE_ERR_ARG;
    }
    return ORBFE_OK;
}

// the surviving points of nframes keyframes into d_out (cap records), in order; *total = how many (also when they do not fit)
static orbfe_status cloud_generate(orbfe_cloud *h, const CloudPlanes &p, int nframes, const float *intrinsics, const double *T,
                                   orbfe_cloud_point *d_out, int cap, int32_t *counts, int *total, hipStream_t st)
{
    *total = 0;
    if (nframes == 0) return ORBFE_OK;
    ClFrame *f = h->frames.as<ClFrame>();
    for (int b = 0; b < nframes; b++) {
        f[b].fx = intrinsics[4 * b];
        f[b].fy = intrinsics[4 * b + 1];
        f[b].cx = intrinsics[4 * b + 2];
        f[b].cy = intrinsics[4 * b + 3];
        for (int e = 0; e < 12; e++) f[b].m[e] = T[16 * (size_t)b + e];
    }
    ORBFE_HIP(hipMemcpyAsync(h->d_frames, f, (size_t)nframes * sizeof(ClFrame), hipMemcpyHostToDevice, st));
    ClGen a = {};
    a.depth = (const char *)p.d_depth;
    a.bgr = p.d_bgr;
    a.depth_stride = p.depth_stride;
    a.depth_fs = p.depth_fs;
    a.bgr_stride = p.bgr_stride;
    a.bgr_fs = p.bgr_fs;
    a.w = h->w;
    a.npix = h->w * h->ht;
    a.frames = h->d_frames;
    a.blk = h->d_blk;
    a.out = (float4 *)d_out;
    const unsigned bpf = blocks_of(a.npix);
    const dim3 grid(bpf, (unsigned)nframes);
    k_cloud_generate<0><<<grid, CL_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    const orbfe_status s = cloud_scan(h, (int)bpf * nframes, (int)bpf, nframes, total, st);
    if (s != ORBFE_OK) return s;
    if (*total > cap) return ORBFE_ERR_CAP;
    if (*total > 0) {
        k_cloud_generate<1><<<grid, CL_T, 0, st>>>(a);
        ORBFE_HIP(hipGetLastError());
    }
    if (counts) ORBFE_HIP(hipMemcpyAsync(counts, h->d_counts, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

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
static orbfe_status cloud_voxel(orbfe_cloud *h, const orbfe_cloud_point *d_in, int n, orbfe_cloud_point *d_out, int cap, bool copy_through,
                                int *nv, int *overflow, hipStream_t st)
{
    *nv = 0;
    *overflow = 0;
    if (n == 0) return ORBFE_OK;
    const unsigned mm0[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u, 0u};
    unsigned mm[8];
    ORBFE_HIP(hipMemcpyAsync(h->d_mm, mm0, sizeof(mm0), hipMemcpyHostToDevice, st));
    const unsigned nb = blocks_of(n);
    k_cloud_minmax<<<nb < 1024 ? nb : 1024, CL_T, 0, st>>>((const float4 *)d_in, n, h->d_mm);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(mm, h->d_mm, sizeof(mm), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    const int nfin = (int)mm[6];
    if (nfin == 0) return ORBFE_OK;
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) mn[k] = ord2f(mm[k]), mx[k] = ord2f(mm[3 + k]);
    ClGrid g;
    long long cells = 0;
    if (cloud_grid(h->leaf, mn, mx, &g, &cells)) {
        *overflow = 1;
        *nv = n;
        if (!copy_through) return ORBFE_OK;
        if (n > cap) return ORBFE_ERR_CAP;
        ORBFE_HIP(hipMemcpyAsync(d_out, d_in, (size_t)n * 16, hipMemcpyDeviceToDevice, st));
        ORBFE_HIP(hipStreamSynchronize(st));
        return ORBFE_OK;
    }
    k_cloud_keys<<<nb, CL_T, 0, st>>>((const float4 *)d_in, n, g, h->d_keys, h->d_vals);
    ORBFE_HIP(hipGetLastError());
    unsigned bits = 32;   // the key of a point that is not finite is all ones
    if (nfin == n) {
        bits = 1;
        while (bits < 32 && (1LL << bits) < cells) bits++;
    }
    size_t tmp = 0;
    ORBFE_HIP(rocprim::radix_sort_pairs(nullptr, tmp, h->d_keys, h->d_keys2, h->d_vals, h->d_vals2, (size_t)n, 0u, bits, st));
    ORBFE_HIP(h->sort.ensure(tmp ? tmp : 256));
    ORBFE_HIP(rocprim::radix_sort_pairs(h->sort.p, tmp, h->d_keys, h->d_keys2, h->d_vals, h->d_vals2, (size_t)n, 0u, bits, st));
    const unsigned hb = blocks_of(nfin);
    k_cloud_heads<0><<<hb, CL_T, 0, st>>>(h->d_keys2, nfin, h->d_blk, h->d_starts);
    ORBFE_HIP(hipGetLastError());
    const orbfe_status s = cloud_scan(h, (int)hb, 0, 0, nv, st);
    if (s != ORBFE_OK) return s;
    if (*nv > cap) return ORBFE_ERR_CAP;
    k_cloud_heads<1><<<hb, CL_T, 0, st>>>(h->d_keys2, nfin, h->d_blk, h->d_starts);
    ORBFE_HIP(hipGetLastError());
    k_cloud_centroids<<<blocks_of(*nv), CL_T, 0, st>>>((const float4 *)d_in, h->d_vals2, h->d_starts, *nv, nfin, (float4 *)d_out);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_cloud_generate_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, size_t depth_frame_stride,
                                                    const uint8_t *d_bgr, size_t bgr_stride, size_t bgr_frame_stride, int32_t nframes,
                                                    const float *intrinsics, const double *T, orbfe_cloud_point *d_out, int32_t cap,
                                                    int32_t *counts, int32_t *n_out, void *stream)
{
    if (!h || !n_out || cap < 0 || (cap > 0 && !d_out) || !aligned16(d_out)) {
        orbfe_set_error("orbfe_cloud_generate_device: a required pointer is NULL, cap < 0 or d_out is not 16-byte aligned");
        return ORBFE_ERR_ARG;
    }
    const CloudPlanes p = {d_depth, depth_stride, depth_frame_stride, d_bgr, bgr_stride, bgr_frame_stride};
    orbfe_status s = cloud_check_planes(h, p, nframes, intrinsics, T, "orbfe_cloud_generate_device");
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(h->device);
    int total = 0;
    s = cloud_generate(h, p, nframes, intrinsics, T, d_out, cap, counts, &total, (hipStream_t)stream);
    *n_out = total;
    if (s == ORBFE_ERR_CAP) orbfe_set_error("orbfe_cloud_generate_device: %d points exceed cap %d", total, cap);
    return s;
}

extern "C" orbfe_status orbfe_cloud_insert_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, size_t depth_frame_stride,
                                                  const uint8_t *d_bgr, size_t bgr_stride, size_t bgr_frame_stride, int32_t nframes,
                                                  const float *intrinsics, const double *T, int32_t *counts, int32_t *n_out, int32_t *overflow,
                                                  void *stream)
{
    if (!h || !n_out) {
        orbfe_set_error("orbfe_cloud_insert_device: a required pointer is NULL");
        return ORBFE_ERR_ARG;
    }
    const CloudPlanes p = {d_depth, depth_stride, depth_frame_stride, d_bgr, bgr_stride, bgr_frame_stride};
    orbfe_status s = cloud_check_planes(h, p, nframes, intrinsics, T, "orbfe_cloud_insert_device");
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(h->device);
    hipStream_t st = (hipStream_t)stream;
    int total = 0;
    s = cloud_generate(h, p, nframes, intrinsics, T, h->d_map + h->size, h->max_points - h->size, counts, &total, st);
    if (s == ORBFE_ERR_CAP) {
        *n_out = h->size + total;
        orbfe_set_error("orbfe_cloud_insert_device: %d points exceed max_points %d", h->size + total, h->max_points);
    }
    if (s != ORBFE_OK) return s;
    int nv = 0, ovf = 0;
    s = cloud_voxel(h, h->d_map, h->size + total, h->d_map2, h->max_points, false, &nv, &ovf, st);
    if (s != ORBFE_OK) return s;
    if (!ovf) {   // on overflow the appended map stays as it is
        orbfe_cloud_point *t = h->d_map;
        h->d_map = h->d_map2;
        h->d_map2 = t;
    }
    h->size = nv;
    *n_out = nv;
    if (overflow) *overflow = ovf;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_cloud_insert(orbfe_cloud *h, const float *depth, const uint8_t *bgr, const float *intrinsics, const double *T,
                                           int32_t *n_out, int32_t *overflow)
{
    if (!h || !depth || !bgr || !intrinsics || !T || !n_out) {
        orbfe_set_error("orbfe_cloud_insert: a required pointer is NULL");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    const size_t np = (size_t)h->w * h->ht;
    ORBFE_HIP(h->depth.ensure(np * 4));
    ORBFE_HIP(h->bgr.ensure(np * 3));
    ORBFE_HIP(hipMemcpyAsync(h->depth.p, depth, np * 4, hipMemcpyHostToDevice, h->stream));
    ORBFE_HIP(hipMemcpyAsync(h->bgr.p, bgr, np * 3, hipMemcpyHostToDevice, h->stream));
    return orbfe_cloud_insert_device(h, h->depth.as<float>(), (size_t)h->w * 4, np * 4, h->bgr.as<uint8_t>(), (size_t)h->w * 3, np * 3, 1, intrinsics,
                                     T, nullptr, n_out, overflow, h->stream);
}

extern "C" orbfe_status orbfe_cloud_voxel_filter_device(orbfe_cloud *h, const orbfe_cloud_point *d_in, int32_t n, orbfe_cloud_point *d_out,
                                                        int32_t cap, int32_t *n_out, int32_t *overflow, void *stream)
{
    if (!h || !n_out || n < 0 || cap < 0 || (n > 0 && !d_in) || (cap > 0 && !d_out) || !aligned16(d_in) || !aligned16(d_out)) {
        orbfe_set_error("orbfe_cloud_voxel_filter_device: a required pointer is NULL, a size is negative or a buffer is not 16-byte aligned");
        return ORBFE_ERR_ARG;
    }
    if (n > h->max_points) {
        orbfe_set_error("orbfe_cloud_voxel_filter_device: %d points exceed max_points %d", n, h->max_points);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    int nv = 0, ovf = 0;
    const orbfe_status s = cloud_voxel(h, d_in, n, d_out, cap, true, &nv, &ovf, (hipStream_t)stream);
    *n_out = nv;
    if (overflow) *overflow = ovf;
    if (s == ORBFE_ERR_CAP) orbfe_set_error("orbfe_cloud_voxel_filter_device: %d records exceed cap %d", nv, cap);
    return s;
}

extern "C" orbfe_status orbfe_cloud_download(orbfe_cloud *h, orbfe_cloud_point *dst, int32_t cap, int32_t *n_out)
{
    if (!h || !n_out || cap < 0 || (cap > 0 && !dst)) return ORBFE_ERR_ARG;
    *n_out = h->size;
    if (h->size > cap) return ORBFE_ERR_CAP;
    if (h->size == 0) return ORBFE_OK;
    DeviceGuard dg(h->device);
    ORBFE_HIP(hipMemcpy(dst, h->d_map, (size_t)h->size * 16, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_cloud_upload_device(orbfe_cloud *h, const orbfe_cloud_point *d_points, int32_t n, void *stream)
{
    if (!h || n < 0 || (n > 0 && !d_points)) return ORBFE_ERR_ARG;
    if (n > h->max_points) {
        orbfe_set_error("orbfe_cloud_upload_device: %d points exceed max_points %d", n, h->max_points);
        return ORBFE_ERR_CAP;
    }
    DeviceGuard dg(h->device);
    if (n > 0) {
        ORBFE_HIP(hipMemcpyAsync(h->d_map, d_points, (size_t)n * 16, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        ORBFE_HIP(hipStreamSynchronize((hipStream_t)stream));
    }
    h->size = n;
    return ORBFE_OK;
}

// the flat indices [lo, hi] the reference touches for the box; false: none
static bool box_touched(const ClBox &b, int w, long long *lo, long long *hi)
{
    bool any = false;
    auto see = [&](long long a, long long e) {   // [a, e)
        if (e <= a) return;
        if (!any || a < *lo) *lo = a;
        if (!any || e - 1 > *hi) *hi = e - 1;
        any = true;
    };
    for (int k = (int)(b.H * 0.3); (double)k < b.H * 0.7; k++) {
        const long long start = (long long)b.beg + (long long)k * w;
        see((long long)((double)start + b.W * 0.3), (long long)((double)start + b.W * 0.7));
    }
    for (int k = 0; k < b.H - 1; k++) {
        const long long start = (long long)b.beg + (long long)k * w;
        see(start, start + b.W - 1 - 1);
    }
    return any;
}

extern "C" orbfe_status orbfe_cloud_paint_boxes_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, uint8_t *d_bgr,
                                                       size_t bgr_stride, const float *boxes, const uint8_t *colors, int32_t nboxes,
                                                       int32_t *d_indices, int32_t idx_cap, int32_t *counts, int32_t *n_out, void *stream)
{
    if (!h || !n_out || nboxes < 0 || idx_cap < 0 || (nboxes > 0 && (!d_depth || !d_bgr || !boxes || !colors)) || (idx_cap > 0 && !d_indices)) {
        orbfe_set_error("orbfe_cloud_paint_boxes_device: a required pointer is NULL or a size is negative");
        return ORBFE_ERR_ARG;
    }
    *n_out = 0;
    if (nboxes == 0) return ORBFE_OK;
    if (depth_stride < (size_t)h->w * 4 || (depth_stride & 3) || bgr_stride < (size_t)h->w * 3) {
        orbfe_set_error("orbfe_cloud_paint_boxes_device: a stride is shorter than a row, or the depth stride is no multiple of 4");
        return ORBFE_ERR_ARG;
    }
    std::vector<ClBox> bx((size_t)nboxes);
    const long long npix = (long long)h->w * h->ht;
    long long most = 0;
    for (int b = 0; b < nboxes; b++) {
        const float *r = boxes + 4 * (size_t)b;
        for (int e = 0; e < 4; e++)
            if (!isfinite(r[e]) || fabsf(r[e]) >= (float)CL_BOX_LIMIT) {
                orbfe_set_error("orbfe_cloud_paint_boxes_device: box %d is not finite or reaches 2^20", b);
                return ORBFE_ERR_ARG;
            }
        const long long beg = (long long)(int)r[0] + ((long long)(int)r[1] - 1) * h->w - 1;
        if (beg < -(1LL << 30) || beg > (1LL << 30)) {
            orbfe_set_error("orbfe_cloud_paint_boxes_device: box %d lies outside the image", b);
            return ORBFE_ERR_ARG;
        }
        bx[b].beg = (int)beg;
        bx[b].W = (int)r[2];
        bx[b].H = (int)r[3];
        for (int e = 0; e < 3; e++) bx[b].c[e] = colors[3 * (size_t)b + e];
        long long lo = 0, hi = 0;
        if (box_touched(bx[b], h->w, &lo, &hi) && (lo < 0 || hi >= npix)) {
            orbfe_set_error("orbfe_cloud_paint_boxes_device: box %d reaches outside the image (indices %lld .. %lld of %lld)", b, lo, hi, npix);
            return ORBFE_ERR_ARG;
        }
        if (bx[b].W - 2 > h->w) {
            orbfe_set_error("orbfe_cloud_paint_boxes_device: box %d is wider than the image", b);
            return ORBFE_ERR_ARG;
        }
        if (bx[b].W > 2 && bx[b].H > 1) most += (long long)(bx[b].W - 2) * (bx[b].H - 1);
    }
    if (most > idx_cap) {
        *n_out = most > INT32_MAX ? INT32_MAX : (int32_t)most;
        orbfe_set_error("orbfe_cloud_paint_boxes_device: the boxes can record %lld indices, idx_cap is %d", most, idx_cap);
        return ORBFE_ERR_CAP;
    }
    DeviceGuard dg(h->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(h->box_counts.ensure((size_t)nboxes * 4));
    ORBFE_HIP(hipMemsetAsync(h->d_scal + 1, 0, 4, st));
    ClPaint a = {};
    a.depth = (const char *)d_depth;
    a.bgr = d_bgr;
    a.depth_stride = depth_stride;
    a.bgr_stride = bgr_stride;
    a.w = h->w;
    a.running = h->d_scal + 1;
    a.counts = h->box_counts.as<int>();
    a.indices = d_indices;
    for (int b = 0; b < nboxes; b++) {   // in list order: a later box paints over an earlier one
        k_cloud_paint<<<1, CL_T, 0, st>>>(a, bx[b], b);
        ORBFE_HIP(hipGetLastError());
    }
    if (counts) ORBFE_HIP(hipMemcpyAsync(counts, a.counts, (size_t)nboxes * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(n_out, h->d_scal + 1, 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

// Converter::toSE3Quat + Isometry3d::inverse().matrix() (oracle P15, P16)
extern "C" orbfe_status orbfe_cloud_pose_matrix(const float Tcw[16], double out[16])
{
    if (!Tcw || !out) return ORBFE_ERR_ARG;
    double R[3][3], t[3], q[4] = {0, 0, 0, 0};   // q = x, y, z, w
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[i][j] = (double)Tcw[4 * i + j];
        t[i] = (double)Tcw[4 * i + 3];
    }
    const double tr = (R[0][0] + R[1][1]) + R[2][2];
    if (tr > 0) {
        double s = sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[1][0] - R[0][1]) * s;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0);
        q[i] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[k][j] - R[j][k]) * s;
        q[j] = (R[j][i] + R[i][j]) * s;
        q[k] = (R[k][i] + R[i][k]) * s;
    }
    if (q[3] < 0)
        for (int e = 0; e < 4; e++) q[e] *= -1.0;
    const double nrm = sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
    const double x = q[0] / nrm, y = q[1] / nrm, z = q[2] / nrm, w = q[3] / nrm;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double Rn[3][3] = {{1.0 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1.0 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1.0 - (txx + tyy)}};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) out[4 * r + c] = Rn[c][r];
        out[4 * r + 3] = -((Rn[0][r] * t[0] + Rn[1][r] * t[1]) + Rn[2][r] * t[2]);
    }
    out[12] = out[13] = out[14] = 0.0;
    out[15] = 1.0;
    return ORBFE_OK;
}
