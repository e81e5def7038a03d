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
// The per-pixel point, the scan and the VoxelGrid kernels with their driver live in orbfe_cloud_dev.h, which orbfe_objects.hip
// (the outlier filter and the 3-D objects) shares.
#include <new>

#include "orbfe_cloud_dev.h"

namespace {

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
        float x, y, z;
        cloud_point(f, r, c, d, &x, &y, &z);
        keep = finite3(x, y, z);
        if (W && keep) {
            const uint8_t *p = a.bgr + b * a.bgr_fs + r * a.bgr_stride + 3 * (size_t)c;
            rec = make_float4(x, y, z, __uint_as_float(cloud_rgba(p)));
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

}  // namespace

static void cloud_free(orbfe_cloud *h)
{
    h->sort.release();
    h->depth.release();
    h->bgr.release();
    h->box_counts.release();
    h->frames.release();
    orbfe_objects_scratch_free(h->obj);
    h->obj = nullptr;
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

static orbfe_status cloud_scan(orbfe_cloud *h, int n, int seg, int nseg, int *total, hipStream_t st)
{
    return cloud_scan_blocks(h->d_blk, h->d_counts, h->d_scal, n, seg, nseg, total, st);
}

static orbfe_status cloud_voxel(orbfe_cloud *h, const orbfe_cloud_point *d_in, int n, orbfe_cloud_point *d_out, int cap, bool copy_through,
                                int *nv, int *overflow, hipStream_t st)
{
    const ClVoxScratch s = {h->d_keys, h->d_keys2, h->d_vals, h->d_vals2, h->d_starts, h->d_blk, h->d_scal, h->d_mm, &h->sort};
    return cloud_voxel_run(s, h->leaf, d_in, n, d_out, cap, copy_through, nv, overflow, st);
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
