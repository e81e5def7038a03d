// orbfe_objects.hip -- the fork's 3-D objects (reference src/pointcloudmapping.cc:441-479 and sem_merge, :246-322): per detected
// box ExtractIndices, pcl::StatisticalOutlierRemoval, pcl::VoxelGrid, compute3DCentroid, getMinMax3D on the GPU, and the cluster
// database on the host.  Every step restates tests/objects_oracle.py (assumptions O1 .. O12 there) operation for operation, so
// every record is bit-exact against it.  Layout, the stop rule's argument and the kernel table: DESIGN.md section 8g.
//   k_obj_gather        one listed pixel per lane: the organised cloud's point (cloud_point of orbfe_cloud_dev.h) and its colour.
//   k_knn_brute         one query per wave, 4 per workgroup; the object's points pass through LDS 256 at a time, each lane takes
//                       one candidate, the wave keeps its 64 smallest squared distances sorted across the lanes (wave_select).
//   k_obj_cellkeys, rocprim::radix_sort_pairs, k_obj_sorted, k_obj_cellstart, k_knn_grid
//                       the same selection fed from a uniform cell grid the host plans per object: one wave per query walks
//                       Chebyshev shells of cells until the (mean_k + 1)-th smallest cannot be undercut any more.
//   k_obj_mask, k_obj_compact<W>, k_obj_centroid   the keep mask, the ordered compaction (count / scan / write), the serial float
//                       sums of compute3DCentroid.
// The threshold's two serial double sums run on the host over the distances read back: the calls are synchronous anyway.
#include <math.h>

#include <new>
#include <vector>

#include "orbfe_cloud_dev.h"

struct ObjScratch {
    DevBuf pts, dist, keep, sorted, keys, keys2, vals, vals2, cell_start, starts, blk, scal, mm, sort, kept_pts, kept_idx, vox, cen, frame, idx;
    std::vector<float> hdist;
    std::vector<orbfe_filter_stat> stats;
    DevBuf *all[20] = {&pts, &dist, &keep, &sorted, &keys, &keys2, &vals, &vals2, &cell_start, &starts, &blk, &scal, &mm, &sort, &kept_pts, &kept_idx,
                       &vox, &cen, &frame, &idx};
    size_t bytes() const
    {
        size_t b = 0;
        for (const DevBuf *d : all) b += d->bytes;
        return b;
    }
};

void orbfe_objects_scratch_free(ObjScratch *s)
{
    if (!s) return;
    for (DevBuf *d : s->all) d->release();
    delete s;
}

namespace {

constexpr int KNN_AUTO_BRUTE = 2048;   // mode 0: objects of at most this many finite points go through k_knn_brute
constexpr int KNN_MAX_DIM = 1000;      // cells per axis: keeps the cell coordinate's rounding error below 2^-11 of a cell
constexpr long long KNN_MAX_CELLS = 1LL << 22;

// ---- the selection: the 64 smallest of everything seen, ascending across the lanes ------------------------------------------------
__device__ inline float cmpx(float v, int j, bool take_min)
{
    const float o = __shfl_xor(v, j);
    return take_min ? fminf(v, o) : fmaxf(v, o);
}

// c: one candidate per lane (+inf: none).  Candidates that are not below the (mean_k + 1)-th smallest cannot change the first
// mean_k + 1 entries, so a batch without one is dropped.
__device__ inline float wave_select(float best, float c, int mean_k, int lane)
{
    const float kth = __shfl(best, mean_k);
    if (__ballot(c < kth) == 0ull) return best;
    for (int k = 2; k <= 64; k <<= 1)   // bitonic sort of the batch, ascending
        for (int j = k >> 1; j > 0; j >>= 1) c = cmpx(c, j, ((lane & j) == 0) == ((lane & k) == 0));
    c = __shfl(c, 63 - lane);           // descending: min(best, c) holds the 64 smallest of both and is bitonic
    best = fminf(best, c);
    for (int j = 32; j > 0; j >>= 1) best = cmpx(best, j, (lane & j) == 0);
    return best;
}

// FLANN's L2_Simple<float>
__device__ inline float dist2(float qx, float qy, float qz, float px, float py, float pz)
{
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// distances[i] of applyFilterIndices from the sorted selection: entries 1 .. mean_k, square roots in double, summed in order
__device__ inline float knn_mean(float best, int mean_k)
{
    const double root = sqrt((double)best);
    double sum = 0.0;
    for (int k = 1; k <= mean_k; k++) sum += __shfl(root, k);
    return (float)(sum / (double)mean_k);
}

__global__ __launch_bounds__(CL_T) void k_knn_brute(const float4 *pts, int n, int mean_k, float *dist)
{
    __shared__ float4 tile[CL_T];
    const int tid = threadIdx.x, lane = tid & 63, qi = blockIdx.x * (CL_T / 64) + (tid >> 6);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (qi < n) q = pts[qi];
    const bool active = qi < n && finite3(q.x, q.y, q.z);   // the same for every lane of a wave
    float best = INFINITY;
    for (int base = 0; base < n; base += CL_T) {
        const int i = base + tid;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) {
            p = pts[i];
            p.w = finite3(p.x, p.y, p.z) ? 1.f : 0.f;
        }
        tile[tid] = p;
        __syncthreads();
        if (active)
            for (int b = 0; b < CL_T && base + b < n; b += 64) {
                const float4 t = tile[b + lane];
                best = wave_select(best, t.w != 0.f ? dist2(q.x, q.y, q.z, t.x, t.y, t.z) : INFINITY, mean_k, lane);
            }
        __syncthreads();
    }
    if (active) {
        const float d = knn_mean(best, mean_k);
        if (lane == 0) dist[qi] = d;
    }
}

// ---- the cell grid ---------------------------------------------------------------------------------------------------------------
struct KnnGrid {
    int dims[3];
    float mn[3];
    float inv;   // cells per metre
    float sm;    // a little less than a cell's edge: what lies outside shells 0 .. r is further than r * sm away
};

__device__ inline int cell_of(float p, float mn, float inv, int dim)
{
    const int c = (int)((p - mn) * inv);
    return c < dim - 1 ? c : dim - 1;
}

__global__ __launch_bounds__(CL_T) void k_obj_cellkeys(const float4 *pts, int n, KnnGrid g, uint32_t *keys, uint32_t *vals)
{
    const int i = blockIdx.x * CL_T + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    uint32_t key = 0xffffffffu;   // a point that is not finite sorts behind the others
    if (finite3(p.x, p.y, p.z))
        key = (uint32_t)((cell_of(p.z, g.mn[2], g.inv, g.dims[2]) * g.dims[1] + cell_of(p.y, g.mn[1], g.inv, g.dims[1])) * g.dims[0] +
                         cell_of(p.x, g.mn[0], g.inv, g.dims[0]));
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(CL_T) void k_obj_sorted(const float4 *pts, const uint32_t *vals, int nfin, float4 *sorted)
{
    const int j = blockIdx.x * CL_T + threadIdx.x;
    if (j >= nfin) return;
    const uint32_t i = vals[j];
    const float4 p = pts[i];
    sorted[j] = make_float4(p.x, p.y, p.z, __uint_as_float(i));
}

// cell_start[c] = the first sorted position whose key is >= c, c = 0 .. cells
__global__ __launch_bounds__(CL_T) void k_obj_cellstart(const uint32_t *keys, int nfin, int cells, int *cell_start)
{
    const int c = blockIdx.x * CL_T + threadIdx.x;
    if (c > cells) return;
    int lo = 0, hi = nfin;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < (uint32_t)c) lo = mid + 1;
        else hi = mid;
    }
    cell_start[c] = lo;
}

__device__ inline float knn_run(const float4 *sp, int a, int b, float4 q, float best, int mean_k, int lane)
{
    for (int base = a; base < b; base += 64) {
        const int i = base + lane;
        float c = INFINITY;
        if (i < b) {
            const float4 p = sp[i];
            c = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
        }
        best = wave_select(best, c, mean_k, lane);
    }
    return best;
}

__global__ __launch_bounds__(CL_T) void k_knn_grid(const float4 *sp, const int *cell_start, int nfin, KnnGrid g, int mean_k, float *dist)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * (CL_T / 64) + (threadIdx.x >> 6);
    if (j >= nfin) return;   // whole waves
    const float4 q = sp[j];
    const int c0 = cell_of(q.x, g.mn[0], g.inv, g.dims[0]), c1 = cell_of(q.y, g.mn[1], g.inv, g.dims[1]), c2 = cell_of(q.z, g.mn[2], g.inv, g.dims[2]);
    const int d0 = g.dims[0], d1 = g.dims[1], d2 = g.dims[2];
    const int rmax = max(max(max(c0, d0 - 1 - c0), max(c1, d1 - 1 - c1)), max(c2, d2 - 1 - c2));
    float best = INFINITY;
    for (int r = 0;; r++) {
        const int z0 = max(c2 - r, 0), z1 = min(c2 + r, d2 - 1), y0 = max(c1 - r, 0), y1 = min(c1 + r, d1 - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                const int row = (z * d1 + y) * d0;
                if (abs(z - c2) == r || abs(y - c1) == r) {   // a face row: every x of the shell, one run of the sorted points
                    best = knn_run(sp, cell_start[row + max(c0 - r, 0)], cell_start[row + min(c0 + r, d0 - 1) + 1], q, best, mean_k, lane);
                } else {                                      // only the two end cells
                    if (c0 - r >= 0) best = knn_run(sp, cell_start[row + c0 - r], cell_start[row + c0 - r + 1], q, best, mean_k, lane);
                    if (c0 + r < d0) best = knn_run(sp, cell_start[row + c0 + r], cell_start[row + c0 + r + 1], q, best, mean_k, lane);
                }
            }
        if (r >= rmax) break;   // the object has been searched whole
        const float reach = (float)r * g.sm;   // what lies outside shells 0 .. r is further away than this
        if (__shfl(best, mean_k) <= reach * reach) break;
    }
    const float d = knn_mean(best, mean_k);
    if (lane == 0) dist[__float_as_uint(q.w)] = d;
}

// ---- gather, mask, compaction, centroid --------------------------------------------------------------------------------------------
struct ObjGather {
    const char *depth;
    const uint8_t *bgr;
    size_t depth_stride, bgr_stride;
    int w, npix;
    const ClFrame *frame;
    const int *idx;
    int total;
    float4 *out;
};

__global__ __launch_bounds__(CL_T) void k_obj_gather(ObjGather a)
{
    const int e = blockIdx.x * CL_T + threadIdx.x;
    if (e >= a.total) return;
    const int j = a.idx[e];
    float4 rec = make_float4(NAN, NAN, NAN, __uint_as_float(0xff000000u));
    if (j >= 0 && j < a.npix) {
        const int r = j / a.w, c = j - r * a.w;
        const float d = *(const float *)(a.depth + r * a.depth_stride + 4 * (size_t)c);
        cloud_point(*a.frame, r, c, d, &rec.x, &rec.y, &rec.z);
        rec.w = __uint_as_float(cloud_rgba(a.bgr + r * a.bgr_stride + 3 * (size_t)c));
    }
    a.out[e] = rec;
}

__global__ __launch_bounds__(CL_T) void k_obj_mask(const float *dist, int n, double threshold, uint8_t *keep)
{
    const int i = blockIdx.x * CL_T + threadIdx.x;
    if (i < n) keep[i] = (double)dist[i] > threshold ? 0 : 1;
}

template <int W>
__global__ __launch_bounds__(CL_T) void k_obj_compact(const uint8_t *keep, int n, int *blk, const float4 *pts, const int *idx, float4 *out_pts,
                                                      int *out_idx)
{
    __shared__ int sWave[CL_T / 64];
    const int i = blockIdx.x * CL_T + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    const int rank = block_rank(k, sWave);
    if (!W) {
        if (threadIdx.x == 0) blk[blockIdx.x] = block_total(sWave);
    } else if (k) {
        const int o = blk[blockIdx.x] + rank;
        out_pts[o] = pts[i];
        if (idx) out_idx[o] = idx[i];
    }
}

// compute3DCentroid's dense path: one lane, the voxels in order
__global__ void k_obj_centroid(const float4 *vox, int nv, float *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int v = 0; v < nv; v++) {
        const float4 p = vox[v];
        sx += p.x;
        sy += p.y;
        sz += p.z;
    }
    const float cnt = (float)nv;
    out[0] = sx / cnt;
    out[1] = sy / cnt;
    out[2] = sz / cnt;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
orbfe_status obj_scratch(orbfe_cloud *h, ObjScratch **out)
{
    if (!h->obj) h->obj = new (std::nothrow) ObjScratch();
    if (!h->obj) return ORBFE_ERR_NOMEM;
    *out = h->obj;
    return ORBFE_OK;
}

// the cell grid of one object from its bounds and its number of finite points alone; false: no grid can serve (an extent that is
// not finite), the object goes through k_knn_brute
bool knn_plan(const float *mn, const float *mx, int nfin, KnnGrid *g, long long *cells)
{
    float e[3], emax = 0.f;
    for (int k = 0; k < 3; k++) {
        e[k] = mx[k] - mn[k];
        if (!isfinite(e[k])) return false;
        if (e[k] > emax) emax = e[k];
    }
    for (int k = 0; k < 3; k++) g->mn[k] = mn[k], g->dims[k] = 1;
    g->inv = 0.f;
    g->sm = INFINITY;
    *cells = 1;
    if (!(emax > 0.f)) return true;   // every point in one place: one cell
    // shrink the cell until there are about four points to a cell, an axis reaches KNN_MAX_DIM cells or the grid KNN_MAX_CELLS
    double s = (double)emax;
    for (int it = 0; it < 64; it++) {
        const double t = s * 0.8;
        if ((double)emax / t >= (double)(KNN_MAX_DIM - 2)) break;
        long long c = 1;
        for (int k = 0; k < 3; k++) c *= (long long)((double)e[k] / t) + 1;
        if (c > KNN_MAX_CELLS) break;
        s = t;
        if (c * 4 >= nfin) break;
    }
    const float inv = (float)(1.0 / s);
    if (!isfinite(inv) || !(inv > 0.f) || !isnormal(inv) || !isnormal((float)s)) return false;
    g->inv = inv;
    *cells = 1;
    for (int k = 0; k < 3; k++) {
        g->dims[k] = (int)(e[k] * inv) + 1;   // the cell of the largest coordinate as cell_of computes it, plus one
        if (g->dims[k] > KNN_MAX_DIM + 8) return false;
        *cells *= g->dims[k];
    }
    float sm = (float)((1.0 - 1.0 / 512.0) / (double)inv);
    sm = nextafterf(sm, 0.f);
    g->sm = sm;
    return true;
}

orbfe_status knn_object(ObjScratch *s, const float4 *pts, int n, int nfin, const float *mn, const float *mx, int mean_k, int mode, float *d_dist,
                        orbfe_knn_plan *plan, hipStream_t st)
{
    KnnGrid g = {};
    long long cells = 0;
    bool grid = mode == 2 || (mode == 0 && nfin > KNN_AUTO_BRUTE);
    if (grid) grid = knn_plan(mn, mx, nfin, &g, &cells);
    if (plan) {
        memset(plan, 0, sizeof(*plan));
        plan->used = grid ? 2 : 1;
        plan->n_finite = nfin;
        if (grid) {
            for (int k = 0; k < 3; k++) plan->dims[k] = g.dims[k], plan->origin[k] = g.mn[k];
            plan->inv_cell = g.inv;
            plan->cells = (int32_t)cells;
        }
    }
    if (!grid) {
        k_knn_brute<<<(unsigned)((n + 3) / 4), CL_T, 0, st>>>(pts, n, mean_k, d_dist);
        ORBFE_HIP(hipGetLastError());
        return ORBFE_OK;
    }
    const size_t np = (size_t)n;
    ORBFE_HIP(s->keys.ensure(np * 4));
    ORBFE_HIP(s->keys2.ensure(np * 4));
    ORBFE_HIP(s->vals.ensure(np * 4));
    ORBFE_HIP(s->vals2.ensure(np * 4));
    ORBFE_HIP(s->sorted.ensure((size_t)nfin * 16));
    ORBFE_HIP(s->cell_start.ensure(((size_t)cells + 1) * 4));
    k_obj_cellkeys<<<blocks_of(n), CL_T, 0, st>>>(pts, n, g, s->keys.as<uint32_t>(), s->vals.as<uint32_t>());
    ORBFE_HIP(hipGetLastError());
    unsigned bits = 32;
    if (nfin == n) {
        bits = 1;
        while (bits < 32 && (1LL << bits) < cells) bits++;
    }
    size_t tmp = 0;
    ORBFE_HIP(rocprim::radix_sort_pairs(nullptr, tmp, s->keys.as<uint32_t>(), s->keys2.as<uint32_t>(), s->vals.as<uint32_t>(), s->vals2.as<uint32_t>(), np,
                                        0u, bits, st));
    ORBFE_HIP(s->sort.ensure(tmp ? tmp : 256));
    ORBFE_HIP(rocprim::radix_sort_pairs(s->sort.p, tmp, s->keys.as<uint32_t>(), s->keys2.as<uint32_t>(), s->vals.as<uint32_t>(), s->vals2.as<uint32_t>(),
                                        np, 0u, bits, st));
    k_obj_sorted<<<blocks_of(nfin), CL_T, 0, st>>>(pts, s->vals2.as<uint32_t>(), nfin, s->sorted.as<float4>());
    ORBFE_HIP(hipGetLastError());
    k_obj_cellstart<<<blocks_of(cells + 1), CL_T, 0, st>>>(s->keys2.as<uint32_t>(), nfin, (int)cells, s->cell_start.as<int>());
    ORBFE_HIP(hipGetLastError());
    k_knn_grid<<<(unsigned)((nfin + 3) / 4), CL_T, 0, st>>>(s->sorted.as<float4>(), s->cell_start.as<int>(), nfin, g, mean_k, d_dist);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// StatisticalOutlierRemoval over nobj point sets (CSR offsets, host): distances and keep flags on the device, the figures in stats
orbfe_status objects_filter(ObjScratch *s, const float4 *d_pts, const int32_t *off, int nobj, int mean_k, double stddev_mul, int mode, float *d_dist,
                            uint8_t *d_keep, orbfe_filter_stat *stats, orbfe_knn_plan *plans, hipStream_t st)
{
    const int total = off[nobj];
    ORBFE_HIP(s->mm.ensure(32));
    if (total > 0) {
        ORBFE_HIP(hipMemsetAsync(d_dist, 0, (size_t)total * 4, st));
        ORBFE_HIP(hipMemsetAsync(d_keep, 1, (size_t)total, st));
    }
    for (int o = 0; o < nobj; o++) {
        const int n = off[o + 1] - off[o];
        orbfe_filter_stat &f = stats[o];
        memset(&f, 0, sizeof(f));
        if (plans) memset(&plans[o], 0, sizeof(plans[o]));
        f.n_in = f.n_kept = n;
        f.status = ORBFE_OBJECT_EMPTY;
        if (n == 0) continue;
        float mn[3], mx[3];
        int nfin = 0;
        const orbfe_status ms = cloud_minmax(s->mm.as<unsigned>(), d_pts + off[o], n, mn, mx, &nfin, st);
        if (ms != ORBFE_OK) return ms;
        f.n_finite = nfin;
        f.status = ORBFE_OBJECT_TOO_FEW;
        if (nfin < mean_k + 1) continue;
        f.status = ORBFE_OBJECT_OK;
        const orbfe_status ks = knn_object(s, d_pts + off[o], n, nfin, mn, mx, mean_k, mode, d_dist + off[o], plans ? &plans[o] : nullptr, st);
        if (ks != ORBFE_OK) return ks;
    }
    if (total == 0) return ORBFE_OK;
    s->hdist.resize((size_t)total);
    ORBFE_HIP(hipMemcpyAsync(s->hdist.data(), d_dist, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    for (int o = 0; o < nobj; o++) {
        orbfe_filter_stat &f = stats[o];
        if (f.status != ORBFE_OBJECT_OK) continue;
        const float *d = s->hdist.data() + off[o];
        double sum = 0.0, sq = 0.0;
        for (int i = 0; i < f.n_in; i++) {
            const float dd = d[i] * d[i];
            sum += (double)d[i];
            sq += (double)dd;
        }
        const double valid = (double)f.n_finite;
        f.mean = sum / valid;
        const double variance = (sq - sum * sum / valid) / (valid - 1.0);
        f.stddev = sqrt(variance);
        f.threshold = f.mean + stddev_mul * f.stddev;
        int kept = 0;
        for (int i = 0; i < f.n_in; i++) kept += (double)d[i] > f.threshold ? 0 : 1;
        f.n_kept = kept;
        k_obj_mask<<<blocks_of(f.n_in), CL_T, 0, st>>>(d_dist + off[o], f.n_in, f.threshold, d_keep + off[o]);
        ORBFE_HIP(hipGetLastError());
    }
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

bool filter_args_ok(int mean_k, double stddev_mul, int mode, const char *who)
{
    if (mean_k < 1 || mean_k > 63 || mode < 0 || mode > 2 || isnan(stddev_mul)) {
        orbfe_set_error("%s: mean_k must be in [1, 63], mode 0, 1 or 2 and stddev_mul a number", who);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int64_t orbfe_cloud_objects_scratch_bytes(const orbfe_cloud *h) { return h && h->obj ? (int64_t)h->obj->bytes() : 0; }

extern "C" orbfe_status orbfe_cloud_outlier_filter_device(orbfe_cloud *h, const orbfe_cloud_point *d_points, const int32_t *offsets, int32_t nobj,
                                                          int32_t mean_k, double stddev_mul, int32_t mode, float *d_distances, uint8_t *d_keep,
                                                          orbfe_filter_stat *stats, orbfe_knn_plan *plans, void *stream)
{
    if (!h || !offsets || nobj < 0 || (nobj > 0 && !stats)) {
        orbfe_set_error("orbfe_cloud_outlier_filter_device: a required pointer is NULL or nobj < 0");
        return ORBFE_ERR_ARG;
    }
    if (!filter_args_ok(mean_k, stddev_mul, mode, "orbfe_cloud_outlier_filter_device")) return ORBFE_ERR_ARG;
    if (offsets[0] != 0) {
        orbfe_set_error("orbfe_cloud_outlier_filter_device: offsets[0] must be 0");
        return ORBFE_ERR_ARG;
    }
    for (int o = 0; o < nobj; o++)
        if (offsets[o + 1] < offsets[o]) {
            orbfe_set_error("orbfe_cloud_outlier_filter_device: offsets must not decrease");
            return ORBFE_ERR_ARG;
        }
    const int total = offsets[nobj];
    if (total > 0 && (!d_points || !d_distances || !d_keep || ((uintptr_t)d_points & 15))) {
        orbfe_set_error("orbfe_cloud_outlier_filter_device: a device buffer is NULL or the records are not 16-byte aligned");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    ObjScratch *s = nullptr;
    const orbfe_status as = obj_scratch(h, &s);
    if (as != ORBFE_OK) return as;
    return objects_filter(s, (const float4 *)d_points, offsets, nobj, mean_k, stddev_mul, mode, d_distances, d_keep, stats, plans, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_cloud_objects_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, const uint8_t *d_bgr, size_t bgr_stride,
                                                   const float *intrinsics, const double *T, const int32_t *d_indices, const int32_t *counts,
                                                   int32_t nboxes, int32_t mean_k, double stddev_mul, int32_t mode, orbfe_object *objects,
                                                   int32_t *d_kept, int32_t kept_cap, orbfe_cloud_point *d_voxels, int32_t voxel_cap,
                                                   int32_t *n_kept, int32_t *n_voxels, void *stream)
{
    const char *who = "orbfe_cloud_objects_device";
    if (!h || nboxes < 0 || kept_cap < 0 || voxel_cap < 0 || (nboxes > 0 && (!counts || !objects || !intrinsics || !T)) ||
        ((uintptr_t)d_voxels & 15)) {
        orbfe_set_error("%s: a required pointer is NULL, a size is negative or d_voxels is not 16-byte aligned", who);
        return ORBFE_ERR_ARG;
    }
    if (!filter_args_ok(mean_k, stddev_mul, mode, who)) return ORBFE_ERR_ARG;
    std::vector<int32_t> off((size_t)nboxes + 1, 0);
    for (int b = 0; b < nboxes; b++) {
        if (counts[b] < 0 || (long long)off[b] + counts[b] > (1LL << 30)) {
            orbfe_set_error("%s: counts[%d] is negative or the counts add up to more than 2^30", who, b);
            return ORBFE_ERR_ARG;
        }
        off[b + 1] = off[b] + counts[b];
    }
    const int total = off[nboxes];
    if (total > 0 && (!d_depth || !d_bgr || !d_indices)) {
        orbfe_set_error("%s: a device buffer is NULL", who);
        return ORBFE_ERR_ARG;
    }
    if (total > 0 && (depth_stride < (size_t)h->w * 4 || (depth_stride & 3) || bgr_stride < (size_t)h->w * 3)) {
        orbfe_set_error("%s: a stride is shorter than a row, or the depth stride is no multiple of 4", who);
        return ORBFE_ERR_ARG;
    }
    if (n_kept) *n_kept = 0;
    if (n_voxels) *n_voxels = 0;
    DeviceGuard dg(h->device);
    hipStream_t st = (hipStream_t)stream;
    ObjScratch *s = nullptr;
    orbfe_status rs = obj_scratch(h, &s);
    if (rs != ORBFE_OK) return rs;
    s->stats.resize((size_t)nboxes);
    const size_t nt = (size_t)(total > 0 ? total : 1);
    const unsigned tb = blocks_of(total);
    ORBFE_HIP(s->pts.ensure(nt * 16));
    ORBFE_HIP(s->dist.ensure(nt * 4));
    ORBFE_HIP(s->keep.ensure(nt));
    ORBFE_HIP(s->kept_pts.ensure(nt * 16));
    ORBFE_HIP(s->kept_idx.ensure(nt * 4));
    ORBFE_HIP(s->vox.ensure(nt * 16));
    ORBFE_HIP(s->keys.ensure(nt * 4));
    ORBFE_HIP(s->keys2.ensure(nt * 4));
    ORBFE_HIP(s->vals.ensure(nt * 4));
    ORBFE_HIP(s->vals2.ensure(nt * 4));
    ORBFE_HIP(s->starts.ensure(nt * 4));
    ORBFE_HIP(s->blk.ensure(((size_t)tb + 2) * 4));
    ORBFE_HIP(s->scal.ensure(16));
    ORBFE_HIP(s->mm.ensure(32));
    ORBFE_HIP(s->cen.ensure(16));
    ORBFE_HIP(s->frame.ensure(sizeof(ClFrame)));
    int total_kept = 0;
    if (total > 0) {
        // 1. ExtractIndices on the organised cloud
        ClFrame f;
        f.fx = intrinsics[0], f.fy = intrinsics[1], f.cx = intrinsics[2], f.cy = intrinsics[3];
        for (int e = 0; e < 12; e++) f.m[e] = T[e];
        ORBFE_HIP(hipMemcpyAsync(s->frame.p, &f, sizeof(f), hipMemcpyHostToDevice, st));
        ORBFE_HIP(hipStreamSynchronize(st));   // f is on the stack
        ObjGather a = {};
        a.depth = (const char *)d_depth;
        a.bgr = d_bgr;
        a.depth_stride = depth_stride;
        a.bgr_stride = bgr_stride;
        a.w = h->w;
        a.npix = h->w * h->ht;
        a.frame = s->frame.as<ClFrame>();
        a.idx = d_indices;
        a.total = total;
        a.out = s->pts.as<float4>();
        k_obj_gather<<<tb, CL_T, 0, st>>>(a);
        ORBFE_HIP(hipGetLastError());
    }
    // 2. StatisticalOutlierRemoval
    rs = objects_filter(s, s->pts.as<float4>(), off.data(), nboxes, mean_k, stddev_mul, mode, s->dist.as<float>(), s->keep.as<uint8_t>(),
                        s->stats.data(), nullptr, st);
    if (rs != ORBFE_OK) return rs;
    if (total > 0) {
        // 3. the kept points and their flat indices, in order
        k_obj_compact<0><<<tb, CL_T, 0, st>>>(s->keep.as<uint8_t>(), total, s->blk.as<int>(), nullptr, nullptr, nullptr, nullptr);
        ORBFE_HIP(hipGetLastError());
        rs = cloud_scan_blocks(s->blk.as<int>(), nullptr, s->scal.as<int>(), (int)tb, 0, 0, &total_kept, st);
        if (rs != ORBFE_OK) return rs;
        k_obj_compact<1><<<tb, CL_T, 0, st>>>(s->keep.as<uint8_t>(), total, s->blk.as<int>(), s->pts.as<float4>(), d_indices, s->kept_pts.as<float4>(),
                                              s->kept_idx.as<int>());
        ORBFE_HIP(hipGetLastError());
    }
    // 4. VoxelGrid, centroid and bounds per object
    std::vector<orbfe_object> recs((size_t)nboxes);
    const ClVoxScratch vs = {s->keys.as<uint32_t>(), s->keys2.as<uint32_t>(), s->vals.as<uint32_t>(), s->vals2.as<uint32_t>(), s->starts.as<int>(),
                             s->blk.as<int>(), s->scal.as<int>(), s->mm.as<unsigned>(), &s->sort};
    int koff = 0, voff = 0;
    for (int b = 0; b < nboxes; b++) {
        const orbfe_filter_stat &f = s->stats[b];
        orbfe_object &o = recs[b];
        memset(&o, 0, sizeof(o));
        o.status = f.status;
        o.n_in = f.n_in;
        o.n_kept = f.n_kept;
        o.threshold = f.threshold;
        o.mean = f.mean;
        o.stddev = f.stddev;
        const int k0 = koff;
        koff += f.n_kept;
        if (f.status != ORBFE_OBJECT_OK) continue;
        int nv = 0, ovf = 0;
        orbfe_cloud_point *vox = s->vox.as<orbfe_cloud_point>() + voff;
        rs = cloud_voxel_run(vs, h->leaf, s->kept_pts.as<orbfe_cloud_point>() + k0, f.n_kept, vox, f.n_kept, true, &nv, &ovf, st);
        if (rs != ORBFE_OK) return rs;
        o.n_voxels = nv;
        if (nv == 0) {
            o.status = ORBFE_OBJECT_EMPTY;
            continue;
        }
        voff += nv;
        k_obj_centroid<<<1, 64, 0, st>>>((const float4 *)vox, nv, s->cen.as<float>());
        ORBFE_HIP(hipGetLastError());
        ORBFE_HIP(hipMemcpyAsync(o.centroid, s->cen.p, 12, hipMemcpyDeviceToHost, st));
        int nfin = 0;
        rs = cloud_minmax(s->mm.as<unsigned>(), (const float4 *)vox, nv, o.min, o.max, &nfin, st);   // drains the stream
        if (rs != ORBFE_OK) return rs;
        if (nfin == 0)
            for (int k = 0; k < 3; k++) o.min[k] = o.max[k] = 0.f;
    }
    if (koff != total_kept) {
        orbfe_set_error("%s: internal: %d flags kept on the device, %d on the host", who, total_kept, koff);
        return ORBFE_ERR_HIP;
    }
    if (n_kept) *n_kept = total_kept;
    if (n_voxels) *n_voxels = voff;
    if ((d_kept && total_kept > kept_cap) || (d_voxels && voff > voxel_cap)) {
        orbfe_set_error("%s: %d kept indices / %d voxels exceed kept_cap %d / voxel_cap %d", who, total_kept, voff, kept_cap, voxel_cap);
        return ORBFE_ERR_CAP;
    }
    if (d_kept && total_kept > 0) ORBFE_HIP(hipMemcpyAsync(d_kept, s->kept_idx.p, (size_t)total_kept * 4, hipMemcpyDeviceToDevice, st));
    if (d_voxels && voff > 0) ORBFE_HIP(hipMemcpyAsync(d_voxels, s->vox.p, (size_t)voff * 16, hipMemcpyDeviceToDevice, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < nboxes; b++) objects[b] = recs[b];
    return ORBFE_OK;
}

// one keyframe from HOST planes and HOST boxes: the paint, then the objects, on the handle's stream
extern "C" orbfe_status orbfe_cloud_objects(orbfe_cloud *h, const float *depth, uint8_t *bgr, const float *intrinsics, const double *T,
                                            const float *boxes, const uint8_t *colors, int32_t nboxes, int32_t mean_k, double stddev_mul,
                                            int32_t mode, orbfe_object *objects)
{
    if (!h || !depth || !bgr || !intrinsics || !T || nboxes < 0 || (nboxes > 0 && (!boxes || !colors || !objects))) {
        orbfe_set_error("orbfe_cloud_objects: a required pointer is NULL or nboxes < 0");
        return ORBFE_ERR_ARG;
    }
    if (!filter_args_ok(mean_k, stddev_mul, mode, "orbfe_cloud_objects")) return ORBFE_ERR_ARG;
    DeviceGuard dg(h->device);
    ObjScratch *s = nullptr;
    orbfe_status rs = obj_scratch(h, &s);
    if (rs != ORBFE_OK) return rs;
    const size_t np = (size_t)h->w * h->ht;
    long long most = 0;
    for (int b = 0; b < nboxes; b++) {
        const float *r = boxes + 4 * (size_t)b;
        if (isfinite(r[2]) && isfinite(r[3]) && fabsf(r[2]) < 1048576.f && fabsf(r[3]) < 1048576.f && (int)r[2] > 2 && (int)r[3] > 1)
            most += (long long)((int)r[2] - 2) * ((int)r[3] - 1);
    }
    if (most > (1LL << 30)) {
        orbfe_set_error("orbfe_cloud_objects: the boxes can record more than 2^30 indices");
        return ORBFE_ERR_ARG;
    }
    ORBFE_HIP(h->depth.ensure(np * 4));
    ORBFE_HIP(h->bgr.ensure(np * 3));
    ORBFE_HIP(s->idx.ensure((size_t)(most > 0 ? most : 1) * 4));
    ORBFE_HIP(hipMemcpyAsync(h->depth.p, depth, np * 4, hipMemcpyHostToDevice, h->stream));
    ORBFE_HIP(hipMemcpyAsync(h->bgr.p, bgr, np * 3, hipMemcpyHostToDevice, h->stream));
    std::vector<int32_t> counts((size_t)nboxes + 1, 0);
    int32_t n = 0;
    rs = orbfe_cloud_paint_boxes_device(h, h->depth.as<float>(), (size_t)h->w * 4, h->bgr.as<uint8_t>(), (size_t)h->w * 3, boxes, colors, nboxes,
                                        s->idx.as<int32_t>(), (int32_t)most, counts.data(), &n, h->stream);
    if (rs != ORBFE_OK) return rs;
    ORBFE_HIP(hipMemcpyAsync(bgr, h->bgr.p, np * 3, hipMemcpyDeviceToHost, h->stream));   // the painted plane back to the caller
    return orbfe_cloud_objects_device(h, h->depth.as<float>(), (size_t)h->w * 4, h->bgr.as<uint8_t>(), (size_t)h->w * 3, intrinsics, T,
                                      s->idx.as<int32_t>(), counts.data(), nboxes, mean_k, stddev_mul, mode, objects, nullptr, 0, nullptr, 0, nullptr,
                                      nullptr, h->stream);
}

// ---- sem_merge and the clusters vector (host only) ----------------------------------------------------------------------------------
struct orbfe_objects {
    float obj_size[ORBFE_OBJECT_CLASSES];
    std::vector<orbfe_cluster> clusters;
};

extern "C" orbfe_status orbfe_objects_create(const float *obj_size, orbfe_objects **out)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    orbfe_objects *db = new (std::nothrow) orbfe_objects();
    if (!db) return ORBFE_ERR_NOMEM;
    for (int i = 0; i < ORBFE_OBJECT_CLASSES; i++) db->obj_size[i] = obj_size ? obj_size[i] : (float)0.6;
    if (!obj_size) {   // the reference's table: bottle, chair, person, tvmonitor
        db->obj_size[5] = (float)0.06;
        db->obj_size[9] = (float)0.5;
        db->obj_size[15] = (float)0.35;
        db->obj_size[20] = (float)0.25;
    }
    *out = db;
    return ORBFE_OK;
}

extern "C" void orbfe_objects_destroy(orbfe_objects *db) { delete db; }
extern "C" int32_t orbfe_objects_size(const orbfe_objects *db) { return db ? (int32_t)db->clusters.size() : 0; }
extern "C" void orbfe_objects_clear(orbfe_objects *db)
{
    if (db) db->clusters.clear();
}

extern "C" orbfe_status orbfe_objects_get(const orbfe_objects *db, int32_t i, orbfe_cluster *out)
{
    if (!db || !out || i < 0 || (size_t)i >= db->clusters.size()) {
        orbfe_set_error("orbfe_objects_get: a NULL pointer or an index outside the database");
        return ORBFE_ERR_ARG;
    }
    *out = db->clusters[(size_t)i];
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_objects_merge(orbfe_objects *db, int32_t class_id, float prob, const float *centroid, const float *min_pt,
                                            const float *max_pt, int32_t *index_out)
{
    if (!db || !centroid || !min_pt || !max_pt || class_id < 0 || class_id >= ORBFE_OBJECT_CLASSES) {
        orbfe_set_error("orbfe_objects_merge: a NULL pointer or a class_id outside [0, %d)", ORBFE_OBJECT_CLASSES);
        return ORBFE_ERR_ARG;
    }
    int best = -1;
    float center_distance = 100.f;
    for (size_t i = 0; i < db->clusters.size(); i++) {
        const orbfe_cluster &c = db->clusters[i];
        if (c.class_id != class_id) continue;
        const float dx = centroid[0] - c.centroid[0], dy = centroid[1] - c.centroid[1], dz = centroid[2] - c.centroid[2];
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (dist < center_distance) {
            center_distance = dist;
            best = (int)i;
        }
    }
    if (best >= 0 && center_distance < db->obj_size[class_id]) {
        orbfe_cluster &c = db->clusters[(size_t)best];
        c.prob = (float)((double)(c.prob + prob) / 2.0);
        for (int k = 0; k < 3; k++) {
            c.centroid[k] = (c.centroid[k] + centroid[k]) / 2.f;
            c.min[k] = c.min[k] > min_pt[k] ? min_pt[k] : c.min[k];
            c.max[k] = c.max[k] > max_pt[k] ? max_pt[k] : c.max[k];   // the smaller maximum, as the reference has it
        }
        if (index_out) *index_out = best;
        return ORBFE_OK;
    }
    orbfe_cluster c;
    c.class_id = class_id;
    c.prob = prob;
    for (int k = 0; k < 3; k++) c.centroid[k] = centroid[k], c.min[k] = min_pt[k], c.max[k] = max_pt[k];
    db->clusters.push_back(c);
    if (index_out) *index_out = (int32_t)db->clusters.size() - 1;
    return ORBFE_OK;
}
