// orbfe_geometry.hip -- DynaSLAM::Geometry on the device (perfect/src/Geometry.cc): the key-frame ring, ExtractDynPoints,
// RegionGrowing, DepthRegionGrowing and GeometricModelCorrection; GetRefFrames on the host.  The per-point arithmetic is
// csrc/orbfe_geometry_dev.h; tests/geometry_oracle.py restates everything here and the kernels are bit-exact against it.
// Layout: DESIGN.md section 8m.
#include <math.h>

#include <algorithm>
#include <new>

#include "orbfe_common.h"
#include "orbfe_host.h"
#include "orbfe_geometry_dev.h"

namespace {

constexpr int GE_DB = ORBFE_GEOMETRY_DB_SIZE, GE_REFS = ORBFE_GEOMETRY_REF_FRAMES;
constexpr int GE_MAX_CHUNK = 8;        // current frames per internal pass
constexpr int GE_MIN_SIDE = 45;        // a 41x41 window strictly inside a 21-pixel border needs 2 * 22 + 1
constexpr int GE_DMAX = 20, GE_WIN = 2 * GE_DMAX + 1;
constexpr int GE_RAD = 15;             // dilation_size (:502)
constexpr int GE_T = 256;
constexpr int GE_NCOUNT = 8;
// the frontier list of one seed: its first GE_LDS_ENTRIES entries live in LDS (144 KiB of the CU's 160), the rest in global scratch
constexpr int GE_LDS_ENTRIES = 18432;
constexpr size_t GE_SCRATCH_BUDGET = (size_t)4 << 30;

enum { C_READ = 0, C_DEPTH = 1, C_PAR = 2, C_D7 = 3, C_IN = 4, C_FOUND = 5, C_GATE = 6, C_DYN = 7 };
enum { F_PAR = 1, F_D7 = 2, F_DYN = 4 };

struct GeoKF {   // one ring slot, as the kernels see it
    int32_t n, w, h, pad;
    float t[3];
    float pad2;
    GeoLU4 lu;
};

struct GeoFrame {
    float T[16];
    int32_t ref[GE_REFS];
    int32_t nref;
};

struct GeoCall {
    GeoFrame fr[GE_MAX_CHUNK];
    float K[9], Kinv[9];
    int32_t w, h;
};

struct GeoEll { int8_t hw[2 * GE_RAD + 1]; };

struct GeoEntry { float d; int32_t idx; };

__device__ inline unsigned long long wave_min_u64(unsigned long long v)
{
    for (int off = 32; off; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// ---- ExtractDynPoints, steps 1 - 4.1: one thread per (frame, reference, keypoint) ---------------------------------------------
__global__ __launch_bounds__(GE_T) void k_geo_points(GeoCall call, const GeoKF *kf, const float *kf_depth, size_t kf_plane,
                                                     const float2 *kf_keys, const float2 *kf_un, int maxkp, float4 *pts, uint8_t *flags,
                                                     int32_t *counts)
{
    const int f = blockIdx.y, slot = blockIdx.x * GE_T + threadIdx.x;
    if (slot >= GE_REFS * maxkp) return;
    const GeoFrame &fr = call.fr[f];
    const int r = slot / maxkp, j = slot % maxkp;
    uint8_t fl = 0;
    float4 out = {0.f, 0.f, 0.f, 0.f};
    if (r < fr.nref) {
        const int s = fr.ref[r];
        const GeoKF &k = kf[s];
        if (j < k.n) {
            int32_t *cnt = counts + f * GE_NCOUNT;
            atomicAdd(&cnt[C_READ], 1);
            const float2 kp = kf_keys[(size_t)s * maxkp + j], un = kf_un[(size_t)s * maxkp + j];
            float d = 0.f;
            if (kp.x > -1.f && kp.x < (float)k.w && kp.y > -1.f && kp.y < (float)k.h)
                d = kf_depth[(size_t)s * kf_plane + (size_t)(int)kp.y * k.w + (int)kp.x];
            if (d > 0 && d < 6) {
                atomicAdd(&cnt[C_DEPTH], 1);
                float b[4];
                geo_backproject(call.Kinv, un.x, un.y, d, b);
                const float invd = b[3];
                geo_lu4_solve(&k.lu, b);
                const float tcur[3] = {fr.T[3], fr.T[7], fr.T[11]};
                if (geo_parallax_ok(b, invd, k.t, tcur)) {
                    atomicAdd(&cnt[C_PAR], 1);
                    fl = F_PAR;
                    float o[4];
                    geo_to_current(fr.T, b, o);
                    out = make_float4(o[0], o[1], o[2], o[3]);
                    if (o[2] < 7) {
                        atomicAdd(&cnt[C_D7], 1);
                        fl |= F_D7;
                    }
                }
            }
        }
    }
    const size_t at = (size_t)f * GE_REFS * maxkp + slot;
    pts[at] = out;
    flags[at] = fl;
}

// ---- steps 4.2 - 4.4: one wave per point that passed depth < 7 ------------------------------------------------------------------
__global__ __launch_bounds__(GE_T) void k_geo_search(GeoCall call, const float *depth, size_t dstride, size_t dfs, int maxkp,
                                                     const float4 *pts, uint8_t *flags, int2 *pix, int32_t *counts)
{
    const int f = blockIdx.y, slot = blockIdx.x * (GE_T / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= GE_REFS * maxkp) return;
    const size_t at = (size_t)f * GE_REFS * maxkp + slot;
    const uint8_t fl = flags[at];
    if (!(fl & F_D7)) return;
    int32_t *cnt = counts + f * GE_NCOUNT;
    const int w = call.w, h = call.h;
    const float4 p = pts[at];
    const float X[4] = {p.x, p.y, p.z, p.w};
    float x, y;
    geo_project(call.K, X, geo_proj_mode(cnt[C_D7], cnt[C_PAR]), &x, &y);
    if (!geo_in_frame(x, y, w, h)) return;
    const char *plane = (const char *)depth + (size_t)f * dfs;
    const int xi = (int)x, yi = (int)y;
    if (!(*(const float *)(plane + (size_t)yi * dstride + (size_t)xi * 4) > 0)) return;
    if (lane == 0) atomicAdd(&cnt[C_IN], 1);
    const float proj = p.z;
    // the 41x41 search: x offset outer, y offset inner; key = (proj - d', scan index), the first minimum wins
    unsigned long long best = ~0ull;
    for (int m = lane; m < GE_WIN * GE_WIN; m += 64) {
        const int xx = xi + m / GE_WIN - GE_DMAX, yy = yi + m % GE_WIN - GE_DMAX;
        const float dd = *(const float *)(plane + (size_t)yy * dstride + (size_t)xx * 4);
        if (dd > 0 && dd < proj) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(proj - dd) << 32) | (unsigned)m;
            best = key < best ? key : best;
        }
    }
    best = wave_min_u64(best);
    if (best == ~0ull) return;
    if (lane == 0) atomicAdd(&cnt[C_FOUND], 1);
    const float diff = __uint_as_float((unsigned)(best >> 32));
    if (!(diff > 0.6f)) return;
    if (lane == 0) atomicAdd(&cnt[C_GATE], 1);
    // cv::meanStdDev of the 41x41 patch: double sums in row order (modules/core/src/stat.cpp sqsum_), every lane the same chain
    double s = 0., sq = 0.;
    for (int yy = yi - GE_DMAX; yy <= yi + GE_DMAX; yy++) {
        const float *row = (const float *)(plane + (size_t)yy * dstride);
        for (int xx = xi - GE_DMAX; xx <= xi + GE_DMAX; xx++) {
            const float v = row[xx];
            s += v;
            sq += (double)v * v;
        }
    }
    const double scale = 1. / (GE_WIN * GE_WIN);
    s *= scale;
    const double sd = sqrt(fmax(sq * scale - s * s, 0.));
    const double var = sd * sd;
    if (!(var < (double)0.001f)) return;
    if (lane == 0) {
        flags[at] = fl | F_DYN;
        pix[at] = make_int2(xi, yi);
    }
}

// ---- the ordered compaction of the dynamic points: one block per frame ----------------------------------------------------------
__global__ __launch_bounds__(GE_T) void k_geo_compact(int maxkp, const uint8_t *flags, const int2 *pix, int32_t *dyn, int32_t *counts)
{
    __shared__ int scan[GE_T];
    __shared__ int base;
    const int f = blockIdx.x, n = GE_REFS * maxkp;
    const size_t at0 = (size_t)f * n;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    if (counts[f * GE_NCOUNT + C_GATE] == 0) return;   // nothing past the 0.6 gate: no flag is set (uniform)
    for (int c0 = 0; c0 < n; c0 += GE_T) {
        const int i = c0 + threadIdx.x;
        const int keep = i < n && (flags[at0 + i] & F_DYN) ? 1 : 0;
        scan[threadIdx.x] = keep;
        __syncthreads();
        for (int off = 1; off < GE_T; off <<= 1) {
            const int v = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        if (keep) {
            const int pos = base + scan[threadIdx.x] - 1;
            const int2 p = pix[at0 + i];
            int32_t *o = dyn + (at0 + pos) * 3;
            o[0] = p.x, o[1] = p.y, o[2] = i / maxkp;
        }
        __syncthreads();
        if (threadIdx.x == GE_T - 1) base += scan[GE_T - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[f * GE_NCOUNT + C_DYN] = base;
}

// ---- RegionGrowing: one workgroup per seed of the pass, the steps of a seed serial ----------------------------------------------
// the seeds of pass `pass` that exist: min(max_seeds, ndyn - pass * max_seeds), <= 0 when the pass is empty
__device__ inline int pass_seeds(const int32_t *counts, int f, int pass, int max_seeds)
{
    return min(max_seeds, counts[f * GE_NCOUNT + C_DYN] - pass * max_seeds);
}

__global__ void k_geo_zero_planes(const int32_t *counts, int pass, int max_seeds, int wh, uint8_t *planes, size_t plane_fs)
{
    const int f = blockIdx.z, s = blockIdx.y;
    if (s >= pass_seeds(counts, f, pass, max_seeds)) return;
    uint32_t *p = (uint32_t *)(planes + (size_t)f * plane_fs + (size_t)s * wh);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < wh / 4; i += gridDim.x * blockDim.x) p[i] = 0u;
}

__global__ __launch_bounds__(GE_T) void k_geo_grow(const int32_t *counts, int pass, int max_seeds, int dyn_cap, const int32_t *dyn,
                                                   const float *depth, size_t dstride, size_t dfs, int w, int h, int wh4,
                                                   const uint8_t *uni, uint8_t *planes, size_t plane_fs, GeoEntry *spill,
                                                   size_t spill_seed)
{
    extern __shared__ GeoEntry lds_list[];
    __shared__ unsigned long long s_red[GE_T / 64];
    __shared__ int s_n;
    __shared__ float s_mean;
    const int f = blockIdx.y, s = blockIdx.x;
    if (s >= pass_seeds(counts, f, pass, max_seeds)) return;
    const int32_t *seed = dyn + ((size_t)f * dyn_cap + (size_t)pass * max_seeds + s) * 3;
    const char *plane = (const char *)depth + (size_t)f * dfs;
    uint8_t *J = planes + (size_t)f * plane_fs + (size_t)s * wh4;
    GeoEntry *glist = spill + ((size_t)f * max_seeds + s) * spill_seed;
    int x = seed[0], y = seed[1];
    const float d0 = *(const float *)(plane + (size_t)y * dstride + (size_t)x * 4);
    // DepthRegionGrowing's test against the union carried in from the earlier passes; the seeds of this pass are resolved after it
    if (!(d0 > 0) || uni[(size_t)f * wh4 + (size_t)y * w + x]) return;

    auto get = [&](int i) { return i < GE_LDS_ENTRIES ? lds_list[i] : glist[i - GE_LDS_ENTRIES]; };
    auto put = [&](int i, GeoEntry e) {
        if (i < GE_LDS_ENTRIES) lds_list[i] = e;
        else glist[i - GE_LDS_ENTRIES] = e;
    };
    // thread 0's state
    float reg_mean = d0;
    int reg_size = 1, neg_pos = -1;
    const int total = w * h;
    auto add_neighbours = [&]() {
        const int nx[4] = {x - 1, x + 1, x, x}, ny[4] = {y, y, y - 1, y + 1};
        bool ins[4];
        uint8_t jv[4];
        float dv[4];
        for (int q = 0; q < 4; q++) {
            ins[q] = nx[q] >= 0 && ny[q] >= 0 && nx[q] < w && ny[q] < h;
            jv[q] = ins[q] ? J[(size_t)ny[q] * w + nx[q]] : 1;
            dv[q] = ins[q] ? *(const float *)(plane + (size_t)ny[q] * dstride + (size_t)nx[q] * 4) : 0.f;
        }
        for (int q = 0; q < 4; q++)
            if (ins[q] && jv[q] == 0) {
                neg_pos++;
                put(neg_pos, GeoEntry{dv[q], ny[q] * w + nx[q]});
                J[(size_t)ny[q] * w + nx[q]] = 1;
            }
    };
    if (threadIdx.x == 0) {
        add_neighbours();
        s_n = neg_pos;   // the candidates are the entries below neg_pos: the last one is never one
        s_mean = reg_mean;
    }
    __syncthreads();
    for (;;) {
        const int n = s_n;
        if (n < 1) break;   // minMaxLoc of the empty matrix: index -1, the growth stops
        const float mean = s_mean;
        unsigned long long best = ~0ull;
        for (int i = threadIdx.x; i < n; i += GE_T) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(fabsf(get(i).d - mean)) << 32) | (unsigned)i;
            best = key < best ? key : best;
        }
        best = wave_min_u64(best);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < GE_T / 64; q++) best = s_red[q] < best ? s_red[q] : best;
            const int index = (int)(unsigned)best;
            const double pixdist = (double)__uint_as_float((unsigned)(best >> 32));
            J[(size_t)y * w + x] = 1;
            reg_size += 1;
            const GeoEntry e = get(index);
            reg_mean = (reg_mean * reg_size + e.d) / (reg_size + 1);
            x = e.idx % w;
            y = e.idx / w;
            put(index, get(neg_pos));
            neg_pos -= 1;
            if (pixdist < (double)0.20f && reg_size < total) {
                add_neighbours();
                s_n = neg_pos;
                s_mean = reg_mean;
            } else
                s_n = 0;
        }
        __syncthreads();
    }
}

// DepthRegionGrowing's seed order within the pass: seed i is grown iff its depth is > 0 and neither the carried union nor the
// region of an earlier grown seed of the pass covers it.  One block per frame.
__global__ __launch_bounds__(GE_T) void k_geo_resolve(const int32_t *counts, int pass, int max_seeds, int dyn_cap, const int32_t *dyn,
                                                      const float *depth, size_t dstride, size_t dfs, int w, int wh4, const uint8_t *uni,
                                                      const uint8_t *planes, size_t plane_fs, uint8_t *acc)
{
    const int f = blockIdx.x, n = pass_seeds(counts, f, pass, max_seeds);
    if (n <= 0) return;
    const int32_t *seeds = dyn + ((size_t)f * dyn_cap + (size_t)pass * max_seeds) * 3;
    uint8_t *a = acc + (size_t)f * dyn_cap + (size_t)pass * max_seeds;
    const uint8_t *P = planes + (size_t)f * plane_fs;
    const char *plane = (const char *)depth + (size_t)f * dfs;
    for (int i = 0; i < n; i++) {
        const int x = seeds[i * 3], y = seeds[i * 3 + 1];
        const size_t p = (size_t)y * w + x;
        int cov = 0;
        for (int j = threadIdx.x; j < i; j += GE_T)
            if (a[j] && P[(size_t)j * wh4 + p]) cov = 1;
        cov = __syncthreads_or(cov);
        if (threadIdx.x == 0) {
            const float d = *(const float *)(plane + (size_t)y * dstride + (size_t)x * 4);
            a[i] = (d > 0 && !uni[(size_t)f * wh4 + p] && !cov) ? 1 : 0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GE_T) void k_geo_union(const int32_t *counts, int pass, int max_seeds, int dyn_cap, int wh, int wh4,
                                                    const uint8_t *planes, size_t plane_fs, const uint8_t *acc, uint8_t *uni)
{
    const int f = blockIdx.y, n = pass_seeds(counts, f, pass, max_seeds);
    if (n <= 0) return;
    const int p = blockIdx.x * GE_T + threadIdx.x;
    if (p >= wh) return;
    const uint8_t *a = acc + (size_t)f * dyn_cap + (size_t)pass * max_seeds;
    const uint8_t *P = planes + (size_t)f * plane_fs;
    uint8_t v = uni[(size_t)f * wh4 + p];
    for (int j = 0; j < n && !v; j++)
        if (a[j] && P[(size_t)j * wh4 + p]) v = 1;
    uni[(size_t)f * wh4 + p] = v;
}

// ---- the 31x31 ellipse dilation (zeros outside the image), mask = 1 - union, count of ones --------------------------------------
// k_flow_morph's sibling for a radius given at run time: tile 64 x 16, the window's rows as prefix sums, one range test per
// kernel row.  computed == 0 frames are written as all ones.
constexpr int GD_TW = 64, GD_TH = 16;
__global__ __launch_bounds__(GE_T) void k_geo_dilate_mask(const uint8_t *uni, int wh4, GeoEll ell, int w, int h, uint8_t *mask,
                                                          int mstride, size_t mfs, int32_t *ones)
{
    __shared__ uint16_t pre[GD_TH + 2 * GE_RAD][GD_TW + 2 * GE_RAD + 1];
    __shared__ int cnt;
    const int f = blockIdx.z, x0 = blockIdx.x * GD_TW, y0 = blockIdx.y * GD_TH;
    const uint8_t *U = uni + (size_t)f * wh4;
    if (threadIdx.x == 0) cnt = 0;
    if (threadIdx.x < GD_TH + 2 * GE_RAD) {
        const int yy = y0 + (int)threadIdx.x - GE_RAD;
        uint16_t acc = 0;
        pre[threadIdx.x][0] = 0;
        for (int c = 0; c < GD_TW + 2 * GE_RAD; c++) {
            const int xx = x0 + c - GE_RAD;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) acc += U[(size_t)yy * w + xx] != 0;
            pre[threadIdx.x][c + 1] = acc;
        }
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
    int mine = 0;
    for (int ty = ty0; ty < GD_TH; ty += GE_T / 64) {
        const int x = x0 + tx, y = y0 + ty;
        if (x >= w || y >= h) continue;
        int hit = 0;
        for (int dy = 0; dy <= 2 * GE_RAD; dy++) {
            const int hw = ell.hw[dy], c = tx + GE_RAD;
            hit |= pre[ty + dy][c + hw + 1] != pre[ty + dy][c - hw];
        }
        const uint8_t v = hit ? 0 : 1;
        mask[(size_t)f * mfs + (size_t)y * mstride + x] = v;
        mine += v;
    }
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && cnt && ones) atomicAdd(&ones[f], cnt);
}

__global__ void k_geo_kat_acos(const double *in, double *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = geo_acos(in[i]);
}

inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

struct orbfe_geometry {
    int device = 0;
    hipStream_t stream = nullptr, last_stream = nullptr;
    int maxw = 0, maxh = 0, maxkp = 0, max_seeds = 0, chunk = 0, dyn_cap = 0;
    size_t plane = 0;   // maxw * maxh rounded up to 4
    GeoEll ell;
    // DataBase
    int ini = 0, fin = 0, num = 0, inserts = 0;
    int slot_insert[GE_DB];
    float db_T[GE_DB][16];
    GeoKF kf[GE_DB];
    // the ring on the device
    float *d_kf_depth = nullptr;
    float2 *d_kf_keys = nullptr, *d_kf_un = nullptr;
    GeoKF *d_kf = nullptr;
    orbfe_keypoint *d_stage = nullptr;   // insert's staging of host keypoints
    // scratch of one chunk
    float *d_cur = nullptr;   // the host calls' depth plane
    float4 *d_pts = nullptr;
    uint8_t *d_flags = nullptr, *d_acc = nullptr, *d_planes = nullptr, *d_union = nullptr, *d_mask = nullptr;
    int2 *d_pix = nullptr;
    int32_t *d_counts = nullptr, *d_dyn = nullptr;
    GeoEntry *d_spill = nullptr;
    // what the taps read
    int tap_n = 0, tap_w = 0, tap_h = 0;
    int tap_computed[GE_MAX_CHUNK];
};

static void geometry_free(orbfe_geometry *g)
{
    orb_free_all(g->stream, {g->d_kf_depth, g->d_kf_keys, g->d_kf_un, g->d_kf, g->d_stage, g->d_cur, g->d_pts, g->d_flags, g->d_acc,
                             g->d_planes, g->d_union, g->d_mask, g->d_pix, g->d_counts, g->d_dyn, g->d_spill});
}

static void geometry_clear_db(orbfe_geometry *g)
{
    g->ini = g->fin = g->num = g->inserts = 0;
    for (int i = 0; i < GE_DB; i++) {
        g->slot_insert[i] = -1;
        g->kf[i] = GeoKF{};
    }
}

extern "C" orbfe_status orbfe_geometry_ellipse(int32_t r, int32_t *half_width)
{
    if (r < 0 || r > 1024 || !half_width) return ORBFE_ERR_ARG;
    for (int i = 0; i <= 2 * r; i++) half_width[i] = geo_ellipse_half_width(r, i);
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_geometry_create(int32_t device, int32_t max_w, int32_t max_h, int32_t max_keypoints, int32_t max_seeds,
                                              orbfe_geometry **out)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    if (max_w < GE_MIN_SIDE || max_h < GE_MIN_SIDE || (int64_t)max_w * max_h > (1 << 26) || max_keypoints < 1 ||
        max_keypoints > (1 << 20) || max_seeds < 1 || max_seeds > 65535)
        return ORBFE_ERR_ARG;
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    orbfe_geometry *g = new (std::nothrow) orbfe_geometry();
    if (!g) return ORBFE_ERR_NOMEM;
    DeviceGuard dg(device);
    g->device = device;
    g->maxw = max_w, g->maxh = max_h, g->maxkp = max_keypoints, g->max_seeds = max_seeds;
    g->dyn_cap = GE_REFS * max_keypoints;
    g->plane = ((size_t)max_w * max_h + 3) & ~(size_t)3;
    for (int i = 0; i <= 2 * GE_RAD; i++) g->ell.hw[i] = (int8_t)geo_ellipse_half_width(GE_RAD, i);
    geometry_clear_db(g);
    const size_t spill_seed = g->plane > (size_t)GE_LDS_ENTRIES ? g->plane - GE_LDS_ENTRIES : 1;
    const size_t per_frame = (size_t)max_seeds * (g->plane + spill_seed * sizeof(GeoEntry));
    g->chunk = (int)std::max<size_t>(1, std::min<size_t>(GE_MAX_CHUNK, GE_SCRATCH_BUDGET / per_frame));
    const size_t c = g->chunk, slots = (size_t)g->dyn_cap;
    const bool ok = orb_alloc_all(
        &g->stream,
        {orb_blk(&g->d_kf_depth, GE_DB * g->plane * sizeof(float)), orb_blk(&g->d_kf_keys, (size_t)GE_DB * max_keypoints * sizeof(float2)),
         orb_blk(&g->d_kf_un, (size_t)GE_DB * max_keypoints * sizeof(float2)), orb_blk(&g->d_kf, GE_DB * sizeof(GeoKF)),
         orb_blk(&g->d_stage, (size_t)2 * max_keypoints * sizeof(orbfe_keypoint)), orb_blk(&g->d_cur, g->plane * sizeof(float)),
         orb_blk(&g->d_pts, c * slots * sizeof(float4)), orb_blk(&g->d_flags, c * slots), orb_blk(&g->d_acc, c * slots),
         orb_blk(&g->d_planes, c * max_seeds * g->plane), orb_blk(&g->d_union, c * g->plane), orb_blk(&g->d_mask, g->plane),
         orb_blk(&g->d_pix, c * slots * sizeof(int2)), orb_blk(&g->d_counts, c * GE_NCOUNT * sizeof(int32_t)),
         orb_blk(&g->d_dyn, c * slots * 3 * sizeof(int32_t)),
         orb_blk(&g->d_spill, c * max_seeds * spill_seed * sizeof(GeoEntry))});
    hipError_t e = ok ? hipFuncSetAttribute((const void *)k_geo_grow, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(GE_LDS_ENTRIES * sizeof(GeoEntry)))
                      : hipSuccess;
    if (ok && e == hipSuccess) e = hipMemset(g->d_kf, 0, GE_DB * sizeof(GeoKF));
    return orb_create_finish(ok && e == hipSuccess, "orbfe_geometry_create", g, geometry_free, out);
}

extern "C" void orbfe_geometry_destroy(orbfe_geometry *g) { orb_destroy(g, geometry_free); }

extern "C" orbfe_status orbfe_geometry_reset(orbfe_geometry *g)
{
    if (!g) return ORBFE_ERR_ARG;
    DeviceGuard dg(g->device);
    ORBFE_HIP(hipStreamSynchronize(g->last_stream));
    geometry_clear_db(g);
    ORBFE_HIP(hipMemset(g->d_kf, 0, GE_DB * sizeof(GeoKF)));
    return ORBFE_OK;
}

extern "C" void *orbfe_geometry_get_stream(orbfe_geometry *g) { return g ? (void *)g->stream : nullptr; }
extern "C" int32_t orbfe_geometry_chunk(orbfe_geometry *g) { return g ? g->chunk : 0; }

extern "C" orbfe_status orbfe_geometry_db_state(orbfe_geometry *g, int32_t *num_elem, int32_t *ini, int32_t *fin, int32_t *slot_insert)
{
    if (!g) return ORBFE_ERR_ARG;
    if (num_elem) *num_elem = g->num;
    if (ini) *ini = g->ini;
    if (fin) *fin = g->fin;
    if (slot_insert)
        for (int i = 0; i < GE_DB; i++) slot_insert[i] = g->slot_insert[i];
    return ORBFE_OK;
}

static bool geometry_size_ok(const orbfe_geometry *g, int w, int h, size_t stride)
{
    return w >= GE_MIN_SIDE && h >= GE_MIN_SIDE && w <= g->maxw && h <= g->maxh && (size_t)w * h <= g->plane && stride >= (size_t)w * 4 &&
           stride % 4 == 0;
}

__global__ void k_geo_keys_xy(const orbfe_keypoint *k, int n, float2 *xy)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xy[i] = make_float2(k[i].x, k[i].y);
}

extern "C" orbfe_status orbfe_geometry_insert_keyframe(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride,
                                                       const orbfe_keypoint *kps, const orbfe_keypoint *kps_un, int32_t n, const float *Tcw,
                                                       int32_t on_device)
{
    if (!g || !depth || !Tcw || n < 0 || n > g->maxkp || (n && (!kps || !kps_un))) return ORBFE_ERR_ARG;
    if (!geometry_size_ok(g, w, h, depth_stride)) return ORBFE_ERR_SIZE;
    DeviceGuard dg(g->device);
    ORBFE_HIP(hipStreamSynchronize(g->last_stream));
    // DataBase::InsertFrame2DB (:532-550)
    const bool full = g->ini == (g->fin + 1) % GE_DB;
    const int slot = full ? g->ini : g->fin;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    ORBFE_HIP(hipMemcpy2DAsync(g->d_kf_depth + (size_t)slot * g->plane, (size_t)w * 4, depth, depth_stride, (size_t)w * 4, h, kind, g->stream));
    if (n) {
        const orbfe_keypoint *dk = kps, *du = kps_un;
        if (!on_device) {
            ORBFE_HIP(hipMemcpyAsync(g->d_stage, kps, (size_t)n * sizeof(orbfe_keypoint), hipMemcpyHostToDevice, g->stream));
            ORBFE_HIP(hipMemcpyAsync(g->d_stage + g->maxkp, kps_un, (size_t)n * sizeof(orbfe_keypoint), hipMemcpyHostToDevice, g->stream));
            dk = g->d_stage, du = g->d_stage + g->maxkp;
        }
        k_geo_keys_xy<<<nblk(n, GE_T), GE_T, 0, g->stream>>>(dk, n, g->d_kf_keys + (size_t)slot * g->maxkp);
        k_geo_keys_xy<<<nblk(n, GE_T), GE_T, 0, g->stream>>>(du, n, g->d_kf_un + (size_t)slot * g->maxkp);
    }
    GeoKF kf{};
    kf.n = n, kf.w = w, kf.h = h;
    kf.t[0] = Tcw[3], kf.t[1] = Tcw[7], kf.t[2] = Tcw[11];
    geo_lu4_factor(Tcw, &kf.lu);
    ORBFE_HIP(hipMemcpyAsync(g->d_kf + slot, &kf, sizeof(kf), hipMemcpyHostToDevice, g->stream));
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(g->stream));
    g->kf[slot] = kf;
    memcpy(g->db_T[slot], Tcw, sizeof(g->db_T[slot]));
    g->slot_insert[slot] = g->inserts++;
    if (!full) {
        g->fin = (g->fin + 1) % GE_DB;
        g->num += 1;
    } else {
        g->fin = g->ini;
        g->ini = (g->ini + 1) % GE_DB;
    }
    return ORBFE_OK;
}

// ---- GetRefFrames (:83-127), host ------------------------------------------------------------------------------------------------
// rotm2euler (:553-573) as it behaves: R is the CV_32F 3x3 block of the pose (row step 16 bytes) read through at<double>, so
// "R(i, j)" is the double made of the 8 bytes at offset i * 16 + j * 8 of the pose; sy, x, y, z are floats.
static double pose_as_double(const float *T, int i, int j)
{
    double v;
    memcpy(&v, (const char *)T + i * 16 + j * 8, 8);
    return v;
}

static void rotm2euler(const float *T, double *e)
{
    const float sy = (float)sqrt(pose_as_double(T, 0, 0) * pose_as_double(T, 0, 0) + pose_as_double(T, 1, 0) * pose_as_double(T, 1, 0));
    const bool singular = sy < 1e-6;
    float x, y, z;
    if (!singular) {
        x = (float)atan2(pose_as_double(T, 2, 1), pose_as_double(T, 2, 2));
        y = (float)atan2(-pose_as_double(T, 2, 0), (double)sy);
        z = (float)atan2(pose_as_double(T, 1, 0), pose_as_double(T, 0, 0));
    } else {
        x = (float)atan2(-pose_as_double(T, 1, 2), pose_as_double(T, 1, 1));
        y = (float)atan2(-pose_as_double(T, 2, 0), (double)sy);
        z = 0;
    }
    e[0] = x, e[1] = y, e[2] = z;
}

extern "C" orbfe_status orbfe_geometry_select_ref_frames(const float *cur_Tcw, const float *db_Tcw, int32_t n, int32_t *idx, int32_t *nref)
{
    if (!cur_Tcw || !db_Tcw || !idx || !nref || n < 1 || n > GE_DB) return ORBFE_ERR_ARG;
    double e1[3], vdist[GE_DB], vrot[GE_DB];
    rotm2euler(cur_Tcw, e1);
    for (int i = 0; i < n; i++) {
        const float *T = db_Tcw + i * 16;
        double e2[3], sr = 0., st = 0.;
        rotm2euler(T, e2);
        for (int k = 0; k < 3; k++) {   // cv::norm(a, b, NORM_L2): normL2Sqr's v = a - b in the data's type, squares summed in double
            const double v = e2[k] - e1[k];
            sr += v * v;
        }
        for (int k = 0; k < 3; k++) {
            const double v = (double)(T[k * 4 + 3] - cur_Tcw[k * 4 + 3]);
            st += v * v;
        }
        vrot[i] = sqrt(sr);
        vdist[i] = sqrt(st);
    }
    double maxd = vdist[0], maxr = vrot[0];
    for (int i = 1; i < n; i++) {
        if (vdist[i] > maxd) maxd = vdist[i];
        if (vrot[i] > maxr) maxr = vrot[i];
    }
    // Mat /= double is convertTo(.., 1. / s): v * (1 / max) + 0; 0.7 * a + 0.3 * b is addWeighted: a * 0.7 + b * 0.3 + 0
    const double sd = 1. / maxd, sr = 1. / maxr;
    double score[GE_DB];
    bool used[GE_DB] = {};
    for (int i = 0; i < n; i++) score[i] = (vdist[i] * sd + 0.) * 0.7 + (vrot[i] * sr + 0.) * 0.3 + 0.;
    *nref = std::min((int)GE_REFS, (int)n);
    for (int r = 0; r < *nref; r++) {   // descending; equal scores are outside the contract
        int b = -1;
        for (int i = 0; i < n; i++)
            if (!used[i] && (b < 0 || score[i] > score[b])) b = i;
        used[b] = true;
        idx[r] = b;
    }
    return ORBFE_OK;
}

// ---- the stages of one chunk -------------------------------------------------------------------------------------------------------
// region growing, union, dilation and mask for n frames whose dynamic points (d_dyn, counts[C_DYN]) are on the device; seed_bound
// = what the host knows the seed count cannot exceed
static orbfe_status geometry_regions(orbfe_geometry *g, int n, const float *d_depth, size_t dstride, size_t dfs, int w, int h,
                                     int seed_bound, uint8_t *d_mask, int mstride, size_t mfs, int32_t *d_ones, hipStream_t st)
{
    const int wh = w * h, wh4 = (wh + 3) & ~3;
    const size_t plane_fs = (size_t)g->max_seeds * g->plane;
    const size_t spill_seed = g->plane > (size_t)GE_LDS_ENTRIES ? g->plane - GE_LDS_ENTRIES : 1;
    ORBFE_HIP(hipMemsetAsync(g->d_union, 0, (size_t)n * wh4, st));
    ORBFE_HIP(hipMemsetAsync(g->d_acc, 0, (size_t)n * g->dyn_cap, st));
    if (d_ones) ORBFE_HIP(hipMemsetAsync(d_ones, 0, (size_t)n * sizeof(int32_t), st));
    const int passes = (seed_bound + g->max_seeds - 1) / g->max_seeds;
    for (int pass = 0; pass < passes; pass++) {
        const int ns = std::min(g->max_seeds, seed_bound - pass * g->max_seeds);
        k_geo_zero_planes<<<dim3(std::min(64u, nblk(wh4 / 4, GE_T)), ns, n), GE_T, 0, st>>>(g->d_counts, pass, g->max_seeds, wh4, g->d_planes,
                                                                                           plane_fs);
        k_geo_grow<<<dim3(ns, n), GE_T, GE_LDS_ENTRIES * sizeof(GeoEntry), st>>>(g->d_counts, pass, g->max_seeds, g->dyn_cap, g->d_dyn, d_depth,
                                                                                dstride, dfs, w, h, wh4, g->d_union, g->d_planes, plane_fs,
                                                                                g->d_spill, spill_seed);
        k_geo_resolve<<<n, GE_T, 0, st>>>(g->d_counts, pass, g->max_seeds, g->dyn_cap, g->d_dyn, d_depth, dstride, dfs, w, wh4, g->d_union,
                                          g->d_planes, plane_fs, g->d_acc);
        k_geo_union<<<dim3(nblk(wh, GE_T), n), GE_T, 0, st>>>(g->d_counts, pass, g->max_seeds, g->dyn_cap, wh, wh4, g->d_planes, plane_fs,
                                                              g->d_acc, g->d_union);
    }
    k_geo_dilate_mask<<<dim3(nblk(w, GD_TW), nblk(h, GD_TH), n), GE_T, 0, st>>>(g->d_union, wh4, g->ell, w, h, d_mask, mstride, mfs, d_ones);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

static orbfe_status geometry_chunk(orbfe_geometry *g, int n, const float *d_depth, size_t dstride, size_t dfs, int w, int h,
                                   const float *Tcw, const float *K, uint8_t *d_mask, int mstride, size_t mfs, int32_t *d_ones,
                                   int32_t *computed, hipStream_t st)
{
    GeoCall call{};
    call.w = w, call.h = h;
    memcpy(call.K, K, sizeof(call.K));
    geo_inv3(K, call.Kinv);
    const bool run = Tcw && g->num >= GE_REFS;
    int seed_bound = 0;
    for (int f = 0; f < n; f++) {
        g->tap_computed[f] = run;
        if (computed) computed[f] = run;
        if (!run) continue;
        GeoFrame &fr = call.fr[f];
        memcpy(fr.T, Tcw + f * 16, sizeof(fr.T));
        int32_t idx[GE_REFS], nref = 0;
        const orbfe_status s = orbfe_geometry_select_ref_frames(fr.T, &g->db_T[0][0], g->num, idx, &nref);
        if (s != ORBFE_OK) return s;
        fr.nref = nref;
        int bound = 0;
        for (int r = 0; r < nref; r++) {
            fr.ref[r] = idx[r];
            bound += g->kf[idx[r]].n;
        }
        seed_bound = std::max(seed_bound, bound);
    }
    ORBFE_HIP(hipMemsetAsync(g->d_counts, 0, (size_t)n * GE_NCOUNT * sizeof(int32_t), st));
    if (run) {
        const int slots = g->dyn_cap;
        k_geo_points<<<dim3(nblk(slots, GE_T), n), GE_T, 0, st>>>(call, g->d_kf, g->d_kf_depth, g->plane, g->d_kf_keys, g->d_kf_un, g->maxkp,
                                                                  g->d_pts, g->d_flags, g->d_counts);
        k_geo_search<<<dim3(nblk(slots, GE_T / 64), n), GE_T, 0, st>>>(call, d_depth, dstride, dfs, g->maxkp, g->d_pts, g->d_flags, g->d_pix,
                                                                       g->d_counts);
        k_geo_compact<<<n, GE_T, 0, st>>>(g->maxkp, g->d_flags, g->d_pix, g->d_dyn, g->d_counts);
    }
    g->tap_n = n, g->tap_w = w, g->tap_h = h;
    return geometry_regions(g, n, d_depth, dstride, dfs, w, h, seed_bound, d_mask, mstride, mfs, d_ones, st);
}

extern "C" orbfe_status orbfe_geometry_correct_batch_device(orbfe_geometry *g, const float *d_depth, int32_t nframes, int32_t w, int32_t h,
                                                            size_t depth_stride, size_t depth_frame_stride, const float *Tcw, float fx,
                                                            float fy, float cx, float cy, uint8_t *d_mask, int32_t mask_stride,
                                                            size_t mask_frame_stride, int32_t *d_mask_ones, int32_t *computed, void *stream)
{
    if (!g || !d_depth || !d_mask || nframes < 1 || mask_stride < w) return ORBFE_ERR_ARG;
    if (!geometry_size_ok(g, w, h, depth_stride) || depth_frame_stride % 4) return ORBFE_ERR_SIZE;
    DeviceGuard dg(g->device);
    hipStream_t st = (hipStream_t)stream;
    if (g->last_stream != st) ORBFE_HIP(hipStreamSynchronize(g->last_stream));   // the scratch is shared
    g->last_stream = st;
    float K[9];
    geo_make_K(fx, fy, cx, cy, K);
    for (int f0 = 0; f0 < nframes; f0 += g->chunk) {
        const int n = std::min(g->chunk, nframes - f0);
        const orbfe_status s = geometry_chunk(g, n, (const float *)((const char *)d_depth + (size_t)f0 * depth_frame_stride), depth_stride,
                                              depth_frame_stride, w, h, Tcw ? Tcw + (size_t)f0 * 16 : nullptr, K,
                                              d_mask + (size_t)f0 * mask_frame_stride, mask_stride, mask_frame_stride,
                                              d_mask_ones ? d_mask_ones + f0 : nullptr, computed ? computed + f0 : nullptr, st);
        if (s != ORBFE_OK) return s;
    }
    return ORBFE_OK;
}

// one host plane into d_cur (rows w floats apart)
static orbfe_status geometry_upload(orbfe_geometry *g, const float *depth, int w, int h, size_t stride)
{
    ORBFE_HIP(hipStreamSynchronize(g->last_stream));
    g->last_stream = g->stream;
    ORBFE_HIP(hipMemcpy2DAsync(g->d_cur, (size_t)w * 4, depth, stride, (size_t)w * 4, h, hipMemcpyHostToDevice, g->stream));
    return ORBFE_OK;
}

static orbfe_status geometry_download(orbfe_geometry *g, int w, int h, uint8_t *mask, int mask_stride)
{
    ORBFE_HIP(hipMemcpy2DAsync(mask, mask_stride, g->d_mask, w, w, h, hipMemcpyDeviceToHost, g->stream));
    ORBFE_HIP(hipStreamSynchronize(g->stream));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_geometry_correct(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride,
                                               const float *Tcw, float fx, float fy, float cx, float cy, uint8_t *mask, int32_t mask_stride,
                                               int32_t *computed)
{
    if (!g || !depth || !mask || mask_stride < w) return ORBFE_ERR_ARG;
    if (!geometry_size_ok(g, w, h, depth_stride)) return ORBFE_ERR_SIZE;
    DeviceGuard dg(g->device);
    orbfe_status s = geometry_upload(g, depth, w, h, depth_stride);
    if (s != ORBFE_OK) return s;
    float K[9];
    geo_make_K(fx, fy, cx, cy, K);
    s = geometry_chunk(g, 1, g->d_cur, (size_t)w * 4, 0, w, h, Tcw, K, g->d_mask, w, 0, nullptr, computed, g->stream);
    if (s != ORBFE_OK) return s;
    return geometry_download(g, w, h, mask, mask_stride);
}

extern "C" orbfe_status orbfe_geometry_depth_region_growing(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride,
                                                            const int32_t *seeds_xy, int32_t n, uint8_t *mask, int32_t mask_stride)
{
    if (!g || !depth || !mask || mask_stride < w || n < 0 || n > g->dyn_cap || (n && !seeds_xy)) return ORBFE_ERR_ARG;
    if (!geometry_size_ok(g, w, h, depth_stride)) return ORBFE_ERR_SIZE;
    std::vector<int32_t> dyn((size_t)n * 3);
    for (int i = 0; i < n; i++) {
        const int x = seeds_xy[i * 2], y = seeds_xy[i * 2 + 1];
        if (x < 0 || y < 0 || x >= w || y >= h) return ORBFE_ERR_ARG;
        dyn[(size_t)i * 3] = x, dyn[(size_t)i * 3 + 1] = y, dyn[(size_t)i * 3 + 2] = 0;
    }
    DeviceGuard dg(g->device);
    orbfe_status s = geometry_upload(g, depth, w, h, depth_stride);
    if (s != ORBFE_OK) return s;
    int32_t counts[GE_NCOUNT] = {};
    counts[C_DYN] = n;
    ORBFE_HIP(hipMemcpyAsync(g->d_counts, counts, sizeof(counts), hipMemcpyHostToDevice, g->stream));
    if (n) ORBFE_HIP(hipMemcpyAsync(g->d_dyn, dyn.data(), dyn.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    ORBFE_HIP(hipStreamSynchronize(g->stream));   // counts and dyn are this call's locals
    g->tap_n = 1, g->tap_w = w, g->tap_h = h, g->tap_computed[0] = 1;
    s = geometry_regions(g, 1, g->d_cur, (size_t)w * 4, 0, w, h, n, g->d_mask, w, 0, nullptr, g->stream);
    if (s != ORBFE_OK) return s;
    return geometry_download(g, w, h, mask, mask_stride);
}

extern "C" orbfe_status orbfe_geometry_tap(orbfe_geometry *g, int32_t frame, int32_t stage, int32_t index, void *dst, size_t cap,
                                           int32_t *count)
{
    if (!g || !dst || !count) return ORBFE_ERR_ARG;
    if (frame < 0 || frame >= g->tap_n || !g->tap_computed[frame]) return ORBFE_ERR_STATE;
    DeviceGuard dg(g->device);
    ORBFE_HIP(hipStreamSynchronize(g->last_stream));
    int32_t counts[GE_NCOUNT];
    ORBFE_HIP(hipMemcpy(counts, g->d_counts + frame * GE_NCOUNT, sizeof(counts), hipMemcpyDeviceToHost));
    const int wh = g->tap_w * g->tap_h, wh4 = (wh + 3) & ~3;
    const void *src = nullptr;
    size_t bytes = 0;
    switch (stage) {
    case ORBFE_GEOMETRY_TAP_COUNTS:
        *count = GE_NCOUNT;
        if (cap < sizeof(counts)) return ORBFE_ERR_CAP;
        memcpy(dst, counts, sizeof(counts));
        return ORBFE_OK;
    case ORBFE_GEOMETRY_TAP_DYN:
        *count = counts[C_DYN];
        src = g->d_dyn + (size_t)frame * g->dyn_cap * 3, bytes = (size_t)counts[C_DYN] * 3 * sizeof(int32_t);
        break;
    case ORBFE_GEOMETRY_TAP_SEEDS:
        *count = counts[C_DYN];
        src = g->d_acc + (size_t)frame * g->dyn_cap, bytes = (size_t)counts[C_DYN];
        break;
    case ORBFE_GEOMETRY_TAP_UNION:
        *count = wh;
        src = g->d_union + (size_t)frame * wh4, bytes = wh;
        break;
    case ORBFE_GEOMETRY_TAP_REGION: {
        if (index < 0 || index >= g->max_seeds) return ORBFE_ERR_ARG;
        *count = wh;
        if (counts[C_DYN] < 1) return ORBFE_ERR_STATE;
        const int last = (counts[C_DYN] - 1) / g->max_seeds;   // the last pass that had seeds: the later ones touch nothing
        if (index >= counts[C_DYN] - last * g->max_seeds) return ORBFE_ERR_STATE;
        if (cap < (size_t)wh) return ORBFE_ERR_CAP;
        uint8_t grown = 0;   // a seed of the pass that an earlier seed of the pass covers was grown beside it, and is not part of the result
        ORBFE_HIP(hipMemcpy(&grown, g->d_acc + (size_t)frame * g->dyn_cap + (size_t)last * g->max_seeds + index, 1, hipMemcpyDeviceToHost));
        if (!grown) {
            memset(dst, 0, wh);
            return ORBFE_OK;
        }
        src = g->d_planes + (size_t)frame * g->max_seeds * g->plane + (size_t)index * wh4, bytes = wh;
        break;
    }
    default:
        return ORBFE_ERR_ARG;
    }
    if (cap < bytes) return ORBFE_ERR_CAP;
    if (bytes) ORBFE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_geometry_kat(int32_t what, int32_t n, const double *in, double *out)
{
    if (what != ORBFE_GEOMETRY_KAT_ACOS || n < 1 || !in || !out) return ORBFE_ERR_ARG;
    return orb_kat_run("orbfe_geometry_kat", in, (size_t)n * 8, out, (size_t)n * 8, 0, [&](void *d_in, void *d_out, void *) {
        k_geo_kat_acos<<<nblk(n, GE_T), GE_T>>>((const double *)d_in, (double *)d_out, n);
    });
}
