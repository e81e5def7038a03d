// orbfe_tri_search.hip -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:827-1019) as LocalMapping::CreateNewMapPoints runs it
// (src/LocalMapping.cc:349-422), for a batch of keyframe pairs, device-resident (include/orbfe.h "SearchForTriangulation, batched";
// DESIGN.md 8n):
//   k_tri_pairs        the baseline gate, ComputeF12 and the epipole of every pair (csrc/orbfe_f12.h), one thread per pair
//   k_tri_ranges       the merge walk over the two FeatureVectors as a lookup: every entry of keyframe 1's FeatureVector finds its
//                      node in keyframe 2's ascending node list
//   k_tri_search       one workgroup per (pair, keyframe-1 node): the node's keyframe-2 features staged in LDS tiles, a group of
//                      lanes per keyframe-1 feature, the minimum of dist << 16 | (0xFFFF - position) over the passing candidates
//   k_tri_search_flat  the same result with one thread per keyframe-1 feature and no staging (orbfe_matcher_set_triangulation_kernel;
//                      kept for the measurement and as a second opinion in the tests)
//   k_tri_replay       the rotation histogram, ComputeThreeMaxima, nmatches and vMatchedPairs, one workgroup per pair
// Everything is enqueued on the caller's stream; nothing waits and nothing writes host memory.
#include <string.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"
#include "orbfe_track_dev.h"
#include "orbfe_f12.h"

static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float) && offsetof(orbfe_keypoint, octave) == 20 && offsetof(orbfe_keypoint, angle) == 12,
              "keypoint record = 7 floats: (x, y) first, angle fourth, octave sixth");

#define TRI_T 256                // threads of every workgroup here
#define TRI_L 8                  // lanes per keyframe-1 feature in k_tri_search: 32 queries per pass
#define TRI_TILE 64              // keyframe-2 features per LDS tile
#define TRI_REC 12               // dwords per staged feature: descriptor 8, x, y, flags | octave << 8, one of padding (48 bytes: 16-byte
                                 // aligned rows, and the 8 lanes of a group read 8 different banks at a stride of 12 dwords)
#define TRI_NODE_WGS 128         // workgroups per pair; they take the keyframe-1 nodes round robin
#define TRI_MAX_CAP 8192         // the BoW block's limit; a list position fits the key's 16 bits
#define TRI_NOKEY 0xFFFFFFFFu
static_assert(TRI_T == TRK_GT, "k_tri_replay compacts with trk_compact_pos");
static_assert(TRI_TILE * 4 == TRI_T && TRI_T % TRI_L == 0 && TRI_MAX_CAP <= 0x10000, "staging: four waves fill one tile");

struct TriBatchArgs {
    orbfe_tri_keyframes K;
    const int32_t *kf1, *kf2;
    int32_t npairs;
    const float *F12, *epi;
    const uint8_t *skip;
    TrkLevels scale, sigma2;
    int32_t nlevels, th_low, only_stereo, check_ori;
    int32_t per_node;            // what `range` is indexed by: 1 keyframe-1 node (k_tri_search), 0 keyframe-1 feature (k_tri_search_flat)
    int32_t *range;              // [P][cap][2]: the slice of keyframe 2's fv_idx that belongs to the node / the feature's node, (0, 0) = none
    orbfe_tri_out O;
};

// one keyframe of the block, counts clamped into [0, cap]
struct TriFrame {
    const float *kps;
    const uint8_t *desc, *has_mp;
    const float *uright;
    const uint32_t *node, *off, *idx;
    int n, nfv, total;
};
__device__ __forceinline__ bool tri_frame(const TriBatchArgs &a, int f, TriFrame &F)
{
    if (f < 0 || f >= a.K.nframes) return false;
    const int cap = a.K.cap;
    const int64_t fb = (int64_t)f * cap;
    F.kps = (const float *)a.K.d_kps + fb * 7;
    F.desc = a.K.d_desc + fb * 32;
    F.has_mp = a.K.d_has_mp ? a.K.d_has_mp + fb : nullptr;
    F.uright = a.K.d_uright ? a.K.d_uright + fb : nullptr;
    F.node = a.K.d_fv_node + fb;
    F.off = a.K.d_fv_off + (int64_t)f * (cap + 1);
    F.idx = a.K.d_fv_idx + fb;
    F.n = min(max(a.K.d_n[f], 0), cap);
    F.nfv = min(max(a.K.d_counts[(int64_t)f * 4 + 1], 0), cap);
    F.total = F.nfv > 0 ? (int)min(F.off[F.nfv], (uint32_t)cap) : 0;
    return true;
}
// the two keyframes of pair p; false = the pair makes no matches (skipped, or a frame index outside the block)
__device__ __forceinline__ bool tri_pair(const TriBatchArgs &a, int p, TriFrame &F1, TriFrame &F2)
{
    if (a.skip && a.skip[p]) return false;
    return tri_frame(a, a.kf1[p], F1) && tri_frame(a, a.kf2[p], F2);
}
__device__ __forceinline__ bool tri_stereo(const TriFrame &F, int i) { return F.uright && F.uright[i] >= 0.f; }
// :868-880 / :884-891: no MapPoint in the slot, and stereo if bOnlyStereo
__device__ __forceinline__ bool tri_elig(const TriBatchArgs &a, const TriFrame &F, int i)
{
    return !(F.has_mp && F.has_mp[i]) && (!a.only_stereo || tri_stereo(F, i));
}

// ---------------------------------------------------------------------------------------------------
// 0. src/LocalMapping.cc:390-417 + src/ORBmatcher.cc:833-843 for every pair
// ---------------------------------------------------------------------------------------------------
struct TriPairArgs {
    const float *Tcw, *Ow, *median;
    int32_t nframes, npairs, mono;
    orbfe_track_camera cam;
    float mb;
    const int32_t *kf1, *kf2;
    float *F12, *epi;
    uint8_t *skip;
};
__global__ __launch_bounds__(TRI_T) void k_tri_pairs(TriPairArgs a)
{
    const int p = blockIdx.x * TRI_T + threadIdx.x;
    if (p >= a.npairs) return;
    const int k1 = a.kf1[p], k2 = a.kf2[p];
    float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ex = 0.f, ey = 0.f;
    bool skip = true;
    if (k1 >= 0 && k1 < a.nframes && k2 >= 0 && k2 < a.nframes) {
        const float *T1 = a.Tcw + (int64_t)k1 * 12, *T2 = a.Tcw + (int64_t)k2 * 12, *O1 = a.Ow + (int64_t)k1 * 3, *O2 = a.Ow + (int64_t)k2 * 3;
        f12_compute(T1, T2, a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy, F);
        f12_epipole(T2, O1, a.cam.fx, a.cam.fy, a.cam.cx, a.cam.cy, &ex, &ey);
        skip = f12_baseline_skip(O1, O2, a.mono, a.mb, a.mono ? a.median[k2] : 0.f);
    }
    for (int k = 0; k < 9; ++k) a.F12[(int64_t)p * 9 + k] = F[k];
    a.epi[(int64_t)p * 2] = ex;
    a.epi[(int64_t)p * 2 + 1] = ey;
    a.skip[p] = skip ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------
// 1. The merge walk of :849-964 without the walk.  Both node lists ascend, so the walk pairs exactly the entries with equal node
// ids, whether it steps or skips with lower_bound; entry e of keyframe 1's fv_idx finds its node a by the offsets and a's id in
// keyframe 2's list by bisection.  `range` is zero before the launch: (0, 0) = no common node, a feature in no node, a
// pair that is skipped.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_T) void k_tri_ranges(TriBatchArgs a)
{
    const int p = blockIdx.x, e = blockIdx.y * TRI_T + threadIdx.x, cap = a.K.cap;
    TriFrame F1, F2;
    if (!tri_pair(a, p, F1, F2) || e >= F1.total) return;
    int lo = 0, hi = F1.nfv;   // the first node whose end lies behind e
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (F1.off[mid + 1] > (uint32_t)e) hi = mid; else lo = mid + 1;
    }
    if (lo >= F1.nfv || F1.off[lo] > (uint32_t)e) return;
    if (a.per_node && (uint32_t)e != F1.off[lo]) return;   // the node's first entry writes for the node
    const uint32_t node = F1.node[lo];
    int b = -1, l = 0, h = F2.nfv - 1;
    while (l <= h) {
        const int mid = (l + h) >> 1;
        const uint32_t v = F2.node[mid];
        if (v == node) { b = mid; break; }
        if (v < node) l = mid + 1; else h = mid - 1;
    }
    if (b < 0) return;
    const int s = (int)min(F2.off[b], (uint32_t)cap), t = (int)min(F2.off[b + 1], (uint32_t)cap);
    if (t <= s) return;
    int64_t at = lo;
    if (!a.per_node) {
        const uint32_t f1 = F1.idx[e];
        if (f1 >= (uint32_t)F1.n) return;
        at = f1;
    }
    a.range[((int64_t)p * cap + at) * 2] = s;
    a.range[((int64_t)p * cap + at) * 2 + 1] = t;
}

// ---------------------------------------------------------------------------------------------------
// 2. The search.  The reference's loop over a node's keyframe-2 features never sets vbMatched2, a candidate that fails a gate leaves
// bestDist alone and one that passes with dist <= bestDist takes over: the result of a query is, among the candidates that pass every
// gate with dist <= th_low, the smallest distance and the LAST list position on ties = the minimum of dist << 16 | (0xFFFF - pos).
// A minimum needs no order, so the lanes of a group take the tile's candidates interleaved and merge with cross-lane moves.
// ---------------------------------------------------------------------------------------------------
// a staged keyframe-2 feature, as tri_candidate reads it
struct TriTileCand {
    const uint32_t *r;
    const float *s_scale, *s_sigma2;
    __device__ __forceinline__ bool elig() const { return (r[10] & 1u) != 0; }
    __device__ __forceinline__ const uint32_t *desc() const { return r; }
    __device__ __forceinline__ float x() const { return __uint_as_float(r[8]); }
    __device__ __forceinline__ float y() const { return __uint_as_float(r[9]); }
    __device__ __forceinline__ bool stereo() const { return (r[10] & 2u) != 0; }
    __device__ __forceinline__ float scale() const { return s_scale[r[10] >> 8]; }
    __device__ __forceinline__ float sigma2() const { return s_sigma2[r[10] >> 8]; }
};

__global__ __launch_bounds__(TRI_T) void k_tri_search(TriBatchArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_c[TRI_TILE * TRI_REC];
    __shared__ float s_scale[TRK_MAX_LEVELS], s_sigma2[TRK_MAX_LEVELS];
    const int p = blockIdx.x, tid = threadIdx.x, sub = tid % TRI_L, grp = tid / TRI_L, cap = a.K.cap;
    TriFrame F1, F2;
    if (!tri_pair(a, p, F1, F2)) return;   // workgroup-uniform
    if (tid < TRK_MAX_LEVELS) {
        s_scale[tid] = a.scale.v[tid];
        s_sigma2[tid] = a.sigma2.v[tid];
    }
    float F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = a.F12[(int64_t)p * 9 + k];
    const float ex = a.epi[(int64_t)p * 2], ey = a.epi[(int64_t)p * 2 + 1];
    int32_t *match12 = a.O.d_match12 + (int64_t)p * cap;
    for (int an = blockIdx.y; an < F1.nfv; an += gridDim.y) {   // every condition below is workgroup-uniform
        const int lo = a.range[((int64_t)p * cap + an) * 2], hi = a.range[((int64_t)p * cap + an) * 2 + 1];
        const int q0 = (int)min(F1.off[an], (uint32_t)cap), q1 = (int)min(F1.off[an + 1], (uint32_t)cap);
        if (hi <= lo || q1 <= q0) continue;
        const int n2 = hi - lo, ntiles = (n2 + TRI_TILE - 1) / TRI_TILE;
        for (int qb = q0; qb < q1; qb += TRI_T / TRI_L) {
            const int q = qb + grp;
            uint32_t f1 = 0;
            bool qok = q < q1;
            if (qok) {
                f1 = F1.idx[q];
                qok = f1 < (uint32_t)F1.n && tri_elig(a, F1, (int)f1);
            }
            Desc8 d1;
            TriLine line;
            bool st1 = false;
            if (qok) {
                d1 = load_desc8(F1.desc + (int64_t)f1 * 32);
                st1 = tri_stereo(F1, (int)f1);
                line = tri_line(F1.kps[(int64_t)f1 * 7], F1.kps[(int64_t)f1 * 7 + 1], F);
            }
            uint32_t key = TRI_NOKEY;
            for (int t = 0; t < ntiles; ++t) {
                if (ntiles > 1 || qb == q0) {   // a list of one tile is staged once for all the node's queries
                    __syncthreads();            // the readers of what the tile held are done
                    const int c = tid & (TRI_TILE - 1), part = tid / TRI_TILE, pos = t * TRI_TILE + c;
                    uint32_t w0 = 0, w1 = 0, meta = 0;
                    uint32_t f2 = 0xFFFFFFFFu;
                    if (pos < n2) f2 = F2.idx[lo + pos];
                    if (f2 < (uint32_t)F2.n) {   // an entry >= n is no candidate, nor is a feature whose octave has no level
                        const int o2 = ((const int32_t *)F2.kps)[(int64_t)f2 * 7 + 5];
                        if (o2 >= 0 && o2 < a.nlevels) {
                            const uint32_t *dp = (const uint32_t *)(F2.desc + (int64_t)f2 * 32) + part * 2;
                            w0 = dp[0];
                            w1 = dp[1];
                            meta = (tri_elig(a, F2, (int)f2) ? 1u : 0u) | (tri_stereo(F2, (int)f2) ? 2u : 0u) | ((uint32_t)o2 << 8);
                        }
                    }
                    uint32_t *r = s_c + c * TRI_REC;
                    r[part * 2] = w0;
                    r[part * 2 + 1] = w1;
                    if (part == 0) {
                        const bool live = (meta & 1u) != 0;
                        r[8] = live ? __float_as_uint(F2.kps[(int64_t)f2 * 7]) : 0u;
                        r[9] = live ? __float_as_uint(F2.kps[(int64_t)f2 * 7 + 1]) : 0u;
                        r[10] = meta;
                    }
                    __syncthreads();
                }
                if (qok) {
                    const int cnt = min(TRI_TILE, n2 - t * TRI_TILE);
                    for (int c = sub; c < cnt; c += TRI_L) {
                        const int dist = tri_candidate(d1, st1, line, ex, ey, a.th_low, TriTileCand{s_c + c * TRI_REC, s_scale, s_sigma2});
                        if (dist >= 0) key = min(key, ((uint32_t)dist << 16) | (uint32_t)(0xFFFF - (t * TRI_TILE + c)));
                    }
                }
            }
#pragma unroll
            for (int s = TRI_L / 2; s > 0; s >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, s, TRI_L));
            if (qok && sub == 0) match12[f1] = key == TRI_NOKEY ? -1 : (int32_t)F2.idx[lo + (0xFFFF - (int)(key & 0xFFFFu))];
        }
    }
}

// keyframe-2 feature f of the pair read in place, for the kernel without staging
struct TriFrameCand {
    const TriBatchArgs &a;
    const TriFrame &F2;
    uint32_t f;
    int o2;
    __device__ __forceinline__ bool elig() const { return o2 >= 0 && o2 < a.nlevels && tri_elig(a, F2, (int)f); }
    __device__ __forceinline__ const uint32_t *desc() const { return (const uint32_t *)(F2.desc + (int64_t)f * 32); }
    __device__ __forceinline__ float x() const { return F2.kps[(int64_t)f * 7]; }
    __device__ __forceinline__ float y() const { return F2.kps[(int64_t)f * 7 + 1]; }
    __device__ __forceinline__ bool stereo() const { return tri_stereo(F2, (int)f); }
    __device__ __forceinline__ float scale() const { return a.scale.v[o2]; }
    __device__ __forceinline__ float sigma2() const { return a.sigma2.v[o2]; }
};

// one thread per keyframe-1 feature walks its node's list in order, as k_triangulation does for one pair
__global__ __launch_bounds__(TRI_T) void k_tri_search_flat(TriBatchArgs a)
{
    const int p = blockIdx.x, f1 = blockIdx.y * TRI_T + threadIdx.x, cap = a.K.cap;
    TriFrame F1, F2;
    if (!tri_pair(a, p, F1, F2) || f1 >= F1.n) return;
    const int lo = a.range[((int64_t)p * cap + f1) * 2], hi = a.range[((int64_t)p * cap + f1) * 2 + 1];
    if (hi <= lo || !tri_elig(a, F1, f1)) return;
    const Desc8 d1 = load_desc8(F1.desc + (int64_t)f1 * 32);
    const bool st1 = tri_stereo(F1, f1);
    float F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = a.F12[(int64_t)p * 9 + k];
    const float ex = a.epi[(int64_t)p * 2], ey = a.epi[(int64_t)p * 2 + 1];
    const TriLine line = tri_line(F1.kps[(int64_t)f1 * 7], F1.kps[(int64_t)f1 * 7 + 1], F);
    int best = -1, bestDist = a.th_low;
    for (int i2 = lo; i2 < hi; ++i2) {
        const uint32_t f2 = F2.idx[i2];
        if (f2 >= (uint32_t)F2.n) continue;
        const int dist = tri_candidate(d1, st1, line, ex, ey, bestDist, TriFrameCand{a, F2, f2, ((const int32_t *)F2.kps)[(int64_t)f2 * 7 + 5]});
        if (dist >= 0) {
            best = (int)f2;
            bestDist = dist;
        }
    }
    a.O.d_match12[(int64_t)p * cap + f1] = best;
}

// ---------------------------------------------------------------------------------------------------
// 3. :919-997 from match12, one workgroup per pair: the 30-bin histogram of kp1.angle - kp2.angle (rot_bin: + 360 when negative,
// times 1.0f / 30 -- the reference's factor, sic --, round, 30 -> 0), ComputeThreeMaxima, the matches of the other bins cleared,
// nmatches = what stands, and vMatchedPairs = the standing matches in ascending keyframe-1 index (order-preserving compaction).
// The histogram counts with LDS atomics; a count does not depend on their order.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_T) void k_tri_replay(TriBatchArgs a)
{
    __shared__ int s_hist[ORBFE_HISTO_LENGTH], s_keep[3], s_wave[TRI_T / 64];
    const int p = blockIdx.x, tid = threadIdx.x, cap = a.K.cap;
    TriFrame F1, F2;
    const bool live = tri_pair(a, p, F1, F2);   // workgroup-uniform
    const int n1 = live ? F1.n : 0, n2 = live ? F2.n : 0;
    int32_t *match12 = a.O.d_match12 + (int64_t)p * cap;
    auto bin_of = [&](int i, int m) { return rot_bin_clamped(F1.kps[(int64_t)i * 7 + 3], F2.kps[(int64_t)m * 7 + 3]); };
    if (a.check_ori) {
        if (tid < ORBFE_HISTO_LENGTH) s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n1; i += TRI_T) {
            const int m = match12[i];
            if (m >= 0 && m < n2) atomicAdd(&s_hist[bin_of(i, m)], 1);
        }
        __syncthreads();
        if (tid == 0) rot_three_maxima(s_hist, ORBFE_HISTO_LENGTH, s_keep);
        __syncthreads();
    }
    int base = 0;
    for (int i0 = 0; i0 < cap; i0 += TRI_T) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        int m = i < n1 ? match12[i] : -1;
        if (m >= n2) m = -1;
        if (m >= 0 && a.check_ori && !rot_keeps(s_keep, bin_of(i, m))) m = -1;
        if (i < cap) match12[i] = m;
        int tot;
        const int pos = base + trk_compact_pos(m >= 0, s_wave, &tot);
        if (m >= 0 && a.O.d_pairs) {
            a.O.d_pairs[((int64_t)p * cap + pos) * 2] = i;
            a.O.d_pairs[((int64_t)p * cap + pos) * 2 + 1] = m;
        }
        base += tot;
    }
    if (tid == 0) {
        a.O.d_nmatches[p] = base;
        if (a.O.d_npairs) a.O.d_npairs[p] = base;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace
{
bool tri_limits_ok(int64_t npairs, int64_t cap) { return npairs >= 0 && cap >= 1 && cap <= TRI_MAX_CAP && npairs * cap < TRK_MAX_SLOTS; }
size_t tri_range_bytes(int32_t npairs, int32_t cap) { return orb_align256(std::max<size_t>((size_t)npairs * (size_t)cap * 8, 4)); }
}  // namespace

extern "C" int64_t orbfe_tri_search_scratch_bytes(int32_t npairs, int32_t cap)
{
    if (!tri_limits_ok(npairs, cap)) return -1;
    return (int64_t)tri_range_bytes(npairs, cap);
}

extern "C" int32_t orbfe_tri_search_info(int32_t what)
{
    switch (what) {
    case ORBFE_TRI_INFO_LANES: return TRI_L;
    case ORBFE_TRI_INFO_TILE: return TRI_TILE;
    case ORBFE_TRI_INFO_QUERIES_PER_PASS: return TRI_T / TRI_L;
    case ORBFE_TRI_INFO_NODE_WORKGROUPS: return TRI_NODE_WGS;
    case ORBFE_TRI_INFO_MAX_CAP: return TRI_MAX_CAP;
    default: return -1;
    }
}

extern "C" orbfe_status orbfe_matcher_set_triangulation_kernel(orbfe_matcher *m, int32_t kernel)
{
    if (!m || kernel < 0 || kernel > 1) {
        orbfe_set_error("orbfe_matcher_set_triangulation_kernel: 0 = LDS tiles, 1 = one thread per feature");
        return ORBFE_ERR_ARG;
    }
    m->tri_kernel = kernel;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_compute_f12(const float *Tcw1, const float *Tcw2, const orbfe_track_camera *cam, float *F12)
{
    if (!Tcw1 || !Tcw2 || !cam || !F12) {
        orbfe_set_error("bad argument to orbfe_compute_f12");
        return ORBFE_ERR_ARG;
    }
    f12_compute(Tcw1, Tcw2, cam->fx, cam->fy, cam->cx, cam->cy, F12);
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_triangulation_pairs_batch_device(orbfe_matcher *m, const float *d_Tcw, const float *d_Ow, int32_t nframes,
                                                               const orbfe_track_camera *cam, float mb, int32_t mono,
                                                               const float *d_median_depth, const int32_t *d_kf1, const int32_t *d_kf2,
                                                               int32_t npairs, float *d_F12, float *d_epi, uint8_t *d_pair_skip,
                                                               void *stream)
{
    if (!m || !cam || nframes < 0 || npairs < 0 || (mono && npairs > 0 && !d_median_depth) ||
        (npairs > 0 && (!d_Tcw || !d_Ow || !d_kf1 || !d_kf2 || !d_F12 || !d_epi || !d_pair_skip))) {
        orbfe_set_error("bad argument to orbfe_triangulation_pairs_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    TriPairArgs a;
    a.Tcw = d_Tcw; a.Ow = d_Ow; a.median = d_median_depth;
    a.nframes = nframes; a.npairs = npairs; a.mono = mono ? 1 : 0;
    a.cam = *cam;
    a.mb = mb;
    a.kf1 = d_kf1; a.kf2 = d_kf2;
    a.F12 = d_F12; a.epi = d_epi; a.skip = d_pair_skip;
    hipLaunchKernelGGL(k_tri_pairs, dim3((npairs + TRI_T - 1) / TRI_T), dim3(TRI_T), 0, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_search_for_triangulation_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const int32_t *d_kf1,
                                                                    const int32_t *d_kf2, int32_t npairs, const float *d_F12,
                                                                    const float *d_epi, const uint8_t *d_pair_skip,
                                                                    const float *scale_factors, const float *level_sigma2, int32_t nlevels,
                                                                    int32_t th_low, int32_t only_stereo, int32_t check_ori,
                                                                    const orbfe_tri_out *out, void *stream)
{
    const char *who = "orbfe_search_for_triangulation_batch_device";
    if (!m || !kf || !out || npairs < 0 || kf->nframes < 0 || kf->cap < 1 || !scale_factors || !level_sigma2 || nlevels < 1 || th_low < 0 ||
        (!out->d_pairs) != (!out->d_npairs) ||
        (npairs > 0 && (!kf->d_kps || !kf->d_desc || !kf->d_n || !kf->d_fv_node || !kf->d_fv_off || !kf->d_fv_idx || !kf->d_counts || !d_kf1 ||
                        !d_kf2 || !d_F12 || !d_epi || !out->d_match12 || !out->d_nmatches))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    if (th_low > 255) { orbfe_set_error("%s: th_low must be below 256", who); return ORBFE_ERR_ARG; }
    if (nlevels > TRK_MAX_LEVELS) { orbfe_set_error("%s: at most %d levels", who, TRK_MAX_LEVELS); return ORBFE_ERR_SIZE; }
    if (!tri_limits_ok(npairs, kf->cap)) {
        orbfe_set_error("%s: cap <= %d and npairs * cap < 2^25", who, TRI_MAX_CAP);
        return ORBFE_ERR_SIZE;
    }
    if (npairs == 0) return ORBFE_OK;
    const int32_t cap = kf->cap;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const size_t rb = tri_range_bytes(npairs, cap);
    ORBFE_HIP(m->b[6].ensure(rb));
    TriBatchArgs a;
    memset(&a, 0, sizeof(a));
    a.K = *kf;
    a.kf1 = d_kf1; a.kf2 = d_kf2;
    a.npairs = npairs;
    a.F12 = d_F12; a.epi = d_epi; a.skip = d_pair_skip;
    for (int k = 0; k < TRK_MAX_LEVELS; ++k) {   // a level past nlevels is never indexed
        a.scale.v[k] = k < nlevels ? scale_factors[k] : 0.f;
        a.sigma2.v[k] = k < nlevels ? level_sigma2[k] : 0.f;
    }
    a.nlevels = nlevels; a.th_low = th_low; a.only_stereo = only_stereo ? 1 : 0; a.check_ori = check_ori ? 1 : 0;
    a.per_node = m->tri_kernel == 1 ? 0 : 1;
    a.range = m->b[6].as<int32_t>();
    a.O = *out;
    ORBFE_HIP(hipMemsetAsync(m->b[6].p, 0, rb, st));
    ORBFE_HIP(hipMemsetAsync(out->d_match12, 0xFF, (size_t)npairs * (size_t)cap * 4, st));
    const dim3 per_feature(npairs, (cap + TRI_T - 1) / TRI_T);   // pairs in x: the batch may exceed 65535
    hipLaunchKernelGGL(k_tri_ranges, per_feature, dim3(TRI_T), 0, st, a);
    if (m->tri_kernel == 1) hipLaunchKernelGGL(k_tri_search_flat, per_feature, dim3(TRI_T), 0, st, a);
    else hipLaunchKernelGGL(k_tri_search, dim3(npairs, std::min(cap, TRI_NODE_WGS)), dim3(TRI_T), 0, st, a);
    hipLaunchKernelGGL(k_tri_replay, dim3(npairs), dim3(TRI_T), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}
