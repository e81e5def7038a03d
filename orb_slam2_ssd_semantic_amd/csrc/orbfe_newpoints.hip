// orbfe_newpoints.hip -- the rest of LocalMapping::CreateNewMapPoints' neighbour loop (src/LocalMapping.cc:424-615) and
// KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:724-754) on the keyframe block of the batched SearchForTriangulation,
// device-resident (include/orbfe.h "CreateNewMapPoints, device-resident"):
//   k_np_triangulate   one workgroup per (pair, chunk of NP_T matches), one thread per match: np_triangulate_match
//                      (csrc/orbfe_newpoints.h, the body the host orbfe_triangulate_match runs) with the 4 x 4 Jacobi workspace
//                      in LDS, lane-interleaved; writes the verdict and the point of every match
//   k_np_compact       one workgroup per pair: the accepted matches in vMatchedIndices order (trk_compact_pos, no atomics)
//   k_np_median        one workgroup per keyframe: the depths of the occupied slots as order-preserving keys in LDS, an exact
//                      radix selection of the ((count - 1) / q)-th smallest
//   k_np_claim_max / k_np_claim_write   the slots of a round's new points: the maximum id per slot, then the winner's data
// orbfe_create_new_map_points_batch_device chains these with the pair preparation and the search of orbfe_tri_search.hip round by
// round on the caller's stream; nothing waits and nothing writes host memory.  orbfe_newpoints_plan_rounds is host only.
#include <string.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_track_dev.h"
#include "orbfe_newpoints.h"

#define NP_T 256             // threads of every workgroup here
#define NP_MAX_CAP 8192      // the BoW block's limit; k_np_median keeps cap keys in LDS (32 KiB)
static_assert(NP_T == TRK_GT, "k_np_compact and k_np_median compact with trk_compact_pos");

struct NpArgs {
    orbfe_tri_keyframes K;
    orbfe_newpt_geom G;
    const int32_t *kf1, *kf2;
    const int32_t *pairs, *npairs;
    TrkLevels scale, sigma2;
    int32_t nlevels;
    float *xyz_all;          // [P][cap][3] scratch: the point of every match
    orbfe_newpt_out O;
};

// the number of matches of pair p that are looked at: 0 for a frame index outside the block
__device__ __forceinline__ int np_count(const NpArgs &a, int p)
{
    const int k1 = a.kf1[p], k2 = a.kf2[p];
    if (k1 < 0 || k1 >= a.K.nframes || k2 < 0 || k2 >= a.K.nframes) return 0;
    return min(max(a.npairs[p], 0), a.K.cap);
}

__device__ __forceinline__ bool np_key(const NpArgs &a, int f, int idx, orbfe_newpt_key &k)
{
    const int cap = a.K.cap, n = min(max(a.K.d_n[f], 0), cap);
    if (idx < 0 || idx >= n) return false;
    const int64_t at = (int64_t)f * cap + idx;
    const float *un = (const float *)a.K.d_kps + at * 7;
    const float *raw = a.G.d_kps_raw ? (const float *)a.G.d_kps_raw + at * 7 : un;
    k.ux = un[0];
    k.uy = un[1];
    k.octave = ((const int32_t *)un)[5];
    k.rx = raw[0];
    k.ry = raw[1];
    k.uright = a.K.d_uright ? a.K.d_uright[at] : -1.f;
    k.depth = a.G.d_depth ? a.G.d_depth[at] : -1.f;
    return k.octave >= 0 && k.octave < a.nlevels;
}

__global__ __launch_bounds__(NP_T) void k_np_triangulate(NpArgs a)
{
    __shared__ float s_At[16 * NP_T], s_Vt[16 * NP_T];
    __shared__ double s_W[4 * NP_T];
    __shared__ float s_T[24], s_O[6], s_scale[TRK_MAX_LEVELS], s_sigma2[TRK_MAX_LEVELS];
    const int p = blockIdx.x, tid = threadIdx.x, j = blockIdx.y * NP_T + tid, cap = a.K.cap;
    const int cnt = np_count(a, p);
    if ((int)blockIdx.y * NP_T >= cnt) return;   // workgroup-uniform
    const int f1 = a.kf1[p], f2 = a.kf2[p];
    if (tid < 24) s_T[tid] = a.G.d_Tcw[(int64_t)(tid < 12 ? f1 : f2) * 12 + tid % 12];
    if (tid >= 32 && tid < 38) s_O[tid - 32] = a.G.d_Ow[(int64_t)(tid < 35 ? f1 : f2) * 3 + (tid - 32) % 3];
    if (tid >= 64 && tid < 64 + TRK_MAX_LEVELS) {
        s_scale[tid - 64] = a.scale.v[tid - 64];
        s_sigma2[tid - 64] = a.sigma2.v[tid - 64];
    }
    __syncthreads();
    if (j >= cnt) return;
    const int64_t e = (int64_t)p * cap + j;
    const int idx1 = a.pairs[e * 2], idx2 = a.pairs[e * 2 + 1];
    orbfe_newpt_key k1, k2;
    float x[3] = {0.f, 0.f, 0.f};
    int verdict = ORBFE_NEWPT_IGNORED;
    const bool ok1 = np_key(a, f1, idx1, k1), ok2 = np_key(a, f2, idx2, k2);
    if (ok1 && ok2)
        verdict = np_triangulate_match(s_T, s_O, s_T + 12, s_O + 3, a.G.cam, a.G.mb, k1, k2, s_scale, s_sigma2, a.G.scale_factor,
                                       LdsLane<float, NP_T>{s_At + tid}, LdsLane<double, NP_T>{s_W + tid}, LdsLane<float, NP_T>{s_Vt + tid}, x);
    a.O.d_verdict[e] = (uint8_t)verdict;
    a.xyz_all[e * 3] = x[0];
    a.xyz_all[e * 3 + 1] = x[1];
    a.xyz_all[e * 3 + 2] = x[2];
}

__global__ __launch_bounds__(NP_T) void k_np_compact(NpArgs a)
{
    __shared__ int s_wave[NP_T / 64];
    const int p = blockIdx.x, tid = threadIdx.x, cap = a.K.cap;
    const int cnt = np_count(a, p);
    int base = 0;
    for (int j0 = 0; j0 < cnt; j0 += NP_T) {   // workgroup-uniform trip count
        const int j = j0 + tid;
        const int64_t e = (int64_t)p * cap + j;
        const bool ok = j < cnt && a.O.d_verdict[e] == ORBFE_NEWPT_OK;
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok) {
            const int64_t o = (int64_t)p * cap + pos;
            a.O.d_new_idx[o * 2] = a.pairs[e * 2];
            a.O.d_new_idx[o * 2 + 1] = a.pairs[e * 2 + 1];
            a.O.d_new_xyz[o * 3] = a.xyz_all[e * 3];
            a.O.d_new_xyz[o * 3 + 1] = a.xyz_all[e * 3 + 1];
            a.O.d_new_xyz[o * 3 + 2] = a.xyz_all[e * 3 + 2];
        }
        base += tot;
    }
    if (tid == 0) a.O.d_nnew[p] = base;
}

// ---------------------------------------------------------------------------------------------------
// KeyFrame::ComputeSceneMedianDepth.  sort() + vDepths[(size - 1) / q] = the element of that rank; the rank is found most significant
// byte first: a 256-bin histogram of the keys that share the prefix found so far, the bin that holds the rank, four times.  Counts
// are LDS atomics (a count does not depend on their order).  Chosen over a bitonic sort of the LDS array: four passes over the
// keys instead of 91 compare-exchange steps at cap = 8192, and no padding to a power of two.
// ---------------------------------------------------------------------------------------------------
struct NpMedianArgs {
    const float *Tcw, *xyz;
    const uint8_t *has_mp;
    const int32_t *n;
    const int32_t *frames;   // NULL: workgroup b takes keyframe b; else keyframe frames[b]
    int32_t nframes, cap, q;
    float *median;
};
__device__ __forceinline__ uint32_t np_order_key(float z)
{
    const uint32_t u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float np_order_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k); }

__global__ __launch_bounds__(NP_T) void k_np_median(NpMedianArgs a)
{
    __shared__ uint32_t s_key[NP_MAX_CAP];
    __shared__ int s_hist[256], s_wave[NP_T / 64];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rank;
    const int tid = threadIdx.x, cap = a.cap;
    const int f = a.frames ? a.frames[blockIdx.x] : (int)blockIdx.x;
    if (f < 0 || f >= a.nframes) return;   // workgroup-uniform
    const int n = min(max(a.n[f], 0), cap);
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = a.Tcw[(int64_t)f * 12 + k];
    int count = 0;
    for (int i0 = 0; i0 < n; i0 += NP_T) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        const int64_t at = (int64_t)f * cap + i;
        const bool occ = i < n && a.has_mp[at] != 0;
        float z = 0.f;
        if (occ) {
            const float x[3] = {a.xyz[at * 3], a.xyz[at * 3 + 1], a.xyz[at * 3 + 2]};
            z = np_scene_depth(T, x);
        }
        int tot;
        const int pos = count + trk_compact_pos(occ, s_wave, &tot);
        if (occ) s_key[pos] = np_order_key(z);   // pos < n <= cap
        count += tot;
    }
    if (count == 0) {   // undefined in the reference; this library's definition
        if (tid == 0) a.median[f] = -1.0f;
        return;
    }
    if (tid == 0) {
        s_prefix = 0;
        s_rank = (count - 1) / a.q;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();   // also: s_key and s_prefix are written
        const uint32_t mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8), prefix = s_prefix;
        for (int i = tid; i < count; i += NP_T) {
            const uint32_t k = s_key[i];
            if ((k & mask) == (prefix & mask)) atomicAdd(&s_hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int r = s_rank, b = 0;
            while (b < 255 && r >= s_hist[b]) r -= s_hist[b++];
            s_rank = r;
            s_prefix = prefix | ((uint32_t)b << shift);
        }
        __syncthreads();
    }
    if (tid == 0) a.median[f] = np_order_value(s_prefix);
}

// ---------------------------------------------------------------------------------------------------
// The claim of a round's pairs [p0, p0 + np): KeyFrame::AddMapPoint overwrites, so a slot two points claim holds the one created
// last = the larger id.  A maximum does not depend on the order of the atomics; the second launch finds exactly one winner per slot.
// ---------------------------------------------------------------------------------------------------
struct NpClaimArgs {
    const int32_t *kf1, *kf2;
    const int32_t *new_idx, *nnew;
    const float *new_xyz;
    int32_t p0, cap, nframes, id_base;
    const int32_t *n;
    orbfe_newpt_state S;
};
template <bool WRITE>
__global__ __launch_bounds__(NP_T) void k_np_claim(NpClaimArgs a)
{
    const int p = a.p0 + blockIdx.x, k = blockIdx.y * NP_T + threadIdx.x, cap = a.cap;
    const int f1 = a.kf1[p], f2 = a.kf2[p];
    if (f1 < 0 || f1 >= a.nframes || f2 < 0 || f2 >= a.nframes) return;
    if (k >= min(max(a.nnew[p], 0), cap)) return;
    const int64_t o = (int64_t)p * cap + k;
    const int32_t id = a.id_base + (int32_t)o;
    const int idx[2] = {a.new_idx[o * 2], a.new_idx[o * 2 + 1]}, f[2] = {f1, f2};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (idx[s] < 0 || idx[s] >= cap) continue;   // accepted matches are below d_n <= cap; keeps the write inside whatever came in
        const int64_t slot = (int64_t)f[s] * cap + idx[s];
        if (!WRITE)
            atomicMax(&a.S.d_mp_id[slot], id);
        else if (a.S.d_mp_id[slot] == id) {
            a.S.d_has_mp[slot] = 1;
            a.S.d_mp_xyz[slot * 3] = a.new_xyz[o * 3];
            a.S.d_mp_xyz[slot * 3 + 1] = a.new_xyz[o * 3 + 1];
            a.S.d_mp_xyz[slot * 3 + 2] = a.new_xyz[o * 3 + 2];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace
{
bool np_limits_ok(int64_t npairs, int64_t cap) { return npairs >= 0 && cap >= 1 && cap <= NP_MAX_CAP && npairs * cap < TRK_MAX_SLOTS; }
size_t np_xyz_bytes(int64_t npairs, int64_t cap) { return orb_align256(std::max<size_t>((size_t)npairs * (size_t)cap * 12, 4)); }
// the layout of b[7]: xyz_all, F12, epi, pair_skip, median
struct NpScratch {
    size_t xyz, f12, epi, skip, median, total;
    NpScratch(int64_t npairs, int64_t cap, int64_t nframes)
    {
        xyz = 0;
        f12 = xyz + np_xyz_bytes(npairs, cap);
        epi = f12 + orb_align256((size_t)npairs * 36 + 4);
        skip = epi + orb_align256((size_t)npairs * 8 + 4);
        median = skip + orb_align256((size_t)npairs + 4);
        total = median + orb_align256((size_t)nframes * 4 + 4);
    }
};

bool np_common_args_ok(const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *g, const float *sf, const float *s2, int32_t nlevels)
{
    return kf && g && sf && s2 && nlevels >= 1 && kf->nframes >= 0 && kf->cap >= 1;
}

void np_fill(NpArgs &a, const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *g, const float *sf, const float *s2, int32_t nlevels)
{
    memset(&a, 0, sizeof(a));
    a.K = *kf;
    a.G = *g;
    for (int k = 0; k < TRK_MAX_LEVELS; ++k) {   // a level past nlevels is never indexed
        a.scale.v[k] = k < nlevels ? sf[k] : 0.f;
        a.sigma2.v[k] = k < nlevels ? s2[k] : 0.f;
    }
    a.nlevels = nlevels;
}

// the two launches of the triangulation for the pairs [p0, p0 + np) of the arrays in `a`
void np_launch_triangulate(NpArgs a, int32_t p0, int32_t np, hipStream_t st)
{
    const int64_t cap = a.K.cap;
    a.kf1 += p0; a.kf2 += p0;
    a.pairs += (int64_t)p0 * cap * 2; a.npairs += p0;
    a.xyz_all += (int64_t)p0 * cap * 3;
    a.O.d_verdict += (int64_t)p0 * cap;
    a.O.d_new_idx += (int64_t)p0 * cap * 2;
    a.O.d_new_xyz += (int64_t)p0 * cap * 3;
    a.O.d_nnew += p0;
    hipLaunchKernelGGL(k_np_triangulate, dim3(np, (a.K.cap + NP_T - 1) / NP_T), dim3(NP_T), 0, st, a);   // pairs in x: may exceed 65535
    hipLaunchKernelGGL(k_np_compact, dim3(np), dim3(NP_T), 0, st, a);
}

bool np_geom_ok(const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *g)
{
    return kf->d_kps && kf->d_n && g->d_Tcw && g->d_Ow && (!kf->d_uright || g->d_depth);
}
bool np_out_ok(const orbfe_newpt_out *o) { return o && o->d_verdict && o->d_new_idx && o->d_new_xyz && o->d_nnew; }
}  // namespace

extern "C" int64_t orbfe_newpoints_scratch_bytes(int32_t npairs, int32_t cap, int32_t nframes)
{
    if (!np_limits_ok(npairs, cap) || nframes < 0) return -1;
    return (int64_t)NpScratch(npairs, cap, nframes).total;
}

extern "C" int32_t orbfe_triangulate_match(const float *Tcw1, const float *Ow1, const float *Tcw2, const float *Ow2, const orbfe_track_camera *cam,
                                           float mb, const orbfe_newpt_key *k1, const orbfe_newpt_key *k2, const float *scale_factors,
                                           const float *level_sigma2, int32_t nlevels, float scale_factor, float *x3D)
{
    if (!Tcw1 || !Ow1 || !Tcw2 || !Ow2 || !cam || !k1 || !k2 || !scale_factors || !level_sigma2 || !x3D || nlevels < 1 || k1->octave < 0 ||
        k1->octave >= nlevels || k2->octave < 0 || k2->octave >= nlevels) {
        orbfe_set_error("bad argument to orbfe_triangulate_match");
        return -1;
    }
    float At[16], Vt[16];
    double W[4];
    return np_triangulate_match(Tcw1, Ow1, Tcw2, Ow2, *cam, mb, *k1, *k2, scale_factors, level_sigma2, scale_factor, At, W, Vt, x3D);
}

extern "C" orbfe_status orbfe_triangulate_pairs_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *geom,
                                                             const int32_t *d_kf1, const int32_t *d_kf2, int32_t npairs,
                                                             const int32_t *d_pairs, const int32_t *d_npairs, const float *scale_factors,
                                                             const float *level_sigma2, int32_t nlevels, const orbfe_newpt_out *out,
                                                             void *stream)
{
    const char *who = "orbfe_triangulate_pairs_batch_device";
    if (!m || !np_common_args_ok(kf, geom, scale_factors, level_sigma2, nlevels) || npairs < 0 || !out ||
        (npairs > 0 && (!np_geom_ok(kf, geom) || !np_out_ok(out) || !d_kf1 || !d_kf2 || !d_pairs || !d_npairs))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    if (nlevels > TRK_MAX_LEVELS) { orbfe_set_error("%s: at most %d levels", who, TRK_MAX_LEVELS); return ORBFE_ERR_SIZE; }
    if (!np_limits_ok(npairs, kf->cap)) {
        orbfe_set_error("%s: cap <= %d and npairs * cap < 2^25", who, NP_MAX_CAP);
        return ORBFE_ERR_SIZE;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[7].ensure(np_xyz_bytes(npairs, kf->cap)));
    NpArgs a;
    np_fill(a, kf, geom, scale_factors, level_sigma2, nlevels);
    a.kf1 = d_kf1; a.kf2 = d_kf2;
    a.pairs = d_pairs; a.npairs = d_npairs;
    a.xyz_all = m->b[7].as<float>();
    a.O = *out;
    np_launch_triangulate(a, 0, npairs, st);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_scene_median_depth_batch_device(orbfe_matcher *m, const float *d_Tcw, const uint8_t *d_has_mp,
                                                              const float *d_mp_xyz, const int32_t *d_n, int32_t nframes, int32_t cap,
                                                              int32_t q, float *d_median, void *stream)
{
    const char *who = "orbfe_scene_median_depth_batch_device";
    if (!m || nframes < 0 || cap < 1 || q < 1 || (nframes > 0 && (!d_Tcw || !d_has_mp || !d_mp_xyz || !d_n || !d_median))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    if (cap > NP_MAX_CAP) { orbfe_set_error("%s: cap <= %d", who, NP_MAX_CAP); return ORBFE_ERR_SIZE; }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    NpMedianArgs a;
    a.Tcw = d_Tcw; a.xyz = d_mp_xyz; a.has_mp = d_has_mp; a.n = d_n; a.frames = nullptr;
    a.nframes = nframes; a.cap = cap; a.q = q;
    a.median = d_median;
    hipLaunchKernelGGL(k_np_median, dim3(nframes), dim3(NP_T), 0, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_create_new_map_points_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *geom,
                                                                 const orbfe_newpt_state *state, int32_t mono, const int32_t *d_kf1,
                                                                 const int32_t *d_kf2, int32_t npairs, const int32_t *round_off,
                                                                 int32_t nrounds, const float *scale_factors, const float *level_sigma2,
                                                                 int32_t nlevels, int32_t th_low, int32_t only_stereo, int32_t check_ori,
                                                                 int32_t id_base, uint8_t *d_pair_skip, const orbfe_tri_out *tri_out,
                                                                 const orbfe_newpt_out *out, void *stream)
{
    const char *who = "orbfe_create_new_map_points_batch_device";
    if (!m || !np_common_args_ok(kf, geom, scale_factors, level_sigma2, nlevels) || !state || !tri_out || !out || npairs < 0 || nrounds < 0 ||
        !round_off || id_base < 0 ||
        (npairs > 0 && (!np_geom_ok(kf, geom) || !np_out_ok(out) || !d_kf1 || !d_kf2 || !state->d_has_mp || !state->d_mp_xyz ||
                        !state->d_mp_id || !tri_out->d_match12 || !tri_out->d_nmatches || !tri_out->d_pairs || !tri_out->d_npairs))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    if (round_off[0] != 0 || round_off[nrounds] != npairs) {
        orbfe_set_error("%s: round_off runs from 0 to npairs", who);
        return ORBFE_ERR_ARG;
    }
    int32_t widest = 0;
    for (int r = 0; r < nrounds; ++r) {
        if (round_off[r + 1] < round_off[r]) { orbfe_set_error("%s: round_off must not decrease", who); return ORBFE_ERR_ARG; }
        widest = std::max(widest, round_off[r + 1] - round_off[r]);
    }
    if (th_low < 0 || th_low > 255) { orbfe_set_error("%s: th_low must be in [0, 255]", who); return ORBFE_ERR_ARG; }   // the search's limit, before anything is enqueued
    if (nlevels > TRK_MAX_LEVELS) { orbfe_set_error("%s: at most %d levels", who, TRK_MAX_LEVELS); return ORBFE_ERR_SIZE; }
    if (!np_limits_ok(npairs, kf->cap) || (int64_t)id_base + (int64_t)npairs * kf->cap > 0x7FFFFFFF) {
        orbfe_set_error("%s: cap <= %d, npairs * cap < 2^25, ids below 2^31", who, NP_MAX_CAP);
        return ORBFE_ERR_SIZE;
    }
    if (npairs == 0) return ORBFE_OK;
    const int32_t cap = kf->cap, nframes = kf->nframes;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const NpScratch L(npairs, cap, nframes);
    ORBFE_HIP(m->b[7].ensure(L.total));
    ORBFE_HIP(m->b[6].ensure(orb_align256(std::max<size_t>((size_t)widest * (size_t)cap * 8, 4))));   // the search's: no growth between rounds
    char *base = m->b[7].as<char>();
    float *F12 = (float *)(base + L.f12), *epi = (float *)(base + L.epi), *median = (float *)(base + L.median);
    uint8_t *skip = d_pair_skip ? d_pair_skip : (uint8_t *)(base + L.skip);
    orbfe_tri_keyframes K = *kf;
    K.d_has_mp = state->d_has_mp;
    NpArgs a;
    np_fill(a, &K, geom, scale_factors, level_sigma2, nlevels);
    a.kf1 = d_kf1; a.kf2 = d_kf2;
    a.pairs = tri_out->d_pairs; a.npairs = tri_out->d_npairs;
    a.xyz_all = (float *)(base + L.xyz);
    a.O = *out;
    NpClaimArgs c;
    c.kf1 = d_kf1; c.kf2 = d_kf2;
    c.new_idx = out->d_new_idx; c.nnew = out->d_nnew; c.new_xyz = out->d_new_xyz;
    c.cap = cap; c.nframes = nframes; c.id_base = id_base;
    c.n = kf->d_n;
    c.S = *state;
    for (int r = 0; r < nrounds; ++r) {
        const int32_t p0 = round_off[r], np = round_off[r + 1] - p0;
        if (np == 0) continue;
        if (mono) {
            NpMedianArgs ma;
            ma.Tcw = geom->d_Tcw; ma.xyz = state->d_mp_xyz; ma.has_mp = state->d_has_mp; ma.n = kf->d_n; ma.frames = d_kf2 + p0;
            ma.nframes = nframes; ma.cap = cap; ma.q = 2;
            ma.median = median;
            hipLaunchKernelGGL(k_np_median, dim3(np), dim3(NP_T), 0, st, ma);
        }
        orbfe_status s = orbfe_triangulation_pairs_batch_device(m, geom->d_Tcw, geom->d_Ow, nframes, &geom->cam, geom->mb, mono, median, d_kf1 + p0,
                                                                d_kf2 + p0, np, F12 + (int64_t)p0 * 9, epi + (int64_t)p0 * 2, skip + p0, st);
        if (s != ORBFE_OK) return s;
        orbfe_tri_out to = *tri_out;
        to.d_match12 += (int64_t)p0 * cap; to.d_nmatches += p0;
        to.d_pairs += (int64_t)p0 * cap * 2; to.d_npairs += p0;
        s = orbfe_search_for_triangulation_batch_device(m, &K, d_kf1 + p0, d_kf2 + p0, np, F12 + (int64_t)p0 * 9, epi + (int64_t)p0 * 2, skip + p0,
                                                        scale_factors, level_sigma2, nlevels, th_low, only_stereo, check_ori, &to, st);
        if (s != ORBFE_OK) return s;
        np_launch_triangulate(a, p0, np, st);
        c.p0 = p0;
        const dim3 grid(np, (cap + NP_T - 1) / NP_T);
        hipLaunchKernelGGL(k_np_claim<false>, grid, dim3(NP_T), 0, st, c);
        hipLaunchKernelGGL(k_np_claim<true>, grid, dim3(NP_T), 0, st, c);
    }
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" int32_t orbfe_newpoints_plan_rounds(const int32_t *kf1, const int32_t *kf2, int32_t npairs, int32_t *round_of, int32_t *order,
                                               int32_t *round_off)
{
    if (npairs < 0 || !round_off || (npairs > 0 && (!kf1 || !kf2 || !round_of || !order))) {
        orbfe_set_error("bad argument to orbfe_newpoints_plan_rounds");
        return -1;
    }
    return np_plan_rounds(kf1, kf2, npairs, round_of, order, round_off);
}
