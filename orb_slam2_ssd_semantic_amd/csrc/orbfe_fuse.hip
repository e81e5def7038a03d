// orbfe_fuse.hip -- ORBmatcher::Fuse, both overloads, for a batch of (keyframe, list of MapPoints) pairs, device-resident
// (include/orbfe.h "Fuse, batched"):
//   orbfe_fuse_search_batch_device   k_fuse_search: gate (trk_gate_fuse) + window search, one wave per list entry
//   orbfe_fuse_batch_device          the search, then k_fuse_replay: the action the reference takes on every entry
//   orbfe_fuse_candidates_device     vpFuseCandidates of LocalMapping::SearchInNeighbors from the slot state, in order
//   orbfe_fuse_gate_points (host), orbfe_fuse_scratch_bytes (host)
// The bestIdx of an entry depends on the point, the pose and the keyframe's features only -- no claims, no ratio rule, no second
// best -- so there is no candidate-entry buffer and no relaxation round: one wave finds the first minimum in GetFeaturesInArea
// order and is done.  Everything is enqueued on the caller's stream; no call waits for the device, none writes host memory.
#include <stddef.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"
#include "orbfe_track_dev.h"
#include "orbfe_track_geom.h"

static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float) && offsetof(orbfe_keypoint, octave) == 20, "keypoint record = 7 floats, octave sixth");

#define FUSE_ST 256              // threads of the search workgroup: four waves, one list entry each
#define FUSE_RT 1024             // threads of the replay workgroup (one pair)
#define FUSE_NOFIRST 0x7FFFFFFF

struct FuseArgs {
    orbfe_track_frames F;
    int32_t nkf;
    TrkCam cam;
    float th, log_sf;
    int32_t nlevels, th_low, mode;
    TrkLevels sf, inv_sigma2;
    orbfe_track_map map;
    const int32_t *nobs, *slot_mp;
    const int32_t *pair_kf;
    const float *Tcw, *Ow;
    const uint32_t *list_off;
    const int32_t *list_idx;
    const uint8_t *list_skip;
    uint32_t nentries;
    int32_t npairs;
    int32_t *match, *dist;
    uint8_t *action;
    int32_t *other, *nfused, *first;
};

// the walk's view of keyframe row kf (0 <= kf < nkf); d_slot is not read: Fuse skips no occupied slot
__device__ __forceinline__ ProjArgs fuse_frame_args(const FuseArgs &b, int kf)
{
    ProjArgs a = proj_frame_view(b.F, kf);
    if (b.F.d_uright) a.uRight = b.F.d_uright + (int64_t)kf * b.F.cap;
    a.nlevels = b.nlevels;
    a.th = b.th_low; a.ratio_rule = 0; a.nnratio = 0.f;
    return a;
}

// the last pair p with list_off[p] <= e (npairs >= 1); the caller checks that e lies inside it
__device__ __forceinline__ int fuse_pair_of(const uint32_t *off, int npairs, uint32_t e)
{
    int lo = 0, hi = npairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------
// 1. gate + search: one wave per list entry.  Every lane evaluates the gate (same inputs, same result: the branches on it are
// wave-uniform), lane `sub` walks its contiguous share of the window's cell sequence and keeps its first minimum (strict <);
// the wave takes the minimum of (distance, lane), so the winner is the first candidate in GetFeaturesInArea order with the
// smallest distance: the reference's `dist < bestDist`.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FUSE_ST) void k_fuse_search(FuseArgs a)
{
    const uint32_t e = blockIdx.x * (FUSE_ST / 64) + (threadIdx.x >> 6);
    const int sub = threadIdx.x & 63;
    if (e >= a.nentries) return;   // whole waves leave together
    const int p = fuse_pair_of(a.list_off, a.npairs, e);
    const bool in_pair = a.list_off[p] <= e && e < a.list_off[p + 1];
    const int kf = in_pair ? a.pair_kf[p] : -1;
    const int idx = a.list_idx[e];
    bool live = kf >= 0 && kf < a.nkf && idx >= 0 && idx < a.map.npoints && !(a.list_skip && a.list_skip[e]);
    if (live) live = !a.map.d_bad[idx];
    orbfe_proj_query Q;
    int32_t level;
    if (live)
        live = trk_gate_fuse(a.Tcw + (int64_t)p * 12, a.Ow + (int64_t)p * 3, a.cam, a.map.d_world_pos + (int64_t)idx * 3,
                             a.map.d_normal + (int64_t)idx * 3, a.map.d_min_dist[idx], a.map.d_max_dist[idx], a.th, a.sf.v, a.log_sf,
                             a.nlevels, a.mode == ORBFE_FUSE_PLAIN, &Q, &level);
    int best = 256, bestIdx = -1;
    if (live) {
        const ProjArgs pa = fuse_frame_args(a, kf);
        ProjRect R;
        if (proj_rect(pa, Q, R)) {
            const Desc8 dq = load_desc8(a.map.d_desc + (int64_t)idx * 32);
            proj_walk(pa, Q, R, sub, [&](uint32_t k) {
                if (k >= (uint32_t)pa.nF) return;
                const int o = pa.octF[(size_t)pa.os * k];
                if (o < 0 || o >= a.nlevels) return;   // the reference would index mvInvLevelSigma2 outside its bounds
                const bool skip = proj_gate_skip(pa, Q, k, 1, true, [&](int lv) { return a.inv_sigma2.v[lv]; });
                const int d = (int)proj_dist(pa, dq, k, skip);
                if (d < best) {   // PJ_SKIP (511) never is
                    best = d;
                    bestIdx = (int)k;
                }
            });
        }
    }
    uint32_t key = ((uint32_t)best << 6) | (uint32_t)sub;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
    const int winner = (int)(key & 63u), bd = (int)(key >> 6);
    const int bi = __shfl(bestIdx, winner, 64);
    if (sub == 0) {
        a.match[e] = bd <= a.th_low ? bi : -1;
        a.dist[e] = bd;
    }
}

// ---------------------------------------------------------------------------------------------------
// 2. replay: one workgroup per pair.  first[slot] = the smallest in-pair position among the entries that matched the slot (LDS
// atomicMin, 60 KB at the cap); the second pass gives every entry its action from the slot state AT ENTRY, which is never written.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FUSE_RT) void k_fuse_replay(FuseArgs a)
{
    extern __shared__ int32_t s_first[];   // [cap]
    __shared__ int s_nf;
    const int p = blockIdx.x, tid = threadIdx.x;
    const uint32_t e1 = min(a.list_off[p + 1], a.nentries), e0 = min(a.list_off[p], e1);
    const int kf = a.pair_kf[p];
    const bool kf_ok = kf >= 0 && kf < a.nkf;
    const int nF = kf_ok ? min(max(a.F.d_n[kf], 0), a.F.cap) : 0;
    for (int k = tid; k < a.F.cap; k += FUSE_RT) s_first[k] = FUSE_NOFIRST;
    if (tid == 0) s_nf = 0;
    __syncthreads();
    int cnt = 0;
    for (uint32_t e = e0 + tid; e < e1; e += FUSE_RT) {
        const int m = a.match[e];
        if (m >= 0 && m < nF) {
            atomicMin(&s_first[m], (int)(e - e0));
            ++cnt;
        }
    }
    if (cnt) atomicAdd(&s_nf, cnt);
    __syncthreads();
    for (uint32_t e = e0 + tid; e < e1; e += FUSE_RT) {
        const int m = a.match[e];
        int action = ORBFE_FUSE_NONE, other = -1;
        if (m >= 0 && m < nF) {
            const int i = (int)(e - e0), f = s_first[m];
            int s = a.slot_mp ? a.slot_mp[(int64_t)kf * a.F.cap + m] : -1;
            if (s < 0 || s >= a.map.npoints) s = -1;
            if (s >= 0 && a.map.d_bad[s]) {
                action = ORBFE_FUSE_COUNTED;                        // :1162 / :1303 false: only nFused++
            } else if (a.mode == ORBFE_FUSE_SIM3) {
                if (s >= 0) { action = ORBFE_FUSE_REPLACE_CANDIDATE; other = s; }
                else if (f == i) action = ORBFE_FUSE_ADD;
                else { action = ORBFE_FUSE_REPLACE_CANDIDATE; other = a.list_idx[e0 + (uint32_t)f]; }   // the point the first matcher added
            } else if (f != i) {
                action = ORBFE_FUSE_DEFERRED;
                other = f;
            } else if (s < 0) {
                action = ORBFE_FUSE_ADD;
            } else {
                const int pi = a.list_idx[e];   // in range: the search matched it
                action = a.nobs[s] > a.nobs[pi] ? ORBFE_FUSE_REPLACE_POINT : ORBFE_FUSE_REPLACE_SLOT;
                other = s;
            }
        }
        a.action[e] = (uint8_t)action;
        a.other[e] = other;
    }
    if (tid == 0) a.nfused[p] = s_nf;
    if (a.first)
        for (int k = tid; k < a.F.cap; k += FUSE_RT) a.first[(int64_t)p * a.F.cap + k] = s_first[k] == FUSE_NOFIRST ? -1 : s_first[k];
}

// ---------------------------------------------------------------------------------------------------
// 3. vpFuseCandidates (src/LocalMapping.cc:705-725): the good points of the targets' occupied slots in (target, slot) order,
// every occurrence after the first dropped (the mnFuseCandidateForKF stamp).  Position j = target * cap + slot.  mark: the
// smallest position of every point (atomicMin on a VALUE: deterministic); count + scan + write: an ordered compaction of the
// positions that are their point's first, so no atomic takes an output place.
// ---------------------------------------------------------------------------------------------------
struct FuseCandArgs {
    const int32_t *slot_mp, *n;
    int32_t nkf, cap;
    const int32_t *targets;
    int32_t ntargets, cur_kf;
    const uint8_t *bad;
    int32_t npoints;
    int32_t *first_pos;          // [npoints]
    uint8_t *in_cur;             // [npoints]
    uint32_t *cnt, *off;         // [nblocks], [nblocks + 1]
    int32_t *cand;
    uint8_t *skip;
    int32_t *ncand;
    int32_t cand_cap;
};

// the good MapPoint at slot `slot` of keyframe row kf, or -1
__device__ __forceinline__ int fuse_cand_slot(const FuseCandArgs &a, int kf, int slot)
{
    if (kf < 0 || kf >= a.nkf || slot >= min(max(a.n[kf], 0), a.cap)) return -1;
    const int p = a.slot_mp[(int64_t)kf * a.cap + slot];
    return (p >= 0 && p < a.npoints) ? p : -1;
}

__device__ __forceinline__ int fuse_cand_point(const FuseCandArgs &a, int64_t j)
{
    if (j >= (int64_t)a.ntargets * a.cap) return -1;
    const int p = fuse_cand_slot(a, a.targets[j / a.cap], (int)(j % a.cap));
    return (p >= 0 && !a.bad[p]) ? p : -1;
}

__global__ __launch_bounds__(TRK_GT) void k_fuse_cand_mark(FuseCandArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * TRK_GT + threadIdx.x, total = (int64_t)a.ntargets * a.cap;
    if (j < total) {
        const int p = fuse_cand_point(a, j);
        if (p >= 0) atomicMin(&a.first_pos[p], (int)j);
    } else if (j < total + a.cap && a.cur_kf >= 0) {   // the blocks behind the targets: MapPoint::IsInKeyFrame(current keyframe)
        const int p = fuse_cand_slot(a, a.cur_kf, (int)(j - total));
        if (p >= 0) a.in_cur[p] = 1;
    }
}

__global__ __launch_bounds__(TRK_GT) void k_fuse_cand_count(FuseCandArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    const int64_t j = (int64_t)blockIdx.x * TRK_GT + threadIdx.x;
    const int p = fuse_cand_point(a, j);
    int tot;
    trk_compact_pos(p >= 0 && a.first_pos[p] == (int)j, s_wave, &tot);
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = (uint32_t)tot;
}

__global__ __launch_bounds__(TRK_GT) void k_fuse_cand_write(FuseCandArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    const int64_t j = (int64_t)blockIdx.x * TRK_GT + threadIdx.x;
    const int p = fuse_cand_point(a, j);
    const bool ok = p >= 0 && a.first_pos[p] == (int)j;
    int tot;
    const uint32_t pos = a.off[blockIdx.x] + (uint32_t)trk_compact_pos(ok, s_wave, &tot);
    if (ok && pos < (uint32_t)a.cand_cap) {
        a.cand[pos] = p;
        if (a.skip) a.skip[pos] = a.cur_kf >= 0 ? a.in_cur[p] : 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t all = a.off[gridDim.x];
        a.ncand[0] = (int32_t)min(all, (uint32_t)a.cand_cap);
        a.ncand[1] = (int32_t)all;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace
{
// every refusal of the two batch calls, before any launch; fills `a` except the outputs
orbfe_status fuse_check(const char *who, orbfe_matcher *m, const orbfe_track_frames *F, int32_t nkf, const orbfe_fuse_lists *L,
                        const orbfe_track_camera *cam, const orbfe_track_map *map, float th, const float *scale_factors,
                        const float *inv_level_sigma2, int32_t nlevels, float log_scale_factor, int32_t th_low, int32_t mode, FuseArgs *a)
{
    if (!m || !L || !cam || !map || nkf < 0 || L->npairs < 0 || L->nentries < 0 || !trk_frames_ok(F, nkf, 0) || map->npoints < 0 ||
        !trk_levels_of(scale_factors, nlevels, &a->sf) || !trk_levels_of(inv_level_sigma2, nlevels, &a->inv_sigma2) ||
        (mode != ORBFE_FUSE_PLAIN && mode != ORBFE_FUSE_SIM3) || th_low < 0 || th_low > 255 ||
        (L->npairs > 0 && (!L->d_pair_kf || !L->d_Tcw || !L->d_Ow || !L->d_list_off)) || (L->nentries > 0 && !L->d_list_idx) ||
        (map->npoints > 0 && (!map->d_world_pos || !map->d_normal || !map->d_min_dist || !map->d_max_dist || !map->d_bad || !map->d_desc))) {
        orbfe_set_error("bad argument to %s (nlevels 1..%d, th_low 0..255, mode ORBFE_FUSE_PLAIN or ORBFE_FUSE_SIM3)", who, TRK_MAX_LEVELS);
        return ORBFE_ERR_ARG;
    }
    if (F->cap > PJ_MAX_NF) { orbfe_set_error("%s: at most %d features per keyframe", who, PJ_MAX_NF); return ORBFE_ERR_ARG; }
    if (L->nentries > TRK_MAX_SLOTS) { orbfe_set_error("%s: at most 2^25 list entries per call", who); return ORBFE_ERR_ARG; }
    a->F = *F;
    a->nkf = nkf;
    a->cam = *cam;
    a->th = th; a->log_sf = log_scale_factor;
    a->nlevels = nlevels; a->th_low = th_low; a->mode = mode;
    a->map = *map;
    a->nobs = nullptr; a->slot_mp = nullptr;
    a->pair_kf = L->d_pair_kf; a->Tcw = L->d_Tcw; a->Ow = L->d_Ow;
    a->list_off = L->d_list_off; a->list_idx = L->d_list_idx; a->list_skip = L->d_list_skip;
    a->nentries = (uint32_t)L->nentries;
    a->npairs = L->npairs;
    a->match = a->dist = a->other = a->nfused = a->first = nullptr;
    a->action = nullptr;
    return ORBFE_OK;
}

void search_launch(const FuseArgs &a, hipStream_t st)
{
    if (a.nentries == 0 || a.npairs == 0) return;
    const unsigned nb = (a.nentries + FUSE_ST / 64 - 1) / (FUSE_ST / 64);
    hipLaunchKernelGGL(k_fuse_search, dim3(nb), dim3(FUSE_ST), 0, st, a);
}
}  // namespace

extern "C" orbfe_status orbfe_fuse_gate_points(const float *Tcw, const float *Ow, const orbfe_track_camera *cam, float th,
                                               const float *scale_factors, float log_scale_factor, int32_t nlevels, int32_t mode,
                                               int32_t n, const float *world_pos, const float *normal, const float *min_dist,
                                               const float *max_dist, orbfe_proj_query *q, int32_t *level, uint8_t *ok)
{
    if (!Tcw || !Ow || !cam || !scale_factors || nlevels < 1 || n < 0 || (mode != ORBFE_FUSE_PLAIN && mode != ORBFE_FUSE_SIM3) ||
        (n > 0 && (!world_pos || !normal || !min_dist || !max_dist || !q || !level || !ok))) {
        orbfe_set_error("bad argument to orbfe_fuse_gate_points");
        return ORBFE_ERR_ARG;
    }
    const TrkCam c = *cam;
    for (int i = 0; i < n; ++i) {
        orbfe_proj_query e;
        memset(&e, 0, sizeof(e));
        int32_t lv = -1;
        ok[i] = trk_gate_fuse(Tcw, Ow, c, world_pos + 3 * (size_t)i, normal + 3 * (size_t)i, min_dist[i], max_dist[i], th, scale_factors,
                              log_scale_factor, nlevels, mode == ORBFE_FUSE_PLAIN, &e, &lv)
                    ? 1 : 0;
        if (!ok[i]) {
            memset(&e, 0, sizeof(e));
            lv = -1;
        }
        q[i] = e;
        level[i] = lv;
    }
    return ORBFE_OK;
}

extern "C" int64_t orbfe_fuse_scratch_bytes(int32_t npoints, int32_t ntargets, int32_t cap)
{
    if (npoints < 0 || ntargets < 0 || cap < 1 || cap > PJ_MAX_NF || (int64_t)ntargets * cap >= TRK_MAX_SLOTS) return -1;
    const size_t nb = (size_t)(((int64_t)ntargets * cap + TRK_GT - 1) / TRK_GT);
    // first positions | in-current flags | block counts | block offsets: what orbfe_fuse_candidates_device asks the scratch for
    return (int64_t)(orb_align256(std::max<size_t>((size_t)npoints * 4, 4)) + orb_align256(std::max<size_t>((size_t)npoints, 4)) +
                     orb_align256(std::max<size_t>(nb * 4, 4)) + orb_align256((nb + 1) * 4));
}

extern "C" orbfe_status orbfe_fuse_search_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const orbfe_fuse_lists *lists,
                                                       const orbfe_track_camera *cam, const orbfe_track_map *map, float th,
                                                       const float *scale_factors, const float *inv_level_sigma2, int32_t nlevels,
                                                       float log_scale_factor, int32_t th_low, int32_t mode, int32_t *d_match,
                                                       int32_t *d_dist, void *stream)
{
    FuseArgs a;
    const orbfe_status rs = fuse_check("orbfe_fuse_search_batch_device", m, kf, nkf, lists, cam, map, th, scale_factors, inv_level_sigma2,
                                       nlevels, log_scale_factor, th_low, mode, &a);
    if (rs != ORBFE_OK) return rs;
    if (lists->nentries > 0 && (!d_match || !d_dist)) {
        orbfe_set_error("bad argument to orbfe_fuse_search_batch_device");
        return ORBFE_ERR_ARG;
    }
    a.match = d_match; a.dist = d_dist;
    DeviceGuard g(m->device);
    search_launch(a, (hipStream_t)stream);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_fuse_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const orbfe_fuse_lists *lists,
                                                const orbfe_track_camera *cam, const orbfe_track_map *map, const int32_t *d_nobs,
                                                const int32_t *d_slot_mp, float th, const float *scale_factors,
                                                const float *inv_level_sigma2, int32_t nlevels, float log_scale_factor, int32_t th_low,
                                                int32_t mode, const orbfe_fuse_out *out, void *stream)
{
    FuseArgs a;
    const orbfe_status rs = fuse_check("orbfe_fuse_batch_device", m, kf, nkf, lists, cam, map, th, scale_factors, inv_level_sigma2, nlevels,
                                       log_scale_factor, th_low, mode, &a);
    if (rs != ORBFE_OK) return rs;
    if (!out || (lists->nentries > 0 && (!out->d_match || !out->d_dist || !out->d_action || !out->d_other)) ||
        (lists->npairs > 0 && !out->d_nfused) || (mode == ORBFE_FUSE_PLAIN && map->npoints > 0 && d_slot_mp && !d_nobs)) {
        orbfe_set_error("bad argument to orbfe_fuse_batch_device (the plain overload compares Observations(): d_nobs)");
        return ORBFE_ERR_ARG;
    }
    a.nobs = d_nobs; a.slot_mp = d_slot_mp;
    a.match = out->d_match; a.dist = out->d_dist; a.action = out->d_action; a.other = out->d_other;
    a.nfused = out->d_nfused; a.first = out->d_first;
    if (lists->npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    search_launch(a, st);
    hipLaunchKernelGGL(k_fuse_replay, dim3(lists->npairs), dim3(FUSE_RT), (size_t)std::max(kf->cap, 1) * 4, st, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_fuse_candidates_device(orbfe_matcher *m, const int32_t *d_slot_mp, const int32_t *d_n, int32_t nkf, int32_t cap,
                                                     const int32_t *d_targets, int32_t ntargets, int32_t cur_kf, const uint8_t *d_bad,
                                                     int32_t npoints, int32_t *d_cand, uint8_t *d_cand_skip, int32_t cand_cap,
                                                     int32_t *d_ncand, void *stream)
{
    if (!m || nkf < 0 || cap < 1 || ntargets < 0 || npoints < 0 || cand_cap < 0 || cur_kf >= nkf || !d_ncand ||
        (ntargets > 0 && (!d_slot_mp || !d_n || !d_targets)) || (cur_kf >= 0 && (!d_slot_mp || !d_n)) || (npoints > 0 && !d_bad) ||
        (cand_cap > 0 && !d_cand)) {
        orbfe_set_error("bad argument to orbfe_fuse_candidates_device");
        return ORBFE_ERR_ARG;
    }
    if (cap > PJ_MAX_NF || (int64_t)ntargets * cap >= TRK_MAX_SLOTS) {
        orbfe_set_error("orbfe_fuse_candidates_device: cap <= %d and ntargets * cap < 2^25", PJ_MAX_NF);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    if (ntargets == 0 || npoints == 0) {
        ORBFE_HIP(hipMemsetAsync(d_ncand, 0, 8, st));
        return ORBFE_OK;
    }
    const int64_t total = (int64_t)ntargets * cap;
    const unsigned nb = (unsigned)((total + TRK_GT - 1) / TRK_GT), nb_cur = (unsigned)((cap + TRK_GT - 1) / TRK_GT);
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[2].ensure((size_t)nb * 4));
    ORBFE_HIP(m->b[4].ensure((size_t)(nb + 1) * 4));
    ORBFE_HIP(m->b[6].ensure((size_t)npoints * 4));
    ORBFE_HIP(m->b[7].ensure((size_t)npoints));
    FuseCandArgs a;
    a.slot_mp = d_slot_mp; a.n = d_n; a.nkf = nkf; a.cap = cap;
    a.targets = d_targets; a.ntargets = ntargets; a.cur_kf = cur_kf < 0 ? -1 : cur_kf;
    a.bad = d_bad; a.npoints = npoints;
    a.first_pos = m->b[6].as<int32_t>(); a.in_cur = m->b[7].as<uint8_t>();
    a.cnt = m->b[2].as<uint32_t>(); a.off = m->b[4].as<uint32_t>();
    a.cand = d_cand; a.skip = d_cand_skip; a.ncand = d_ncand; a.cand_cap = cand_cap;
    ORBFE_HIP(hipMemsetAsync(a.first_pos, 0x7F, (size_t)npoints * 4, st));   // 0x7F7F7F7F: above every position (< 2^25)
    ORBFE_HIP(hipMemsetAsync(a.in_cur, 0, (size_t)npoints, st));
    hipLaunchKernelGGL(k_fuse_cand_mark, dim3(nb + nb_cur), dim3(TRK_GT), 0, st, a);
    hipLaunchKernelGGL(k_fuse_cand_count, dim3(nb), dim3(TRK_GT), 0, st, a);
    orbfe_internal_launch_scan_u32((const uint32_t *)a.cnt, (int)nb, a.off, st);
    hipLaunchKernelGGL(k_fuse_cand_write, dim3(nb), dim3(TRK_GT), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}
