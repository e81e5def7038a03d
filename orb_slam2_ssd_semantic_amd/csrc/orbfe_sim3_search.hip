// orbfe_sim3_search.hip -- the two ORBmatcher members of LoopClosing::ComputeSim3 that had no device form, for a batch of loop
// candidates, device-resident (include/orbfe.h "SearchBySim3 and the loop's SearchByProjection, batched"):
//   orbfe_sim3_pair_pose (host), orbfe_sim3_pair_poses_device      (sR12 | t12), (sR21 | t21) of every candidate: trk_sim3_pair_pose
//   orbfe_sim3_gate_points (host)                                  trk_gate_sim3 for n points of one direction
//   orbfe_search_by_sim3_batch_device     k_s3_gate (one thread per slot, live queries compacted in slot order) ->
//                                         k_s3_search (one wave per live query) -> k_s3_agree (one workgroup per pair)
//   orbfe_mark_list_members_device        k_s3_members: an open-addressing set of a row in LDS, one workgroup per pair
//   orbfe_search_by_projection_sim3_batch_device   members -> k_ps3_slots + k_ps3_gate (trk_gate_fuse, list order) -> the batch
//                                         core of orbfe_search_by_projection_batch_device, unchanged -> k_ps3_replay
//   orbfe_sim3_search_scratch_bytes (host)
//   orbfe_sim3_invert_matches_device, orbfe_sim3_correspondences_device, orbfe_sim3_keep_inliers_device   the glue between the
//                                         batched SearchByBoW, the batched Sim3 solver and SearchBySim3 (k_s3_invert, k_s3_corr, k_s3_keep)
// A SearchBySim3 query's bestIdx depends on the point, the poses and the other keyframe's features only, so its search is
// k_fuse_search's: one wave finds the first minimum in GetFeaturesInArea order.  The loop's SearchByProjection has claims
// (vpMatched[idx] is written inside the loop), so its search is the relaxation core.  Everything is enqueued on the caller's
// stream; no call waits for the device, none writes host memory.
#include <stddef.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"
#include "orbfe_track_dev.h"
#include "orbfe_track_geom.h"

static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float) && offsetof(orbfe_keypoint, octave) == 20, "keypoint record = 7 floats, octave sixth");

#define S3_ST 256                // threads of the search workgroup: four waves, one live query each per turn
#define S3_SG 128                // search workgroups per (pair, direction) at most: the waves stride over the live queries
#define S3_MT 1024               // threads of the member workgroup (one pair)

struct S3Args {
    orbfe_track_frames F;
    int32_t nkf;
    TrkCam cam;
    float th, log_sf;
    int32_t nlevels, th_high;
    TrkLevels sf;
    orbfe_track_map map;
    const float *Tcw;
    const int32_t *slot_mp;
    const int32_t *kf1, *kf2;
    const float *T12, *T21;
    const uint8_t *pair_skip;
    int32_t npairs;
    int32_t *match12, *nfound, *out1, *out2;
    // scratch, [npairs][2][cap] each but nq [npairs][2]: direction 0 = keyframe 1's points searched in keyframe 2
    orbfe_proj_query *q;
    int32_t *qslot, *qmp, *nq, *vn;
};

__device__ __forceinline__ bool s3_pair_ok(const S3Args &a, int p, int &k1, int &k2)
{
    k1 = a.kf1[p];
    k2 = a.kf2[p];
    return k1 >= 0 && k1 < a.nkf && k2 >= 0 && k2 < a.nkf && !(a.pair_skip && a.pair_skip[p]);
}

__device__ __forceinline__ int s3_count(const S3Args &a, int kf) { return min(max(a.F.d_n[kf], 0), a.F.cap); }

// the walk's view of keyframe row kf (0 <= kf < nkf): no blocked slots, no right-image gate, no chi2 gate
__device__ __forceinline__ ProjArgs s3_frame_args(const S3Args &b, int kf)
{
    ProjArgs a = proj_frame_view(b.F, kf);
    a.nlevels = b.nlevels;
    a.th = b.th_high; a.ratio_rule = 0; a.nnratio = 0.f;
    return a;
}

// ---------------------------------------------------------------------------------------------------
// 0. the poses: one thread per candidate
// ---------------------------------------------------------------------------------------------------
struct S3PoseArgs {
    const char *base;
    int64_t stride;
    int32_t off_s, off_R, off_t, off_found;
    int32_t npairs;
    float *T12, *T21;
    uint8_t *skip;
};

__global__ __launch_bounds__(TRK_GT) void k_s3_poses(S3PoseArgs a)
{
    const int p = blockIdx.x * TRK_GT + threadIdx.x;
    if (p >= a.npairs) return;
    const char *rec = a.base + (int64_t)p * a.stride;
    const bool found = a.off_found < 0 || *(const int32_t *)(rec + a.off_found) != 0;
    float T12[12], T21[12];
    if (found) {
        float R[9], t[3];
        for (int k = 0; k < 9; ++k) R[k] = ((const float *)(rec + a.off_R))[k];
        for (int k = 0; k < 3; ++k) t[k] = ((const float *)(rec + a.off_t))[k];
        trk_sim3_pair_pose(*(const float *)(rec + a.off_s), R, t, T12, T21);
    } else {
        for (int k = 0; k < 12; ++k) T12[k] = T21[k] = 0.f;
    }
    for (int k = 0; k < 12; ++k) {
        a.T12[(int64_t)p * 12 + k] = T12[k];
        a.T21[(int64_t)p * 12 + k] = T21[k];
    }
    if (a.skip) a.skip[p] = found ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------
// 1. SearchBySim3, the gate: workgroup (direction, pair), one thread per slot of the own keyframe.  vbAlreadyMatched2 is a bit
// table in LDS built from the pair's row of vpMatches12; the live queries leave compacted in slot order (trk_compact_pos: no
// atomic takes a place), so the search spends no wave on a slot that is NULL, bad, already matched or gated out.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_GT) void k_s3_gate(S3Args a)
{
    __shared__ int s_wave[TRK_GT / 64];
    __shared__ uint32_t s_matched[(PJ_MAX_NF + 31) / 32];
    __shared__ float s_own[12], s_to[12];
    const int d = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, cap = a.F.cap;
    const int64_t pd = (int64_t)p * 2 + d, base_q = pd * cap;
    for (int k = tid; k < cap; k += TRK_GT) a.vn[base_q + k] = -1;
    int k1, k2;
    if (!s3_pair_ok(a, p, k1, k2)) {   // workgroup-uniform
        if (tid == 0) a.nq[pd] = 0;
        return;
    }
    const int own = d ? k2 : k1;
    const int n1 = s3_count(a, k1), n2 = s3_count(a, k2), n_own = d ? n2 : n1;
    if (tid < 12) {
        s_own[tid] = a.Tcw[(int64_t)own * 12 + tid];
        s_to[tid] = (d ? a.T12 : a.T21)[(int64_t)p * 12 + tid];
    }
    const int32_t *row = a.match12 + (int64_t)p * cap;
    if (d) {
        for (int k = tid; k < (cap + 31) / 32; k += TRK_GT) s_matched[k] = 0;
        __syncthreads();
        for (int i = tid; i < n1; i += TRK_GT) {   // :1371-1381
            const int j = row[i];
            if (j >= 0 && j < n2) atomicOr(&s_matched[j >> 5], 1u << (j & 31));
        }
    }
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < n_own; c0 += TRK_GT) {   // workgroup-uniform trip count
        const int i = c0 + tid;
        bool ok = false;
        orbfe_proj_query Q;
        int mp = -1;
        if (i < n_own) {
            mp = a.slot_mp[(int64_t)own * cap + i];
            const bool already = d ? ((s_matched[i >> 5] >> (i & 31)) & 1u) != 0 : row[i] != -1;
            if (mp >= 0 && mp < a.map.npoints && !already && !a.map.d_bad[mp]) {
                int32_t lv;
                ok = trk_gate_sim3(s_own, s_to, a.cam, a.map.d_world_pos + (int64_t)mp * 3, a.map.d_min_dist[mp], a.map.d_max_dist[mp], a.th,
                                   a.sf.v, a.log_sf, a.nlevels, &Q, &lv);
            }
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok) {   // pos < n_own <= cap
            a.q[base_q + pos] = Q;
            a.qslot[base_q + pos] = i;
            a.qmp[base_q + pos] = mp;
        }
        base += tot;
    }
    if (tid == 0) a.nq[pd] = base;
}

// ---------------------------------------------------------------------------------------------------
// 2. SearchBySim3, the search: the waves of (pair, direction) stride over its live queries.  As in k_fuse_search lane `sub` walks
// its contiguous share of the window's cell sequence and keeps its first minimum (strict <); the wave takes the minimum of
// (distance, lane): the first candidate in GetFeaturesInArea order with the smallest distance, accepted iff <= th_high.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(S3_ST) void k_s3_search(S3Args a)
{
    const int pd = blockIdx.y, p = pd >> 1, d = pd & 1, sub = threadIdx.x & 63, cap = a.F.cap;
    const int nq = min(a.nq[pd], cap);
    if (nq <= 0) return;   // also every pair the gate refused: their keyframe rows are not read
    const int other = d ? a.kf1[p] : a.kf2[p];
    const ProjArgs pa = s3_frame_args(a, other);
    const int64_t base_q = (int64_t)pd * cap;
    for (int qi = blockIdx.x * (S3_ST / 64) + (threadIdx.x >> 6); qi < nq; qi += gridDim.x * (S3_ST / 64)) {   // wave-uniform
        const orbfe_proj_query Q = a.q[base_q + qi];
        const int slot = a.qslot[base_q + qi], mp = a.qmp[base_q + qi];
        int best = 256, bestIdx = -1;
        ProjRect R;
        if (proj_rect(pa, Q, R)) {
            const Desc8 dq = load_desc8(a.map.d_desc + (int64_t)mp * 32);
            proj_walk(pa, Q, R, sub, [&](uint32_t k) {
                if (k >= (uint32_t)pa.nF) return;
                const int dist = (int)proj_dist(pa, dq, k, false);
                if (dist < best) {
                    best = dist;
                    bestIdx = (int)k;
                }
            });
        }
        uint32_t key = ((uint32_t)best << 6) | (uint32_t)sub;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 64));
        const int winner = (int)(key & 63u), bd = (int)(key >> 6);
        const int bi = __shfl(bestIdx, winner, 64);
        if (sub == 0 && slot >= 0 && slot < cap) a.vn[base_q + slot] = bd <= a.th_high ? bi : -1;
    }
}

// ---------------------------------------------------------------------------------------------------
// 3. SearchBySim3, the agreement pass (:1542-1555): one workgroup per pair
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_GT) void k_s3_agree(S3Args a)
{
    __shared__ int s_cnt;
    const int p = blockIdx.x, tid = threadIdx.x, cap = a.F.cap;
    const int32_t *vn1 = a.vn + (int64_t)p * 2 * cap, *vn2 = vn1 + cap;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int k1, k2, cnt = 0;
    if (s3_pair_ok(a, p, k1, k2)) {
        const int n1 = s3_count(a, k1), n2 = s3_count(a, k2);
        for (int i1 = tid; i1 < n1; i1 += TRK_GT) {
            const int idx2 = vn1[i1];
            if (idx2 >= 0 && idx2 < n2 && vn2[idx2] == i1) {
                a.match12[(int64_t)p * cap + i1] = idx2;
                ++cnt;
            }
        }
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) a.nfound[p] = s_cnt;
    for (int k = tid; k < cap; k += TRK_GT) {
        if (a.out1) a.out1[(int64_t)p * cap + k] = vn1[k];
        if (a.out2) a.out2[(int64_t)p * cap + k] = vn2[k];
    }
}

// ---------------------------------------------------------------------------------------------------
// 4. list membership: d_list_skip[e] = the point of list entry e stands in row pair_row[p] (spAlreadyFound.count(pMP) with the row
// = vpMatched; IsInKeyFrame(pKF) with the row = the keyframe's slot table).  One workgroup per pair: the row's non-negative
// values go into an open-addressing set in LDS (linear probing; 2 * cap <= table size, so a probe always meets an empty place),
// then every entry is looked up.  Which place a value takes depends on the order of the atomics, whether it is a member does not.
// ---------------------------------------------------------------------------------------------------
struct S3MemberArgs {
    const int32_t *rows;
    int32_t nrows, cap;
    const int32_t *pair_row;
    const uint32_t *list_off;
    const int32_t *list_idx;
    uint32_t nentries;
    uint8_t *skip;
    int32_t shift;               // 32 - log2(table size)
};

__global__ __launch_bounds__(S3_MT) void k_s3_members(S3MemberArgs a)
{
    extern __shared__ int32_t s_set[];   // [1 << (32 - shift)]
    const int p = blockIdx.x, tid = threadIdx.x;
    const uint32_t H = 1u << (32 - a.shift), mask = H - 1u;
    const uint32_t e1 = min(a.list_off[p + 1], a.nentries), e0 = min(a.list_off[p], e1);
    const int row = a.pair_row ? a.pair_row[p] : p;
    if (row < 0 || row >= a.nrows) {   // workgroup-uniform
        for (uint32_t e = e0 + tid; e < e1; e += S3_MT) a.skip[e] = 0;
        return;
    }
    for (uint32_t k = tid; k < H; k += S3_MT) s_set[k] = -1;
    __syncthreads();
    for (int k = tid; k < a.cap; k += S3_MT) {
        const int v = a.rows[(int64_t)row * a.cap + k];
        if (v < 0) continue;
        uint32_t h = ((uint32_t)v * 2654435761u) >> a.shift;
        for (;;) {
            const int old = atomicCAS(&s_set[h], -1, v);
            if (old == -1 || old == v) break;
            h = (h + 1u) & mask;
        }
    }
    __syncthreads();
    for (uint32_t e = e0 + tid; e < e1; e += S3_MT) {
        const int v = a.list_idx[e];
        bool found = false;
        if (v >= 0) {
            uint32_t h = ((uint32_t)v * 2654435761u) >> a.shift;
            for (;;) {
                const int cur = s_set[h];
                if (cur == v) { found = true; break; }
                if (cur == -1) break;
                h = (h + 1u) & mask;
            }
        }
        a.skip[e] = found ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------
// 5. SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): slot states, gate, replay around the batch core
// ---------------------------------------------------------------------------------------------------
struct PS3Args {
    int32_t npairs, cap, qcap;
    const float *Tcw, *Ow;
    TrkCam cam;
    float th, log_sf;
    int32_t nlevels;
    TrkLevels sf;
    orbfe_track_map map;
    const uint32_t *list_off;
    const int32_t *list_idx;
    const uint8_t *list_skip;
    uint32_t nentries;
    int32_t *matched, *nmatches;
    uint8_t *slot;               // [npairs][cap] 2 = vpMatched[idx] != NULL at entry (the core skips the slot), else 0
    orbfe_proj_query *q;
    int32_t *qsrc, *nq;
    const int32_t *match;
};

__global__ __launch_bounds__(TRK_GT) void k_ps3_slots(PS3Args a)
{
    const int64_t j = (int64_t)blockIdx.x * TRK_GT + threadIdx.x;
    if (j < (int64_t)a.npairs * a.cap) a.slot[j] = a.matched[j] != -1 ? 2 : 0;
}

// one workgroup per pair, one thread per list entry, queries compacted in list order (k_trk_gate_map's scheme)
__global__ __launch_bounds__(TRK_GT) void k_ps3_gate(PS3Args a)
{
    __shared__ int s_wave[TRK_GT / 64];
    __shared__ float s_T[12], s_Ow[3];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid < 12) s_T[tid] = a.Tcw[(int64_t)p * 12 + tid];
    if (tid < 3) s_Ow[tid] = a.Ow[(int64_t)p * 3 + tid];
    __syncthreads();
    const uint32_t e1 = min(a.list_off[p + 1], a.nentries), e0 = min(a.list_off[p], e1);
    int base = 0;
    for (uint32_t c0 = e0; c0 < e1; c0 += TRK_GT) {   // workgroup-uniform trip count
        const uint32_t e = c0 + tid;
        bool ok = false;
        orbfe_proj_query Q;
        int idx = -1;
        if (e < e1) {
            idx = a.list_idx[e];
            if (idx >= 0 && idx < a.map.npoints && !a.list_skip[e] && !a.map.d_bad[idx]) {
                int32_t lv;
                ok = trk_gate_fuse(s_T, s_Ow, a.cam, a.map.d_world_pos + (int64_t)idx * 3, a.map.d_normal + (int64_t)idx * 3, a.map.d_min_dist[idx],
                                   a.map.d_max_dist[idx], a.th, a.sf.v, a.log_sf, a.nlevels, 0, &Q, &lv);
                if (ok) Q.flags = ORBFE_PROJ_CLAIMS;   // vpMatched[bestIdx] = pMP: every later scan skips the slot (:472)
            }
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok && pos < a.qcap) {
            a.q[(int64_t)p * a.qcap + pos] = Q;
            a.qsrc[(int64_t)p * a.qcap + pos] = idx;
        }
        base += tot;
    }
    if (tid == 0) a.nq[p] = min(base, a.qcap);
}

// :490-494.  The claims leave every slot with at most one query, so the writes do not meet.
__global__ __launch_bounds__(TRK_GT) void k_ps3_replay(PS3Args a)
{
    __shared__ int s_cnt;
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int nq = min(max(a.nq[p], 0), a.qcap);
    int cnt = 0;
    for (int i = tid; i < nq; i += TRK_GT) {
        const int f = a.match[(int64_t)p * a.qcap + i];
        if (f >= 0 && f < a.cap) {
            a.matched[(int64_t)p * a.cap + f] = a.qsrc[(int64_t)p * a.qcap + i];
            ++cnt;
        }
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) a.nmatches[p] = s_cnt;
}

// ---------------------------------------------------------------------------------------------------
// 6. the glue of a ComputeSim3 round: SearchByBoW's result inverted to vpMatches12, Sim3Solver's constructor (src/Sim3Solver.cc:
// 43-115) as a CSR over the pairs, and iterate's vbInliers applied to vpMatches12 (src/LoopClosing.cc:410-416)
// ---------------------------------------------------------------------------------------------------
struct S3GlueArgs {
    orbfe_track_frames F;
    int32_t nkf, npairs, corr_cap, nlevels;
    TrkLevels sigma2;
    orbfe_track_map map;
    const float *Tcw;
    const int32_t *slot_mp, *kf1, *kf2;
    const int32_t *bow_match;    // [npairs][cap]: keyframe-1 feature assigned to keyframe-2 feature i, -1 none
    const uint8_t *key_mask;     // [npairs][cap]
    int32_t *match12;            // [npairs][cap]
    uint32_t *cnt, *off;         // [npairs], [npairs + 1]
    float *X1, *X2, *s1, *s2;
    int32_t *idx1;
};

__global__ __launch_bounds__(TRK_GT) void k_s3_invert(S3GlueArgs a)
{
    const int p = blockIdx.x, tid = threadIdx.x, cap = a.F.cap;
    int32_t *row = a.match12 + (int64_t)p * cap;
    for (int k = tid; k < cap; k += TRK_GT) row[k] = -1;
    __syncthreads();
    const int k2 = a.kf2[p];
    if (k2 < 0 || k2 >= a.nkf) return;   // workgroup-uniform
    const int n2 = min(max(a.F.d_n[k2], 0), cap);
    for (int i = tid; i < n2; i += TRK_GT) {
        const int j = a.bow_match[(int64_t)p * cap + i];
        if (j >= 0 && j < cap) atomicMax(&row[j], i);   // SearchByBoW assigns a keyframe-1 feature once: the max is that one
    }
}

// one workgroup per pair; WRITE = false counts the correspondences, true writes them behind off[p] in i1 order
template <bool WRITE>
__global__ __launch_bounds__(TRK_GT) void k_s3_corr(S3GlueArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    const int p = blockIdx.x, tid = threadIdx.x, cap = a.F.cap;
    const int k1 = a.kf1[p], k2 = a.kf2[p];
    const bool pair_ok = k1 >= 0 && k1 < a.nkf && k2 >= 0 && k2 < a.nkf;
    const int n1 = pair_ok ? min(max(a.F.d_n[k1], 0), cap) : 0, n2 = pair_ok ? min(max(a.F.d_n[k2], 0), cap) : 0;
    const int32_t *oct = (const int32_t *)a.F.d_kps + 5;
    int base = 0;
    for (int c0 = 0; c0 < n1; c0 += TRK_GT) {   // workgroup-uniform trip count
        const int i1 = c0 + tid;
        bool ok = false;
        int j = -1, mp1 = -1, mp2 = -1, o1 = 0, o2 = 0;
        if (i1 < n1) {
            j = a.match12[(int64_t)p * cap + i1];
            if (j >= 0 && j < n2) {
                mp1 = a.slot_mp[(int64_t)k1 * cap + i1];
                mp2 = a.slot_mp[(int64_t)k2 * cap + j];
                o1 = oct[((int64_t)k1 * cap + i1) * 7];
                o2 = oct[((int64_t)k2 * cap + j) * 7];
                ok = mp1 >= 0 && mp1 < a.map.npoints && mp2 >= 0 && mp2 < a.map.npoints && o1 >= 0 && o1 < a.nlevels && o2 >= 0 && o2 < a.nlevels;
                if (ok) ok = !a.map.d_bad[mp1] && !a.map.d_bad[mp2];
            }
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (WRITE && ok) {
            const int64_t at = (int64_t)a.off[p] + pos;
            if (at < a.corr_cap) {
                trk_to_camera(a.Tcw + (int64_t)k1 * 12, a.map.d_world_pos + (int64_t)mp1 * 3, a.X1 + at * 3);   // k_sim3_prepare's arithmetic
                trk_to_camera(a.Tcw + (int64_t)k2 * 12, a.map.d_world_pos + (int64_t)mp2 * 3, a.X2 + at * 3);
                a.s1[at] = a.sigma2.v[o1];
                a.s2[at] = a.sigma2.v[o2];
                a.idx1[at] = i1;
            }
        }
        base += tot;
    }
    if (!WRITE && tid == 0) a.cnt[p] = (uint32_t)base;
}

__global__ __launch_bounds__(TRK_GT) void k_s3_keep(S3GlueArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * TRK_GT + threadIdx.x;
    if (j < (int64_t)a.npairs * a.F.cap && !a.key_mask[j]) a.match12[j] = -1;
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace
{
// table size of the member set for `cap` row entries: a power of two >= 2 * cap, at least 64
int member_log2(int32_t cap)
{
    int lg = 6;
    while (((int64_t)1 << lg) < 2 * (int64_t)cap) ++lg;
    return lg;
}

orbfe_status members_launch(const int32_t *d_rows, int32_t nrows, int32_t cap, const int32_t *d_pair_row, const uint32_t *d_list_off,
                            const int32_t *d_list_idx, uint32_t nentries, int32_t npairs, uint8_t *d_list_skip, hipStream_t st)
{
    // up to 128 KB of LDS at the cap; set per call: the attribute belongs to the current device's copy of the kernel
    ORBFE_HIP(hipFuncSetAttribute((const void *)k_s3_members, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ORBFE_LDS_MAX));
    S3MemberArgs a;
    const int lg = member_log2(cap);
    a.rows = d_rows; a.nrows = nrows; a.cap = cap; a.pair_row = d_pair_row;
    a.list_off = d_list_off; a.list_idx = d_list_idx; a.nentries = nentries; a.skip = d_list_skip;
    a.shift = 32 - lg;
    hipLaunchKernelGGL(k_s3_members, dim3(npairs), dim3(S3_MT), ((size_t)1 << lg) * 4, st, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
}  // namespace

extern "C" orbfe_status orbfe_sim3_pair_pose(float s12, const float *R12, const float *t12, float *T12, float *T21)
{
    if (!R12 || !t12 || !T12 || !T21) {
        orbfe_set_error("bad argument to orbfe_sim3_pair_pose");
        return ORBFE_ERR_ARG;
    }
    trk_sim3_pair_pose(s12, R12, t12, T12, T21);
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_gate_points(const float *T_own, const float *T_to_other, const orbfe_track_camera *cam, float th,
                                               const float *scale_factors, float log_scale_factor, int32_t nlevels, int32_t n,
                                               const float *world_pos, const float *min_dist, const float *max_dist, orbfe_proj_query *q,
                                               int32_t *level, uint8_t *ok)
{
    if (!T_own || !T_to_other || !cam || !scale_factors || nlevels < 1 || n < 0 ||
        (n > 0 && (!world_pos || !min_dist || !max_dist || !q || !level || !ok))) {
        orbfe_set_error("bad argument to orbfe_sim3_gate_points");
        return ORBFE_ERR_ARG;
    }
    const TrkCam c = *cam;
    for (int i = 0; i < n; ++i) {
        orbfe_proj_query e;
        memset(&e, 0, sizeof(e));
        int32_t lv = -1;
        ok[i] = trk_gate_sim3(T_own, T_to_other, c, world_pos + 3 * (size_t)i, min_dist[i], max_dist[i], th, scale_factors, log_scale_factor,
                              nlevels, &e, &lv)
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

extern "C" orbfe_status orbfe_sim3_pair_poses_device(orbfe_matcher *m, const void *d_src, int64_t stride, int32_t off_s, int32_t off_R,
                                                     int32_t off_t, int32_t off_found, int32_t npairs, float *d_T12, float *d_T21,
                                                     uint8_t *d_pair_skip, void *stream)
{
    if (!m || npairs < 0 || stride < 0 || (stride & 3) || off_s < 0 || off_R < 0 || off_t < 0 || ((off_s | off_R | off_t) & 3) ||
        (off_found >= 0 && (off_found & 3)) || (npairs > 0 && (!d_src || !d_T12 || !d_T21)) || ((uintptr_t)d_src & 3)) {
        orbfe_set_error("bad argument to orbfe_sim3_pair_poses_device (stride and offsets in bytes, multiples of 4)");
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    S3PoseArgs a;
    a.base = (const char *)d_src; a.stride = stride;
    a.off_s = off_s; a.off_R = off_R; a.off_t = off_t; a.off_found = off_found < 0 ? -1 : off_found;
    a.npairs = npairs; a.T12 = d_T12; a.T21 = d_T21; a.skip = d_pair_skip;
    hipLaunchKernelGGL(k_s3_poses, dim3((npairs + TRK_GT - 1) / TRK_GT), dim3(TRK_GT), 0, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" int64_t orbfe_sim3_search_scratch_bytes(int32_t npairs, int32_t cap, int32_t qcap, int64_t nentries, int64_t ent_cap)
{
    if (npairs < 0 || cap < 1 || cap > PJ_MAX_NF || qcap < 0 || nentries < 0 || ent_cap < 0 || (int64_t)npairs * 2 * cap >= TRK_MAX_SLOTS ||
        (int64_t)npairs * qcap >= TRK_MAX_SLOTS || nentries > TRK_MAX_SLOTS || ent_cap > 0xFFFFFFFFll)
        return -1;
    if (qcap == 0) {
        // orbfe_search_by_sim3_batch_device: queries | slots | points | counts | vnMatch1 / vnMatch2
        const size_t ns = (size_t)npairs * 2 * (size_t)cap;
        return (int64_t)(orb_align256(std::max<size_t>(ns * sizeof(orbfe_proj_query), 4)) + 3 * orb_align256(std::max<size_t>(ns * 4, 4)) +
                         orb_align256(std::max<size_t>((size_t)npairs * 8, 4)));
    }
    // orbfe_search_by_projection_sim3_batch_device: queries | sources | counts | match, best, second | slot states | skip bytes,
    // and the batch core's own blocks
    const size_t nq = (size_t)npairs * (size_t)qcap;
    const int64_t core = orbfe_track_scratch_bytes(npairs, qcap, ent_cap);
    if (core < 0) return -1;
    return (int64_t)(orb_align256(std::max<size_t>(nq * sizeof(orbfe_proj_query), 4)) + 4 * orb_align256(std::max<size_t>(nq * 4, 4)) +
                     orb_align256(std::max<size_t>((size_t)npairs * 4, 4)) + orb_align256(std::max<size_t>((size_t)npairs * cap, 4)) +
                     orb_align256(std::max<size_t>((size_t)nentries, 4))) + core;
}

extern "C" orbfe_status orbfe_search_by_sim3_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const float *d_Tcw,
                                                          const int32_t *d_slot_mp, const orbfe_track_map *map,
                                                          const orbfe_track_camera *cam, const int32_t *d_kf1, const int32_t *d_kf2,
                                                          const float *d_T12, const float *d_T21, const uint8_t *d_pair_skip,
                                                          int32_t npairs, float th, int32_t th_high, const float *scale_factors,
                                                          int32_t nlevels, float log_scale_factor, int32_t *d_match12, int32_t *d_nfound,
                                                          int32_t *d_match1, int32_t *d_match2, void *stream)
{
    S3Args a;
    if (!m || !cam || !map || nkf < 0 || npairs < 0 || !trk_frames_ok(kf, nkf, 1) || !trk_levels_of(scale_factors, nlevels, &a.sf) || th_high < 0 ||
        th_high > 255 || map->npoints < 0 || (nkf > 0 && (!d_Tcw || !d_slot_mp)) ||
        (npairs > 0 && (!d_kf1 || !d_kf2 || !d_T12 || !d_T21 || !d_match12 || !d_nfound)) ||
        (map->npoints > 0 && (!map->d_world_pos || !map->d_min_dist || !map->d_max_dist || !map->d_bad || !map->d_desc))) {
        orbfe_set_error("bad argument to orbfe_search_by_sim3_batch_device (nlevels 1..%d, th_high 0..255)", TRK_MAX_LEVELS);
        return ORBFE_ERR_ARG;
    }
    if (kf->cap > PJ_MAX_NF || (int64_t)npairs * 2 * kf->cap >= TRK_MAX_SLOTS) {
        orbfe_set_error("orbfe_search_by_sim3_batch_device: cap <= %d and npairs * 2 * cap < 2^25", PJ_MAX_NF);
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    const int cap = kf->cap;
    const size_t ns = (size_t)npairs * 2 * (size_t)cap;
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[8].ensure(ns * sizeof(orbfe_proj_query)));
    ORBFE_HIP(m->b[9].ensure(ns * 4));
    ORBFE_HIP(m->b[10].ensure(ns * 4));
    ORBFE_HIP(m->b[11].ensure(ns * 4));
    ORBFE_HIP(m->b[12].ensure((size_t)npairs * 8));
    a.F = *kf;
    a.nkf = nkf;
    a.cam = *cam;
    a.th = th; a.log_sf = log_scale_factor; a.nlevels = nlevels; a.th_high = th_high;
    a.map = *map;
    a.Tcw = d_Tcw; a.slot_mp = d_slot_mp;
    a.kf1 = d_kf1; a.kf2 = d_kf2; a.T12 = d_T12; a.T21 = d_T21; a.pair_skip = d_pair_skip; a.npairs = npairs;
    a.match12 = d_match12; a.nfound = d_nfound; a.out1 = d_match1; a.out2 = d_match2;
    a.q = m->b[8].as<orbfe_proj_query>(); a.qslot = m->b[9].as<int32_t>(); a.qmp = m->b[10].as<int32_t>(); a.vn = m->b[11].as<int32_t>();
    a.nq = m->b[12].as<int32_t>();
    const unsigned sg = (unsigned)std::min((cap + S3_ST / 64 - 1) / (S3_ST / 64), S3_SG);
    hipLaunchKernelGGL(k_s3_gate, dim3(2, npairs), dim3(TRK_GT), 0, st, a);
    hipLaunchKernelGGL(k_s3_search, dim3(sg, 2 * npairs), dim3(S3_ST), 0, st, a);
    hipLaunchKernelGGL(k_s3_agree, dim3(npairs), dim3(TRK_GT), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_mark_list_members_device(orbfe_matcher *m, const int32_t *d_rows, int32_t nrows, int32_t cap,
                                                       const int32_t *d_pair_row, const uint32_t *d_list_off, const int32_t *d_list_idx,
                                                       int64_t nentries, int32_t npairs, uint8_t *d_list_skip, void *stream)
{
    if (!m || nrows < 0 || cap < 1 || npairs < 0 || nentries < 0 || (nrows > 0 && !d_rows) || (npairs > 0 && !d_list_off) ||
        (nentries > 0 && (!d_list_idx || !d_list_skip))) {
        orbfe_set_error("bad argument to orbfe_mark_list_members_device");
        return ORBFE_ERR_ARG;
    }
    if (cap > PJ_MAX_NF || nentries > TRK_MAX_SLOTS) {
        orbfe_set_error("orbfe_mark_list_members_device: cap <= %d and nentries <= 2^25", PJ_MAX_NF);
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0 || nentries == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    return members_launch(d_rows, nrows, cap, d_pair_row, d_list_off, d_list_idx, (uint32_t)nentries, npairs, d_list_skip, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_search_by_projection_sim3_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t npairs,
                                                                     const float *d_Tcw, const float *d_Ow, const orbfe_track_camera *cam,
                                                                     const orbfe_track_map *map, const uint32_t *d_list_off,
                                                                     const int32_t *d_list_idx, const uint8_t *d_list_skip, int64_t nentries,
                                                                     float th, const float *scale_factors, int32_t nlevels,
                                                                     float log_scale_factor, int32_t th_low, int32_t qcap, int64_t ent_cap,
                                                                     int32_t *d_matched, int32_t *d_nmatches, int32_t *d_status, void *stream)
{
    PS3Args a;
    if (!m || !cam || !map || npairs < 0 || nentries < 0 || qcap < 1 || ent_cap < 0 || !trk_frames_ok(kf, npairs, 1) ||
        !trk_levels_of(scale_factors, nlevels, &a.sf) || th_low < 0 || th_low > 255 || map->npoints < 0 ||
        (npairs > 0 && (!d_Tcw || !d_Ow || !d_list_off || !d_matched || !d_nmatches || !d_status)) || (nentries > 0 && !d_list_idx) ||
        (map->npoints > 0 && (!map->d_world_pos || !map->d_normal || !map->d_min_dist || !map->d_max_dist || !map->d_bad || !map->d_desc))) {
        orbfe_set_error("bad argument to orbfe_search_by_projection_sim3_batch_device (nlevels 1..%d, th_low 0..255, qcap >= 1)", TRK_MAX_LEVELS);
        return ORBFE_ERR_ARG;
    }
    if (kf->cap > PJ_MAX_NF || (int64_t)npairs * qcap >= TRK_MAX_SLOTS || nentries > TRK_MAX_SLOTS || ent_cap > 0xFFFFFFFFll) {
        orbfe_set_error("orbfe_search_by_projection_sim3_batch_device: cap <= %d, npairs * qcap < 2^25, nentries <= 2^25, ent_cap < 2^32", PJ_MAX_NF);
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    const int cap = kf->cap;
    const size_t nq = (size_t)npairs * (size_t)qcap;
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[8].ensure(nq * sizeof(orbfe_proj_query)));
    ORBFE_HIP(m->b[9].ensure(nq * 4));
    ORBFE_HIP(m->b[10].ensure(nq * 4));
    ORBFE_HIP(m->b[11].ensure(nq * 4));
    ORBFE_HIP(m->b[12].ensure((size_t)npairs * 4));
    ORBFE_HIP(m->b[13].ensure(nq * 4));
    ORBFE_HIP(m->b[14].ensure((size_t)npairs * cap));
    ORBFE_HIP(m->b[15].ensure((size_t)nentries));
    a.npairs = npairs; a.cap = cap; a.qcap = qcap;
    a.Tcw = d_Tcw; a.Ow = d_Ow;
    a.cam = *cam;
    a.th = th; a.log_sf = log_scale_factor; a.nlevels = nlevels;
    a.map = *map;
    a.list_off = d_list_off; a.list_idx = d_list_idx; a.nentries = (uint32_t)nentries;
    a.matched = d_matched; a.nmatches = d_nmatches;
    a.slot = m->b[14].as<uint8_t>();
    a.q = m->b[8].as<orbfe_proj_query>(); a.qsrc = m->b[9].as<int32_t>(); a.nq = m->b[12].as<int32_t>();
    int32_t *match = m->b[10].as<int32_t>(), *best = m->b[11].as<int32_t>(), *second = m->b[13].as<int32_t>();
    a.match = match;
    if (d_list_skip) {
        a.list_skip = d_list_skip;
    } else {
        uint8_t *skip = m->b[15].as<uint8_t>();
        a.list_skip = skip;
        if (nentries > 0) {   // spAlreadyFound (:399-400) from the rows AT ENTRY
            const orbfe_status ms = members_launch(d_matched, npairs, cap, nullptr, d_list_off, d_list_idx, (uint32_t)nentries, npairs, skip, st);
            if (ms != ORBFE_OK) return ms;
        }
    }
    hipLaunchKernelGGL(k_ps3_slots, dim3((unsigned)(((int64_t)npairs * cap + TRK_GT - 1) / TRK_GT)), dim3(TRK_GT), 0, st, a);
    hipLaunchKernelGGL(k_ps3_gate, dim3(npairs), dim3(TRK_GT), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    orbfe_track_frames F = *kf;
    F.d_slot = a.slot;
    F.d_uright = nullptr;   // the KeyFrame forms have no right-image gate
    const orbfe_status cs = orbfe_search_by_projection_batch_device(m, &F, npairs, a.q, a.qsrc, a.nq, qcap, map->d_desc, map->npoints, 0, nullptr,
                                                                    nlevels, th_low, 0.f, 0, ent_cap, match, best, second, d_status, st);
    if (cs != ORBFE_OK) return cs;
    hipLaunchKernelGGL(k_ps3_replay, dim3(npairs), dim3(TRK_GT), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_invert_matches_device(orbfe_matcher *m, const int32_t *d_bow_match, const int32_t *d_kf2, const int32_t *d_n,
                                                         int32_t nkf, int32_t cap, int32_t npairs, int32_t *d_match12, void *stream)
{
    if (!m || nkf < 0 || cap < 1 || cap > PJ_MAX_NF || npairs < 0 || (int64_t)npairs * cap >= TRK_MAX_SLOTS ||
        (npairs > 0 && (!d_bow_match || !d_kf2 || !d_n || !d_match12))) {
        orbfe_set_error("bad argument to orbfe_sim3_invert_matches_device (cap <= %d, npairs * cap < 2^25)", PJ_MAX_NF);
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    S3GlueArgs a;
    memset(&a, 0, sizeof(a));
    a.F.d_n = d_n; a.F.cap = cap;
    a.nkf = nkf; a.npairs = npairs; a.kf2 = d_kf2; a.bow_match = d_bow_match; a.match12 = d_match12;
    hipLaunchKernelGGL(k_s3_invert, dim3(npairs), dim3(TRK_GT), 0, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_correspondences_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const float *d_Tcw,
                                                          const int32_t *d_slot_mp, const orbfe_track_map *map, const int32_t *d_kf1,
                                                          const int32_t *d_kf2, int32_t npairs, const int32_t *d_match12,
                                                          const float *level_sigma2, int32_t nlevels, int32_t corr_cap, int32_t *d_offsets,
                                                          float *d_X1, float *d_X2, float *d_sigma2_1, float *d_sigma2_2, int32_t *d_idx1,
                                                          void *stream)
{
    S3GlueArgs a;
    memset(&a, 0, sizeof(a));
    if (!m || !map || nkf < 0 || npairs < 0 || corr_cap < 0 || !kf || kf->cap < 1 || kf->cap > PJ_MAX_NF || !trk_levels_of(level_sigma2, nlevels, &a.sigma2) ||
        (int64_t)npairs * kf->cap >= TRK_MAX_SLOTS || corr_cap < (int64_t)npairs * kf->cap || map->npoints < 0 || !d_offsets ||
        (npairs > 0 && (!kf->d_kps || !kf->d_n || !d_Tcw || !d_slot_mp || !d_kf1 || !d_kf2 || !d_match12)) ||
        (corr_cap > 0 && (!d_X1 || !d_X2 || !d_sigma2_1 || !d_sigma2_2 || !d_idx1)) || (map->npoints > 0 && (!map->d_world_pos || !map->d_bad))) {
        orbfe_set_error("bad argument to orbfe_sim3_correspondences_device (cap <= %d, nlevels 1..%d, npairs * cap < 2^25, corr_cap >= npairs * cap)", PJ_MAX_NF, TRK_MAX_LEVELS);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    if (npairs == 0) {
        ORBFE_HIP(hipMemsetAsync(d_offsets, 0, 4, st));
        return ORBFE_OK;
    }
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[12].ensure((size_t)npairs * 4));
    a.F = *kf;
    a.nkf = nkf; a.npairs = npairs; a.corr_cap = corr_cap; a.nlevels = nlevels;
    a.map = *map;
    a.Tcw = d_Tcw; a.slot_mp = d_slot_mp; a.kf1 = d_kf1; a.kf2 = d_kf2;
    a.match12 = (int32_t *)d_match12;   // read only here
    a.cnt = m->b[12].as<uint32_t>(); a.off = (uint32_t *)d_offsets;
    a.X1 = d_X1; a.X2 = d_X2; a.s1 = d_sigma2_1; a.s2 = d_sigma2_2; a.idx1 = d_idx1;
    hipLaunchKernelGGL(k_s3_corr<false>, dim3(npairs), dim3(TRK_GT), 0, st, a);
    orbfe_internal_launch_scan_u32((const uint32_t *)a.cnt, npairs, a.off, st);
    hipLaunchKernelGGL(k_s3_corr<true>, dim3(npairs), dim3(TRK_GT), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_keep_inliers_device(orbfe_matcher *m, const uint8_t *d_key_mask, int32_t cap, int32_t npairs,
                                                       int32_t *d_match12, void *stream)
{
    if (!m || cap < 1 || npairs < 0 || (int64_t)npairs * cap >= TRK_MAX_SLOTS || (npairs > 0 && (!d_key_mask || !d_match12))) {
        orbfe_set_error("bad argument to orbfe_sim3_keep_inliers_device (npairs * cap < 2^25)");
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    S3GlueArgs a;
    memset(&a, 0, sizeof(a));
    a.F.cap = cap; a.npairs = npairs; a.key_mask = d_key_mask; a.match12 = d_match12;
    hipLaunchKernelGGL(k_s3_keep, dim3((unsigned)(((int64_t)npairs * cap + TRK_GT - 1) / TRK_GT)), dim3(TRK_GT), 0, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
