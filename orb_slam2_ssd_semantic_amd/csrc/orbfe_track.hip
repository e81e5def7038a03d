// orbfe_track.hip -- the projection searches of the per-frame tracker, batched and device-resident (include/orbfe.h "Tracker"):
//   orbfe_unproject_select_batch_device        Frame::UnprojectStereo + Tracking::UpdateLastFrame's close-point rule
//   orbfe_gate_last_frame_batch_device         the gating of SearchByProjection(CurrentFrame, LastFrame, th, bMono)
//   orbfe_gate_local_map_batch_device          Frame::isInFrustum + MapPoint::PredictScale + the gating of SearchByProjection(F, vpMapPoints, th)
//   orbfe_search_by_projection_batch_device    count -> scan -> fill -> resolve: the search of orbfe_proj_dev.h with a frame dimension
//   orbfe_track_replay_batch_device            what the reference's loops leave in mvpMapPoints, the rotation histogram, the point pairs
//   orbfe_track_last_frame_batch_device, orbfe_track_local_map_batch_device   the chains
//   orbfe_frustum_points (host), orbfe_track_scratch_bytes (host)
// Everything is enqueued on the caller's stream; no call waits for the device, none writes host memory.  DESIGN.md 8k.
#include <stddef.h>

#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"
#include "orbfe_track_dev.h"
#include "orbfe_track_geom.h"

static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float) && offsetof(orbfe_keypoint, octave) == 20 && offsetof(orbfe_keypoint, angle) == 12,
              "keypoint record = 7 floats: (x, y) first, angle fourth, octave sixth");

#define TRK_UT 1024              // threads of the unproject / selection workgroup

// ---------------------------------------------------------------------------------------------------
// 1. Frame::UnprojectStereo (src/Frame.cc:879-899) for every keypoint with depth > 0, and the selection of
// Tracking::UpdateLastFrame (:1833-1883): the reference sorts (z, i), visits in that order and stops behind the first visited
// entry with z > th_depth && visited > 100.  With c = #{z > 0 && !(z > th_depth)} that is the first min(n_pos, max(c, 100) + 1)
// entries in (z, i) order, so a rank by counting inside the frame's workgroup decides it (depths in LDS, no global sort).
// ---------------------------------------------------------------------------------------------------
struct TrkUnprojArgs {
    const float *kps, *depth;
    const int32_t *n;
    int32_t cap;
    const float *Tcw;
    TrkCam cam;
    float invfx, invfy, th_depth;
    const uint8_t *keeps;
    float *world_pos;
    uint8_t *created;
};

__global__ __launch_bounds__(TRK_UT) void k_trk_unproject(TrkUnprojArgs a)
{
    extern __shared__ float s_z[];   // [cap]
    __shared__ int s_npos, s_close;
    __shared__ float s_T[12], s_Ow[3];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.n[f], 0), a.cap);
    const int64_t fb = (int64_t)f * a.cap;
    if (tid < 12) s_T[tid] = a.Tcw[(int64_t)f * 12 + tid];
    if (tid == 0) { s_npos = 0; s_close = 0; }
    __syncthreads();
    if (tid == 0) trk_camera_centre(s_T, s_Ow);
    int npos = 0, nclose = 0;
    for (int i = tid; i < n; i += TRK_UT) {
        const float z = a.depth[fb + i];
        s_z[i] = z;
        if (z > 0.0f) {
            ++npos;
            if (!(z > a.th_depth)) ++nclose;
        }
    }
    if (npos) atomicAdd(&s_npos, npos);
    if (nclose) atomicAdd(&s_close, nclose);
    __syncthreads();
    const int nsel = min(s_npos, max(s_close, 100) + 1);
    for (int i = tid; i < a.cap; i += TRK_UT) {
        float xw[3] = {0.f, 0.f, 0.f};
        uint8_t created = 0;
        const float z = i < n ? s_z[i] : 0.0f;
        if (z > 0.0f) {
            trk_unproject(s_T, s_Ow, a.cam, a.invfx, a.invfy, a.kps[(fb + i) * 7], a.kps[(fb + i) * 7 + 1], z, xw);
            int rank = 0;
            for (int j = 0; j < n && rank < nsel; ++j) {
                const float zj = s_z[j];
                if (zj > 0.0f && (zj < z || (zj == z && j < i))) ++rank;
            }
            created = rank < nsel && !(a.keeps && a.keeps[fb + i]);
        }
        a.world_pos[(fb + i) * 3] = xw[0];
        a.world_pos[(fb + i) * 3 + 1] = xw[1];
        a.world_pos[(fb + i) * 3 + 2] = xw[2];
        a.created[fb + i] = created;
    }
}

// ---------------------------------------------------------------------------------------------------
// 2. the gating of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1590-1644): one lane per
// last-frame feature, queries compacted in feature order
// ---------------------------------------------------------------------------------------------------
struct TrkGateLastArgs {
    const float *Tcw_cur, *Tcw_last;
    TrkCam cam;
    float mb, th;
    int32_t mono, nlevels;
    TrkLevels sf;
    const uint8_t *valid, *obs_gt0;
    const float *world_pos;
    const float *last_kps;
    const int32_t *nlast;
    int32_t cap_last, qcap;
    orbfe_proj_query *q;
    int32_t *qsrc, *nq;
};

__global__ __launch_bounds__(TRK_GT) void k_trk_gate_last(TrkGateLastArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    __shared__ float s_T[12];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid < 12) s_T[tid] = a.Tcw_cur[(int64_t)f * 12 + tid];
    __syncthreads();
    const int n = min(max(a.nlast[f], 0), a.cap_last);
    const int64_t fb = (int64_t)f * a.cap_last;
    const int motion = trk_motion(s_T, a.Tcw_last + (int64_t)f * 12, a.mb, a.mono);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += TRK_GT) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        bool ok = false;
        orbfe_proj_query Q;
        if (i < n && a.valid[fb + i]) {
            const int oct = ((const int32_t *)a.last_kps)[(fb + i) * 7 + 5];
            if (oct >= 0 && oct < a.nlevels)
                ok = trk_gate_last(s_T, a.cam, a.world_pos + (fb + i) * 3, oct, a.th, a.sf.v, motion, a.obs_gt0[fb + i], &Q);
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok && pos < a.qcap) {
            a.q[(int64_t)f * a.qcap + pos] = Q;
            a.qsrc[(int64_t)f * a.qcap + pos] = i;
        }
        base += tot;
    }
    if (tid == 0) a.nq[f] = min(base, a.qcap);
}

// ---------------------------------------------------------------------------------------------------
// 3. Frame::isInFrustum + PredictScale + the gating of SearchByProjection(F, vpMapPoints, th) over every frame's list of local
// map points (Tracking::SearchLocalPoints): one lane per list entry, queries compacted in list order
// ---------------------------------------------------------------------------------------------------
struct TrkGateMapArgs {
    const float *Tcw;
    TrkCam cam;
    float th, log_sf;
    int32_t nlevels;
    TrkLevels sf;
    orbfe_track_map map;
    const uint32_t *list_off;
    const int32_t *list_idx;
    const uint8_t *seen;
    uint32_t nentries;
    int32_t qcap;
    orbfe_proj_query *q;
    int32_t *qsrc, *nq, *visible;
    orbfe_track_proj *proj;
};

__global__ __launch_bounds__(TRK_GT) void k_trk_gate_map(TrkGateMapArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    __shared__ float s_T[12], s_Ow[3];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (tid < 12) s_T[tid] = a.Tcw[(int64_t)f * 12 + tid];
    __syncthreads();
    if (tid == 0) trk_camera_centre(s_T, s_Ow);
    __syncthreads();
    const uint32_t e1 = min(a.list_off[f + 1], a.nentries), e0 = min(a.list_off[f], e1);
    int base = 0;
    for (uint32_t c0 = e0; c0 < e1; c0 += TRK_GT) {   // workgroup-uniform trip count
        const uint32_t e = c0 + tid;
        bool ok = false;
        orbfe_proj_query Q;
        TrkProj P;
        int p = -1;
        if (e < e1) {
            p = a.list_idx[e];
            if (p >= 0 && p < a.map.npoints && !(a.seen && a.seen[e]) && !a.map.d_bad[p]) {
                ok = trk_frustum(s_T, s_Ow, a.cam, a.map.d_world_pos + (int64_t)p * 3, a.map.d_normal + (int64_t)p * 3, a.map.d_min_dist[p],
                                 a.map.d_max_dist[p], a.log_sf, a.nlevels, &P);
                if (ok) trk_query_local_map(P, a.th, a.sf.v, a.map.d_obs_gt0[p], &Q);
            }
            if (a.proj) {
                orbfe_track_proj o;
                o.u = ok ? P.u : 0.f; o.v = ok ? P.v : 0.f; o.ur = ok ? P.ur : 0.f; o.view_cos = ok ? P.view_cos : 0.f;
                o.level = ok ? P.level : -1;
                a.proj[e] = o;
            }
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok && pos < a.qcap) {
            a.q[(int64_t)f * a.qcap + pos] = Q;
            a.qsrc[(int64_t)f * a.qcap + pos] = p;
        }
        base += tot;
    }
    if (tid == 0) {
        a.nq[f] = min(base, a.qcap);
        if (a.visible) a.visible[f] = base;
    }
}

// ---------------------------------------------------------------------------------------------------
// 4. the search core with a frame dimension (TrkCoreArgs and a frame's view of it: orbfe_track_dev.h)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_trk_count(TrkCoreArgs b)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, g = t / PJ_LC;
    const int sub = (int)(t % PJ_LC);
    if (t == 0) { b.status[0] = 0; b.status[1] = 0; }
    if (g >= (int64_t)b.nframes * b.qcap) return;   // whole waves leave together
    const int f = (int)(g / b.qcap), i = (int)(g % b.qcap);
    const ProjArgs a = trk_frame_args(b, f);
    orbfe_proj_query Q;
    ProjRect R;
    int src;
    const bool any = trk_query(b, f, i, a, Q, R, src);
    proj_count(a, Q, R, any, sub, b.lcnt, b.cnt, g);
}

__global__ __launch_bounds__(256) void k_trk_fill(TrkCoreArgs b)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, g = t / PJ_LC;
    const int sub = (int)(t % PJ_LC);
    const int64_t ng = (int64_t)b.nframes * b.qcap;
    if (g >= ng || b.off[ng] > b.ent_cap) return;
    const int f = (int)(g / b.qcap), i = (int)(g % b.qcap);
    const ProjArgs a = trk_frame_args(b, f);
    orbfe_proj_query Q;
    ProjRect R;
    int src;
    if (!trk_query(b, f, i, a, Q, R, src)) return;   // wave-uniform
    const int mine = b.lcnt[g * PJ_LC + sub];
    uint32_t o = b.off[g] + (uint32_t)(wave_incl_scan_m(mine) - mine);
    const Desc8 dq = load_desc8(b.pool + ((int64_t)f * b.pool_frame_rows + src) * 32);
    // a slot blocks from state 2 on: a MapPoint with observations before the call
    proj_walk(a, Q, R, sub, [&](uint32_t k) {
        const bool skip = proj_gate_skip(a, Q, k, 2, b.has_sigma2 != 0, [&](int lv) { return b.inv_sigma2.v[lv]; });
        const uint32_t d = proj_dist(a, dq, k, skip);
        b.ent[o++] = k | (d << 16);
    });
}

// the relaxation rounds of k_proj_resolve, one workgroup per frame, the owner table (4 bytes per frame feature) in LDS; the loop
// is that kernel's, kept as a copy (orbfe_proj_dev.h says why)
__global__ __launch_bounds__(PJ_T) void k_trk_resolve(TrkCoreArgs b)
{
    extern __shared__ int32_t s_owner[];   // [cap]
    __shared__ int s_changed;
    const int f = blockIdx.x, tid = threadIdx.x, sub = tid % PJ_L, grp = tid / PJ_L;
    const int64_t ng = (int64_t)b.nframes * b.qcap, g0 = (int64_t)f * b.qcap;
    const ProjArgs a = trk_frame_args(b, f);
    const int nq = min(max(b.nq[f], 0), b.qcap), nF = a.nF;
    int32_t *match = b.match + g0, *best = b.best + g0, *second = b.second + g0;
    const uint32_t *off = b.off + g0;
    const orbfe_proj_query *q = b.q + g0;
    for (int i = tid; i < b.qcap; i += PJ_T) match[i] = -1;
    const uint32_t total = b.off[ng];
    if (total > b.ent_cap) {   // workgroup-uniform: the caller grows the entry buffer and calls again
        if (tid == 0) b.status[0] = (int32_t)total;
        return;
    }
    for (int k = tid; k < nF; k += PJ_T) s_owner[k] = 0x7FFFFFFF;
    __syncthreads();
    int round = 0;
    for (; round <= nq + 1; ++round) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool changed = false;
        for (int i0 = 0; i0 < nq; i0 += PJ_T / PJ_L) {
            const int i = i0 + grp;
            uint32_t k1 = PJ_NOKEY, k2 = PJ_NOKEY;   // the two smallest keys (dist << 16 | position) among the free slots
            uint32_t o = 0, e = 0;
            if (i < nq) { o = off[i]; e = off[i + 1]; }
            for (uint32_t k = o + sub; k < e; k += PJ_L) {
                const uint32_t en = b.ent[k];
                const uint32_t ft = en & 0xFFFFu, d = en >> 16;
                if (d == PJ_SKIP || s_owner[ft] < i) continue;   // the slot was taken by an earlier query of this call
                const uint32_t key = (d << 16) | (k - o);
                if (key < k1) { k2 = k1; k1 = key; }
                else if (key < k2) k2 = key;
            }
#pragma unroll
            for (int s = PJ_L / 2; s > 0; s >>= 1) {   // merge the lanes' pairs: the two smallest keys of the group
                const uint32_t o1 = __shfl_xor(k1, s, PJ_L), o2 = __shfl_xor(k2, s, PJ_L);
                const uint32_t lo = min(k1, o1), hi = max(k1, o1);
                k2 = min(hi, min(k2, o2));
                k1 = lo;
            }
            if (i < nq && sub == 0) {
                const int bestDist = k1 == PJ_NOKEY ? 256 : (int)(k1 >> 16), bestDist2 = k2 == PJ_NOKEY ? 256 : (int)(k2 >> 16);
                int mt = -1;
                if (bestDist <= b.th) {            // :143-148 / :1673
                    const int bestIdx = (int)(b.ent[o + (k1 & 0xFFFFu)] & 0xFFFFu);
                    bool reject = false;
                    if (b.ratio_rule) {
                        const int bestLevel = a.octF[(size_t)a.os * bestIdx];
                        const int bestLevel2 = k2 == PJ_NOKEY ? -1 : a.octF[(size_t)a.os * (b.ent[o + (k2 & 0xFFFFu)] & 0xFFFFu)];
                        reject = bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(b.nnratio, (float)bestDist2);
                    }
                    if (!reject) mt = bestIdx;
                }
                if (mt != match[i]) {
                    match[i] = mt;
                    changed = true;
                }
                best[i] = bestDist;
                second[i] = bestDist2;
            }
        }
        if (changed) s_changed = 1;
        __syncthreads();
        if (!s_changed) break;                 // workgroup-uniform
        for (int k = tid; k < nF; k += PJ_T) s_owner[k] = 0x7FFFFFFF;
        __syncthreads();
        for (int i = tid; i < nq; i += PJ_T) {
            const int mt = match[i];
            if (mt >= 0 && (q[i].flags & ORBFE_PROJ_CLAIMS)) atomicMin(&s_owner[mt], i);
        }
        __syncthreads();
    }
    if (tid == 0) atomicMax(&b.status[1], round + 1);
}

// ---------------------------------------------------------------------------------------------------
// 5. the replay (tests/proj_cases.py replay_last_frame / replay_local_map): one workgroup per frame.  A slot ends with the
// LAST query in order that matched it (LDS atomicMax over the query positions), goes back to -1 if ANY match to it lies in a
// dropped rotation bin, nmatches = matches - dropped entries, and the (source, slot) pairs leave in match order.
// ---------------------------------------------------------------------------------------------------
struct TrkReplayArgs {
    orbfe_track_frames F;
    const int32_t *match, *qsrc, *nq;
    int32_t qcap;
    const float *last_kps;   // check_ori: the query sources are keypoints of this block
    int32_t cap_last, check_ori;
    int32_t *assigned, *nmatches, *pairs, *npairs;
};

__global__ __launch_bounds__(TRK_GT) void k_trk_replay(TrkReplayArgs a)
{
    extern __shared__ int32_t s_last[];   // [cap]: the last query that matched the slot, -1 none, -2 dropped
    __shared__ int s_hist[ORBFE_HISTO_LENGTH], s_keep[3], s_wave[TRK_GT / 64], s_drop;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t fb = (int64_t)f * a.F.cap, g0 = (int64_t)f * a.qcap;
    const int nF = min(max(a.F.d_n[f], 0), a.F.cap), nq = min(max(a.nq[f], 0), a.qcap);
    const float *ang_cur = (const float *)a.F.d_kps + fb * 7 + 3;
    const float *ang_last = a.check_ori ? a.last_kps + (int64_t)f * a.cap_last * 7 + 3 : nullptr;
    for (int k = tid; k < a.F.cap; k += TRK_GT) s_last[k] = -1;
    if (tid < ORBFE_HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) s_drop = 0;
    __syncthreads();
    auto bin_of = [&](int i, int m) {
        const int src = min(max(a.qsrc[g0 + i], 0), a.cap_last - 1);
        return rot_bin_clamped(ang_last[(int64_t)src * 7], ang_cur[(int64_t)m * 7]);
    };
    int base = 0;
    for (int i0 = 0; i0 < nq; i0 += TRK_GT) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        int m = i < nq ? a.match[g0 + i] : -1;
        if (m >= nF) m = -1;
        const bool ok = m >= 0;
        if (ok) {
            atomicMax(&s_last[m], i);
            if (a.check_ori) atomicAdd(&s_hist[bin_of(i, m)], 1);
        }
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok && a.pairs) {
            a.pairs[(g0 + pos) * 2] = a.qsrc[g0 + i];
            a.pairs[(g0 + pos) * 2 + 1] = m;
        }
        base += tot;
    }
    __syncthreads();
    if (a.check_ori) {
        if (tid == 0) rot_three_maxima(s_hist, ORBFE_HISTO_LENGTH, s_keep);
        __syncthreads();
        int dropped = 0;
        for (int i = tid; i < nq; i += TRK_GT) {
            const int m = a.match[g0 + i];
            if (m < 0 || m >= nF) continue;
            if (!rot_keeps(s_keep, bin_of(i, m))) {
                s_last[m] = -2;   // every writer of this phase writes -2; nobody reads before the barrier
                ++dropped;
            }
        }
        if (dropped) atomicAdd(&s_drop, dropped);
        __syncthreads();
    }
    for (int k = tid; k < a.F.cap; k += TRK_GT) {
        const int l = k < nF ? s_last[k] : -1;
        int v = (a.F.d_slot && a.F.d_slot[fb + k] > 0) ? -2 : -1;   // -2: the MapPoint the slot held before the call
        if (l >= 0) v = a.qsrc[g0 + l];
        else if (l == -2) v = -1;
        a.assigned[fb + k] = v;
    }
    if (tid == 0) {
        a.nmatches[f] = base - s_drop;
        if (a.npairs) a.npairs[f] = base;
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// count -> scan -> fill (orbfe_track_dev.h), for the chains below and for orbfe_init_search.hip
orbfe_status orbfe_internal_track_lists_launch(orbfe_matcher *m, TrkCoreArgs &b, int64_t ent_cap, hipStream_t st)
{
    const int64_t ng = (int64_t)b.nframes * b.qcap;
    ORBFE_HIP(m->b[2].ensure((size_t)ng * 4));
    ORBFE_HIP(m->b[3].ensure((size_t)ng * PJ_LC * 2));
    ORBFE_HIP(m->b[4].ensure((size_t)(ng + 1) * 4));
    ORBFE_HIP(m->b[5].ensure((size_t)std::max<int64_t>(ent_cap, 1) * 4));
    b.cnt = m->b[2].as<uint32_t>();
    b.lcnt = m->b[3].as<uint16_t>();
    b.off = m->b[4].as<uint32_t>();
    b.ent = m->b[5].as<uint32_t>();
    b.ent_cap = (uint32_t)ent_cap;
    const unsigned ngrp = (unsigned)((ng * PJ_LC + 255) / 256);
    hipLaunchKernelGGL(k_trk_count, dim3(ngrp), dim3(256), 0, st, b);
    orbfe_internal_launch_scan_u32((const uint32_t *)b.cnt, (int)ng, b.off, st);
    hipLaunchKernelGGL(k_trk_fill, dim3(ngrp), dim3(256), 0, st, b);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

namespace
{
// the launches of the search core on `st`: the lists (orbfe_internal_track_lists_launch sizes the scratch blocks), then the rounds
orbfe_status core_launch(orbfe_matcher *m, const orbfe_track_frames *F, int32_t nframes, const orbfe_proj_query *d_q, const int32_t *d_qsrc,
                         const int32_t *d_nq, int32_t qcap, const uint8_t *d_qpool, int32_t pool_rows, int32_t pool_frame_rows,
                         const float *inv_level_sigma2, int32_t nlevels, int32_t th, float nnratio, int32_t ratio_rule,
                         int64_t ent_cap, int32_t *d_match, int32_t *d_best, int32_t *d_second, int32_t *d_status, hipStream_t st)
{
    TrkCoreArgs b;
    b.F = *F;
    b.nframes = nframes;
    b.has_sigma2 = inv_level_sigma2 ? 1 : 0;
    b.nlevels = inv_level_sigma2 ? nlevels : 1;
    for (int i = 0; i < TRK_MAX_LEVELS; ++i) b.inv_sigma2.v[i] = (inv_level_sigma2 && i < nlevels) ? inv_level_sigma2[i] : 0.f;
    b.q = d_q; b.qsrc = d_qsrc; b.nq = d_nq; b.qcap = qcap;
    b.pool = d_qpool; b.pool_rows = pool_rows; b.pool_frame_rows = pool_frame_rows;
    b.th = th; b.ratio_rule = ratio_rule ? 1 : 0; b.nnratio = nnratio;
    b.match = d_match; b.best = d_best; b.second = d_second; b.status = d_status;
    const orbfe_status ls = orbfe_internal_track_lists_launch(m, b, ent_cap, st);
    if (ls != ORBFE_OK) return ls;
    hipLaunchKernelGGL(k_trk_resolve, dim3(nframes), dim3(PJ_T), (size_t)std::max(F->cap, 1) * 4, st, b);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

orbfe_status core_check(const char *who, orbfe_matcher *m, const orbfe_track_frames *F, int32_t nframes, int32_t qcap, int32_t th,
                        int64_t ent_cap, const float *inv_level_sigma2, int32_t nlevels)
{
    if (!m || nframes < 0 || qcap < 1 || ent_cap < 0 || !trk_frames_ok(F, nframes, 0) || (inv_level_sigma2 && (nlevels < 1 || nlevels > TRK_MAX_LEVELS))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    if (F->cap > PJ_MAX_NF) { orbfe_set_error("%s: at most %d features per frame", who, PJ_MAX_NF); return ORBFE_ERR_SIZE; }
    if (th > 255) { orbfe_set_error("%s: th must be below 256 (256 is the 'no candidate' distance)", who); return ORBFE_ERR_ARG; }
    if ((int64_t)nframes * qcap >= TRK_MAX_SLOTS || ent_cap > 0xFFFFFFFFll) {
        orbfe_set_error("%s: nframes * qcap must stay below 2^25 and ent_cap below 2^32", who);
        return ORBFE_ERR_SIZE;
    }
    return ORBFE_OK;
}

void replay_launch(const orbfe_track_frames *F, int32_t nframes, const int32_t *d_match, const int32_t *d_qsrc, const int32_t *d_nq,
                   int32_t qcap, const orbfe_keypoint *d_last_kps, int32_t cap_last, int32_t check_ori, int32_t *d_assigned,
                   int32_t *d_nmatches, int32_t *d_pairs, int32_t *d_npairs, hipStream_t st)
{
    TrkReplayArgs r;
    r.F = *F;
    r.match = d_match; r.qsrc = d_qsrc; r.nq = d_nq; r.qcap = qcap;
    r.last_kps = (const float *)d_last_kps;
    r.cap_last = cap_last;
    r.check_ori = check_ori ? 1 : 0;
    r.assigned = d_assigned; r.nmatches = d_nmatches; r.pairs = d_pairs; r.npairs = d_npairs;
    hipLaunchKernelGGL(k_trk_replay, dim3(nframes), dim3(TRK_GT), (size_t)std::max(F->cap, 1) * 4, st, r);
}

orbfe_status gate_last_launch(const float *d_Tcw_cur, const orbfe_track_last *L, const orbfe_track_camera *cam, float mb, int32_t mono,
                              float th, const TrkLevels &sf, int32_t nlevels, int32_t nframes, orbfe_proj_query *d_q, int32_t *d_qsrc,
                              int32_t *d_nq, int32_t qcap, hipStream_t st)
{
    TrkGateLastArgs g;
    g.Tcw_cur = d_Tcw_cur; g.Tcw_last = L->d_Tcw;
    g.cam = *cam;
    g.mb = mb; g.th = th; g.mono = mono ? 1 : 0; g.nlevels = nlevels; g.sf = sf;
    g.valid = L->d_valid; g.obs_gt0 = L->d_obs_gt0; g.world_pos = L->d_world_pos;
    g.last_kps = (const float *)L->d_kps;
    g.nlast = L->d_n; g.cap_last = L->cap; g.qcap = qcap;
    g.q = d_q; g.qsrc = d_qsrc; g.nq = d_nq;
    hipLaunchKernelGGL(k_trk_gate_last, dim3(nframes), dim3(TRK_GT), 0, st, g);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

bool last_ok(const orbfe_track_last *L, int32_t nframes)
{
    return L && L->cap >= 1 && (nframes == 0 || (L->d_kps && L->d_n && L->d_valid && L->d_world_pos && L->d_obs_gt0 && L->d_Tcw));
}

orbfe_status gate_map_launch(const float *d_Tcw, const orbfe_track_camera *cam, float th, const TrkLevels &sf, int32_t nlevels,
                             float log_scale_factor, const orbfe_track_map *map, const uint32_t *d_list_off, const int32_t *d_list_idx,
                             const uint8_t *d_seen, uint32_t nentries, int32_t nframes, orbfe_proj_query *d_q, int32_t *d_qsrc,
                             int32_t *d_nq, int32_t qcap, int32_t *d_visible, orbfe_track_proj *d_proj, hipStream_t st)
{
    TrkGateMapArgs g;
    g.Tcw = d_Tcw;
    g.cam = *cam;
    g.th = th; g.log_sf = log_scale_factor; g.nlevels = nlevels; g.sf = sf;
    g.map = *map;
    g.list_off = d_list_off; g.list_idx = d_list_idx; g.seen = d_seen; g.nentries = nentries; g.qcap = qcap;
    g.q = d_q; g.qsrc = d_qsrc; g.nq = d_nq; g.visible = d_visible; g.proj = d_proj;
    hipLaunchKernelGGL(k_trk_gate_map, dim3(nframes), dim3(TRK_GT), 0, st, g);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

bool map_ok(const orbfe_track_map *M)
{
    return M && M->npoints >= 0 &&
           (M->npoints == 0 || (M->d_world_pos && M->d_normal && M->d_min_dist && M->d_max_dist && M->d_bad && M->d_obs_gt0));
}
}  // namespace

extern "C" int64_t orbfe_track_scratch_bytes(int32_t nframes, int32_t qcap, int64_t ent_cap)
{
    if (nframes < 0 || qcap < 1 || ent_cap < 0 || (int64_t)nframes * qcap >= TRK_MAX_SLOTS || ent_cap > 0xFFFFFFFFll) return -1;
    const size_t ng = (size_t)nframes * (size_t)qcap;
    // counts | per-lane counts | offsets | entries: the blocks core_launch asks the matcher's scratch for
    return (int64_t)(orb_align256(std::max<size_t>(ng * 4, 4)) + orb_align256(std::max<size_t>(ng * PJ_LC * 2, 4)) + orb_align256((ng + 1) * 4) +
                     orb_align256((size_t)std::max<int64_t>(ent_cap, 1) * 4));
}

extern "C" orbfe_status orbfe_frustum_points(const float *Tcw, const orbfe_track_camera *cam, float log_scale_factor, int32_t nlevels,
                                             int32_t n, const float *world_pos, const float *normal, const float *min_dist,
                                             const float *max_dist, const uint8_t *seen, const uint8_t *bad, orbfe_track_proj *proj,
                                             uint8_t *in_view)
{
    if (!Tcw || !cam || n < 0 || nlevels < 1 || (n > 0 && (!world_pos || !normal || !min_dist || !max_dist || !proj || !in_view))) {
        orbfe_set_error("bad argument to orbfe_frustum_points");
        return ORBFE_ERR_ARG;
    }
    const TrkCam c = *cam;
    float Ow[3];
    trk_camera_centre(Tcw, Ow);
    for (int i = 0; i < n; ++i) {
        TrkProj P;
        orbfe_track_proj o;
        o.u = o.v = o.ur = o.view_cos = 0.f;
        o.level = -1;
        in_view[i] = 0;
        if (!(seen && seen[i]) && !(bad && bad[i]) &&
            trk_frustum(Tcw, Ow, c, world_pos + 3 * (size_t)i, normal + 3 * (size_t)i, min_dist[i], max_dist[i], log_scale_factor, nlevels, &P)) {
            o.u = P.u; o.v = P.v; o.ur = P.ur; o.view_cos = P.view_cos; o.level = P.level;
            in_view[i] = 1;
        }
        proj[i] = o;
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_unproject_select_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const float *d_depth,
                                                            const int32_t *d_n, int32_t cap, int32_t nframes, const float *d_Tcw,
                                                            const orbfe_track_camera *cam, float th_depth, const uint8_t *d_keeps,
                                                            float *d_world_pos, uint8_t *d_created, void *stream)
{
    if (!m || !cam || cap < 1 || nframes < 0 || (nframes > 0 && (!d_kps || !d_depth || !d_n || !d_Tcw || !d_world_pos || !d_created))) {
        orbfe_set_error("bad argument to orbfe_unproject_select_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (cap > PJ_MAX_NF) { orbfe_set_error("orbfe_unproject_select_batch_device: at most %d features per frame", PJ_MAX_NF); return ORBFE_ERR_SIZE; }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    TrkUnprojArgs a;
    a.kps = (const float *)d_kps; a.depth = d_depth; a.n = d_n; a.cap = cap; a.Tcw = d_Tcw;
    a.cam = *cam;
    a.invfx = 1.0f / cam->fx;   // Frame's invfx / invfy
    a.invfy = 1.0f / cam->fy;
    a.th_depth = th_depth;
    a.keeps = d_keeps; a.world_pos = d_world_pos; a.created = d_created;
    hipLaunchKernelGGL(k_trk_unproject, dim3(nframes), dim3(TRK_UT), (size_t)cap * 4, (hipStream_t)stream, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_gate_last_frame_batch_device(orbfe_matcher *m, const float *d_Tcw_cur, const orbfe_track_last *last,
                                                           const orbfe_track_camera *cam, float mb, int32_t mono, float th,
                                                           const float *scale_factors, int32_t nlevels, int32_t nframes,
                                                           orbfe_proj_query *d_q, int32_t *d_qsrc, int32_t *d_nq, int32_t qcap,
                                                           void *stream)
{
    TrkLevels sf;
    if (!m || !cam || nframes < 0 || qcap < 1 || !last_ok(last, nframes) || !trk_levels_of(scale_factors, nlevels, &sf) ||
        (nframes > 0 && (!d_Tcw_cur || !d_q || !d_qsrc || !d_nq))) {
        orbfe_set_error("bad argument to orbfe_gate_last_frame_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    return gate_last_launch(d_Tcw_cur, last, cam, mb, mono, th, sf, nlevels, nframes, d_q, d_qsrc, d_nq, qcap, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_gate_local_map_batch_device(orbfe_matcher *m, const float *d_Tcw, const orbfe_track_camera *cam, float th,
                                                          const float *scale_factors, int32_t nlevels, float log_scale_factor,
                                                          const orbfe_track_map *map, const uint32_t *d_list_off,
                                                          const int32_t *d_list_idx, const uint8_t *d_seen, int64_t nentries,
                                                          int32_t nframes, orbfe_proj_query *d_q, int32_t *d_qsrc, int32_t *d_nq,
                                                          int32_t qcap, int32_t *d_visible, orbfe_track_proj *d_proj, void *stream)
{
    TrkLevels sf;
    if (!m || !cam || nframes < 0 || qcap < 1 || nentries < 0 || nentries > 0x7FFFFFFFll || !map_ok(map) ||
        !trk_levels_of(scale_factors, nlevels, &sf) || (nframes > 0 && (!d_Tcw || !d_list_off || !d_q || !d_qsrc || !d_nq)) ||
        (nentries > 0 && !d_list_idx)) {
        orbfe_set_error("bad argument to orbfe_gate_local_map_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    return gate_map_launch(d_Tcw, cam, th, sf, nlevels, log_scale_factor, map, d_list_off, d_list_idx, d_seen, (uint32_t)nentries, nframes,
                           d_q, d_qsrc, d_nq, qcap, d_visible, d_proj, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_search_by_projection_batch_device(orbfe_matcher *m, const orbfe_track_frames *frames, int32_t nframes,
                                                                const orbfe_proj_query *d_q, const int32_t *d_qsrc, const int32_t *d_nq,
                                                                int32_t qcap, const uint8_t *d_qpool, int32_t pool_rows,
                                                                int32_t pool_frame_rows, const float *inv_level_sigma2, int32_t nlevels,
                                                                int32_t th, float nnratio, int32_t ratio_rule, int64_t ent_cap,
                                                                int32_t *d_match, int32_t *d_best, int32_t *d_second, int32_t *d_status,
                                                                void *stream)
{
    const orbfe_status rs = core_check("orbfe_search_by_projection_batch_device", m, frames, nframes, qcap, th, ent_cap, inv_level_sigma2, nlevels);
    if (rs != ORBFE_OK) return rs;
    if (pool_rows < 0 || pool_frame_rows < 0 ||
        (nframes > 0 && (!d_q || !d_qsrc || !d_nq || !d_match || !d_best || !d_second || !d_status || (pool_rows > 0 && !d_qpool)))) {
        orbfe_set_error("bad argument to orbfe_search_by_projection_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const orbfe_status ls = core_launch(m, frames, nframes, d_q, d_qsrc, d_nq, qcap, d_qpool, pool_rows, pool_frame_rows, inv_level_sigma2,
                                        nlevels, th, nnratio, ratio_rule, ent_cap, d_match, d_best, d_second, d_status, st);
    if (ls != ORBFE_OK) return ls;
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_track_replay_batch_device(orbfe_matcher *m, const orbfe_track_frames *frames, int32_t nframes,
                                                        const int32_t *d_match, const int32_t *d_qsrc, const int32_t *d_nq, int32_t qcap,
                                                        const orbfe_keypoint *d_last_kps, int32_t cap_last, int32_t check_ori,
                                                        int32_t *d_assigned, int32_t *d_nmatches, int32_t *d_pairs, int32_t *d_npairs,
                                                        void *stream)
{
    if (!m || nframes < 0 || qcap < 1 || !frames || frames->cap < 0 || (check_ori && (!d_last_kps || cap_last < 1)) ||
        (nframes > 0 && (!frames->d_kps || !frames->d_n || !d_match || !d_qsrc || !d_nq || !d_assigned || !d_nmatches))) {
        orbfe_set_error("bad argument to orbfe_track_replay_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (frames->cap > PJ_MAX_NF) { orbfe_set_error("orbfe_track_replay_batch_device: at most %d features per frame", PJ_MAX_NF); return ORBFE_ERR_SIZE; }
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    replay_launch(frames, nframes, d_match, d_qsrc, d_nq, qcap, d_last_kps, cap_last, check_ori, d_assigned, d_nmatches, d_pairs, d_npairs,
                  (hipStream_t)stream);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

static bool out_ok(const orbfe_track_out *o, int32_t nframes)
{
    return o && o->qcap >= 1 &&
           (nframes == 0 || (o->d_q && o->d_qsrc && o->d_nq && o->d_match && o->d_best && o->d_second && o->d_status && o->d_assigned && o->d_nmatches));
}

extern "C" orbfe_status orbfe_track_last_frame_batch_device(orbfe_matcher *m, const orbfe_track_frames *cur, const float *d_Tcw_cur,
                                                            const orbfe_track_last *last, const orbfe_track_camera *cam, float mb,
                                                            int32_t mono, float th, const float *scale_factors, int32_t nlevels,
                                                            int32_t th_high, int32_t check_ori, int64_t ent_cap, int32_t nframes,
                                                            const orbfe_track_out *out, void *stream)
{
    TrkLevels sf;
    if (!out_ok(out, nframes) || !cam || !last_ok(last, nframes) || !trk_levels_of(scale_factors, nlevels, &sf) || (nframes > 0 && (!d_Tcw_cur || !last->d_mpdesc))) {
        orbfe_set_error("bad argument to orbfe_track_last_frame_batch_device");
        return ORBFE_ERR_ARG;
    }
    const orbfe_status rs = core_check("orbfe_track_last_frame_batch_device", m, cur, nframes, out->qcap, th_high, ent_cap, nullptr, 0);
    if (rs != ORBFE_OK) return rs;
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    orbfe_status s = gate_last_launch(d_Tcw_cur, last, cam, mb, mono, th, sf, nlevels, nframes, out->d_q, out->d_qsrc, out->d_nq, out->qcap, st);
    if (s != ORBFE_OK) return s;
    // :1673: no ratio rule
    s = core_launch(m, cur, nframes, out->d_q, out->d_qsrc, out->d_nq, out->qcap, last->d_mpdesc, last->cap, last->cap, nullptr, 0, th_high,
                    0.0f, 0, ent_cap, out->d_match, out->d_best, out->d_second, out->d_status, st);
    if (s != ORBFE_OK) return s;
    replay_launch(cur, nframes, out->d_match, out->d_qsrc, out->d_nq, out->qcap, last->d_kps, last->cap, check_ori, out->d_assigned,
                  out->d_nmatches, out->d_pairs, out->d_npairs, st);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_track_local_map_batch_device(orbfe_matcher *m, const orbfe_track_frames *cur, const float *d_Tcw,
                                                           const orbfe_track_camera *cam, float th, const float *scale_factors,
                                                           int32_t nlevels, float log_scale_factor, const orbfe_track_map *map,
                                                           const uint32_t *d_list_off, const int32_t *d_list_idx, const uint8_t *d_seen,
                                                           int64_t nentries, int32_t th_high, float nnratio, int64_t ent_cap,
                                                           int32_t nframes, const orbfe_track_out *out, int32_t *d_visible,
                                                           orbfe_track_proj *d_proj, void *stream)
{
    TrkLevels sf;
    if (!out_ok(out, nframes) || !cam || !map_ok(map) || nentries < 0 || nentries > 0x7FFFFFFFll || !trk_levels_of(scale_factors, nlevels, &sf) ||
        (nframes > 0 && (!d_Tcw || !d_list_off || (map->npoints > 0 && !map->d_desc))) || (nentries > 0 && !d_list_idx)) {
        orbfe_set_error("bad argument to orbfe_track_local_map_batch_device");
        return ORBFE_ERR_ARG;
    }
    const orbfe_status rs = core_check("orbfe_track_local_map_batch_device", m, cur, nframes, out->qcap, th_high, ent_cap, nullptr, 0);
    if (rs != ORBFE_OK) return rs;
    if (nframes == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    orbfe_status s = gate_map_launch(d_Tcw, cam, th, sf, nlevels, log_scale_factor, map, d_list_off, d_list_idx, d_seen, (uint32_t)nentries,
                                     nframes, out->d_q, out->d_qsrc, out->d_nq, out->qcap, d_visible, d_proj, st);
    if (s != ORBFE_OK) return s;
    // :143-146: the ratio rule is on; one pool of MapPoint descriptors for all frames
    s = core_launch(m, cur, nframes, out->d_q, out->d_qsrc, out->d_nq, out->qcap, map->d_desc, map->npoints, 0, nullptr, 0, th_high, nnratio,
                    1, ent_cap, out->d_match, out->d_best, out->d_second, out->d_status, st);
    if (s != ORBFE_OK) return s;
    replay_launch(cur, nframes, out->d_match, out->d_qsrc, out->d_nq, out->qcap, nullptr, 0, 0, out->d_assigned, out->d_nmatches, out->d_pairs,
                  out->d_npairs, st);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}
