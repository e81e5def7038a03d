// orbfe_track_dev.h -- what the batched, device-resident searches share.  Device side: the order-preserving compaction of the
// gating and replay kernels (trk_compact_pos), a row of an orbfe_track_frames block as the walk's ProjArgs (proj_frame_view), the
// argument block of the search core with a frame dimension (TrkCoreArgs) with its view of a frame (trk_frame_args, trk_query)
// and the one launch site of the core's count -> scan -> fill.  The slot limit of a call (TRK_MAX_SLOTS) stands with the other
// limits at the top; host side, at the end: the level tables (trk_levels_of) and the frame-block check (trk_frames_ok).  The rotation histogram's rules are
// orbfe_match_dev.h's (rot_bin_clamped, rot_three_maxima, rot_keeps); the camera block is orbfe_track_geom.h's TrkCam.
// For orbfe_track.hip (the tracker's two SearchByProjection calls) and orbfe_init_search.hip (SearchForInitialization), which
// share the core and differ in their gating and acceptance rule; for orbfe_fuse.hip and orbfe_sim3_search.hip, which take the
// frame view, the compaction and the host checks; for orbfe_tri_search.hip and orbfe_newpoints.hip, which take the compaction
// and the slot limit.
#pragma once

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_proj_dev.h"

#define TRK_MAX_LEVELS 16        // orbfe_params.nlevels is 1..16: the per-level tables travel in the kernel arguments
#define TRK_GT 256               // threads of the gating and replay workgroups
// what one call may address -- frames x queries, pairs x features, list entries: every device-resident search refuses more, and
// every message that names the limit says 2^25
#define TRK_MAX_SLOTS ((int64_t)1 << 25)

struct TrkLevels {
    float v[TRK_MAX_LEVELS];
};

// Order-preserving compaction inside one workgroup of TRK_GT threads: the position of this lane's item among the items of the
// chunk (ballot + prefix inside the wave, the waves' totals through LDS) above the running base of the chunks before it.  No
// atomic takes a slot, so item order = lane order = the reference's loop order.  Returns the position; *total = the chunk's
// count.  All threads of the workgroup call it.
__device__ __forceinline__ int trk_compact_pos(bool ok, int *s_wave /* [TRK_GT / 64] */, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(ok);
    const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[w] = __popcll(mask);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < TRK_GT / 64; ++k) {
        const int c = s_wave[k];
        if (k < w) base += c;
        tot += c;
    }
    __syncthreads();   // s_wave is free again
    *total = tot;
    return base + prefix;
}

// Row `row` of a block of frames as the walk sees it: every field of ProjArgs that the block alone decides.  No slot blocks, no
// right-image gate and no chi2 table until the form sets them (trk_frame_args, fuse_frame_args, s3_frame_args), with its
// nlevels, th, ratio_rule and nnratio.
__device__ __forceinline__ ProjArgs proj_frame_view(const orbfe_track_frames &F, int row)
{
    ProjArgs a;
    const int64_t fb = (int64_t)row * F.cap;
    a.descF = F.d_desc + fb * 32;
    a.xyF = (const float *)F.d_kps + fb * 7;
    a.octF = (const int32_t *)F.d_kps + fb * 7 + 5;
    a.nF = min(max(F.d_n[row], 0), F.cap);
    a.xs = 7; a.os = 7;
    a.cell_off = F.d_cell_off + (int64_t)row * (GRID_NC + 1);
    a.cell_idx = F.d_cell_idx + fb;
    a.minx = F.minx; a.miny = F.miny; a.gwi = F.gw_inv; a.ghi = F.gh_inv;
    a.uRight = nullptr;
    a.blocked = nullptr;
    a.inv_sigma2 = nullptr;
    return a;
}

// The search core with a frame dimension.  Global query g = f * qcap + i; lanes of queries beyond nq[f] count zero
// candidates, so ONE flat scan over nframes * qcap counts lays every frame's entries into one buffer (a scan per frame would
// be nframes launches or a second level; the flat one is a single launch whatever the batch).  Features are read in place
// from the keypoint records (stride 7), query descriptors are gathered as pool[qsrc], the slot table holds states (0 empty,
// 1 a MapPoint without observations, 2 one with: only 2 blocks) and the level table (at most 16 entries) travels in the kernel
// arguments.  The count, the gates and the distances are orbfe_proj_dev.h's, through the frame's view (trk_frame_args).
struct TrkCoreArgs {
    orbfe_track_frames F;
    int32_t nframes;
    TrkLevels inv_sigma2;
    int32_t has_sigma2, nlevels;
    const orbfe_proj_query *q;
    const int32_t *qsrc, *nq;
    int32_t qcap;
    const uint8_t *pool;
    int32_t pool_rows, pool_frame_rows;   // rows a query may address; rows between consecutive frames' pools (0: one pool)
    int32_t th, ratio_rule;
    float nnratio;
    int32_t *match, *best, *second;
    uint32_t *cnt;
    uint16_t *lcnt;
    uint32_t *off, *ent;
    uint32_t ent_cap;
    int32_t *status;
};

// the walk's view of frame f
__device__ __forceinline__ ProjArgs trk_frame_args(const TrkCoreArgs &b, int f)
{
    ProjArgs a = proj_frame_view(b.F, f);
    const int64_t fb = (int64_t)f * b.F.cap;
    if (b.F.d_uright) a.uRight = b.F.d_uright + fb;
    if (b.F.d_slot) a.blocked = b.F.d_slot + fb;
    a.nlevels = b.nlevels;
    a.th = b.th; a.ratio_rule = b.ratio_rule; a.nnratio = b.nnratio;
    return a;
}

// query g of the batch: false = it has no candidates (a lane beyond nq[f], a descriptor row outside the pool, an empty window)
__device__ __forceinline__ bool trk_query(const TrkCoreArgs &b, int f, int i, const ProjArgs &a, orbfe_proj_query &Q, ProjRect &R, int &src)
{
    if (i >= min(max(b.nq[f], 0), b.qcap)) return false;
    src = b.qsrc[(int64_t)f * b.qcap + i];
    if (src < 0 || src >= b.pool_rows) return false;
    Q = b.q[(int64_t)f * b.qcap + i];
    return proj_rect(a, Q, R);
}

// k_trk_count -> scan -> k_trk_fill on `st` (orbfe_track.hip, their one launch site): takes the matcher's scratch blocks 2..5
// for the counts, the per-lane counts, the offsets and the ent_cap entries (grow-only, no wait for the device), puts them
// into `b` and leaves off[nframes * qcap] = the entries needed; nothing is written to the entries when that exceeds ent_cap.
// b.status[0..1] are zeroed by the count.  The caller's acceptance kernel runs behind it on the same stream.
__attribute__((visibility("hidden"))) orbfe_status orbfe_internal_track_lists_launch(orbfe_matcher *m, TrkCoreArgs &b, int64_t ent_cap,
                                                                                     hipStream_t st);

// ---------------------------------------------------------------------------------------------------
// host side: the refusals and conversions the entry points of these searches share
// ---------------------------------------------------------------------------------------------------
// a per-level table of the caller (nlevels 1..TRK_MAX_LEVELS entries) as the kernel-argument array, zero behind nlevels
inline bool trk_levels_of(const float *v, int32_t nlevels, TrkLevels *out)
{
    if (!v || nlevels < 1 || nlevels > TRK_MAX_LEVELS) return false;
    for (int i = 0; i < TRK_MAX_LEVELS; ++i) out->v[i] = i < nlevels ? v[i] : 0.f;
    return true;
}

// a block of frames with its required pointers; min_cap is the form's: 0 for the tracker and Fuse (an empty block is a no-op), 1
// for the Sim3 searches
inline bool trk_frames_ok(const orbfe_track_frames *F, int32_t nframes, int32_t min_cap)
{
    return F && F->cap >= min_cap && (nframes == 0 || (F->d_kps && F->d_desc && F->d_n && F->d_cell_off && F->d_cell_idx));
}
