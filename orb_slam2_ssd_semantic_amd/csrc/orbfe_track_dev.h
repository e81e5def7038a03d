// orbfe_track_dev.h -- what the batched, device-resident searches share: the argument block of the search core with a frame
// dimension (TrkCoreArgs), a frame's view of it (trk_frame_args, trk_query), the order-preserving compaction of the gating
// kernels (trk_compact_pos) and the one launch site of the core's count -> scan -> fill.  For orbfe_track.hip (the tracker's two
// SearchByProjection calls) and orbfe_init_search.hip (SearchForInitialization), which differ in their gating and in their
// acceptance rule, not in how the candidate lists are made.
#pragma once

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_proj_dev.h"

#define TRK_MAX_LEVELS 16        // orbfe_params.nlevels is 1..16: the per-level tables travel in the kernel arguments
#define TRK_GT 256               // threads of the gating and replay workgroups

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

// ComputeThreeMaxima (src/ORBmatcher.cc:1912-1957) over the 30 bins of a rotation histogram: keep[0..2] = the bins that stay, -1
// where the second / third is under a tenth of the first.  One thread calls it.
__device__ __forceinline__ void trk_three_maxima(const int *hist, int *keep)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < ORBFE_HISTO_LENGTH; ++i) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            i3 = i2; i2 = i1; i1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            i3 = i2; i2 = i;
        } else if (s > max3) {
            max3 = s; i3 = i;
        }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { i2 = -1; i3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) { i3 = -1; }
    keep[0] = i1; keep[1] = i2; keep[2] = i3;
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
    ProjArgs a;
    const int64_t fb = (int64_t)f * b.F.cap;
    a.descF = b.F.d_desc + fb * 32;
    a.xyF = (const float *)b.F.d_kps + fb * 7;
    a.octF = (const int32_t *)b.F.d_kps + fb * 7 + 5;
    a.nF = min(max(b.F.d_n[f], 0), b.F.cap);
    a.xs = 7; a.os = 7;
    a.cell_off = b.F.d_cell_off + (int64_t)f * (GRID_NC + 1);
    a.cell_idx = b.F.d_cell_idx + fb;
    a.minx = b.F.minx; a.miny = b.F.miny; a.gwi = b.F.gw_inv; a.ghi = b.F.gh_inv;
    a.uRight = b.F.d_uright ? b.F.d_uright + fb : nullptr;
    a.blocked = b.F.d_slot ? b.F.d_slot + fb : nullptr;
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
