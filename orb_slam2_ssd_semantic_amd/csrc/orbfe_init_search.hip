// orbfe_init_search.hip -- ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651, Tracking::MonocularInitialization) for
// a batch of frame pairs, device-resident (include/orbfe.h "SearchForInitialization"):
//   k_isrch_gate      one query per level-0 feature of the first frame, compacted in feature order
//   (k_trk_count -> scan -> k_trk_fill of orbfe_track.hip: every window's candidates with their distances)
//   k_isrch_resolve   the in-order acceptance rule with its take-overs, as relaxation rounds over per-feature claim lists
//   k_isrch_finish    the holders, the rotation histogram over ALL accepted queries, matches12, nmatches, prev, and the pairs'
//                     points and matches packed by their counts (CSR), as orbfe_initializer_initialize_device takes them
//   orbfe_search_for_initialization_batch_device, orbfe_search_for_initialization (host buffers, one pair),
//   orbfe_init_search_scratch_bytes (host)
// The batch form is enqueued on the caller's stream; it waits for nothing and writes no host memory.
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"
#include "orbfe_track_dev.h"

static_assert(sizeof(orbfe_keypoint) == 7 * sizeof(float) && offsetof(orbfe_keypoint, octave) == 20 && offsetof(orbfe_keypoint, angle) == 12,
              "keypoint record = 7 floats: (x, y) first, angle fourth, octave sixth");

#define ISR_END 0xFFFFu          // "no next claimant" in a claim word; query positions stay below it (cap <= PJ_MAX_NF)
static_assert(PJ_MAX_NF < ISR_END, "a claim word holds the next claimant in 16 bits");

struct IsrchArgs {
    TrkCoreArgs c;               // c.F = the second frames, c.pool = the first frames' descriptors, c.qcap = cap1
    const float *kps1;           // [npairs][cap1][7]
    const int32_t *n1;
    const float *prev_in;        // [npairs][cap1][2] or null: the features' own positions
    float window;
    int32_t check_ori, min_matches;
    orbfe_proj_query *q;         // the writable views of c.q / c.qsrc / c.nq
    int32_t *qsrc, *nq;
    uint32_t *claim;             // [npairs][cap1]: distance << 16 | next claimant on the same feature (ISR_END: none)
    int32_t *matches12, *nmatches;
    float *prev_out;
    int32_t *offsets1, *offsets2, *matches_csr;   // the packed (CSR) outputs, each may be null
    float *keys1_xy, *keys2_xy;
};

// ---------------------------------------------------------------------------------------------------
// 1. :537-545: every feature of the first frame with octave 0 asks GetFeaturesInArea(prev.x, prev.y, window, 0, 0)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_GT) void k_isrch_gate(IsrchArgs a)
{
    __shared__ int s_wave[TRK_GT / 64];
    const int f = blockIdx.x, tid = threadIdx.x, cap1 = a.c.qcap;
    const int n = min(max(a.n1[f], 0), cap1);
    const int64_t fb = (int64_t)f * cap1;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += TRK_GT) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        const bool ok = i < n && ((const int32_t *)a.kps1)[(fb + i) * 7 + 5] == 0;
        int tot;
        const int pos = base + trk_compact_pos(ok, s_wave, &tot);
        if (ok) {   // pos < n <= cap1: no query is dropped
            const float *p = a.prev_in ? a.prev_in + (fb + i) * 2 : a.kps1 + (fb + i) * 7;
            orbfe_proj_query Q;
            Q.u = p[0]; Q.v = p[1]; Q.r = a.window;
            Q.min_level = 0; Q.max_level = 0;
            Q.ur = 0.f; Q.flags = 0; Q.pad = 0;
            a.q[fb + pos] = Q;
            a.qsrc[fb + pos] = i;
        }
        base += tot;
    }
    if (tid == 0) a.nq[f] = base;
}

// ---------------------------------------------------------------------------------------------------
// 2. :547-612 as relaxation rounds, one workgroup per pair.  The reference's loop skips candidate j of query i when
// vMatchedDistance[j] <= d, and vMatchedDistance[j] is the smallest distance among the EARLIER queries accepted on j: a prefix
// minimum over j's claimants in query order, which no single word per feature holds.  So every round rebuilds, per feature of
// the second frame, the list of the queries accepted on it in the round before (head in LDS, next and distance in claim[]),
// and a candidate scan walks the list of its feature: skipped when any claimant k < i holds it at d_k <= d.  Query i depends
// on queries k < i only, so after round r the first r queries are final and the loop ends in a round that changes nothing.
// Decisions of round r see the claims of round r - 1 only (match / best are read by their own writer and by the rebuild behind
// the barrier), so the number of rounds is a property of the input, not of the schedule.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PJ_T) void k_isrch_resolve(IsrchArgs x)
{
    extern __shared__ int32_t s_head[];   // [cap2]: a claimant of the feature, -1 none
    __shared__ int s_changed;
    const TrkCoreArgs &b = x.c;
    const int f = blockIdx.x, tid = threadIdx.x, sub = tid % PJ_L, grp = tid / PJ_L;
    const int64_t ng = (int64_t)b.nframes * b.qcap, g0 = (int64_t)f * b.qcap;
    const int nq = min(max(b.nq[f], 0), b.qcap), nF = min(max(b.F.d_n[f], 0), b.F.cap);
    int32_t *match = b.match + g0, *best = b.best + g0;
    uint32_t *claim = x.claim + g0;
    const uint32_t *off = b.off + g0;
    for (int i = tid; i < b.qcap; i += PJ_T) match[i] = -1;
    const uint32_t total = b.off[ng];
    if (total > b.ent_cap) {   // workgroup-uniform: the caller grows the entry buffer and calls again
        if (tid == 0) b.status[0] = (int32_t)total;
        return;
    }
    for (int k = tid; k < nF; k += PJ_T) s_head[k] = -1;
    __syncthreads();
    int round = 0;
    for (; round <= nq + 1; ++round) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        bool changed = false;
        for (int i0 = 0; i0 < nq; i0 += PJ_T / PJ_L) {
            const int i = i0 + grp;
            uint32_t k1 = PJ_NOKEY, k2 = PJ_NOKEY;   // the two smallest keys (dist << 16 | position) among the candidates not skipped
            uint32_t o = 0, e = 0;
            if (i < nq) { o = off[i]; e = off[i + 1]; }
            for (uint32_t k = o + sub; k < e; k += PJ_L) {
                const uint32_t en = b.ent[k];
                const uint32_t ft = en & 0xFFFFu, d = en >> 16;
                if (d == PJ_SKIP || ft >= (uint32_t)nF) continue;
                bool held = false;   // :566: an earlier query holds the feature at least as close
                int c = s_head[ft];
                for (int it = 0; c >= 0 && it < nq; ++it) {   // a list has at most nq nodes
                    const uint32_t cl = claim[c];
                    if (c < i && (cl >> 16) <= d) { held = true; break; }
                    const uint32_t nx = cl & 0xFFFFu;
                    c = nx == ISR_END ? -1 : (int)nx;
                }
                if (held) continue;
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
                const int bestDist = k1 == PJ_NOKEY ? 256 : (int)(k1 >> 16);
                // bestDist2 = INT_MAX without a second candidate (:554), as the float the reference's cast gives
                const float second = k2 == PJ_NOKEY ? 2147483648.0f : (float)(int)(k2 >> 16);
                int mt = -1;
                if (bestDist <= b.th && (float)bestDist < __fmul_rn(second, b.nnratio))   // :583-587
                    mt = (int)(b.ent[o + (k1 & 0xFFFFu)] & 0xFFFFu);
                if (mt != match[i] || (mt >= 0 && bestDist != best[i])) {   // the claim (feature, distance) of the query changed
                    match[i] = mt;
                    best[i] = bestDist;
                    changed = true;
                }
            }
        }
        if (changed) s_changed = 1;
        __syncthreads();
        if (!s_changed) break;                 // workgroup-uniform
        for (int k = tid; k < nF; k += PJ_T) s_head[k] = -1;
        __syncthreads();
        for (int i = tid; i < nq; i += PJ_T) {
            const int mt = match[i];
            if (mt >= 0) {
                const int nx = atomicExch(&s_head[mt], i);
                claim[i] = ((uint32_t)best[i] << 16) | (nx < 0 ? ISR_END : (uint32_t)nx);
            }
        }
        __syncthreads();
    }
    if (tid == 0) atomicMax(&b.status[1], round + 1);
}

// ---------------------------------------------------------------------------------------------------
// 3. what the loop leaves behind (:590-598, :600-650), one workgroup per pair: a feature of the second frame ends with the LAST
// query accepted on it (vnMatches21), every accepted query votes in the rotation histogram whether or not it was taken over
// later, a vote in a dropped bin clears the query's entry only if it still stands, nmatches = the entries that stand.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_GT) void k_isrch_finish(IsrchArgs x)
{
    extern __shared__ int32_t s_holder[];   // [cap2]: the last query accepted on the feature, -1 none
    __shared__ int s_hist[ORBFE_HISTO_LENGTH], s_keep[3], s_wave[TRK_GT / 64], s_cnt, s_o1, s_o2;
    const TrkCoreArgs &b = x.c;
    const int f = blockIdx.x, tid = threadIdx.x, cap1 = b.qcap, cap2 = b.F.cap;
    const int64_t fb1 = (int64_t)f * cap1, fb2 = (int64_t)f * cap2;
    const int n1 = min(max(x.n1[f], 0), cap1), n2 = min(max(b.F.d_n[f], 0), cap2), nq = min(max(b.nq[f], 0), cap1);
    const bool short_cap = b.status[0] != 0;   // every pair of the call answers "call again"
    const float *k1 = x.kps1 + fb1 * 7, *k2 = (const float *)b.F.d_kps + fb2 * 7;
    const int32_t *match = b.match + fb1, *qsrc = b.qsrc + fb1;
    for (int k = tid; k < n2; k += TRK_GT) s_holder[k] = -1;
    if (tid < ORBFE_HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) { s_cnt = 0; s_o1 = 0; s_o2 = 0; }
    __syncthreads();
    if (x.offsets1 || x.offsets2) {   // where the pair's packed rows start: the clamped counts of the pairs before it
        int a1 = 0, a2 = 0;
        for (int p = tid; p < f; p += TRK_GT) {
            a1 += min(max(x.n1[p], 0), cap1);
            a2 += min(max(b.F.d_n[p], 0), cap2);
        }
        if (a1) atomicAdd(&s_o1, a1);
        if (a2) atomicAdd(&s_o2, a2);
    }
    auto bin_of = [&](int i1, int m) { return rot_bin_clamped(k1[(int64_t)i1 * 7 + 3], k2[(int64_t)m * 7 + 3]); };
    if (!short_cap) {
        for (int i = tid; i < nq; i += TRK_GT) {
            const int m = match[i];
            if (m < 0 || m >= n2) continue;
            atomicMax(&s_holder[m], i);
            if (x.check_ori) atomicAdd(&s_hist[bin_of(qsrc[i], m)], 1);
        }
    }
    __syncthreads();
    if (x.check_ori) {
        if (tid == 0) rot_three_maxima(s_hist, ORBFE_HISTO_LENGTH, s_keep);
        __syncthreads();
    }
    const int64_t o1 = s_o1, o2 = s_o2;
    if (tid == 0) {
        if (x.offsets1) { x.offsets1[f] = (int32_t)o1; if (f == b.nframes - 1) x.offsets1[f + 1] = (int32_t)o1 + n1; }
        if (x.offsets2) { x.offsets2[f] = (int32_t)o2; if (f == b.nframes - 1) x.offsets2[f + 1] = (int32_t)o2 + n2; }
    }
    int base = 0, mine = 0;
    for (int i0 = 0; i0 < cap1; i0 += TRK_GT) {   // workgroup-uniform trip count
        const int i = i0 + tid;
        const bool isq = i < n1 && ((const int32_t *)k1)[(int64_t)i * 7 + 5] == 0;   // the gate's rule: its position is the query
        int tot;
        const int pos = base + trk_compact_pos(isq, s_wave, &tot);
        base += tot;
        if (i >= cap1) continue;
        int mm = -1;
        if (isq && !short_cap) {
            const int m = match[pos];
            if (m >= 0 && m < n2 && s_holder[m] == pos) {
                const int bin = x.check_ori ? bin_of(i, m) : 0;
                if (!x.check_ori || rot_keeps(s_keep, bin)) mm = m;
            }
        }
        x.matches12[fb1 + i] = mm;
        if (mm >= 0) ++mine;
        const float ox = i < n1 ? k1[(int64_t)i * 7] : 0.f, oy = i < n1 ? k1[(int64_t)i * 7 + 1] : 0.f;
        if (x.prev_out) {
            float px = x.prev_in ? x.prev_in[(fb1 + i) * 2] : ox, py = x.prev_in ? x.prev_in[(fb1 + i) * 2 + 1] : oy;
            if (mm >= 0) { px = k2[(int64_t)mm * 7]; py = k2[(int64_t)mm * 7 + 1]; }   // :646-648
            x.prev_out[(fb1 + i) * 2] = px;
            x.prev_out[(fb1 + i) * 2 + 1] = py;
        }
        if (i < n1) {
            if (x.matches_csr) x.matches_csr[o1 + i] = mm;
            if (x.keys1_xy) {
                x.keys1_xy[(o1 + i) * 2] = ox;
                x.keys1_xy[(o1 + i) * 2 + 1] = oy;
            }
        }
    }
    if (mine) atomicAdd(&s_cnt, mine);
    if (x.keys2_xy) {
        for (int k = tid; k < n2; k += TRK_GT) {
            x.keys2_xy[(o2 + k) * 2] = k2[(int64_t)k * 7];
            x.keys2_xy[(o2 + k) * 2 + 1] = k2[(int64_t)k * 7 + 1];
        }
    }
    __syncthreads();
    const int nm = s_cnt;
    if (tid == 0) x.nmatches[f] = nm;
    if (x.min_matches > 0 && nm < x.min_matches)   // Tracking :660: too few, the pair is not handed to the Initializer
        for (int i = tid; i < cap1; i += TRK_GT) {
            x.matches12[fb1 + i] = -1;
            if (x.matches_csr && i < n1) x.matches_csr[o1 + i] = -1;
        }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace
{
struct IsrchScratch {
    size_t q, qsrc, nq, match, best, claim, total;
};
IsrchScratch isrch_scratch(int32_t npairs, int32_t cap1)
{
    const size_t ng = (size_t)npairs * (size_t)cap1;
    IsrchScratch z;
    z.q = 0;
    z.qsrc = z.q + orb_align256(std::max<size_t>(ng * sizeof(orbfe_proj_query), 4));
    z.nq = z.qsrc + orb_align256(std::max<size_t>(ng * 4, 4));
    z.match = z.nq + orb_align256(std::max<size_t>((size_t)npairs * 4, 4));
    z.best = z.match + orb_align256(std::max<size_t>(ng * 4, 4));
    z.claim = z.best + orb_align256(std::max<size_t>(ng * 4, 4));
    z.total = z.claim + orb_align256(std::max<size_t>(ng * 4, 4));
    return z;
}

orbfe_status limits(const char *who, int32_t npairs, int32_t cap1, int32_t cap2, int32_t th_low, int64_t ent_cap)
{
    if (th_low > 255) { orbfe_set_error("%s: th_low must be below 256 (256 is the 'no candidate' distance)", who); return ORBFE_ERR_ARG; }
    if (cap1 > PJ_MAX_NF || cap2 > PJ_MAX_NF) { orbfe_set_error("%s: at most %d features per frame", who, PJ_MAX_NF); return ORBFE_ERR_SIZE; }
    if ((int64_t)npairs * cap1 >= TRK_MAX_SLOTS || ent_cap > 0xFFFFFFFFll) {
        orbfe_set_error("%s: npairs * cap must stay below 2^25 and ent_cap below 2^32", who);
        return ORBFE_ERR_SIZE;
    }
    return ORBFE_OK;
}

// gate -> count -> scan -> fill -> resolve -> finish on `st`, between the caller's scratch_acquire and scratch_release
orbfe_status isrch_launch(orbfe_matcher *m, const orbfe_init_search_first *first, const orbfe_track_frames *second, int32_t npairs,
                          const float *d_prev_in, int32_t window, int32_t th_low, float nnratio, int32_t check_ori, int32_t min_matches,
                          int64_t ent_cap, const orbfe_init_search_out *out, hipStream_t st)
{
    const int32_t cap1 = first->cap;
    const IsrchScratch z = isrch_scratch(npairs, cap1);
    ORBFE_HIP(m->b[6].ensure(z.total));
    char *base = m->b[6].as<char>();
    IsrchArgs a;
    memset(&a, 0, sizeof(a));
    TrkCoreArgs &b = a.c;
    b.F = *second;
    b.F.d_uright = nullptr;   // :545-566: no right-image gate, no slots taken before the call
    b.F.d_slot = nullptr;
    b.nframes = npairs;
    b.has_sigma2 = 0; b.nlevels = 1;
    a.q = (orbfe_proj_query *)(base + z.q);
    a.qsrc = (int32_t *)(base + z.qsrc);
    a.nq = (int32_t *)(base + z.nq);
    b.q = a.q; b.qsrc = a.qsrc; b.nq = a.nq; b.qcap = cap1;
    b.pool = first->d_desc; b.pool_rows = cap1; b.pool_frame_rows = cap1;
    b.th = th_low; b.ratio_rule = 0; b.nnratio = nnratio;
    b.match = (int32_t *)(base + z.match);
    b.best = (int32_t *)(base + z.best);
    b.second = nullptr;
    b.status = out->d_status;
    a.claim = (uint32_t *)(base + z.claim);
    a.kps1 = (const float *)first->d_kps;
    a.n1 = first->d_n;
    a.prev_in = d_prev_in;
    a.window = (float)window;
    a.check_ori = check_ori ? 1 : 0;
    a.min_matches = min_matches;
    a.matches12 = out->d_matches12; a.nmatches = out->d_nmatches;
    a.prev_out = out->d_prev_out;
    a.offsets1 = out->d_offsets1; a.offsets2 = out->d_offsets2; a.matches_csr = out->d_matches12_csr;
    a.keys1_xy = out->d_keys1_xy; a.keys2_xy = out->d_keys2_xy;
    const size_t lds = (size_t)std::max(second->cap, 1) * 4;
    hipLaunchKernelGGL(k_isrch_gate, dim3(npairs), dim3(TRK_GT), 0, st, a);
    const orbfe_status ls = orbfe_internal_track_lists_launch(m, b, ent_cap, st);
    if (ls != ORBFE_OK) return ls;
    hipLaunchKernelGGL(k_isrch_resolve, dim3(npairs), dim3(PJ_T), lds, st, a);
    hipLaunchKernelGGL(k_isrch_finish, dim3(npairs), dim3(TRK_GT), lds, st, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
}  // namespace

extern "C" int64_t orbfe_init_search_scratch_bytes(int32_t npairs, int32_t cap1, int64_t ent_cap)
{
    const int64_t lists = orbfe_track_scratch_bytes(npairs, cap1, ent_cap);
    if (lists < 0 || cap1 > PJ_MAX_NF) return -1;
    return lists + (int64_t)isrch_scratch(npairs, cap1).total;
}

extern "C" orbfe_status orbfe_search_for_initialization_batch_device(orbfe_matcher *m, const orbfe_init_search_first *first,
                                                                     const orbfe_track_frames *second, int32_t npairs,
                                                                     const float *d_prev_in, int32_t window, int32_t th_low, float nnratio,
                                                                     int32_t check_ori, int32_t min_matches, int64_t ent_cap,
                                                                     const orbfe_init_search_out *out, void *stream)
{
    const char *who = "orbfe_search_for_initialization_batch_device";
    if (!m || !first || !second || !out || npairs < 0 || first->cap < 1 || second->cap < 0 || ent_cap < 0 || window < 0 || min_matches < 0 ||
        (npairs > 0 && (!first->d_kps || !first->d_desc || !first->d_n || !second->d_kps || !second->d_desc || !second->d_n ||
                        !second->d_cell_off || !second->d_cell_idx || !out->d_matches12 || !out->d_nmatches || !out->d_status)) ||
        (((out->d_matches12_csr || out->d_keys1_xy) && !out->d_offsets1) || (out->d_keys2_xy && !out->d_offsets2))) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    const orbfe_status lim = limits(who, npairs, first->cap, second->cap, th_low, ent_cap);
    if (lim != ORBFE_OK) return lim;
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const orbfe_status s = isrch_launch(m, first, second, npairs, d_prev_in, window, th_low, nnratio, check_ori, min_matches, ent_cap, out, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(scratch_release(m, st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_search_for_initialization(orbfe_matcher *m, const float *xy1, const int32_t *oct1, const float *ang1,
                                                        const uint8_t *desc1, int32_t n1, const float *xy2, const int32_t *oct2,
                                                        const float *ang2, const uint8_t *desc2, int32_t n2, const uint32_t *cell_off,
                                                        const uint32_t *cell_idx, float minx, float miny, float gw_inv, float gh_inv,
                                                        float *prev, int32_t window, int32_t th_low, float nnratio, int32_t check_ori,
                                                        int32_t *matches12, int32_t *nmatches)
{
    const char *who = "orbfe_search_for_initialization";
    if (!m || n1 < 0 || n2 < 0 || window < 0 || !cell_off || !nmatches || (n1 > 0 && (!xy1 || !oct1 || !ang1 || !desc1 || !prev || !matches12)) ||
        (n2 > 0 && (!xy2 || !oct2 || !ang2 || !desc2)) || (cell_off[GRID_NC] > 0 && !cell_idx)) {
        orbfe_set_error("bad argument to %s", who);
        return ORBFE_ERR_ARG;
    }
    const orbfe_status lim = limits(who, 1, n1, n2, th_low, 0);
    if (lim != ORBFE_OK) return lim;
    if (!orb_grid_csr_ok(cell_off, cell_idx, n2, "n2")) return ORBFE_ERR_ARG;
    *nmatches = 0;
    if (n1 == 0) return ORBFE_OK;
    // the keypoint records the batch form reads in place: x, y, angle, octave
    std::vector<orbfe_keypoint> kp((size_t)n1 + (size_t)n2);
    memset(kp.data(), 0, kp.size() * sizeof(orbfe_keypoint));
    for (int i = 0; i < n1; ++i) { kp[(size_t)i].x = xy1[2 * i]; kp[(size_t)i].y = xy1[2 * i + 1]; kp[(size_t)i].angle = ang1[i]; kp[(size_t)i].octave = oct1[i]; }
    for (int i = 0; i < n2; ++i) {
        orbfe_keypoint &k = kp[(size_t)n1 + (size_t)i];
        k.x = xy2[2 * i]; k.y = xy2[2 * i + 1]; k.angle = ang2[i]; k.octave = oct2[i];
    }
    const int32_t counts[2] = {n1, n2};
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const StagePiece in[8] = {{kp.data(), (size_t)n1 * sizeof(orbfe_keypoint)}, {desc1, (size_t)n1 * 32},
                              {kp.data() + n1, (size_t)n2 * sizeof(orbfe_keypoint)}, {desc2, (size_t)n2 * 32},
                              {cell_off, (size_t)(GRID_NC + 1) * 4}, {cell_idx, (size_t)cell_off[GRID_NC] * 4},
                              {prev, (size_t)n1 * 8}, {counts, sizeof(counts)}};
    const char *din[8];
    ORBFE_HIP(stage_upload(m, st, in, din));
    // results: matches12 [n1] | prev [n1][2] | nmatches | status [2]
    const size_t o_prev = orb_align256((size_t)n1 * 4), o_nm = o_prev + orb_align256((size_t)n1 * 8), o_total = o_nm + 256;
    ORBFE_HIP(m->b[1].ensure(o_total));
    ORBFE_HIP(m->pin_out.ensure(o_total));
    char *dout = m->b[1].as<char>();
    orbfe_init_search_first first;
    first.d_kps = (const orbfe_keypoint *)din[0];
    first.d_desc = (const uint8_t *)din[1];
    first.d_n = (const int32_t *)din[7];
    first.cap = n1;
    orbfe_track_frames second;
    memset(&second, 0, sizeof(second));
    second.d_kps = (const orbfe_keypoint *)din[2];
    second.d_desc = (const uint8_t *)din[3];
    second.d_n = (const int32_t *)din[7] + 1;
    second.cap = n2;
    second.d_cell_off = (const uint32_t *)din[4];
    second.d_cell_idx = (const uint32_t *)din[5];
    second.minx = minx; second.miny = miny; second.gw_inv = gw_inv; second.gh_inv = gh_inv;
    orbfe_init_search_out out;
    memset(&out, 0, sizeof(out));
    out.d_matches12 = (int32_t *)dout;
    out.d_prev_out = (float *)(dout + o_prev);
    out.d_nmatches = (int32_t *)(dout + o_nm);
    out.d_status = (int32_t *)(dout + o_nm) + 1;
    int64_t ent_cap = std::max<int64_t>((int64_t)n1 * 256, 1 << 16);
    const char *res = m->pin_out.as<const char>();
    for (int attempt = 0;; ++attempt) {
        const orbfe_status s = isrch_launch(m, &first, &second, 1, (const float *)din[6], window, th_low, nnratio, check_ori, 0, ent_cap, &out, st);
        if (s != ORBFE_OK) return s;
        ORBFE_HIP(hipMemcpyAsync(m->pin_out.p, dout, o_total, hipMemcpyDeviceToHost, st));
        ORBFE_HIP(hipStreamSynchronize(st));
        const int32_t need = ((const int32_t *)(res + o_nm))[1];
        if (need == 0) break;
        if (attempt == 1) { orbfe_set_error("%s: candidate scratch still too small (%d entries)", who, need); return ORBFE_ERR_NOMEM; }
        ent_cap = (int64_t)(uint32_t)need;   // the exact need: the second launch cannot fail on it
    }
    ORBFE_HIP(scratch_release(m, st));
    memcpy(matches12, res, (size_t)n1 * 4);
    memcpy(prev, res + o_prev, (size_t)n1 * 8);
    *nmatches = *(const int32_t *)(res + o_nm);
    return ORBFE_OK;
}
