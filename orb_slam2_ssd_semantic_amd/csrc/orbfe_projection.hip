// orbfe_projection.hip -- the projection-gated searches of the matcher handle (include/orbfe.h "Matcher"): orbfe_search_by_projection*,
// orbfe_window_distances, orbfe_search_for_triangulation, on host buffers.  The search's arithmetic is csrc/orbfe_proj_dev.h (shared
// with the batched device-resident form, orbfe_track.hip); the input staging and the grid check are csrc/orbfe_matcher.h.
#include <algorithm>
#include <vector>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"
#include "orbfe_proj_dev.h"

// ---------------------------------------------------------------------------------------------------
// the projection-gated searches of the per-frame tracker
//   ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*>&, th)                 src/ORBmatcher.cc:63-157
//   ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) src/ORBmatcher.cc:1578-1724
//   (+ the perfect/ overload that also returns the 2-D point pairs, perfect/src/ORBmatcher.cc:1727-1911)
// The pose projection and its gates stay on the host (they run on cv::Mat in the caller's arithmetic); what comes here is
// one query per surviving MapPoint: GetFeaturesInArea on the frame's grid, the right-image gate, best / second-best Hamming
// over the candidates whose slot is free, the acceptance rule (all of these: csrc/orbfe_proj_dev.h).  The reference's loop
// is NOT a map over the queries: an accepted query writes its MapPoint into F.mvpMapPoints[bestIdx], and later queries skip a
// slot that holds a point with Observations() > 0 (:108-110 / :1647-1649).  That dependency only points backwards (query i
// sees the assignments of j < i), so the sequential result is the unique fixed point of "every query picks its best among the
// slots no EARLIER claiming query took", and it is reached by relaxation: all queries choose in parallel against the owner
// table of the previous round (owner[f] = lowest claiming query matched to f), the table is rebuilt, until no choice changes.
// Query i is final one round after all j < i are -- rounds = longest dependency chain + 1 (2-4 on real frames, <= nq + 1).
// This form's layout: packed points (2 floats / 1 int apart), query i's descriptor at qdesc + 32 i, `blocked` a table of flags,
// the level table a device pointer of up to 64 entries.
// Launch structure: the candidate lists (GetFeaturesInArea) and the Hamming distances are independent per query and are
// spread over the chip with one wave per query (k_proj_count -> k_scan_u32 -> k_proj_fill; every (cand | dist << 16) entry is
// materialised once); the relaxation rounds only re-scan those entries and run in ONE workgroup (k_proj_resolve, 16 lanes
// per query, owner table in LDS).
// ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_proj_count(ProjArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, i = t / PJ_LC, sub = t % PJ_LC;
    if (i >= a.nq) return;   // whole waves leave together
    const orbfe_proj_query Q = a.q[i];
    ProjRect R;
    const bool any = proj_rect(a, Q, R);
    proj_count(a, Q, R, any, sub, a.lcnt, a.cnt, (size_t)i);
}

__global__ __launch_bounds__(256) void k_proj_fill(ProjArgs a)
{
    const int t = blockIdx.x * 256 + threadIdx.x, i = t / PJ_LC, sub = t % PJ_LC;
    if (i >= a.nq || a.off[a.nq] > a.ent_cap) return;
    const orbfe_proj_query Q = a.q[i];
    ProjRect R;
    if (!proj_rect(a, Q, R)) return;   // wave-uniform
    const int mine = a.lcnt[(size_t)i * PJ_LC + sub];
    uint32_t o = a.off[i] + (uint32_t)(wave_incl_scan_m(mine) - mine);
    const Desc8 dq = load_desc8(a.qdesc + (int64_t)i * 32);
    proj_walk(a, Q, R, sub, [&](uint32_t f) {
        const bool skip = proj_gate_skip(a, Q, f, 1, a.inv_sigma2 != nullptr, [&](int lv) { return a.inv_sigma2[lv]; });
        const uint32_t d = proj_dist(a, dq, f, skip);
        a.ent[o++] = f | (d << 16);
    });
}

__global__ __launch_bounds__(PJ_T) void k_proj_resolve(ProjArgs a)
{
    extern __shared__ int32_t s_owner[];   // [nF]
    __shared__ int s_changed;
    const int tid = threadIdx.x, sub = tid % PJ_L, grp = tid / PJ_L;
    const int nq = a.nq, nF = a.nF;
    if (tid == 0) {
        const uint32_t total = a.off[nq];
        a.status[0] = total > a.ent_cap ? (int32_t)total : 0;
        a.status[1] = 0;
    }
    if (a.off[nq] > a.ent_cap) return;   // workgroup-uniform: the host grows the scratch and launches again
    for (int f = tid; f < nF; f += PJ_T) s_owner[f] = 0x7FFFFFFF;
    for (int i = tid; i < nq; i += PJ_T) a.match[i] = -1;
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
            if (i < nq) { o = a.off[i]; e = a.off[i + 1]; }
            for (uint32_t k = o + sub; k < e; k += PJ_L) {
                const uint32_t en = a.ent[k];
                const uint32_t f = en & 0xFFFFu, d = en >> 16;
                if (d == PJ_SKIP || s_owner[f] < i) continue;   // the slot was taken by an earlier query of this call
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
                // :128-140: bestDist = smallest distance, first in list order; bestDist2 / bestLevel2 = the smallest among the
                // others, first in list order
                const int bestDist = k1 == PJ_NOKEY ? 256 : (int)(k1 >> 16), bestDist2 = k2 == PJ_NOKEY ? 256 : (int)(k2 >> 16);
                int mt = -1;
                if (bestDist <= a.th) {            // :143-148 / :1673
                    const int bestIdx = (int)(a.ent[o + (k1 & 0xFFFFu)] & 0xFFFFu);
                    bool reject = false;
                    if (a.ratio_rule) {
                        const int bestLevel = a.octF[(size_t)a.os * bestIdx];
                        const int bestLevel2 = k2 == PJ_NOKEY ? -1 : a.octF[(size_t)a.os * (a.ent[o + (k2 & 0xFFFFu)] & 0xFFFFu)];
                        reject = bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(a.nnratio, (float)bestDist2);
                    }
                    if (!reject) mt = bestIdx;
                }
                if (mt != a.match[i]) {
                    a.match[i] = mt;
                    changed = true;
                }
                a.best[i] = bestDist;
                a.second[i] = bestDist2;
            }
        }
        if (changed) s_changed = 1;
        __syncthreads();
        if (!s_changed) break;                 // workgroup-uniform
        for (int f = tid; f < nF; f += PJ_T) s_owner[f] = 0x7FFFFFFF;
        __syncthreads();
        for (int i = tid; i < nq; i += PJ_T) {
            const int mt = a.match[i];
            if (mt >= 0 && (a.q[i].flags & ORBFE_PROJ_CLAIMS)) atomicMin(&s_owner[mt], i);
        }
        __syncthreads();
    }
    if (tid == 0) a.status[1] = round + 1;
}


// ---------------------------------------------------------------------------------------------------
// The search in TWO launches instead of four and a copy (the per-frame members of Tracking are launch-bound: count -> scan -> fill ->
// resolve plus a result copy cost more than their kernels).  Same arithmetic, same fixed point:
//   * every query's wave walks its cell rectangle twice inside the launch (count, then fill -- the second walk finds its lines
//     in the cache) and writes its entries into a fixed slab of PJ_SLAB slots at i * PJ_SLAB: no scan over the queries, no
//     second launch.  A query with more candidates raises need[] and the host takes the four-kernel path (below) instead.
//   * while it fills, the wave already reduces the two smallest keys: round 0 of the relaxation (owner table empty) is decided
//     here, spread over the chip, for every query at once.
//   * a second, one-workgroup launch (k_proj_rounds) runs the remaining rounds.  A query re-scans its entries in
//     a round only if it has to: when the slot of its best or of its second-best candidate is now owned by an earlier query, or
//     when it ever skipped an owned slot (that slot may have been freed).  Every other query's two smallest free keys are what
//     they were, so its choice is what a full re-scan would return: the rounds and their results are those of k_proj_resolve.
//     On real frames a few dozen of ~800 queries re-scan.
//   * results go straight to page-locked host memory (match | best | second | status): two launches, no copy back, one wait.
// ---------------------------------------------------------------------------------------------------
#define PJ_SLAB 512
#define PJ_FT 256                // threads per workgroup of k_proj_fused: one wave per query
struct ProjFusedArgs {
    ProjArgs a;
    int32_t *f12;                // [2 * nq] feature of the best / second-best free candidate (-1: none)
    uint8_t *constrained;        // [nq] the query skipped an owned slot in its last scan
    uint32_t *done;              // [1] largest candidate count above PJ_SLAB (0: none); reset by k_proj_rounds
    int32_t *h_out;              // mapped host: match[nq] | best[nq] | second[nq] | status[2]
};

__global__ __launch_bounds__(PJ_FT) void k_proj_fused(ProjFusedArgs p)
{
    const ProjArgs &a = p.a;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nq = a.nq;
    {
        const int i = blockIdx.x * (PJ_FT / 64) + wv;
        if (i < nq) {   // wave-uniform
            const orbfe_proj_query Q = a.q[i];
            ProjRect R;
            const bool any = proj_rect(a, Q, R);
            const int n = proj_walk_count(a, Q, R, any, lane);
            const int incl = wave_incl_scan_m(n);
            const int tot = __shfl(incl, 63, 64);
            uint32_t k1 = PJ_NOKEY, k2 = PJ_NOKEY;
            int f1 = -1, f2 = -1;
            if (tot > PJ_SLAB) {
                if (lane == 0) atomicMax(&p.done[1], (uint32_t)tot);
            } else if (tot > 0) {
                uint32_t o = (uint32_t)(incl - n);
                uint32_t *ent = a.ent + (size_t)i * PJ_SLAB;
                const Desc8 dq = load_desc8(a.qdesc + (int64_t)i * 32);
                proj_walk(a, Q, R, lane, [&](uint32_t f) {
                    const bool skip = proj_gate_skip(a, Q, f, 1, a.inv_sigma2 != nullptr, [&](int lv) { return a.inv_sigma2[lv]; });
                    const uint32_t d = proj_dist(a, dq, f, skip);
                    ent[o] = f | (d << 16);
                    if (!skip) {
                        const uint32_t key = (d << 16) | o;
                        if (key < k1) { k2 = k1; f2 = f1; k1 = key; f1 = (int)f; }
                        else if (key < k2) { k2 = key; f2 = (int)f; }
                    }
                    ++o;
                });
                proj_reduce2<64>(k1, f1, k2, f2);
            }
            if (lane == 0) {
                int bd, bd2;
                a.match[i] = proj_decide(a, k1, k2, f1, f2, bd, bd2);   // round 0: every slot free
                a.best[i] = bd;
                a.second[i] = bd2;
                a.cnt[i] = (uint32_t)min(tot, PJ_SLAB);
                p.f12[2 * i] = f1;
                p.f12[2 * i + 1] = f2;
                p.constrained[i] = 0;
            }
        }
    }
}

// the remaining rounds, ONE workgroup, launched behind k_proj_fused (the launch boundary makes the slabs visible; an in-kernel
// hand-over to "the last workgroup to arrive" was measured: the agent-scope fences cost more than the launch, 95 against 82 us).
// One workgroup is latency, not throughput: every dependent trip to memory is a microsecond.  The per-query state (choice, the
// features of the two smallest free keys, flags, distances, list length) is therefore read ONCE into LDS, the rounds run on LDS
// alone except for the entries of the queries that re-scan, and the results leave from LDS; 1024 threads (64 queries re-scan at
// a time).  Round-5 form: three global phases per round with 256 threads, 47 us for 786 queries.
#define PJ_RT 1024
#define PJ_ROUNDS_WORDS 8        // LDS words per query: list, match, f1, f2, flags, best, second, cnt
__global__ __launch_bounds__(PJ_RT) void k_proj_rounds(ProjFusedArgs p)
{
    extern __shared__ int32_t s_dyn[];     // [nF] owner table, then PJ_ROUNDS_WORDS arrays of [nq]
    __shared__ int s_changed, s_nlist;
    const ProjArgs &a = p.a;
    const int tid = threadIdx.x;
    const int nq = a.nq, nF = a.nF;
    int32_t *s_owner = s_dyn, *s_list = s_dyn + nF, *s_match = s_list + nq, *s_f1 = s_match + nq, *s_f2 = s_f1 + nq;
    int32_t *s_flag = s_f2 + nq, *s_best = s_flag + nq, *s_second = s_best + nq, *s_cnt = s_second + nq;
    const uint32_t need = p.done[1];
    for (int i = tid; i < nq; i += PJ_RT) {
        s_match[i] = a.match[i];
        s_f1[i] = p.f12[2 * i];
        s_f2[i] = p.f12[2 * i + 1];
        s_flag[i] = (a.q[i].flags & ORBFE_PROJ_CLAIMS) ? 1 : 0;   // bit 0: the query claims its slot; bit 1: it skipped an owned slot in its last scan
        s_best[i] = a.best[i];
        s_second[i] = a.second[i];
        s_cnt[i] = (int32_t)a.cnt[i];
    }
    int round = 1;
    if (need == 0) {
        for (; round <= nq + 2; ++round) {
            for (int f = tid; f < nF; f += PJ_RT) s_owner[f] = 0x7FFFFFFF;
            if (tid == 0) { s_changed = 0; s_nlist = 0; }
            __syncthreads();
            for (int i = tid; i < nq; i += PJ_RT) {
                const int mt = s_match[i];
                if (mt >= 0 && (s_flag[i] & 1)) atomicMin(&s_owner[mt], i);
            }
            __syncthreads();
            for (int i = tid; i < nq; i += PJ_RT) {
                const int f1 = s_f1[i], f2 = s_f2[i];
                if ((s_flag[i] & 2) || (f1 >= 0 && s_owner[f1] < i) || (f2 >= 0 && s_owner[f2] < i)) s_list[atomicAdd(&s_nlist, 1)] = i;
            }
            __syncthreads();
            const int nl = s_nlist;
            if (nl == 0) break;               // workgroup-uniform
            const int sub = tid % PJ_L, grp = tid / PJ_L;
            bool changed = false;
            for (int l0 = 0; l0 < nl; l0 += PJ_RT / PJ_L) {
                const int li = l0 + grp;
                const int i = li < nl ? s_list[li] : -1;
                uint32_t k1 = PJ_NOKEY, k2 = PJ_NOKEY;
                int f1 = -1, f2 = -1;
                bool skipped = false;
                if (i >= 0) {
                    const uint32_t *ent = a.ent + (size_t)i * PJ_SLAB;
                    const uint32_t e = (uint32_t)s_cnt[i];
                    for (uint32_t k = sub; k < e; k += PJ_L) {
                        const uint32_t en = ent[k];
                        const uint32_t f = en & 0xFFFFu, d = en >> 16;
                        if (d == PJ_SKIP) continue;
                        if (s_owner[f] < i) { skipped = true; continue; }   // taken by an earlier query of this call
                        const uint32_t key = (d << 16) | k;
                        if (key < k1) { k2 = k1; f2 = f1; k1 = key; f1 = (int)f; }
                        else if (key < k2) { k2 = key; f2 = (int)f; }
                    }
                }
                proj_reduce2<PJ_L>(k1, f1, k2, f2);
#pragma unroll
                for (int s = PJ_L / 2; s > 0; s >>= 1) skipped = skipped || __shfl_xor((int)skipped, s, PJ_L) != 0;
                if (i >= 0 && sub == 0) {
                    int bd, bd2;
                    const int mt = proj_decide(a, k1, k2, f1, f2, bd, bd2);
                    if (mt != s_match[i]) {
                        s_match[i] = mt;
                        changed = true;
                    }
                    s_best[i] = bd;
                    s_second[i] = bd2;
                    s_f1[i] = f1;
                    s_f2[i] = f2;
                    s_flag[i] = (s_flag[i] & 1) | (skipped ? 2 : 0);
                }
            }
            if (changed) s_changed = 1;
            __syncthreads();
            if (!s_changed) break;            // workgroup-uniform
            __syncthreads();
        }
    }
    __syncthreads();
    // results to the host; the counters back to zero for the next call
    for (int i = tid; i < nq; i += PJ_RT) {
        p.h_out[i] = s_match[i];
        p.h_out[nq + i] = s_best[i];
        p.h_out[2 * (size_t)nq + i] = s_second[i];
    }
    if (tid == 0) {
        p.h_out[3 * (size_t)nq] = (int32_t)need;   // > 0: some query has that many candidates; nothing above is valid
        p.h_out[3 * (size_t)nq + 1] = round + 1;
        p.done[1] = 0u;
    }
}

extern "C" orbfe_status orbfe_search_by_projection_chi2(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF,
                                                        int32_t nF, const uint32_t *cell_off, const uint32_t *cell_idx, float minx,
                                                        float miny, float gw_inv, float gh_inv, const float *uRight,
                                                        const uint8_t *blocked, const float *inv_level_sigma2, int32_t nlevels,
                                                        const orbfe_proj_query *q, const uint8_t *qdesc,
                                                        int32_t nq, int32_t th, float nnratio, int32_t ratio_rule, int32_t *match,
                                                        int32_t *best, int32_t *second)
{
    if (inv_level_sigma2 && (nlevels < 1 || nlevels > 64)) {
        orbfe_set_error("bad argument to orbfe_search_by_projection_chi2");
        return ORBFE_ERR_ARG;
    }
    if (!m || nF < 0 || nq < 0 || !cell_off || (nq > 0 && (!q || !qdesc || !match)) || (nF > 0 && (!descF || !xyF || !octF)) ||
        (cell_off[GRID_NC] > 0 && !cell_idx)) {   // an empty grid (no keypoint inside the image bounds) has no cell_idx
        orbfe_set_error("bad argument to orbfe_search_by_projection");
        return ORBFE_ERR_ARG;
    }
    if (nF > PJ_MAX_NF) { orbfe_set_error("orbfe_search_by_projection: at most %d frame features", PJ_MAX_NF); return ORBFE_ERR_SIZE; }
    if (th > 255) { orbfe_set_error("orbfe_search_by_projection: th must be below 256 (256 is the 'no candidate' distance)"); return ORBFE_ERR_ARG; }
    if (!orb_grid_csr_ok(cell_off, cell_idx, nF, "nF")) return ORBFE_ERR_ARG;
    if (nq == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));
    // One pinned staging block in, one out: the per-frame call is latency-bound, nine pageable copies cost more than the kernels
    const StagePiece in[10] = {{descF, (size_t)nF * 32}, {xyF, (size_t)nF * 8}, {octF, (size_t)nF * 4}, {cell_off, (size_t)(GRID_NC + 1) * 4},
                               {cell_idx, (size_t)cell_off[GRID_NC] * 4}, {uRight, uRight ? (size_t)nF * 4 : 0}, {blocked, blocked ? (size_t)nF : 0},
                               {q, (size_t)nq * sizeof(orbfe_proj_query)}, {qdesc, (size_t)nq * 32},
                               {inv_level_sigma2, inv_level_sigma2 ? (size_t)nlevels * 4 : 0}};
    const char *din[10];
    const size_t out_bytes = (size_t)nq * 12 + 8;   // match | best | second | status[2]
    ORBFE_HIP(m->pin_out.ensure(out_bytes));
    ORBFE_HIP(m->b[1].ensure(out_bytes));
    ORBFE_HIP(m->b[2].ensure((size_t)nq * 4));                 // cnt
    ORBFE_HIP(m->b[3].ensure((size_t)nq * PJ_LC * 2));         // lcnt
    ORBFE_HIP(m->b[4].ensure((size_t)(nq + 1) * 4));           // off
    ORBFE_HIP(stage_upload(m, st, in, din));
    ProjArgs a;
    a.descF = (const uint8_t *)din[0];
    a.xyF = (const float *)din[1];
    a.octF = (const int32_t *)din[2];
    a.nF = nF; a.xs = 2; a.os = 1;
    a.cell_off = (const uint32_t *)din[3];
    a.cell_idx = (const uint32_t *)din[4];
    a.minx = minx; a.miny = miny; a.gwi = gw_inv; a.ghi = gh_inv;
    a.uRight = uRight ? (const float *)din[5] : nullptr;
    a.blocked = blocked ? (const uint8_t *)din[6] : nullptr;
    a.inv_sigma2 = inv_level_sigma2 ? (const float *)din[9] : nullptr;
    a.nlevels = nlevels;
    a.q = (const orbfe_proj_query *)din[7];
    a.qdesc = (const uint8_t *)din[8];
    a.nq = nq; a.th = th; a.ratio_rule = ratio_rule ? 1 : 0; a.nnratio = nnratio;
    a.match = m->b[1].as<int32_t>();
    a.best = a.match + nq;
    a.second = a.match + 2 * (size_t)nq;
    a.status = a.match + 3 * (size_t)nq;
    a.cnt = m->b[2].as<uint32_t>();
    a.lcnt = m->b[3].as<uint16_t>();
    a.off = m->b[4].as<uint32_t>();
    const int32_t *hout = m->pin_out.as<const int32_t>();
    auto results_out = [&] {
        memcpy(match, hout, (size_t)nq * 4);
        if (best) memcpy(best, hout + nq, (size_t)nq * 4);
        if (second) memcpy(second, hout + 2 * (size_t)nq, (size_t)nq * 4);
        return ORBFE_OK;
    };
    // ONE launch (k_proj_fused) when the owner table and the re-scan list fit the LDS and no query overflows its slab; else (or on
    // overflow, reported in status[0]) the four-kernel path below
    const size_t fused_lds = ((size_t)std::max(nF, 1) + (size_t)PJ_ROUNDS_WORDS * (size_t)nq) * 4;
    if (m->proj_fused && fused_lds <= 64 * 1024) {
        ORBFE_HIP(m->b[5].ensure((size_t)nq * PJ_SLAB * 4));
        ORBFE_HIP(m->b[6].ensure((size_t)nq * 8));
        ORBFE_HIP(m->b[7].ensure((size_t)nq));
        if (!m->proj_done.p) {
            ORBFE_HIP(m->proj_done.ensure(256));
            ORBFE_HIP(hipMemsetAsync(m->proj_done.p, 0, 256, st));   // the kernel leaves its counters at zero
        }
        ProjFusedArgs fa;
        fa.a = a;
        fa.a.ent = m->b[5].as<uint32_t>();
        fa.a.ent_cap = 0xFFFFFFFFu;
        fa.f12 = m->b[6].as<int32_t>();
        fa.constrained = m->b[7].as<uint8_t>();
        fa.done = m->proj_done.as<uint32_t>();
        fa.h_out = m->pin_out.as<int32_t>();   // page-locked and mapped: the kernel stores the results there
        const int nwg = (nq + PJ_FT / 64 - 1) / (PJ_FT / 64);
        hipLaunchKernelGGL(k_proj_fused, dim3(nwg), dim3(PJ_FT), 0, st, fa);
        hipLaunchKernelGGL(k_proj_rounds, dim3(1), dim3(PJ_RT), fused_lds, st, fa);
        ORBFE_HIP(hipGetLastError());
        ORBFE_HIP(hipStreamSynchronize(st));
        if (hout[3 * (size_t)nq] == 0) return results_out();
    }
    const int ngrp = (nq * PJ_LC + 255) / 256;
    size_t ent_cap = std::max<size_t>((size_t)nq * 96, 1 << 16);
    for (int attempt = 0; attempt < 2; ++attempt) {
        ORBFE_HIP(m->b[5].ensure(ent_cap * 4));
        a.ent = m->b[5].as<uint32_t>();
        a.ent_cap = (uint32_t)std::min<size_t>(m->b[5].bytes / 4, 0xFFFFFFFFu);
        if (attempt == 0) {
            hipLaunchKernelGGL(k_proj_count, dim3(ngrp), dim3(256), 0, st, a);
            orbfe_internal_launch_scan_u32((const uint32_t *)a.cnt, nq, a.off, st);
        }
        hipLaunchKernelGGL(k_proj_fill, dim3(ngrp), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_proj_resolve, dim3(1), dim3(PJ_T), (size_t)std::max(nF, 1) * 4, st, a);
        ORBFE_HIP(hipGetLastError());
        ORBFE_HIP(hipMemcpyAsync(m->pin_out.p, m->b[1].p, out_bytes, hipMemcpyDeviceToHost, st));
        ORBFE_HIP(hipStreamSynchronize(st));
        const int32_t need = hout[3 * (size_t)nq];
        if (need == 0) break;
        if (attempt == 1) { orbfe_set_error("candidate scratch still too small (%d entries)", need); return ORBFE_ERR_NOMEM; }
        ent_cap = (size_t)need;   // the exact need: the second launch cannot fail on it
    }
    return results_out();
}

// The first two stages of the projection search on their own: GetFeaturesInArea for every query and the Hamming distance of
// every candidate, handed back as lists (entry = feature | distance << 16, in the reference's candidate order).  For callers
// whose acceptance rule is sequential in a way the device core does not implement (SearchForInitialization :571-574).
extern "C" orbfe_status orbfe_window_distances(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF, int32_t nF,
                                               const uint32_t *cell_off, const uint32_t *cell_idx, float minx, float miny, float gw_inv,
                                               float gh_inv, const orbfe_proj_query *q, const uint8_t *qdesc, int32_t nq, uint32_t *off,
                                               uint32_t *ent, int32_t cap)
{
    if (!m || nF < 0 || nq < 0 || cap < 0 || !cell_off || !off || (nq > 0 && (!q || !qdesc)) || (nF > 0 && (!descF || !xyF || !octF)) ||
        (cell_off[GRID_NC] > 0 && !cell_idx) || (cap > 0 && !ent)) {
        orbfe_set_error("bad argument to orbfe_window_distances");
        return ORBFE_ERR_ARG;
    }
    if (nF > 65535) { orbfe_set_error("orbfe_window_distances: at most 65535 features (16-bit index in an entry)"); return ORBFE_ERR_SIZE; }
    if (!orb_grid_csr_ok(cell_off, cell_idx, nF, "nF")) return ORBFE_ERR_ARG;
    off[0] = 0;
    if (nq == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const StagePiece in[7] = {{descF, (size_t)nF * 32}, {xyF, (size_t)nF * 8}, {octF, (size_t)nF * 4}, {cell_off, (size_t)(GRID_NC + 1) * 4},
                              {cell_idx, (size_t)cell_off[GRID_NC] * 4}, {q, (size_t)nq * sizeof(orbfe_proj_query)}, {qdesc, (size_t)nq * 32}};
    const char *din[7];
    ORBFE_HIP(m->b[2].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[3].ensure((size_t)nq * PJ_LC * 2));
    ORBFE_HIP(m->b[4].ensure((size_t)(nq + 1) * 4));
    ORBFE_HIP(m->b[5].ensure(std::max<size_t>((size_t)cap, 1) * 4));
    ORBFE_HIP(stage_upload(m, st, in, din));
    ProjArgs a;
    memset(&a, 0, sizeof(a));
    a.descF = (const uint8_t *)din[0];
    a.xyF = (const float *)din[1];
    a.octF = (const int32_t *)din[2];
    a.nF = nF; a.xs = 2; a.os = 1;
    a.cell_off = (const uint32_t *)din[3];
    a.cell_idx = (const uint32_t *)din[4];
    a.minx = minx; a.miny = miny; a.gwi = gw_inv; a.ghi = gh_inv;
    a.q = (const orbfe_proj_query *)din[5];
    a.qdesc = (const uint8_t *)din[6];
    a.nq = nq;
    a.cnt = m->b[2].as<uint32_t>();
    a.lcnt = m->b[3].as<uint16_t>();
    a.off = m->b[4].as<uint32_t>();
    a.ent = m->b[5].as<uint32_t>();
    a.ent_cap = (uint32_t)cap;
    const int ngrp = (nq * PJ_LC + 255) / 256;
    hipLaunchKernelGGL(k_proj_count, dim3(ngrp), dim3(256), 0, st, a);
    orbfe_internal_launch_scan_u32((const uint32_t *)a.cnt, nq, a.off, st);
    hipLaunchKernelGGL(k_proj_fill, dim3(ngrp), dim3(256), 0, st, a);   // writes nothing when the total exceeds cap
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(off, a.off, (size_t)(nq + 1) * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    if (off[nq] > (uint32_t)cap) { orbfe_set_error("orbfe_window_distances: %u entries needed, cap %d", off[nq], cap); return ORBFE_ERR_CAP; }
    if (off[nq] > 0) {
        ORBFE_HIP(hipMemcpyAsync(ent, a.ent, (size_t)off[nq] * 4, hipMemcpyDeviceToHost, st));
        ORBFE_HIP(hipStreamSynchronize(st));
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_search_by_projection(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF,
                                                   int32_t nF, const uint32_t *cell_off, const uint32_t *cell_idx, float minx,
                                                   float miny, float gw_inv, float gh_inv, const float *uRight,
                                                   const uint8_t *blocked, const orbfe_proj_query *q, const uint8_t *qdesc,
                                                   int32_t nq, int32_t th, float nnratio, int32_t ratio_rule, int32_t *match,
                                                   int32_t *best, int32_t *second)
{
    return orbfe_search_by_projection_chi2(m, descF, xyF, octF, nF, cell_off, cell_idx, minx, miny, gw_inv, gh_inv, uRight, blocked,
                                           nullptr, 0, q, qdesc, nq, th, nnratio, ratio_rule, match, best, second);
}

// ---------------------------------------------------------------------------------------------------
// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:827-1012, LocalMapping::CreateNewMapPoints), the
// matching core.  The reference's loop never sets vbMatched2, so the features of keyframe 1 are independent: one thread per
// keyframe-1 feature scans its vocabulary node's features of keyframe 2 in FeatureVector order -- Hamming first, then the
// epipole gate and CheckDistEpipolarLine (:175-196) in the reference's float operation order -- and keeps the smallest
// distance, the LAST in order on ties (`dist > bestDist` skips, an equal distance takes over).
// ---------------------------------------------------------------------------------------------------
struct TriArgs {
    const uint8_t *desc1, *desc2;
    const float *xy1, *xy2;
    const int32_t *oct2;
    const uint8_t *elig1, *stereo1, *elig2, *stereo2;
    const int32_t *range1;      // [n1][2]: the node's slice of idx2 for every keyframe-1 feature, (0, 0) = none
    const uint32_t *idx2;
    float F[9], ex, ey;
    const float *scale2, *sigma2_2;
    int32_t n1, th_low;
    int32_t *match12;
};

// keyframe-2 feature f of the call, as tri_candidate reads it
struct TriGlobalCand {
    const TriArgs &a;
    uint32_t f;
    __device__ __forceinline__ bool elig() const { return a.elig2[f] != 0; }
    __device__ __forceinline__ const uint32_t *desc() const { return (const uint32_t *)(a.desc2 + (int64_t)f * 32); }
    __device__ __forceinline__ float x() const { return a.xy2[2 * f]; }
    __device__ __forceinline__ float y() const { return a.xy2[2 * f + 1]; }
    __device__ __forceinline__ bool stereo() const { return a.stereo2[f] != 0; }
    __device__ __forceinline__ float scale() const { return a.scale2[a.oct2[f]]; }
    __device__ __forceinline__ float sigma2() const { return a.sigma2_2[a.oct2[f]]; }
};

__global__ __launch_bounds__(256) void k_triangulation(TriArgs a)
{
    const int f1 = blockIdx.x * 256 + threadIdx.x;
    if (f1 >= a.n1) return;
    int best = -1;
    const int lo = a.range1[2 * f1], hi = a.range1[2 * f1 + 1];
    if (hi > lo && a.elig1[f1]) {
        const Desc8 d1 = load_desc8(a.desc1 + (int64_t)f1 * 32);
        const bool st1 = a.stereo1[f1] != 0;
        const TriLine l = tri_line(a.xy1[2 * f1], a.xy1[2 * f1 + 1], a.F);
        int bestDist = a.th_low;   // never above th_low: `dist > bestDist` is the whole of :895
        for (int i2 = lo; i2 < hi; ++i2) {
            const uint32_t f2 = a.idx2[i2];
            const int dist = tri_candidate(d1, st1, l, a.ex, a.ey, bestDist, TriGlobalCand{a, f2});
            if (dist >= 0) {
                best = (int)f2;
                bestDist = dist;
            }
        }
    }
    a.match12[f1] = best;
}

extern "C" orbfe_status orbfe_search_for_triangulation(orbfe_matcher *m, const uint8_t *desc1, const float *xy1, const uint8_t *elig1,
                                                       const uint8_t *stereo1, int32_t n1, const uint32_t *node1, const uint32_t *off1,
                                                       const uint32_t *idx1, int32_t nn1, const uint8_t *desc2, const float *xy2,
                                                       const int32_t *oct2, const uint8_t *elig2, const uint8_t *stereo2, int32_t n2,
                                                       const uint32_t *node2, const uint32_t *off2, const uint32_t *idx2, int32_t nn2,
                                                       const float F12[9], float ex, float ey, const float *scale_factors2,
                                                       const float *level_sigma2_2, int32_t nlevels2, int32_t th_low, int32_t *match12)
{
    if (!m || n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || nlevels2 < 1 || !F12 || !scale_factors2 || !level_sigma2_2 ||
        (n1 > 0 && (!desc1 || !xy1 || !elig1 || !stereo1 || !match12)) || (n2 > 0 && (!desc2 || !xy2 || !oct2 || !elig2 || !stereo2)) ||
        (nn1 > 0 && (!node1 || !off1 || !idx1)) || (nn2 > 0 && (!node2 || !off2 || !idx2))) {
        orbfe_set_error("bad argument to orbfe_search_for_triangulation");
        return ORBFE_ERR_ARG;
    }
    if (n1 == 0) return ORBFE_OK;
    for (int i = 0; i < n2; ++i)
        if (oct2[i] < 0 || oct2[i] >= nlevels2) { orbfe_set_error("keyframe-2 octave out of range"); return ORBFE_ERR_ARG; }
    // the merge walk over the two FeatureVectors (:849-964) on the host: every keyframe-1 feature learns its node's slice of idx2
    std::vector<int32_t> range((size_t)n1 * 2, 0);
    const uint32_t total2 = nn2 > 0 ? off2[nn2] : 0;
    for (uint32_t k = 0; k < total2; ++k)
        if (idx2[k] >= (uint32_t)n2) { orbfe_set_error("FeatureVector 2 index out of range"); return ORBFE_ERR_ARG; }
    {
        int a = 0, b = 0;
        while (a < nn1 && b < nn2) {
            if (node1[a] == node2[b]) {
                for (uint32_t k = off1[a]; k < off1[a + 1]; ++k) {
                    if (idx1[k] >= (uint32_t)n1) { orbfe_set_error("FeatureVector 1 index out of range"); return ORBFE_ERR_ARG; }
                    range[2 * (size_t)idx1[k]] = (int32_t)off2[b];
                    range[2 * (size_t)idx1[k] + 1] = (int32_t)off2[b + 1];
                }
                ++a;
                ++b;
            } else if (node1[a] < node2[b]) ++a;
            else ++b;
        }
    }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));
    const StagePiece in[12] = {{desc1, (size_t)n1 * 32}, {xy1, (size_t)n1 * 8}, {elig1, (size_t)n1}, {stereo1, (size_t)n1},
                               {range.data(), (size_t)n1 * 8}, {desc2, (size_t)n2 * 32}, {xy2, (size_t)n2 * 8}, {oct2, (size_t)n2 * 4},
                               {elig2, (size_t)n2}, {stereo2, (size_t)n2}, {idx2, (size_t)total2 * 4},
                               {scale_factors2, (size_t)nlevels2 * 4, level_sigma2_2, (size_t)nlevels2 * 4}};   // the level tables share a piece
    const char *d[12];
    ORBFE_HIP(m->pin_out.ensure((size_t)n1 * 4));
    ORBFE_HIP(m->b[1].ensure((size_t)n1 * 4));
    ORBFE_HIP(stage_upload(m, st, in, d));
    TriArgs a;
    a.desc1 = (const uint8_t *)d[0];
    a.xy1 = (const float *)d[1];
    a.elig1 = (const uint8_t *)d[2];
    a.stereo1 = (const uint8_t *)d[3];
    a.range1 = (const int32_t *)d[4];
    a.desc2 = (const uint8_t *)d[5];
    a.xy2 = (const float *)d[6];
    a.oct2 = (const int32_t *)d[7];
    a.elig2 = (const uint8_t *)d[8];
    a.stereo2 = (const uint8_t *)d[9];
    a.idx2 = (const uint32_t *)d[10];
    a.scale2 = (const float *)d[11];
    a.sigma2_2 = a.scale2 + nlevels2;
    for (int k = 0; k < 9; ++k) a.F[k] = F12[k];
    a.ex = ex; a.ey = ey;
    a.n1 = n1; a.th_low = th_low;
    a.match12 = m->pin_out.as<int32_t>();   // page-locked and mapped: the kernel stores its 4 n1 result bytes there, no copy back
    hipLaunchKernelGGL(k_triangulation, dim3((n1 + 255) / 256), dim3(256), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipStreamSynchronize(st));
    memcpy(match12, m->pin_out.p, (size_t)n1 * 4);
    return ORBFE_OK;
}
