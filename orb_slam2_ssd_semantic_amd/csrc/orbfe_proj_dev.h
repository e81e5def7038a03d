// orbfe_proj_dev.h -- the device side of the projection-gated search, once, for orbfe_projection.hip (one frame, host buffers) and
// orbfe_track.hip (a batch of frames, device-resident), in the order it runs: the argument block, the cell rectangle
// (proj_rect), the walk (proj_walk), the count (proj_count), the gates (proj_gate_skip) and the distance (proj_dist), the
// two-smallest merge (proj_reduce2), the acceptance rule (proj_decide).  The query descriptor is loaded with orbfe_match_dev.h's
// load_desc8.  Two things are NOT here, because shared they measured slower.  The relaxation rounds: k_proj_resolve and
// k_trk_resolve each keep their loop, which inside a shared inlined function compiled to a candidate scan 3 us slower
// (profiles/proj_core_shared.md).  The one-wave first-minimum search of k_fuse_search (orbfe_fuse.hip) and k_s3_search
// (orbfe_sim3_search.hip): each keeps its copy, since through one inlined function k_s3_search ran 5 % slower at 256 pairs
// (profiles/search_helpers_shared.md).
// At the end of the file stands the per-candidate test of SearchForTriangulation (tri_line, tri_candidate), for
// orbfe_projection.hip and orbfe_tri_search.hip.  No relocatable device code: every kernel gets its own inlined copy.
#pragma once

#include "orbfe_common.h"
#include "orbfe_match_dev.h"

#define PJ_T 1024
#define PJ_L 16                  // lanes per query in the relaxation rounds
#define PJ_LC 64                 // lanes per query in the candidate search (one wave: a search window covers ~100 grid cells)
#define PJ_SKIP 0x1FFu           // distance field of an entry whose slot is blocked before the call / fails the right-image gate
#define PJ_NOKEY 0xFFFFFFFFu     // "no candidate" in the reductions; a key is distance (9 bits) << 16 | position in the query's list
#define PJ_MAX_NF 15360          // owner table in LDS (int32 per frame feature)
struct ProjArgs {
    const uint8_t *descF;
    const float *xyF;
    const int32_t *octF;
    int32_t nF, xs, os;          // xs / os: floats / ints between consecutive points (2 / 1 packed, 7 / 7 keypoint records)
    const uint32_t *cell_off, *cell_idx;
    float minx, miny, gwi, ghi;
    const float *uRight;         // may be null
    const uint8_t *blocked;      // per feature, may be null; which values block is the form's (proj_gate_skip)
    const float *inv_sigma2;     // per level, may be null (ORBFE_PROJ_CHI2_GATE then never applies)
    int32_t nlevels;
    const orbfe_proj_query *q;
    const uint8_t *qdesc;
    int32_t nq, th, ratio_rule;
    float nnratio;
    int32_t *match, *best, *second;
    uint32_t *cnt;               // [nq] candidates per query
    uint16_t *lcnt;              // [nq * PJ_LC] candidates found by each lane of the query's wave
    uint32_t *off;               // [nq + 1]
    uint32_t *ent;               // [ent_cap] cand | dist << 16
    uint32_t ent_cap;
    int32_t *status;             // [0] = entries needed when ent_cap is too small (else 0), [1] = rounds run
};

// The cell rectangle of GetFeaturesInArea (:470-484) and the level filter; false = the query has no candidates
struct ProjRect {
    int x0, y0, nx, ny;
    bool check;
};
__device__ __forceinline__ bool proj_rect(const ProjArgs &a, const orbfe_proj_query &Q, ProjRect &R)
{
    int nminx = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.u, a.minx), Q.r), a.gwi));
    nminx = max(nminx, 0);
    if (nminx >= ORBFE_GRID_COLS) return false;
    int nmaxx = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.u, a.minx), Q.r), a.gwi));
    nmaxx = min(nmaxx, ORBFE_GRID_COLS - 1);
    if (nmaxx < 0) return false;
    int nminy = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.v, a.miny), Q.r), a.ghi));
    nminy = max(nminy, 0);
    if (nminy >= ORBFE_GRID_ROWS) return false;
    int nmaxy = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.v, a.miny), Q.r), a.ghi));
    nmaxy = min(nmaxy, ORBFE_GRID_ROWS - 1);
    if (nmaxy < 0) return false;
    R.x0 = nminx; R.y0 = nminy; R.nx = nmaxx - nminx + 1; R.ny = nmaxy - nminy + 1;
    R.check = (Q.min_level > 0) || (Q.max_level >= 0);  // :486
    return R.nx > 0 && R.ny > 0;
}

// Lane `sub` of a query's wave walks its contiguous share of the cell sequence (ix outer, iy inner: the reference's
// order), so lane order = candidate order.  f(k) is called for every feature that passes the level filter and the box test.
template <typename F>
__device__ __forceinline__ void proj_walk(const ProjArgs &a, const orbfe_proj_query &Q, const ProjRect &R, int sub, F f)
{
    const int ncell = R.nx * R.ny, chunk = (ncell + PJ_LC - 1) / PJ_LC;
    const int c0 = sub * chunk, c1 = min(c0 + chunk, ncell);
    for (int c = c0; c < c1; ++c) {
        const int ix = R.x0 + c / R.ny, iy = R.y0 + c % R.ny;
        const int cell = ix * ORBFE_GRID_ROWS + iy;
        for (uint32_t j = a.cell_off[cell]; j < a.cell_off[cell + 1]; ++j) {
            const uint32_t k = a.cell_idx[j];
            if (R.check) {
                const int o = a.octF[(size_t)a.os * k];
                if (o < Q.min_level) continue;
                if (Q.max_level >= 0 && o > Q.max_level) continue;
            }
            const float dx = __fsub_rn(a.xyF[(size_t)a.xs * k], Q.u), dy = __fsub_rn(a.xyF[(size_t)a.xs * k + 1], Q.v);
            if (fabsf(dx) < Q.r && fabsf(dy) < Q.r) f(k);
        }
    }
}

__device__ __forceinline__ int wave_incl_scan_m(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// the candidates lane `sub` of the query's wave finds (none when the query has no rectangle)
__device__ __forceinline__ int proj_walk_count(const ProjArgs &a, const orbfe_proj_query &Q, const ProjRect &R, bool any, int sub)
{
    int n = 0;
    if (any) proj_walk(a, Q, R, sub, [&](uint32_t) { ++n; });
    return n;
}

// The count pass of the wave of query g (size_t or int64_t): every lane's count goes to lcnt[g * PJ_LC + sub] (the fill pass
// places the lane's entries from them), the wave's total to cnt[g].
template <typename I>
__device__ __forceinline__ void proj_count(const ProjArgs &a, const orbfe_proj_query &Q, const ProjRect &R, bool any, int sub,
                                           uint16_t *lcnt, uint32_t *cnt, I g)
{
    const int n = proj_walk_count(a, Q, R, any, sub);
    lcnt[g * PJ_LC + sub] = (uint16_t)n;
    int tot = n;
#pragma unroll
    for (int o = PJ_LC / 2; o > 0; o >>= 1) tot += __shfl_xor(tot, o, PJ_LC);
    if (sub == 0) cnt[g] = (uint32_t)tot;
}

// Does candidate f of query Q get PJ_SKIP for a distance?  When its slot is blocked before the call (a.blocked[f] >= blocks_from:
// 1 for a table of flags, 2 for the tracker's slot states, where 1 is a MapPoint without observations) or a gate rejects it.
// inv_sigma2(level) reads the chi2 gate's table, a pointer in one form and a kernel-argument array in the other.
template <typename S>
__device__ __forceinline__ bool proj_gate_skip(const ProjArgs &a, const orbfe_proj_query &Q, uint32_t f, int blocks_from, bool has_sigma2,
                                               S inv_sigma2)
{
    bool skip = a.blocked && a.blocked[f] >= blocks_from;             // :108-110 / :1647-1649, state before the call
    if (!skip && (Q.flags & ORBFE_PROJ_RIGHT_GATE) && a.uRight) {     // :114-119 / :1654-1660
        const float ur = a.uRight[f];
        skip = ur > 0.f && fabsf(__fsub_rn(Q.ur, ur)) > Q.r;
    }
    if (!skip && (Q.flags & ORBFE_PROJ_CHI2_GATE) && has_sigma2) {    // Fuse :1112-1139: reprojection error against the level's sigma
        const float ex = __fsub_rn(Q.u, a.xyF[(size_t)a.xs * f]), ey = __fsub_rn(Q.v, a.xyF[(size_t)a.xs * f + 1]);
        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        const float kr = a.uRight ? a.uRight[f] : -1.f;
        const int lv = min(max(a.octF[(size_t)a.os * f], 0), a.nlevels - 1);
        double bound = 5.99;
        if (kr >= 0.f) {
            const float er = __fsub_rn(Q.ur, kr);
            e2 = __fadd_rn(e2, __fmul_rn(er, er));
            bound = 7.8;
        }
        skip = (double)__fmul_rn(e2, inv_sigma2(lv)) > bound;
    }
    return skip;
}

__device__ __forceinline__ uint32_t proj_dist(const ProjArgs &a, const Desc8 &dq, uint32_t f, bool skip)
{
    return skip ? PJ_SKIP : (uint32_t)hamming8(dq, (const uint32_t *)(a.descF + (int64_t)f * 32));
}

// ---------------------------------------------------------------------------------------------------
// SearchForTriangulation (src/ORBmatcher.cc:827-1012): the per-candidate test, once, for k_triangulation (orbfe_projection.hip,
// one pair on host buffers) and k_tri_search / k_tri_search_flat (orbfe_tri_search.hip, a batch of pairs).
// ---------------------------------------------------------------------------------------------------
// The epipolar line of a keyframe-1 keypoint in keyframe 2 (:175-182), F12 row-major, every operation rounded separately
struct TriLine {
    float a, b, c, den;          // den = a * a + b * b
};
__device__ __forceinline__ TriLine tri_line(float x1, float y1, const float *F)
{
    TriLine l;
    l.a = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[0]), __fmul_rn(y1, F[3])), F[6]);
    l.b = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[1]), __fmul_rn(y1, F[4])), F[7]);
    l.c = __fadd_rn(__fadd_rn(__fmul_rn(x1, F[2]), __fmul_rn(y1, F[5])), F[8]);
    l.den = __fadd_rn(__fmul_rn(l.a, l.a), __fmul_rn(l.b, l.b));
    return l;
}

// One candidate of one query: its Hamming distance when it passes every gate, -1 when it does not.  In the reference's order:
// eligibility (no MapPoint; stereo if bOnlyStereo), dist > limit (:895; limit = the running bestDist, or th_low where the caller
// takes the minimum itself), the epipole gate (:900-907) only when both keypoints are monocular -- closer than 100 * scale[octave]
// to the epipole, strict, is out --, CheckDistEpipolarLine (:175-196) with den == 0 -> no, and the double comparison against
// 3.84 * sigma2[octave].  The candidate `c` is read through its accessors -- elig(), desc(), x(), y(), stereo(), scale() and
// sigma2() of its level -- only where the reference reads it: global memory in one kernel, an LDS tile in the other.
template <typename C>
__device__ __forceinline__ int tri_candidate(const Desc8 &d1, bool stereo1, const TriLine &l, float ex, float ey, int limit, const C &c)
{
    if (!c.elig()) return -1;
    const int dist = hamming8(d1, c.desc());
    if (dist > limit) return -1;
    const float x2 = c.x(), y2 = c.y();
    if (!stereo1 && !c.stereo()) {
        const float dx = __fsub_rn(ex, x2), dy = __fsub_rn(ey, y2);
        if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.f, c.scale())) return -1;
    }
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(l.a, x2), __fmul_rn(l.b, y2)), l.c);
    if (l.den == 0.f) return -1;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), l.den);
    return (double)dsqr < __dmul_rn(3.84, (double)c.sigma2()) ? dist : -1;
}

// merge (k1, f1, k2, f2) with a partner's over `width` lanes: the two smallest keys and their features
template <int WIDTH>
__device__ __forceinline__ void proj_reduce2(uint32_t &k1, int &f1, uint32_t &k2, int &f2)
{
#pragma unroll
    for (int s = WIDTH / 2; s > 0; s >>= 1) {
        const uint32_t o1 = __shfl_xor(k1, s, WIDTH), o2 = __shfl_xor(k2, s, WIDTH);
        const int g1 = __shfl_xor(f1, s, WIDTH), g2 = __shfl_xor(f2, s, WIDTH);
        // keys are unique inside a query (the position is part of them), NOKEY excepted
        uint32_t hi;
        int fh;
        if (o1 < k1) { hi = k1; fh = f1; k1 = o1; f1 = g1; } else { hi = o1; fh = g1; }
        const uint32_t m2 = min(k2, o2);
        const int fm = k2 <= o2 ? f2 : g2;
        if (hi <= m2) { k2 = hi; f2 = fh; } else { k2 = m2; f2 = fm; }
    }
}

// The decision of :128-148 / :1673 from the two smallest keys of the free candidates and their features (read only where
// the key is not PJ_NOKEY): bestDist = the smallest distance, first in list order; bestDist2 = the smallest among the others,
// first in list order.  Returns the match or -1.
__device__ __forceinline__ int proj_decide(const ProjArgs &a, uint32_t k1, uint32_t k2, int f1, int f2, int &bestDist, int &bestDist2)
{
    bestDist = k1 == PJ_NOKEY ? 256 : (int)(k1 >> 16);
    bestDist2 = k2 == PJ_NOKEY ? 256 : (int)(k2 >> 16);
    if (bestDist > a.th) return -1;
    if (a.ratio_rule) {
        const int bestLevel = a.octF[(size_t)a.os * f1];
        const int bestLevel2 = k2 == PJ_NOKEY ? -1 : a.octF[(size_t)a.os * f2];
        if (bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(a.nnratio, (float)bestDist2)) return -1;
    }
    return f1;
}
