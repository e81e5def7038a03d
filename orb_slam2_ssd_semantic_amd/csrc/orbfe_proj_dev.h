// orbfe_proj_dev.h -- the device side of the projection-gated search that orbfe_projection.hip (one frame, host buffers) and
// orbfe_track.hip (a batch of frames, device-resident) share: the argument block, the cell rectangle of GetFeaturesInArea and the
// walk over it.  The library is built without relocatable device code, so every kernel gets its own inlined copy.
#pragma once

#include "orbfe_common.h"
#include "orbfe_match_dev.h"

#define PJ_T 1024
#define PJ_L 16                  // lanes per query in the relaxation rounds
#define PJ_LC 64                 // lanes per query in the candidate search (one wave: a search window covers ~100 grid cells)
#define PJ_SKIP 0x1FFu           // distance field of an entry whose slot is blocked before the call / fails the right-image gate
#define PJ_MAX_NF 15360          // owner table in LDS (int32 per frame feature)
struct ProjArgs {
    const uint8_t *descF;
    const float *xyF;
    const int32_t *octF;
    int32_t nF, xs, os;          // xs / os: floats / ints between consecutive points (2 / 1 packed, 7 / 7 keypoint records)
    const uint32_t *cell_off, *cell_idx;
    float minx, miny, gwi, ghi;
    const float *uRight;         // may be null
    const uint8_t *blocked;      // may be null
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
