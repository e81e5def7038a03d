// orbfe_match_dev.h -- the device helpers the matcher's translation units share (orbfe_match.hip, orbfe_grid.hip,
// orbfe_projection.hip, orbfe_stereo.hip, orbfe_bow.hip).  The library is built without relocatable device code, so every
// kernel gets its own inlined copy.
#pragma once

#include "orbfe_common.h"

// cells of the frame grid (orbfe_grid.hip builds it, orbfe_projection.hip walks it)
#define GRID_NC (ORBFE_GRID_COLS * ORBFE_GRID_ROWS)

struct Desc8 {
    uint32_t w[8];
};

__device__ __forceinline__ int hamming8(const Desc8 &a, const uint32_t *__restrict__ b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += __popc(a.w[i] ^ b[i]);
    return d;
}

struct Best2 {
    int best, second, idx;
};

// merge of two partial results where `lo` covers the earlier iteration positions (first minimum wins)
__device__ __forceinline__ Best2 merge_best2(const Best2 &lo, const Best2 &hi)
{
    Best2 r;
    if (hi.best < lo.best) {
        r.best = hi.best;
        r.idx = hi.idx;
        r.second = min(lo.best, hi.second);
    } else {
        r.best = lo.best;
        r.idx = lo.idx;
        r.second = min(lo.second, hi.best);
    }
    return r;
}

// ORBmatcher.cc:308-313: rot = a1 - a2 (+360 if < 0); bin = round(rot * (1/HISTO_LENGTH)) (sic)
__device__ __forceinline__ int rot_bin(float a1, float a2)
{
    const float factor = 1.0f / ORBFE_HISTO_LENGTH;
    float rot = __fsub_rn(a1, a2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, factor));
    if (bin == ORBFE_HISTO_LENGTH) bin = 0;
    return bin;
}
