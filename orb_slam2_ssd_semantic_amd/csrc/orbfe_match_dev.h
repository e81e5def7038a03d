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

// ---------------------------------------------------------------------------------------------------
// The ranking key of k_match_bf (orbfe_match.hip, K8).  With every descriptor bit an FP4 (E2M1) +-1 on both sides and the
// E8M0 block scales 2^5 (train) and 2^0 (query), one accumulator of the scaled MFMA chain that started at
// bm_key_start(row) ends at the fp32 value
//     v = 32 * (256 - 2 d) + (32 - row) + BM_KEY_OFFSET            d = Hamming distance, row = train row inside the tile,
// an integer in [2^15, 2^16) for every reachable (d, row).  Inside one binade the fp32 bit pattern of an integer is linear:
//     bits = 0x47000000 + ((v - 2^15) << 8) = 0x47000000 + ((64 * (256 - d) + field) << 8),        field = 32 - row in 1..32,
// so the patterns, compared as plain integers, ARE the keys: larger = closer, the earlier row wins on equal distance.  No
// convert per distance; the ranking works on the patterns.  bits | BM_KEY_FORCE sets the field to 63: the key of an older
// tile, which beats every key of that distance and none of a smaller one.  BM_KEY_NONE (0) lies below all of them.
// ---------------------------------------------------------------------------------------------------
#define BM_FP4_POS 0x2u           // E2M1 +1.0
#define BM_FP4_NEG 0xAu           // E2M1 -1.0
#define BM_SCALE_TRAIN 0x84848484 // E8M0 2^5 in every byte (whichever byte the instruction selects)
#define BM_SCALE_QUERY 0x7F7F7F7F // E8M0 2^0
#define BM_KEY_MULT 32            // 2^5 * 1 * 1: what one agreeing bit adds to v
#define BM_KEY_OFFSET 40960       // 2^15 + 32 * 256: puts v(d = 256) just above 2^15
#define BM_KEY_BASE 0x47000000    // fp32 pattern of 2^15
#define BM_KEY_FORCE (63 << 8)
#define BM_KEY_NONE 0

__host__ __device__ constexpr int bm_key_value(int d, int row) { return BM_KEY_MULT * (256 - 2 * d) + (32 - row) + BM_KEY_OFFSET; }
__host__ __device__ constexpr float bm_key_start(int row) { return (float)(32 - row + BM_KEY_OFFSET); }
// the fp32 pattern of the integer v in [2^15, 2^16)
__host__ __device__ constexpr int bm_key_pattern(int v) { return BM_KEY_BASE + ((v - 32768) << 8); }
__host__ __device__ constexpr int bm_key_bits(int d, int row) { return bm_key_pattern(bm_key_value(d, row)); }
// distance part of a key, larger = closer (0 for BM_KEY_NONE, forced or not) ...
__host__ __device__ constexpr int bm_key_m(int bits) { return bits >> 14; }
// ... and back to the Hamming distance / the train row inside the tile
__host__ __device__ constexpr int bm_m_dist(int m) { return (BM_KEY_BASE >> 14) + 256 - m; }
__host__ __device__ constexpr int bm_key_dist(int bits) { return bm_m_dist(bm_key_m(bits)); }
__host__ __device__ constexpr int bm_key_row(int bits) { return 32 - ((bits >> 8) & 63); }

__host__ __device__ constexpr bool bm_key_in_binade(int bits) { return bits >= BM_KEY_BASE && bits < BM_KEY_BASE + (1 << 23); }
// every property the kernel relies on, for distance d and all 32 rows
__host__ __device__ constexpr bool bm_key_check(int d)
{
    for (int row = 0; row < 32; ++row) {
        const int v = bm_key_value(d, row), k = bm_key_bits(d, row), f = k | BM_KEY_FORCE;
        if (__builtin_bit_cast(int, (float)v) != k) return false;                        // the pattern is the fp32 of v
        if (__builtin_bit_cast(int, bm_key_start(row)) != bm_key_pattern(32 - row + BM_KEY_OFFSET)) return false;
        if (!bm_key_in_binade(k) || !bm_key_in_binade(f)) return false;                    // one binade, forced form included
        if (k <= BM_KEY_NONE || k <= (BM_KEY_NONE | BM_KEY_FORCE)) return false;           // the sentinel lies below
        if (bm_key_dist(k) != d || bm_key_row(k) != row || bm_key_dist(f) != d) return false;  // decode
        if (row < 31 && !(k > bm_key_bits(d, row + 1))) return false;                      // lower row first ...
        if (row == 31 && d < 256 && !(k > bm_key_bits(d + 1, 0))) return false;            // ... smaller distance before that
        if (!(f > bm_key_bits(d, 0)) || (f | BM_KEY_FORCE) != f) return false;             // forced beats the same distance,
        if (d > 0 && !(f < bm_key_bits(d - 1, 31))) return false;                          // and no smaller one
    }
    return true;
}
__host__ __device__ constexpr bool bm_key_check_all()
{
    for (int d = 0; d <= 256; ++d)
        if (!bm_key_check(d)) return false;
    return bm_key_m(BM_KEY_NONE) == 0 && bm_key_m(BM_KEY_NONE | BM_KEY_FORCE) == 0 && bm_key_m(bm_key_bits(256, 31)) > 0;
}
static_assert(bm_key_check_all(), "k_match_bf: the fp32 bit patterns of the accumulators do not rank as (distance, row) keys");

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
