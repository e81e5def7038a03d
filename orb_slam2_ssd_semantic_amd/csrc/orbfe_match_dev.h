// orbfe_match_dev.h -- the helpers the matcher's translation units share: the descriptor (Desc8, load_desc8, hamming8), the
// ranking key of k_match_bf, the two-smallest merge (merge_best2) and the rotation-consistency check of the reference, stated
// once: the bin (rot_bin, rot_bin_clamped), ComputeThreeMaxima (rot_three_maxima, host and device), the keep test (rot_keeps)
// and the whole prune of one match row (rot_prune).  For orbfe_match.hip, orbfe_grid.hip, orbfe_projection.hip,
// orbfe_stereo.hip and orbfe_bow.hip; through orbfe_proj_dev.h / orbfe_track_dev.h for the device-resident searches
// (orbfe_track.hip, orbfe_init_search.hip, orbfe_tri_search.hip); and for the host entry point orbfe_rotation_consistency
// (orbfe_hostgeom.hip), which runs the very rot_three_maxima / rot_keeps the kernels call.  The library is built without
// relocatable device code, so every kernel gets its own inlined copy.
#pragma once

#include "orbfe_common.h"

// cells of the frame grid (orbfe_grid.hip builds it, orbfe_projection.hip walks it)
#define GRID_NC (ORBFE_GRID_COLS * ORBFE_GRID_ROWS)

struct Desc8 {
    uint32_t w[8];
};

__device__ __forceinline__ Desc8 load_desc8(const uint8_t *row)
{
    Desc8 d;
    const uint32_t *p = (const uint32_t *)row;
#pragma unroll
    for (int k = 0; k < 8; ++k) d.w[k] = p[k];
    return d;
}

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

// the replay kernels index their histogram with it: a NaN angle cannot reach outside the 30 bins
__device__ __forceinline__ int rot_bin_clamped(float a1, float a2) { return min(max(rot_bin(a1, a2), 0), ORBFE_HISTO_LENGTH - 1); }

// ComputeThreeMaxima (src/ORBmatcher.cc:1912-1957) over the `len` bins of a rotation histogram: keep[0..2] = the bins that stay,
// the fullest first, an earlier bin winning a tie; -1 where there is none or where the second / third is under a tenth of the
// first.  One thread calls it.  The library is built with -ffp-contract=off: the product is one rounded multiply on both sides.
__host__ __device__ __forceinline__ void rot_three_maxima(const int *hist, int len, int keep[3])
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < len; ++i) {
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
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    keep[0] = i1; keep[1] = i2; keep[2] = i3;
}

// does a match whose rotation fell into `bin` stand?
__host__ __device__ __forceinline__ bool rot_keeps(const int *keep, int bin) { return bin == keep[0] || bin == keep[1] || bin == keep[2]; }

// The rotation prune of one match row by one workgroup of 256 threads (:308-313, :336-349): histogram over the matches
// match[i] = j >= 0 of rot_bin(first(i, j), second(i, j)), three maxima, the matches of the other bins cleared, *nmatches = what
// stands (all of them when check_ori is 0).  Every thread of the workgroup calls it with the same arguments.
template <typename A1, typename A2>
__device__ __forceinline__ void rot_prune(int32_t *match, int n, int check_ori, int32_t *nmatches, A1 first, A2 second)
{
    __shared__ int s_hist[ORBFE_HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_count;
    const int tid = threadIdx.x;
    if (tid < ORBFE_HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (check_ori) {
        for (int i = tid; i < n; i += 256) {
            const int j = match[i];
            if (j >= 0) atomicAdd(&s_hist[rot_bin(first(i, j), second(i, j))], 1);
        }
        __syncthreads();
        if (tid == 0) rot_three_maxima(s_hist, ORBFE_HISTO_LENGTH, s_keep);
        __syncthreads();
    }
    int local = 0;
    for (int i = tid; i < n; i += 256) {
        const int j = match[i];
        if (j < 0) continue;
        if (check_ori && !rot_keeps(s_keep, rot_bin(first(i, j), second(i, j)))) {
            match[i] = -1;
            continue;
        }
        ++local;
    }
    atomicAdd(&s_count, local);
    __syncthreads();
    if (tid == 0) *nmatches = s_count;
}
