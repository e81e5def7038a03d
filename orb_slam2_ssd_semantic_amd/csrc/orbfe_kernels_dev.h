// orbfe_kernels_dev.h -- device helpers and types shared by the extractor's kernel files (orbfe_pyramid.hip, orbfe_fast.hip,
// orbfe_octree.hip, orbfe_blur.hip, orbfe_describe.hip), and the host-side make_src of their launchers.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

#include "orbfe_common.h"
#include "orbfe_kernels.h"

typedef _Float16 orb_h2 __attribute__((ext_vector_type(2)));
typedef short orb_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short orb_u2 __attribute__((ext_vector_type(2)));

struct FrameSrc {
    const uint8_t *l0;   // level-0 frames (caller's buffer)
    int64_t l0_fstride;  // bytes between frames
    int32_t l0_pitch;    // row pitch of level 0
    uint8_t *pyr;        // levels >= 1 (handle-owned)
    int64_t pyr_fstride;
};

__device__ __forceinline__ const uint8_t *level_ptr(const FrameSrc &fs, const OrbLevel &L, int level, int b,
                                                    int *pitch)
{
    if (level == 0) {
        *pitch = fs.l0_pitch;
        return fs.l0 + (int64_t)b * fs.l0_fstride;
    }
    *pitch = L.pitch;
    return fs.pyr + (int64_t)b * fs.pyr_fstride + L.off;
}

__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan over the block (blockDim.x multiple of 64, <= 1024); s_wave = 17 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int *s_wave, int *total)
{
    const int incl = wave_incl_scan(v);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        int t = s_wave[w];
        if (w < wid) base += t;
        tot += t;
    }
    *total = tot;
    return base + incl - v;
}

__device__ __forceinline__ int reflect101(int p, int len)
{
    // cv::borderInterpolate(BORDER_REFLECT_101); len >= 2 in every use here, |overshoot| <= 3
    if (p < 0) p = -p;
    if (p >= len) p = 2 * len - 2 - p;
    return p;
}

// XCD-aware placement for grids of (work item, frame): workgroups are dealt round-robin to the 8 XCDs in launch order
// and every XCD has its own 4 MB L2, while one frame's pyramids are ~2 MB.  With a multiple of 8 frames, all workgroups
// of frame f are steered to XCD f % 8, so rows shared by neighbouring waves / overlapping patches of a frame are
// fetched from HBM once instead of once per XCD.
__device__ __forceinline__ void xcd_frame_remap(int &bx, int &b)
{
    if ((gridDim.y & 7) == 0) {
        const int lin = blockIdx.y * gridDim.x + blockIdx.x, xcd = lin & 7, j = lin >> 3;
        b = xcd + 8 * (j / (int)gridDim.x);
        bx = j % (int)gridDim.x;
    }
}

// The lane mask of a predicate straight from its compare (HIP's __ballot materialises the bool in a VGPR and compares it
// again: two VALU instructions per ballot in the row loops)
__device__ __forceinline__ unsigned long long orb_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int min3i(int a, int b, int c) { return min(min(a, b), c); }
__device__ __forceinline__ int max3i(int a, int b, int c) { return max(max(a, b), c); }

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// ---- packed 16-bit helpers: two pixels per VALU instruction --------------------------------------------
// A pixel pair is held as two u16 halves (values 0..255).  Read as f16 bit patterns those are positive
// denormals, whose order equals the integer order, so gfx950's 3-input packed min/max
// (v_pk_minimum3_f16 / v_pk_maximum3_f16) give exact integer results at two pixels per instruction.

__device__ __forceinline__ uint32_t pk_min3(uint32_t a, uint32_t b, uint32_t c)
{
    const orb_h2 x = __builtin_bit_cast(orb_h2, a), y = __builtin_bit_cast(orb_h2, b), z = __builtin_bit_cast(orb_h2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_minimum(__builtin_elementwise_minimum(x, y), z));  // v_pk_minimum3_f16
}
__device__ __forceinline__ uint32_t pk_max3(uint32_t a, uint32_t b, uint32_t c)
{
    const orb_h2 x = __builtin_bit_cast(orb_h2, a), y = __builtin_bit_cast(orb_h2, b), z = __builtin_bit_cast(orb_h2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(__builtin_elementwise_maximum(x, y), z));  // v_pk_maximum3_f16
}
__device__ __forceinline__ uint32_t pk_sub_i16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(orb_s2, a) - __builtin_bit_cast(orb_s2, b));
}
__device__ __forceinline__ uint32_t pk_max_i16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(orb_s2, a), __builtin_bit_cast(orb_s2, b)));
}
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(orb_u2, a) - __builtin_bit_cast(orb_u2, b));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(orb_u2, a), __builtin_bit_cast(orb_u2, b)));
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(orb_u2, a), __builtin_bit_cast(orb_u2, b)));
}
__device__ __forceinline__ uint32_t pk_subsat_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(orb_u2, a), __builtin_bit_cast(orb_u2, b)));
}

// host side: the frames and the pyramid of a launch as the kernels take them
static FrameSrc make_src(const OrbLaunch &a)
{
    FrameSrc fs;
    fs.l0 = a.d_gray;
    fs.l0_fstride = a.gray_fstride;
    fs.l0_pitch = a.gray_pitch;
    fs.pyr = a.d_pyr;
    fs.pyr_fstride = a.pyr_fstride;
    return fs;
}
