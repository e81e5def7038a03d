// orbfe_pyramid.hip -- K1, the bilinear pyramid (k_pyr_walk), and the padded pyramid of one frame (k_pad_pyramid).
#include "orbfe_pyramid_dev.h"

// ---------------------------------------------------------------------------------------------------
// K1  bilinear pyramid level:  dst(level) = resize(src(level-1))      
// cv::resize(INTER_LINEAR) in its 8-bit fixed-point form: horizontal sums H = S[sx]*a0 + S[sx+1]*a1 with 11-bit
// coefficients, vertical step ((b0*(H0>>4))>>16) + ((b1*(H1>>4))>>16) + 2) >> 2.  The level's geometry travels as kernel
// arguments; the taps (source index + the two coefficients per destination column / row) come from host-built tables
// computed with the exact fp64 / fp32 operation sequence of cv::resize; all kernel math is int32.
// ---------------------------------------------------------------------------------------------------
// (PyrArgs and the walk of one lane, pyr_walk_run: orbfe_pyramid_dev.h)
__global__ __launch_bounds__(256) void k_pyr_walk(PyrArgs a)
{
    extern __shared__ uint2 s_dyn[];
    uint2 *s_yt = s_dyn;                                   // [dh + 8]: the vertical taps, for the mixed waves
    uint32_t *s_out = (uint32_t *)(s_dyn + (a.dh + 8));    // [rb][256]
    const int b = blockIdx.y;
    const int ncol4 = (a.dw + 3) >> 2;
    const int nfull = pyr_nfull(ncol4), tail = max(ncol4 - nfull * 64, 0);
    const int nuni = nfull * a.nrblk, nmix = tail * a.nrblk;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int gw = (int)blockIdx.x * 4 + wv;   // wave of the frame: row-block waves first (run-major), then the mixed waves
    if ((int)blockIdx.x * 4 + 3 >= nuni) {     // a workgroup with a mixed wave (workgroup-uniform): the taps into LDS
        for (int i = threadIdx.x; i < a.dh + 8; i += 256) s_yt[i] = ((const uint2 *)a.ytab)[i];
        __syncthreads();
    }
    if (gw < nuni) {
        const int rblk = gw / nfull;
        pyr_walk_run<true>(a, b, rblk, min((gw - rblk * nfull) * 64 + lane, ncol4 - 1), s_yt, s_out);
    } else if (gw < nuni + ((nmix + 63) >> 6)) {
        const int fl = min((gw - nuni) * 64 + lane, nmix - 1);   // surplus lanes repeat the last lane's work
        const int rblk = fl / tail;
        pyr_walk_run<false>(a, b, rblk, nfull * 64 + fl - rblk * tail, s_yt, s_out);
    }
}

// ---------------------------------------------------------------------------------------------------
// K6  the padded pyramid of ONE frame, all levels in one launch: level l as a (w + 2E) x (h + 2E) block with the
// BORDER_REFLECT_101 frame copyMakeBorder gives it (src/ORBextractor.cc:1136-1142), rows tight (pitch w + 2E), levels back to
// back at pad_off[l] -- the memory shape of the reference's public mvImagePyramid, produced for one device-to-host copy.
// One thread per 4 output bytes.
// ---------------------------------------------------------------------------------------------------
struct PadArgs {
    const uint8_t *src[ORBFE_MAX_LEVELS];
    int32_t pitch[ORBFE_MAX_LEVELS], w[ORBFE_MAX_LEVELS], h[ORBFE_MAX_LEVELS];
    uint32_t off[ORBFE_MAX_LEVELS + 1];   // byte offset of a level's block in the output, off[nlevels] = total (multiples of 4)
    int32_t nlevels;
};
__global__ __launch_bounds__(256) void k_pad_pyramid(PadArgs a, uint8_t *__restrict__ out)
{
    const uint32_t o = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (o >= a.off[a.nlevels]) return;
    int l = 0;
#pragma unroll
    for (int k = 1; k < ORBFE_MAX_LEVELS; ++k)
        if (k < a.nlevels && o >= a.off[k]) l = k;
    const int W = a.w[l], H = a.h[l], PW = W + 2 * ORBFE_EDGE;
    const uint32_t rel = o - a.off[l], total = (uint32_t)PW * (uint32_t)(H + 2 * ORBFE_EDGE);
    uint32_t word = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t r = rel + (uint32_t)j;
        if (r < total) {   // a block's byte count need not be a multiple of 4: the slack up to the next block stays zero
            const int py = (int)(r / (uint32_t)PW), px = (int)(r - (uint32_t)py * (uint32_t)PW);
            const int sy = reflect101(py - ORBFE_EDGE, H), sx = reflect101(px - ORBFE_EDGE, W);
            word |= (uint32_t)a.src[l][(int64_t)sy * a.pitch[l] + sx] << (8 * j);
        }
    }
    *(uint32_t *)(out + o) = word;
}

hipError_t orbk_launch_pad_pyramid(const OrbPyrView &v, const uint32_t *off, uint8_t *d_out, hipStream_t st)
{
    PadArgs a;
    a.nlevels = v.nlevels;
    for (int l = 0; l < v.nlevels; ++l) {
        a.src[l] = v.ptr[l];
        a.pitch[l] = v.pitch[l];
        a.w[l] = v.w[l];
        a.h[l] = v.h[l];
        a.off[l] = off[l];
    }
    a.off[v.nlevels] = off[v.nlevels];
    const uint32_t nthreads = (off[v.nlevels] + 3u) / 4u;
    hipLaunchKernelGGL(k_pad_pyramid, dim3((nthreads + 255u) / 256u), dim3(256), 0, st, a, d_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t orbk_launch_pyramid(const OrbLaunch &a, hipStream_t st)
{
    // Level l reads level l-1 (:1134): one launch per level.  Measured, not kept (profiles/HISTORY.md): two levels per launch,
    // level l + 1 resized from level l's tile while it is in LDS -- byte-exact and SLOWER on this part, 0.574 vs 0.505 ms per
    // 1024 640x480 frames, 0.424 vs 0.397 ms per 128 1080p frames (profiles/r03_ab_experiments.json): the chained kernels are
    // latency-bound, not traffic-bound (3.7 of ~5 TB/s), and the second phase lengthens every workgroup's dependent chain by
    // more than the saved 0.37 GB of reads are worth (single frame: 49 us against 48 us for the seven chained launches).  All
    // levels of a frame in one launch (a 1024-thread workgroup per frame, workgroup barriers between levels): 0.66 ms against
    // 0.63 ms per 1024 frames; with an agent-scope fence between the levels 4.8 ms.
    const int nl = a.h_plan->nlevels;
    for (int l = 1; l < nl; ++l) {
        const OrbLevel &D = a.h_plan->lv[l];
        PyrArgs pa;
        pyr_args(a, l, pa);
        dim3 grid((pyr_walk_waves(D.w, pa.nrblk) + 3) / 4, a.nframes);
        hipLaunchKernelGGL(k_pyr_walk, grid, dim3(256), orbk_pyramid_lds_bytes(D.h), st, pa);
    }
    return hipGetLastError();
}
