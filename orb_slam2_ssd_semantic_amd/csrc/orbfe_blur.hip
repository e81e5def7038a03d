// orbfe_blur.hip -- K4, the 7x7 Gaussian of every level (k_blur7).
#include "orbfe_kernels_dev.h"

// ---------------------------------------------------------------------------------------------------
// K4  7x7 Gaussian, sigma 2, 8-bit fixed-point kernel {18,34,49,55,49,34,18} (sum 257), REFLECT_101 at the
// LEVEL edges.  All levels of all frames in ONE launch.  One wave owns a 256-px wide, BL_RB-row tall
// tile: every lane filters 4 adjacent pixels, walking down the rows with the last 7 row-sums in registers
// (no LDS, no intermediate traffic): per row 3 aligned dword loads (12-byte window), 4 row sums, 4 outputs,
// one dword store.  Reflected borders: rows by a wave-uniform index, columns by a per-byte path on edge lanes.
// ---------------------------------------------------------------------------------------------------
// weights of window dword d (pixels x-4+4d .. x-1+4d) for the output pixel x+j: its taps are window bytes j+1 .. j+7
__host__ __device__ constexpr uint32_t blur_hw(int j, int d)
{
    const int kern[7] = {18, 34, 49, 55, 49, 34, 18};
    uint32_t w = 0u;
    for (int b = 0; b < 4; ++b) {
        const int t = 4 * d + b - j - 1;
        if (t >= 0 && t <= 6) w |= (uint32_t)kern[t] << (8 * b);
    }
    return w;
}

// Work is described per LANE (a 4-pixel column, a short run of rows), packed by the host into single-level waves, so
// no lane idles on narrow levels.  Column borders are branch-free: every lane loads 3 dwords from a per-lane base that
// covers all (reflected) source pixels of its 12-byte window and rearranges them with per-lane byte selectors
// (identity for interior lanes); row borders are a per-lane reflected row index.
#ifndef BL_PF
#define BL_PF 4  // prefetch distance in rows (2 .. 6 measured: profiles/r06_ab_blur.json)
#endif
#ifdef BL_MIN_WAVES
#define BL_BOUNDS __launch_bounds__(256, BL_MIN_WAVES)
#else
#define BL_BOUNDS __launch_bounds__(256)
#endif
// the row walk of one lane; INTERIOR (wave-uniform, compile-time): the 12-byte window holds no reflected column; UP (wave-uniform,
// compile-time): the walk goes from the bottom of the row block to its top.
//
// Instruction budget of a row step (4 pixels per lane): 10 v_dot4 horizontal taps (border waves: 12, below), the vertical taps on
// u16 row-sum PAIRS -- a pair (row 2m, row 2m + 1) is formed once, on the odd step (4 v_lshl_or every other step), and the seven
// rows of an output are three pairs and one single row on even steps, the high half of a pair and three pairs on odd ones, i.e.
// four v_dot2 per pixel either way -- saturate_cast<uchar> by the dot products' own clamp (the accumulator starts at
// 0xFF000000 + the rounding constant, so a value >= 256 runs into 0xFFFFFFFF and byte 2 IS the saturated pixel), three v_perm to
// gather the four bytes, one compare against the lane's row count, one add each for the load and the store offset.
//
// Border waves (reflected columns): BORDER_REFLECT_101 folds the taps that fall outside the row onto pixels inside it, so a
// border lane reads its 12-byte window as it lies (pulled inside the row) and applies FOLDED weights: twelve per-lane weight
// dwords from the plan's table (OrbPlan::blur_wt, four lane types per level) instead of byte selectors -- no v_perm per row.
template <int MODE, bool INTERIOR, bool UP>
__device__ __forceinline__ void blur7_walk(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int pitch, const int dpitch,
                                           const int W, const int H, const int x, const int y0, const int nrows_lane, const bool active,
                                           const int nsteps, const int vec_w, const uint32_t *__restrict__ wtab)
{
    constexpr bool up = UP;
    // all sources of the lane's ten window pixels lie in [base, base + 12) (checked on the host for every level width); at the
    // right edge the window is pulled back so that it ends at the last pixel of the row
    const int base = INTERIOR ? x - 4 : min(max(x - 4, 0), W - 12);
    uint32_t wt[4][3];
    if (!INTERIOR) {
        const int r = W - x;
        const int type = x == 0 ? 1 : (r <= 4 ? 3 : (r <= 8 ? 2 : 0));
        const uint4 *t = (const uint4 *)(wtab + type * 12);
        const uint4 t0 = t[0], t1 = t[1], t2 = t[2];
        wt[0][0] = t0.x; wt[0][1] = t0.y; wt[0][2] = t0.z; wt[1][0] = t0.w;
        wt[1][1] = t1.x; wt[1][2] = t1.y; wt[2][0] = t1.z; wt[2][1] = t1.w;
        wt[2][2] = t2.x; wt[3][0] = t2.y; wt[3][1] = t2.z; wt[3][2] = t2.w;
    }
    const bool full = x + 4 <= W;
    const uint32_t nrows = active ? (uint32_t)nrows_lane : 0u;

    // Row sums are <= 255 * 257 = 65535, i.e. u16.  Q[m & 3] holds, per pixel, the pair (row sum of step 2m, row sum of step
    // 2m + 1) as two u16 halves; hs = the row sums of the even step the pair is waiting for.
    uint32_t Q[4][4], hs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) hs[j] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) Q[k][j] = 0u;

    // raw rows are fetched BL_PF steps ahead into an 8-slot ring (the unroll factor), so a wave keeps several rows in flight
    uint32_t Lr[8][3];
    // A wave none of whose lanes comes within 3 rows of the level's top or bottom (three of four) walks plain rows: the
    // offset advances by the pitch, no reflected row index per step.
    // A lane walks its rows downwards from y0 - 3 or (flag bit 3, odd row blocks) upwards from yend + 2: the taps are symmetric,
    // the sums are the same integers.  Row of step s: ystart + dir * s; the output row of step s lies 3 * dir behind it, i.e. it is
    // output row s - 6 of the lane's block counted from the end the walk started at.
    const int dir = up ? -1 : 1;
    const int yend = y0 + nrows_lane;
    const int ystart = up ? yend + 2 : y0 - 3;
    const int ylast = ystart + dir * (nsteps + BL_PF - 1);   // last row the walk asks for (incl. the prefetch past its end)
    const bool plain_rows = orb_ballot(!(min(ystart, ylast) >= 0 && max(ystart, ylast) < H)) == 0ull;
    uint32_t ro = __umul24((uint32_t)min(max(ystart, 0), H - 1), (uint32_t)pitch) + (uint32_t)base;
    const uint32_t rstep = up ? 0u - (uint32_t)pitch : (uint32_t)pitch;
    uint32_t oo = __umul24((uint32_t)(up ? max(yend - 1, 0) : y0), (uint32_t)dpitch) + (uint32_t)x;   // output offset of step 6
    const uint32_t ostep = up ? 0u - (uint32_t)dpitch : (uint32_t)dpitch;
    auto fetch = [&](int s, uint32_t (&dst3)[3]) {
        const uint8_t *row;
        if (plain_rows) {
            row = src + ro;
            ro += rstep;
        } else {
            const int yy = reflect101(max(min(ystart + dir * s, H + 2), -3), H);
            row = src + (__umul24((uint32_t)yy, (uint32_t)pitch) + (uint32_t)base);
        }
        dst3[0] = *(const uint32_t *)(row);
        dst3[1] = *(const uint32_t *)(row + 4);
        dst3[2] = *(const uint32_t *)(row + 8);
    };
#pragma unroll
    for (int k = 0; k < BL_PF; ++k) fetch(k, Lr[k]);

    constexpr uint32_t ACC0 = 0xFF000000u + 32768u;   // clamp bias (see above) + round half up
    for (int s0 = 0; s0 < nsteps; s0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k;   // s0 is a multiple of 8: the parity of s is the parity of k
            if (s >= nsteps) break;  // wave-uniform
            fetch(s + BL_PF, Lr[(k + BL_PF) % 8]);  // rows past the run re-read a valid (reflected / clamped) row
            const uint32_t w[3] = {Lr[k][0], Lr[k][1], Lr[k][2]};
            // horizontal taps as byte dot products against per-(pixel, dword) weight dwords: compile-time constants in interior
            // waves, the lane's folded weights in border waves
            uint32_t hn[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t h = 0u;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    if (INTERIOR) {
                        if (blur_hw(j, d) != 0u) h = __builtin_amdgcn_udot4(w[d], blur_hw(j, d), h, false);
                    } else {
                        h = __builtin_amdgcn_udot4(w[d], wt[j][d], h, false);
                    }
                }
                hn[j] = h;
            }
            const int m = k >> 1;
            if (k & 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Q[m][j] = hs[j] | (hn[j] << 16);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) hs[j] = hn[j];
            }
            if (s >= 6) {
                uint32_t tq[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // rows y-3 .. y+3 are steps s-6 .. s with taps 18 34 49 55 49 34 18
                    uint32_t acc;
                    if (k & 1) {   // (s-7 | s-6) (s-5 | s-4) (s-3 | s-2) (s-1 | s): the pair just formed is the last
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 1) & 3][j]), __builtin_bit_cast(orb_u2, 0x00120000u), ACC0, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 2) & 3][j]), __builtin_bit_cast(orb_u2, 0x00310022u), acc, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 3) & 3][j]), __builtin_bit_cast(orb_u2, 0x00310037u), acc, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[m][j]), __builtin_bit_cast(orb_u2, 0x00120022u), acc, true);
                    } else {       // (s-6 | s-5) (s-4 | s-3) (s-2 | s-1) and the single row s (a u16 in a dword: its high half is 0)
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 1) & 3][j]), __builtin_bit_cast(orb_u2, 0x00220012u), ACC0, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 2) & 3][j]), __builtin_bit_cast(orb_u2, 0x00370031u), acc, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, Q[(m + 3) & 3][j]), __builtin_bit_cast(orb_u2, 0x00220031u), acc, true);
                        acc = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, hn[j]), __builtin_bit_cast(orb_u2, 0x00000012u), acc, true);
                    }
                    tq[j] = acc;  // byte 2 = the value rounded half-up and saturated (0xFFFFFFFF when it was >= 256)
                }
                if (MODE == 1) {
                    // SSE2 half-even: an exact half (low 16 bits zero) rounds to the even value inside the vectorised part of
                    // the row.  One pixel in 65536 is an exact half, so the test is one wave-uniform branch on the smallest
                    // low half of the lane's four sums; the per-pixel correction runs only when some lane has one.  (A saturated
                    // sum has low half 0xFFFF: never corrected, and 256 or 257 saturate to 255 either way.)
                    const uint32_t lowmin = min(min(tq[0] & 0xFFFFu, tq[1] & 0xFFFFu), min(tq[2] & 0xFFFFu, tq[3] & 0xFFFFu));
                    if (orb_ballot(lowmin == 0u) != 0ull) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if ((tq[j] & 0xFFFFu) == 0u && (x + j) < vec_w && (tq[j] & 0x10000u)) tq[j] -= 0x10000u;
                    }
                }
                const uint32_t p01 = __builtin_amdgcn_perm(tq[1], tq[0], 0x0c0c0602u);
                const uint32_t p23 = __builtin_amdgcn_perm(tq[3], tq[2], 0x06020c0cu);
                const uint32_t packed = p01 | p23;
                if ((uint32_t)(s - 6) < nrows) {
                    if (full) {
                        *(uint32_t *)(dst + oo) = packed;   // uniform base + 32-bit lane offset: no 64-bit address arithmetic
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (x + j < W) dst[oo + (uint32_t)j] = (uint8_t)(packed >> (8 * j));
                    }
                }
                oo += ostep;
            }
        }
    }
}

template <int MODE>
__global__ BL_BOUNDS void k_blur7(const OrbPlan *__restrict__ plan, FrameSrc fs,
                                               const OrbLane *__restrict__ lanes, int nwaves,
                                               uint8_t *__restrict__ blur, int64_t blur_fstride)
{
    int b = blockIdx.y, bx = blockIdx.x;
    xcd_frame_remap(bx, b);
    const int lane = threadIdx.x & 63;
    const int t = bx * 4 + (threadIdx.x >> 6);
    if (t >= nwaves) return;
    const OrbLane ld = lanes[(int64_t)t * 64 + lane];
    const int level = __builtin_amdgcn_readfirstlane((int)(ld.flags >> 8));
    const OrbLevel &L = plan->lv[level];
    int pitch;
    const uint8_t *src = level_ptr(fs, L, level, b, &pitch);
    uint8_t *dst = blur + (int64_t)b * blur_fstride + L.off;
    const int W = L.w, H = L.h;
    const int x = ld.x, y0 = ld.ys, nr = ld.nrows;
    const bool active = !(ld.flags & 1);
    // wave-uniform by construction (the host packs interior and edge columns into separate waves): no reflected column
    const bool interior = __builtin_amdgcn_readfirstlane((int)(ld.flags & 2)) != 0;
    const int vec_w = W & ~3;
    const uint32_t *wtab = plan->blur_wt[level][0];
    int nsteps = ld.nrows;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nsteps = max(nsteps, __shfl_xor(nsteps, o, 64));
    nsteps = __builtin_amdgcn_readfirstlane(nsteps) + 6;  // wave-uniform
    const bool up = __builtin_amdgcn_readfirstlane((int)(ld.flags & 8)) != 0;   // wave-uniform by construction, like `interior`
    if (interior) {
        if (up) blur7_walk<MODE, true, true>(src, dst, pitch, (int)L.pitch, W, H, x, y0, nr, active, nsteps, vec_w, wtab);
        else blur7_walk<MODE, true, false>(src, dst, pitch, (int)L.pitch, W, H, x, y0, nr, active, nsteps, vec_w, wtab);
    } else {
        if (up) blur7_walk<MODE, false, true>(src, dst, pitch, (int)L.pitch, W, H, x, y0, nr, active, nsteps, vec_w, wtab);
        else blur7_walk<MODE, false, false>(src, dst, pitch, (int)L.pitch, W, H, x, y0, nr, active, nsteps, vec_w, wtab);
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t orbk_launch_blur(const OrbLaunch &a, hipStream_t st)
{
    const FrameSrc fs = make_src(a);
    dim3 grid((a.h_plan->nbwaves + 3) / 4, a.nframes);
    if (a.h_plan->blur_rounding == 1)
        hipLaunchKernelGGL(k_blur7<1>, grid, dim3(256), 0, st, a.d_plan, fs, a.d_blanes, a.h_plan->nbwaves, a.d_blur,
                           a.pyr_fstride);
    else
        hipLaunchKernelGGL(k_blur7<0>, grid, dim3(256), 0, st, a.d_plan, fs, a.d_blanes, a.h_plan->nbwaves, a.d_blur,
                           a.pyr_fstride);
    return hipGetLastError();
}
