// orbfe_fast.hip -- K2, FAST-9/16 with the reference's per-cell semantics: the dense forms (k_fast_map, k_fast_map_u) and the
// lane-compacting form (k_fast_map_c).
#include "orbfe_kernels_dev.h"

// ---------------------------------------------------------------------------------------------------
// K2  FAST-9/16 with the reference's per-cell semantics: corner at t <=> A > t for the arc strength
//   A = max(A_dark, A_bright), cv score = A - 1, 3x3 strict NMS inside each cell's detectable interior, iniTh list
//   or -- for a cell where that is empty -- minTh list.
// ---------------------------------------------------------------------------------------------------
// Dense streaming formulation.
//
// k_fast_map   one wave per (level, 256-px strip piece, row block).  Every lane owns 4 adjacent pixels and walks down
//              the rows with the last 7 image rows in registers (each unpacked once into its nine u16 pixel pairs,
//              fast_unpack_row) -- no LDS, no byte loads.  With
//              raw pixel values c[0..15] on the circle,  min over an arc of (v - c) = v - max(c)  and
//              min over an arc of (c - v) = min(c) - v, so
//                  A = max( v - min_k max(c[k..k+8]),  max_k min(c[k..k+8]) - v )
//              needs no per-tap subtraction: two levels of min3/max3 give all 16 nine-arcs (2 ops per arc and
//              polarity).  A is clamped to E = (A > max(minTh,1)) ? A : 0; the 3x3 strict NMS runs in registers on
//              three rows of E (neighbour lanes via shuffles) with the reference's per-cv::FAST-call semantics:
//              neighbours outside the own cell's detectable interior count as 0 (cell seams are per-lane column
//              masks and wave-uniform row flags).  Because iniTh >= minTh, a corner with A > iniTh survives NMS at
//              iniTh iff it survives at minTh, so ONE survivor map  M = survivor ? A : 0  encodes both of the
//              reference's lists: {M > iniTh} and, for cells where that is empty, {M > 0}  (:818-825).
//              Survivors are appended UNORDERED to the level's list {key, ord}; `ord` is computable from the pixel
//              position alone and is a rank key of the reference's candidate order (cell-row-major, raster inside
//              a cell), which is all DistributeOctTree's tie-break needs.  The fallback rule (a cell whose iniTh
//              list is empty contributes its minTh list) is applied per cell in k_octree's prologue.

// (the packed 16-bit helpers, two pixels per VALU instruction: orbfe_kernels_dev.h)

// pixels (IDX, IDX+1) of a 12-byte row window as a u16 pair
template <int IDX>
__device__ __forceinline__ uint32_t rowpair(const uint32_t (&w)[3])
{
    static_assert(IDX >= 0 && IDX < 11, "window pair");
    if ((IDX & 3) < 3)
        return __builtin_amdgcn_perm(0u, w[IDX >> 2], 0x0c000c00u | ((uint32_t)((IDX & 3) + 1) << 16) | (uint32_t)(IDX & 3));
    return __builtin_amdgcn_perm(w[(IDX >> 2) + 1 > 2 ? 2 : (IDX >> 2) + 1], w[IDX >> 2], 0x0c040c03u);
}

// Every row of the ring is unpacked ONCE, when it arrives, into the nine pixel pairs (i, i+1), i = 1..9, of its 12-byte
// window (E[i-1]); each pair is then used by up to three centre rows and by both pixel pairs of the lane, instead of
// being re-extracted with a v_perm at every use (34 -> 9 extractions per row step).
#define FM_NE 9
__device__ __forceinline__ void fast_unpack_row(const uint32_t (&w)[3], uint32_t (&e)[FM_NE])
{
    e[0] = rowpair<1>(w);
    e[1] = rowpair<2>(w);
    e[2] = rowpair<3>(w);
    e[3] = rowpair<4>(w);
    e[4] = rowpair<5>(w);
    e[5] = rowpair<6>(w);
    e[6] = rowpair<7>(w);
    e[7] = rowpair<8>(w);
    e[8] = rowpair<9>(w);
}

// the strength network on values: the 16 circle pixel pairs c[] and the centre pair v of one pixel pair (fast_strength_pair gathers
// them from the register ring of rows, the lane-compacting form, orbfe_fast_body_c.inc, from its LDS pixel ring)
__device__ __forceinline__ uint32_t fast_strength_from(const uint32_t (&c)[16], uint32_t v, uint32_t t)
{
    // Nine-arcs k and k+1 (k even) share the eight pixels c[k+1..k+8], so
    //   max(min arc_k, min arc_k+1) = min(c[k+1..k+8], max(c[k], c[k+9]))     (and dually for the dark polarity):
    // odd-aligned pairs P/Q, three 3-way ops per two arc pairs -- 32 ops per polarity for all 16 arcs.
    uint32_t P[8], Q[8], ex[8], en[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        P[i] = pk_min_u16(c[2 * i + 1], c[(2 * i + 2) & 15]);
        Q[i] = pk_max_u16(c[2 * i + 1], c[(2 * i + 2) & 15]);
        ex[i] = pk_max_u16(c[2 * i], c[(2 * i + 9) & 15]);
        en[i] = pk_min_u16(c[2 * i], c[(2 * i + 9) & 15]);
    }
    // The eight-pixel windows P[i..i+3] of two neighbouring arc pairs share three of their four pairs: one 3-way op
    // (P[i], P[i+1], P[i+2]), i even, serves window i (with P[i+3]) and window i-1 (with P[i-1]) -- 12 ops per polarity for the
    // eight windows instead of 16, the closing op still takes the arc pair's end pixels along.
    uint32_t Wb[8], Wd[8];
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const uint32_t ab = pk_min3(P[i], P[(i + 1) & 7], P[(i + 2) & 7]);
        const uint32_t ad = pk_max3(Q[i], Q[(i + 1) & 7], Q[(i + 2) & 7]);
        Wb[i] = pk_min3(ab, P[(i + 3) & 7], ex[i]);
        Wd[i] = pk_max3(ad, Q[(i + 3) & 7], en[i]);
        Wb[(i + 7) & 7] = pk_min3(P[(i + 7) & 7], ab, ex[(i + 7) & 7]);
        Wd[(i + 7) & 7] = pk_max3(Q[(i + 7) & 7], ad, en[(i + 7) & 7]);
    }
    const uint32_t maxmin = pk_max_u16(pk_max3(pk_max3(pk_max3(Wb[0], Wb[1], Wb[2]), Wb[3], Wb[4]), Wb[5], Wb[6]), Wb[7]);
    const uint32_t minmax = pk_min_u16(pk_min3(pk_min3(pk_min3(Wd[0], Wd[1], Wd[2]), Wd[3], Wd[4]), Wd[5], Wd[6]), Wd[7]);
    // S = max(A, t) - t with A = max(v - min_arcs(max), max_arcs(min) - v, 0): zero for non-corners (A <= t), order
    // preserving for corners; t = 0x3FF in a half switches the pixel off (A <= 255)
    const uint32_t m = pk_max3(pk_subsat_u16(v, minmax), pk_subsat_u16(maxmin, v), t);
    return pk_sub_u16(m, t);
}

// thresholded arc strengths S = max(A - t, 0) of the pixel pair (J, J+1) of the lane, as two u16 halves;
// rows are unpacked windows (fast_unpack_row) of image rows y-3 .. y+3
template <int J>
__device__ __forceinline__ uint32_t fast_strength_pair(const uint32_t (&rm3)[FM_NE], const uint32_t (&rm2)[FM_NE],
                                                       const uint32_t (&rm1)[FM_NE], const uint32_t (&r0)[FM_NE],
                                                       const uint32_t (&rp1)[FM_NE], const uint32_t (&rp2)[FM_NE],
                                                       const uint32_t (&rp3)[FM_NE], uint32_t t)
{
    uint32_t c[16];
    c[0] = rp3[3 + J];
    c[1] = rp3[4 + J];
    c[2] = rp2[5 + J];
    c[3] = rp1[6 + J];
    c[4] = r0[6 + J];
    c[5] = rm1[6 + J];
    c[6] = rm2[5 + J];
    c[7] = rm3[4 + J];
    c[8] = rm3[3 + J];
    c[9] = rm3[2 + J];
    c[10] = rm2[1 + J];
    c[11] = rm1[0 + J];
    c[12] = r0[0 + J];
    c[13] = rp1[0 + J];
    c[14] = rp2[1 + J];
    c[15] = rp3[2 + J];
    const uint32_t v = r0[3 + J];
    return fast_strength_from(c, v, t);
}

// Exact NECESSARY condition for A > t on a pixel pair: every nine-arc of the 16-pixel circle contains at
// least one pixel of each opposite pair, so a bright corner needs max(c0, c8) > v + t AND max(c4, c12) > v + t (and
// dually for dark).  Non-zero half <=> that pixel may be a corner.  15 packed ops against 72 for the strength.
// (on values: the four compass pixel pairs and the centre pair of one pixel pair)
__device__ __forceinline__ uint32_t fast_compass_from(uint32_t c0, uint32_t c8, uint32_t c4, uint32_t c12, uint32_t v, uint32_t t)
{
    const uint32_t mb = pk_min_u16(pk_max_u16(c0, c8), pk_max_u16(c4, c12));
    const uint32_t md = pk_max_u16(pk_min_u16(c0, c8), pk_min_u16(c4, c12));
    return pk_subsat_u16(pk_max_u16(pk_subsat_u16(mb, v), pk_subsat_u16(v, md)), t);
}

// the compass test of the pixel pair (J, J+1) of the lane; rows are unpacked windows of image rows y-3, y, y+3
template <int J>
__device__ __forceinline__ uint32_t fast_compass_pair(const uint32_t (&rm3)[FM_NE], const uint32_t (&r0)[FM_NE],
                                                      const uint32_t (&rp3)[FM_NE], uint32_t t)
{
    return fast_compass_from(rp3[3 + J], rm3[3 + J], r0[6 + J], r0[0 + J], r0[3 + J], t);
}

// Rows the dense walk (orbfe_fast_body.inc) keeps in flight: the raw row of step s + FM_PF is fetched in step s.  The FM_PF + 1
// live 12-byte buffers sit in a ring of FM_RAW slots, the next power of two, so that the slot of a step is a compile-time
// constant under the 8-fold unroll at every depth (a slot that is never live costs no register).
// Depth 4 measured best beside the other stages' kernels (profiles/r07_ab_fast_prefetch.json); each row in flight costs three
// registers, and k_fast_map<1> stands at 167 of the 168 that three waves per SIMD allow.
#ifndef FM_PF
#define FM_PF 4
#endif
static_assert(FM_PF >= 1 && FM_PF <= 4, "FM_PF: 1 .. 4 rows in flight");
#define FM_RAW (FM_PF < 2 ? 2 : FM_PF < 4 ? 4 : 8)

#define FM_BUF 384       // per-wave LDS staging of survivors before one atomic reserves their run in the level's list
#define FM_ROW_MAX 140   // a row adds at most 2 per lane + 1 per lane that straddles a cell seam (<= 9 of them)

// The staged survivors go to the level's list, and every survivor above iniTh marks its FAST cell in the WAVE's cell bitmap
// in LDS (the per-cell threshold fallback :818-825 needs "does this cell have an iniTh corner" before any key can be
// judged, so the quadtree kernel would otherwise spend a whole pass over the keys on it).  The wave's bitmap goes to the
// level's bitmap in global memory once, when the wave ends: a wave covers a 256-px x 40-row strip, i.e. a handful of cells.
__device__ __forceinline__ void fm_flush(uint2 *slist, int32_t *scnt, const uint2 *sbuf, int nbuf, int key_cap, int lane,
                                         uint32_t *lflag, int ini)
{
    int base = 0;
    if (lane == 0) base = atomicAdd(scnt, nbuf);
    base = __shfl(base, 0, 64);
    for (int i = lane; i < nbuf; i += 64) {
        const uint2 e = sbuf[i];
        if (base + i < key_cap) slist[base + i] = e;
        if (orb_key_r(e.x) >= ini) {  // cv score = A - 1 >= iniTh  <=>  A > iniTh
            const uint32_t cell = e.y >> 12;
            atomicOr(&lflag[cell >> 5], 1u << (cell & 31));  // LDS, result unused: ds_or_b32
        }
    }
}

// SPARSE = 1: wave-uniform shortcuts for frames whose corners are sparse (real camera images): a row step whose 256
// pixels all fail the compass test skips the arc evaluation, and an NMS row with no strength in its 3-row
// neighbourhood skips the NMS / emission block.  Results are identical; on corner-saturated frames the tests only cost.
// -DFM_WAVES_PER_EU=n caps the kernel's occupancy (A/B: leaving register file to a memory-bound kernel on a side stream)
#if defined(FM_WAVES_PER_EU)
#define FM_OCC __attribute__((amdgpu_waves_per_eu(FM_WAVES_PER_EU, FM_WAVES_PER_EU)))
#else
#define FM_OCC
#endif
#define FM_SHARED_DECLS                                                                                             \
    __shared__ uint2 s_buf[4][FM_BUF];                                                                              \
    extern __shared__ uint32_t s_cf[]; /* [4][cf_words]: per-wave bitmap of the level's cells with a survivor above iniTh */
#ifdef FM_LDS_CONSTS
// Per-lane constants of the row loop (the six half-word masks of the cell seams and the four `ord` column parts) parked in
// LDS and re-read where they are used: ten registers less in the kernel's peak live set.  At <= 152 registers three of its
// waves leave 56 per SIMD lane -- room for one wave of an HBM-bound kernel (k_pyr_walk: 48) beside them, where 160 leave 32
// and nothing fits (A/B in profiles/r04_ab_experiments.json).
#define FM_LDS_DECLS                                                             \
    __shared__ uint4 s_lcm[4][64]; /* in01, in23, lv01, lv23 */                  \
    __shared__ uint2 s_lcr[4][64]; /* rv01, rv23 */                              \
    __shared__ uint4 s_lco[4][64]; /* ordx[0..3] */
#else
#define FM_LDS_DECLS
#endif

template <int SPARSE>
__global__ __launch_bounds__(256) FM_OCC void k_fast_map(const OrbPlan *__restrict__ plan, FrameSrc fs,
                                                  const OrbLane *__restrict__ lanes, int nwaves,
                                                  uint2 *__restrict__ skeys,      // [B][keys_per_frame] {key, ord}
                                                  int32_t *__restrict__ scount,   // [B][nlevels] * NK_STRIDE, zeroed
                                                  uint32_t *__restrict__ cflags,  // [B][nlevels][cf_words], zeroed
                                                  int32_t cf_words,
                                                  unsigned long long *__restrict__ fstat)  // {row steps, arc skips, nms skips} or null
{
    FM_SHARED_DECLS
    FM_LDS_DECLS
    int b = blockIdx.y, bx = blockIdx.x;
    xcd_frame_remap(bx, b);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int t = bx * (blockDim.x >> 6) + wv;
    if (t >= nwaves) return;
    constexpr bool CELLROWS = false;
#include "orbfe_fast_body.inc"
}

// FM_LDS_CONSTS is an A/B path of the generic dense form only (k_fast_map above): the cell-row and the
// lane-compacting kernel share text with it (orbfe_fast_body.inc, orbfe_fast_colmask.inc) and are compiled with the macro undefined.
#pragma push_macro("FM_LDS_CONSTS")
#undef FM_LDS_CONSTS

// The same pass over a lane list made of whole CELL ROWS, one run of rows per wave (orbfe_fast_body.inc with CELLROWS): what batch
// handles run.  k_fast_map above takes any run of rows per lane (handles made for a few frames per call walk short runs: a small
// call is bound by the length of one wave's walk).
template <int SPARSE>
__global__ __launch_bounds__(256) FM_OCC void k_fast_map_u(const OrbPlan *__restrict__ plan, FrameSrc fs,
                                                    const OrbLane *__restrict__ lanes, int nwaves,
                                                    uint2 *__restrict__ skeys, int32_t *__restrict__ scount,
                                                    uint32_t *__restrict__ cflags, int32_t cf_words,
                                                    unsigned long long *__restrict__ fstat)
{
    FM_SHARED_DECLS
    int b = blockIdx.y, bx = blockIdx.x;
    xcd_frame_remap(bx, b);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int t = bx * (blockDim.x >> 6) + wv;
    if (t >= nwaves) return;
    constexpr bool CELLROWS = true;
#include "orbfe_fast_body.inc"
}

// The lane-compacting form of the same pass (orbfe_fast_body_c.inc): per wave a ring of the pixel rows its lanes fetched (one dword
// per lane and row, 2 x FC_PN slots of FC_PW dwords), a queue of FC_QCAP one-dword tags of parked pixel pairs, four strength rows
// in flight (a byte per pixel) and the survivor staging buffer -- 7.4 KB per wave and 96 registers: five waves per SIMD.
#define FC_QCAP 128      // tags (power of two); a push of <= 64 always finds room once the fill is <= FC_QCAP - 64
#ifndef FC_LAG
#define FC_LAG 3         // rows the suppression runs behind the front: an item never waits longer
#endif
#define FC_PN (6 + FC_LAG)   // rows the pixel ring holds: what step s parked is evaluated before the row of step s + FC_LAG is written
#define FC_PW 66         // dwords per ring slot: the 64 lanes + a pad on both sides
#define FC_SEAMS 16      // lanes of a wave whose pixel pair straddles a cell seam (cells are >= 30 px wide: <= 9)
#define FC_BUF (128 + FC_SEAMS)   // survivor staging: one row's worth; flushed when the next row might not fit
#ifndef FC_OCC
#define FC_OCC
#endif
static_assert(FC_LAG >= 1 && FC_LAG <= 3, "the strength-row ring (srow / snap, 4 slots) is re-used by the front half of step s + 4: the back half of step s must have read it, i.e. lag <= 3");
static_assert(FC_PN >= 6 + FC_LAG && FC_PN >= 7, "pixel ring: the first row of an item parked at step s is overwritten at step s - 6 + FC_PN");
__global__ __launch_bounds__(256) FC_OCC void k_fast_map_c(const OrbPlan *__restrict__ plan, FrameSrc fs,
                                                    const OrbLane *__restrict__ lanes, int nwaves,
                                                    uint2 *__restrict__ skeys, int32_t *__restrict__ scount,
                                                    uint32_t *__restrict__ cflags, int32_t cf_words,
                                                    unsigned long long *__restrict__ fstat)  // {row steps, batches, parked pairs} of sampled waves, or null
{
    __shared__ uint32_t s_pix[4][2 * FC_PN * FC_PW];
#ifdef FC_EXTRA_LDS   // occupancy probe: dead LDS that costs a workgroup slot per CU
    __shared__ uint32_t s_fcpad[FC_EXTRA_LDS / 4];
    if (nwaves < 0) s_fcpad[threadIdx.x] = 1u;
    if (nwaves < -1) scount[0] = (int32_t)s_fcpad[threadIdx.x ^ 1];
#endif
    __shared__ uint32_t s_q[4][FC_QCAP];
    __shared__ uint32_t s_srow[4][4 * 64];
    __shared__ uint2 s_buf[4][FC_BUF];
    extern __shared__ uint32_t s_cf[];
    int b = blockIdx.y, bx = blockIdx.x;
    xcd_frame_remap(bx, b);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int t = bx * (blockDim.x >> 6) + wv;
    if (t >= nwaves) return;
#include "orbfe_fast_body_c.inc"
}
#pragma pop_macro("FM_LDS_CONSTS")

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t orbk_clear_fast(const OrbLaunch &a, hipStream_t st)
{
    // the survivor counts and, right behind them, the cell flags of this call's frames: one clear
    const int nl = a.h_plan->nlevels;
    if ((const char *)a.d_cflag != (const char *)a.d_scount + sizeof(int32_t) * (size_t)a.nframes * nl * ORBFE_NK_STRIDE)
        return hipErrorInvalidValue;
    return hipMemsetAsync(a.d_scount, 0, sizeof(int32_t) * (size_t)a.nframes * nl * ORBFE_NK_STRIDE +
                                             sizeof(uint32_t) * (size_t)a.nframes * nl * a.cf_words, st);
}

// one launch of a dense form (k_fast_map<S> / k_fast_map_u<S>) over the whole lane list
template <typename Kernel>
static void fast_launch_dense(Kernel kernel, const OrbLaunch &a, unsigned long long *fstat, hipStream_t st)
{
    hipLaunchKernelGGL(kernel, dim3((a.h_plan->nfwaves + 3) / 4, a.nframes), dim3(256), (size_t)a.cf_words * 16, st, a.d_plan, make_src(a),
                       a.d_flanes, a.h_plan->nfwaves, a.d_skeys, a.d_scount, a.d_cflag, a.cf_words, fstat);
}

hipError_t orbk_launch_fast(const OrbLaunch &a, hipStream_t st)
{
    unsigned long long *const nostat = nullptr;   // the dense instantiations keep no statistics
    if (a.fast_sparse == 2)
        hipLaunchKernelGGL(k_fast_map_c, dim3((a.h_plan->nfwaves_c + 3) / 4, a.nframes), dim3(256), (size_t)a.cf_words * 16, st, a.d_plan,
                           make_src(a), a.d_flanes_c, a.h_plan->nfwaves_c, a.d_skeys, a.d_scount, a.d_cflag, a.cf_words, a.d_fstat);
    else if (a.h_plan->fast_cellrows) {
        if (a.fast_sparse) fast_launch_dense(k_fast_map_u<1>, a, a.d_fstat, st);
        else fast_launch_dense(k_fast_map_u<0>, a, nostat, st);
    } else if (a.fast_sparse)
        fast_launch_dense(k_fast_map<1>, a, a.d_fstat, st);
    else
        fast_launch_dense(k_fast_map<0>, a, nostat, st);
    return hipGetLastError();
}
