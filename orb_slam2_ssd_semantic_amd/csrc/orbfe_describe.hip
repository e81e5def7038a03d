// orbfe_describe.hip -- K5, orientation + steered BRIEF + keypoint assembly (k_orient_describe), and the constant tables it reads.
#include "orbfe_kernels_dev.h"
#include "orbfe_pattern.inc"

// (the library is built without relocatable device code: a __constant__ table lives in the file of the kernel that reads it)
__constant__ signed char c_pattern[1024];
// umax[v] of the circular patch (src/ORBextractor.cc:449-465): {15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3}
__constant__ int c_umax[16];

hipError_t orbk_upload_moment_weights(const int *umax16);

hipError_t orbk_upload_constants(const int *umax16)
{
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_pattern), orbfe_pattern31_host, 1024);
    if (e != hipSuccess) return e;
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_umax), umax16, 16 * sizeof(int));
    if (e != hipSuccess) return e;
    return orbk_upload_moment_weights(umax16);
}

// ---------------------------------------------------------------------------------------------------
// K5  IC_Angle + steered BRIEF + keypoint assembly.  One wave per output slot.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
    // cv::fastAtan2 (OpenCV 3.2 atan_f32), every operation rounded separately
    const float s = (float)(180 / 3.1415926535897932384626433832795);
    const float p1 = __fmul_rn(0.9997878412794807f, s), p3 = __fmul_rn(-0.3258083974640975f, s);
    const float p5 = __fmul_rn(0.1555786518463281f, s), p7 = __fmul_rn(-0.04432655554792128f, s);
    const float eps = (float)2.2204460492503131e-16;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps));
        c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps));
        c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// canonical (float)cos / (float)sin of angle_deg * pi/180: fixed fp64 operation sequence
__device__ __forceinline__ void canon_sincos(float angle_deg, float *ca, float *sb)
{
    const float factor_pi = (float)(3.1415926535897932384626433832795 / 180.f);
    const float angle = __fmul_rn(angle_deg, factor_pi);
    const double x = (double)angle;
    const double kf = floor(__dadd_rn(__dmul_rn(x, 6.36619772367581382433e-01), 0.5));
    const int k = (int)kf;
    const double r = __dsub_rn(__dsub_rn(x, __dmul_rn(kf, 1.57079632673412561417e+00)),
                               __dmul_rn(kf, 6.07710050650619224932e-11));
    const double z = __dmul_rn(r, r);
    double ps = __dadd_rn(-2.50507602534068634195e-08, __dmul_rn(z, 1.58969099521155010221e-10));
    ps = __dadd_rn(2.75573137070700676789e-06, __dmul_rn(z, ps));
    ps = __dadd_rn(-1.98412698298579493134e-04, __dmul_rn(z, ps));
    ps = __dadd_rn(8.33333333332248946124e-03, __dmul_rn(z, ps));
    ps = __dadd_rn(-1.66666666666666324348e-01, __dmul_rn(z, ps));
    const double sn = __dadd_rn(r, __dmul_rn(__dmul_rn(z, r), ps));
    double pc = __dadd_rn(2.08757232129817482790e-09, __dmul_rn(z, -1.13596475577881948265e-11));
    pc = __dadd_rn(-2.75573143513906633035e-07, __dmul_rn(z, pc));
    pc = __dadd_rn(2.48015872894767294178e-05, __dmul_rn(z, pc));
    pc = __dadd_rn(-1.38888888888741095749e-03, __dmul_rn(z, pc));
    pc = __dadd_rn(4.16666666666666019037e-02, __dmul_rn(z, pc));
    const double cs = __dsub_rn(1.0, __dsub_rn(__dmul_rn(0.5, z), __dmul_rn(__dmul_rn(z, z), pc)));
    double s, c;
    switch (k & 3) {
    case 0: s = sn; c = cs; break;
    case 1: s = cs; c = -sn; break;
    case 2: s = -sn; c = -cs; break;
    default: s = -cs; c = sn; break;
    }
    *ca = __double2float_rn(c);
    *sb = __double2float_rn(s);
}

// 16 lanes per keypoint, 4 keypoints per wave, 4 waves per workgroup.
//   A  IC_Angle moments: the 31 rows of the patch as 8 unaligned dwords each; a lane takes dword k = sub & 7 of rows
//      (sub >> 3) + 2i.  m10 and the row sums come from v_dot4_u32_u8 against per-(row, dword) weight bytes
//      ((u + 15) inside the circle, 1 inside the circle), reduced over the 16 lanes -- integer, any order is exact.
//   B  fastAtan2 / canonical sincos per lane (16x redundant instead of 64x).
//   C  rBRIEF: the 37 x 40 blurred patch is staged in LDS with coalesced dword loads; lane `sub` evaluates pairs
//      16*sub .. 16*sub+15, i.e. descriptor bytes 2*sub and 2*sub+1, from LDS byte reads.
#ifndef DS_PP
#define DS_PP 40   // LDS patch pitch (bytes): columns x-18 .. x+21 (44 = an odd number of dwords per row: A/B in DESIGN.md)
#endif
#define DS_PR 37   // patch rows y-18 .. y+18

__constant__ uint2 c_momw[31 * 8];  // per (row v+15, dword k): .x = weights (u+15) or 0, .y = 1 or 0 per byte

// circular patch of IC_Angle (src/ORBextractor.cc:59-88): row v covers u in [-umax[|v|], umax[|v|]]
hipError_t orbk_upload_moment_weights(const int *umax16)
{
    uint2 h[31 * 8];
    for (int row = 0; row < 31; ++row) {
        const int v = row - 15, d = umax16[v < 0 ? -v : v];
        for (int k = 0; k < 8; ++k) {
            uint32_t w10 = 0, w1 = 0;
            for (int i = 0; i < 4; ++i) {
                const int u = 4 * k + i - 15;
                if (u >= -d && u <= d) {
                    w10 |= (uint32_t)(u + 15) << (8 * i);
                    w1 |= 1u << (8 * i);
                }
            }
            h[row * 8 + k] = make_uint2(w10, w1);
        }
    }
    return hipMemcpyToSymbol(HIP_SYMBOL(c_momw), h, sizeof(h));
}

// Keypoints per workgroup (16 lanes each).  The pattern and moment-weight tables (6 KB) are per workgroup and a keypoint's
// blurred patch takes 1480 B of LDS: 16 keypoints -> 30 KB, 5 workgroups = 80 keypoints per CU; 32 keypoints -> 53 KB, 3
// workgroups = 96 keypoints per CU (A/B: profiles/r04_ab_experiments.json).
#ifndef DS_KPW
#define DS_KPW 16
#endif
// Launch geometry: a workgroup belongs to ONE level (its DS_KPW keypoints are consecutive entries of that level's selection), so
// the address of a keypoint's key follows from the block index and the kernel arguments alone -- no count, no plan in memory in
// front of it.  The dependent chain of a workgroup is then TWO round trips: {all level counts, the keys}, then {the 16 moment
// dwords and the 24 blurred-patch dwords of every lane, requested back to back}; it used to be four (counts + plan, key, moment
// pixels, patch pixels), and with a wave's 2.9 k cycles of arithmetic against tens of thousands of cycles of waiting the chain
// length is part of what the kernel's time follows (-7 %).  The output slot of a keypoint (level-major, :1103-1112) needs the
// counts of the levels before its own: they arrive with the key and are used only by the stores at the very end.
struct DescLevelArg { int32_t sel_off, off, pitch, wg0; float scale, patch_size; int32_t pad[2]; };   // wg0: first workgroup of the level
struct DescArgs {
    int32_t wg0[ORBFE_MAX_LEVELS];   // the same, side by side: one scalar load for the level scan (levels past the last: INT_MAX)
    int32_t nwg;                     // workgroups that belong to a level: sum over the levels of ceil(sel_cap / DS_KPW)
    int32_t pad[3];
    DescLevelArg lv[ORBFE_MAX_LEVELS];
};
__global__ __launch_bounds__(DS_KPW * 16) void k_orient_describe(DescArgs da, FrameSrc fs,
                                                         const uint8_t *__restrict__ blur, int64_t blur_fstride,
                                                         const uint32_t *__restrict__ sel,
                                                         const int32_t *__restrict__ nsel,
                                                         orbfe_keypoint *__restrict__ kps,
                                                         uint8_t *__restrict__ desc, int32_t cap,
                                                         int32_t *__restrict__ n_out, int32_t nl,
                                                         int32_t sel_per_frame, int32_t *__restrict__ ovf)
{
#ifndef DS_PATCH_PAD
#define DS_PATCH_PAD 0   // bytes between the patches of neighbouring keypoints (A/B of a bank stagger: profiles/r06_ab_describe_pad.json)
#endif
    __shared__ __attribute__((aligned(16))) uint8_t s_patch[DS_KPW][DS_PR * DS_PP + DS_PATCH_PAD];
    __shared__ uint2 s_momw[31 * 8];
    __shared__ float4 s_pat[256];  // (x0, y0, x1, y1) of every test pair as floats
#ifdef DS_EXTRA_LDS   // occupancy probe: dead LDS that costs a workgroup slot per CU
    __shared__ uint32_t s_pad[DS_EXTRA_LDS / 4];
    if (nl < 0) s_pad[threadIdx.x] = 1u;
    if (nl < -1) ovf[0] = (int32_t)s_pad[threadIdx.x ^ 1];
#endif
    int b = blockIdx.y, bx = blockIdx.x;
    xcd_frame_remap(bx, b);
    b = __builtin_amdgcn_readfirstlane(b);  // workgroup-uniform: frame offsets are scalar 64-bit products
    bx = __builtin_amdgcn_readfirstlane(bx);
    const int tid = threadIdx.x, lane = tid & 63;
    const int sub = lane & 15, quad = tid >> 4;  // quad 0..DS_KPW-1 inside the workgroup = one keypoint
    // the level of this workgroup (scalar scan of the kernel arguments); workgroups behind the levels' only pad the output
    int level = -1;
    if (bx < da.nwg) {
        level = 0;
#pragma unroll
        for (int j = 1; j < ORBFE_MAX_LEVELS; ++j) level += bx >= da.wg0[j] ? 1 : 0;   // ascending; INT_MAX past the last level
    }
    const int lv = max(level, 0);
    const DescLevelArg L = da.lv[lv];
    const int idx = (bx - L.wg0) * DS_KPW + quad;   // index inside the level's selection
    // ---- round trip 1: the counts of all levels (lane `sub` of every 16-lane group holds level `sub`'s) and the key ----
    static_assert(ORBFE_MAX_LEVELS == 16, "level counts: one level per lane of a 16-lane group");
    const int cnt_l = sub < nl ? nsel[b * nl + sub] : 0;
    uint32_t key = 0;
    // entries behind the level's count are stale but inside its slice of the scratch (sel_cap rounded up to 64): read, not used
    if (level >= 0) key = sel[(int64_t)b * sel_per_frame + L.sel_off + idx];
    // ... and the two tables, requested in the same round trip (both loads before either LDS store: the load counter is in order)
    static_assert(DS_KPW * 16 >= 256, "table fill: one pattern entry and one moment-weight entry per thread");
    const uint2 mw = c_momw[min(tid, 31 * 8 - 1)];
    const uint32_t pt = ((const uint32_t *)c_pattern)[tid & 255];
    if (tid < 31 * 8) s_momw[tid] = mw;
    if (tid < 256) {
        // pair p = 16 * sub + i is stored at [i][sub]: the 16 lanes of a keypoint read consecutive float4s
        s_pat[(tid & 15) * 16 + (tid >> 4)] = make_float4((float)(int8_t)(pt & 0xFF), (float)(int8_t)((pt >> 8) & 0xFF),
                                                         (float)(int8_t)((pt >> 16) & 0xFF), (float)(int8_t)(pt >> 24));
    }
    // inclusive prefix sums of the level counts across the group's lanes (four DPP row shifts)
    int incl = cnt_l;
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xF, 0xF, true);   // row_shr:1 (lanes without a source add 0)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xF, 0xF, true);   // row_shr:2
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xF, 0xF, true);   // row_shr:4
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xF, 0xF, true);   // row_shr:8
    const int total = __builtin_amdgcn_readlane(incl, 15);                 // the same in every group: scalar
    const int mine = __builtin_amdgcn_readlane(cnt_l, lv);                 // keypoints of this workgroup's level
    const int before = lv > 0 ? __builtin_amdgcn_readlane(incl, max(lv - 1, 0)) : 0;   // keypoints of the levels in front of it
    if (bx == 0 && tid == 0) {
        n_out[b] = total;
        if (total > cap) atomicOr(ovf, 4);  // n_out holds the required count; slots >= cap are not written
    }
    {   // zero-fill the padding so the buffers can be all-gathered as they are: workgroup g takes slots total + 16 g ...
        // (the grid has at least cap / DS_KPW workgroups)
        const int zs = total + bx * DS_KPW + quad;
        if (zs < cap) {
            if (sub < 7) ((uint32_t *)(kps + (int64_t)b * cap + zs))[sub] = 0u;
            if (sub < 8) ((uint32_t *)(desc + ((int64_t)b * cap + zs) * 32))[sub] = 0u;
        }
    }
    // A workgroup behind its level's last keypoint (the levels' capacities are what the grid covers), or behind the levels: done.
    // Workgroup-uniform, before the barriers.
    if (level < 0 || (bx - L.wg0) * DS_KPW >= mine) return;
    const int slot = before + idx;
    const bool live = idx < mine && slot < cap;
    orbfe_keypoint *kp = kps + (int64_t)b * cap + slot;
    uint8_t *dd = desc + ((int64_t)b * cap + slot) * 32;
    // dead quads shadow a valid position so that every lane can run the same loads
    const int x = live ? orb_key_x(key) : ORBFE_EDGE, y = live ? orb_key_y(key) : ORBFE_EDGE;
    const int pitch = lv == 0 ? fs.l0_pitch : L.pitch;
    const uint8_t *img = lv == 0 ? fs.l0 + (int64_t)b * fs.l0_fstride : fs.pyr + (int64_t)b * fs.pyr_fstride + L.off;

    // ---- round trip 2: the moment dwords (unblurred level) and the blurred patch of every lane, requested back to back ----
    const int mk = sub & 7, mr0 = sub >> 3;
    uint32_t w[16];
    {
        // 32-bit offsets from 24-bit multiplies (the 32-bit multiply and the 64-bit multiply-add are quarter rate):
        // rows r0, r0 + 2, ...; the 16th row of the odd lanes (31) is clamped to 30 and not used
        const uint8_t *p = img + (__umul24((uint32_t)(y - 15 + mr0), (uint32_t)pitch) + (uint32_t)(x - 15 + 4 * mk));
        // unaligned dwords; the pointer advances by two rows per load (one 64-bit add each instead of a multiply and an add);
        // the last step of the odd lanes is one row (row 30, clamped)
        const uint32_t step2 = 2u * (uint32_t)pitch, step_last = __umul24((uint32_t)(2 - mr0), (uint32_t)pitch);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            w[i] = *(const uint32_t *)p;
            p += i < 14 ? step2 : step_last;
        }
    }
    uint8_t *patch = s_patch[quad];
    uint32_t v[24];
    {
        const int bpitch = L.pitch;
        // uniform base (frame b of the blurred pyramid) + a 32-bit per-lane offset that advances by additions
        typedef const __attribute__((address_space(1))) uint8_t *orb_gptr8;    // global memory, explicitly
        typedef const __attribute__((address_space(1))) uint32_t *orb_gptr32;
        orb_gptr8 bbase;
        {   // pinned to a scalar register pair: the loads below then take it as their SGPR base (the 64-bit product is formed
            // on the vector side, where the compiler no longer knows it is uniform)
            const uint64_t bb = (uint64_t)(blur + (int64_t)b * blur_fstride);
            const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bb);
            const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bb >> 32));
            bbase = (orb_gptr8)(((uint64_t)hi32 << 32) | lo32);
        }
        // dword f = it * 16 + sub of the 37 x 10 dword patch (16 consecutive dwords per step: a row and the start of the
        // next).  With the LDS pitch equal to the 40 patch bytes the LDS offset is simply 4 * f; the row of f is
        // (f * 205) >> 11 (= f / 10 for f < 1029) and the global offset  base + row * (pitch - 40) + 4 * f,  whose
        // "+ 64 * it" rides in the load's immediate offset: three VALU operations per load (the incremental carry logic this
        // replaces took ten).
        static_assert(DS_PR == 37 && DS_PP == 40, "patch staging: LDS pitch == patch bytes");
        uint32_t s205 = (uint32_t)sub * 205u;
        // kept as a value of its own: folded into a multiply-add with the step's constant, every load pays a register move for that
        // constant (the multiply-add cannot take a literal next to its scalar operand); as an addend it takes the literal directly
        asm volatile("" : "+v"(s205));
        const uint32_t bp40 = (uint32_t)bpitch - 40u;
        // uniform base + one 32-bit per-lane offset + immediate: a global_load with an SGPR base, no 64-bit address arithmetic
        const uint32_t o4 = (uint32_t)L.off + __umul24((uint32_t)(y - 18), (uint32_t)bpitch) + (uint32_t)(x - 18 + 4 * sub);
#pragma unroll
        for (int it = 0; it < 23; ++it) {
            const uint32_t row = (s205 + (uint32_t)(it * 16 * 205)) >> 11;
            const uint32_t o = o4 + __umul24(row, bp40);
            v[it] = *(orb_gptr32)((bbase + it * 64) + o);  // unaligned dword
        }
        {   // f = 368 + sub: only f = 368, 369 (row 36, columns 8, 9) exist; the other lanes re-read 369 and store nothing
            const uint32_t fl = 368u + (uint32_t)min(sub, 1);
            v[23] = *(orb_gptr32)(bbase + ((uint32_t)L.off + __umul24((uint32_t)(y + 18), (uint32_t)bpitch) + (uint32_t)(x - 18) + 4u * (fl - 360u)));
        }
    }
    __syncthreads();   // the tables (moment weights, pattern) are in LDS
    // ---- A: moments ----
    int m10 = 0, rs15 = 0, m01 = 0;
    {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = mr0 + 2 * i;
            if (row <= 30) {
                const uint2 wt = s_momw[row * 8 + mk];
                const uint32_t a = __builtin_amdgcn_udot4(w[i], wt.x, 0u, false);  // sum (u+15) * I
                const uint32_t s1 = __builtin_amdgcn_udot4(w[i], wt.y, 0u, false); // sum I
                m10 += (int)a;
                rs15 += (int)s1;
                m01 += __mul24(row - 15, (int)s1);  // |row - 15| <= 15, s1 <= 1020
            }
        }
        m10 -= 15 * rs15;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            m10 += __shfl_xor(m10, o, 64);
            m01 += __shfl_xor(m01, o, 64);
        }
    }
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    // ---- C: blurred patch -> LDS ----
    {
        uint8_t *pl = patch + 4 * sub;
#pragma unroll
        for (int it = 0; it < 23; ++it) *(uint32_t *)(pl + it * 64) = v[it];
        if (sub < 2) *(uint32_t *)(pl + 23 * 64) = v[23];
    }
    float a, bb;
    canon_sincos(angle, &a, &bb);
    __syncthreads();
    const uint8_t *pc = patch + 18 * DS_PP + 18;
    uint32_t bits = 0;
    // rotated sample positions (:100-106): row = cvRound(x*b + y*a), col = cvRound(x*a - y*b), every product and sum
    // rounded separately.  Two coordinates per packed-fp32 instruction; x*a - y*b == x*a + y*(-b) exactly.
    // cvRound by the 1.5 * 2^23 trick: the fp32 add rounds to the nearest integer, ties to even, and leaves it in
    // the low mantissa bits.
    typedef float orb_f2 __attribute__((ext_vector_type(2)));
    const orb_f2 ba = {bb, a}, anb = {a, -bb}, magic = {12582912.f, 12582912.f};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 pt = s_pat[i * 16 + sub];
        const orb_f2 p0 = orb_f2{pt.x, pt.x} * ba + orb_f2{pt.y, pt.y} * anb + magic;  // (row0, col0) + magic
        const orb_f2 p1 = orb_f2{pt.z, pt.z} * ba + orb_f2{pt.w, pt.w} * anb + magic;
        const int r0 = (int)(short)__float_as_int(p0.x), c0 = __float_as_int(p0.y) - 0x4B400000;
        const int r1 = (int)(short)__float_as_int(p1.x), c1 = __float_as_int(p1.y) - 0x4B400000;
        const int t0 = pc[r0 * DS_PP + c0], t1 = pc[r1 * DS_PP + c1];
        bits |= (uint32_t)(t0 < t1) << i;
    }
    if (live) {
        ((uint16_t *)dd)[sub] = (uint16_t)bits;
        if (sub == 0) {
            float fx = (float)x, fy = (float)y;
            if (level != 0) {  // pt *= mvScaleFactor[level] (:1104-1110)
                fx = __fmul_rn(fx, L.scale);
                fy = __fmul_rn(fy, L.scale);
            }
            kp->x = fx;
            kp->y = fy;
            kp->size = L.patch_size;
            kp->angle = angle;
            kp->response = (float)orb_key_r(key);
            kp->octave = level;
            kp->class_id = -1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t orbk_launch_describe(const OrbLaunch &a, hipStream_t st)
{
    const FrameSrc fs = make_src(a);
    const OrbPlan &P = *a.h_plan;
    DescArgs da;
    int wg = 0;
    for (int l = 0; l < ORBFE_MAX_LEVELS; ++l) {
        const OrbLevel &L = P.lv[l < P.nlevels ? l : 0];
        da.lv[l] = DescLevelArg{L.sel_off, L.off, L.pitch, wg, L.scale, L.patch_size, {0, 0}};
        da.wg0[l] = l < P.nlevels ? wg : 0x7FFFFFFF;
        if (l < P.nlevels) wg += (L.sel_cap + DS_KPW - 1) / DS_KPW;
    }
    da.nwg = wg;
    da.pad[0] = da.pad[1] = da.pad[2] = 0;
    // the workgroups of the levels; at least cap / DS_KPW of them: workgroup g also zero-fills the output slots total + 16 g ...
    dim3 grid(std::max(wg, (a.cap + DS_KPW - 1) / DS_KPW), a.nframes);
    hipLaunchKernelGGL(k_orient_describe, grid, dim3(DS_KPW * 16), 0, st, da, fs, a.d_blur, a.pyr_fstride, a.d_sel,
                       a.d_nsel, a.d_kps, a.d_desc, a.cap, a.d_n_out, P.nlevels, P.sel_per_frame, a.d_ovf);
    return hipGetLastError();
}
