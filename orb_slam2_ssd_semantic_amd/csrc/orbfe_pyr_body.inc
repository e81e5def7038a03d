// orbfe_pyr_body.inc -- the row walk of one resize workgroup (K1, see orbfe_pyramid.hip) in its per-lane form, included TEXTUALLY by
// k_fast_pyr.  Expects in scope: a (PyrArgs), bxi (index of the workgroup among the resize workgroups of its frame), b (frame).
    extern __shared__ uint2 s_dyn[];
    uint2 *s_yt = s_dyn;                                   // [dh + 8]: .x = b0 | b1 << 16, .y = sy (low half)
    uint32_t *s_out = (uint32_t *)(s_dyn + (a.dh + 8));    // [rb][256]
    const int W = a.dw, H = a.dh;
    for (int i = threadIdx.x; i < H + 8; i += 256) s_yt[i] = ((const uint2 *)a.ytab)[i];
    const int ncol4 = (W + 3) >> 2;
    const int nlanes = ncol4 * a.nrblk;
    const int fl = min((int)(bxi * 256 + threadIdx.x), nlanes - 1);  // surplus lanes repeat the last lane's work
    const int rblk = fl / ncol4;
    const int dx0 = (fl - rblk * ncol4) * 4;
    const int y0 = rblk * a.rb, yend = min(y0 + a.rb, H);
    const uint8_t *src = a.src + (int64_t)b * a.src_fstride;
    uint8_t *dst = a.dst + (int64_t)b * a.dst_fstride;

    const uint4 tx01 = *(const uint4 *)(a.xtab + dx0), tx23 = *(const uint4 *)(a.xtab + dx0 + 2);
    const uint32_t xc[4] = {tx01.x, tx01.z, tx23.x, tx23.z};
    const int xs[4] = {(int)(short)tx01.y, (int)(short)tx01.w, (int)(short)tx23.y, (int)(short)tx23.w};
    const int sx0 = min(xs[0], a.sw - 8);
    uint32_t sel[4];
    orb_u2 coef[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t o = (uint32_t)min(max(xs[j] - sx0, 0), 7);
        sel[j] = 0x0c000c00u | (min(o + 1u, 7u) << 16) | o;
        coef[j] = __builtin_bit_cast(orb_u2, xc[j]);
    }
    __syncthreads();
    uint2 cur = s_yt[y0];
    const int r0 = (int)(short)cur.y;
    int nsteps = (int)(short)s_yt[yend - 1].y + 2 - r0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nsteps = max(nsteps, __shfl_xor(nsteps, o, 64));
    nsteps = __builtin_amdgcn_readfirstlane(nsteps);
    const uint32_t sp = (uint32_t)a.spitch;
    const int rlast = a.sh - 1;
    // uniform base + 32-bit per-lane offset (global_load with an SGPR base)
    auto fetch = [&](int s, uint2 &q) { q = *(const uint2 *)(src + (__umul24((uint32_t)min(r0 + s, rlast), sp) + (uint32_t)sx0)); };
    auto hsum = [&](const uint2 &q, uint32_t (&h)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            h[j] = __builtin_amdgcn_udot2(__builtin_bit_cast(orb_u2, __builtin_amdgcn_perm(q.y, q.x, sel[j])), coef[j], 0u, false) >> 4;
    };
    uint2 raw[4];
    fetch(0, raw[0]);
    fetch(1, raw[1]);
    fetch(2, raw[2]);
    uint32_t Hp[4];
    hsum(raw[0], Hp);  // step 0: source row sy(y0), completes nothing
    int d = y0;
    uint32_t *park = s_out + threadIdx.x;
    // steps run in groups of four (static ring indices, no exit inside a group): surplus steps re-read the clamped last
    // row and complete nothing
    for (int s0 = 1; s0 < nsteps; s0 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int s = s0 + k;
            fetch(s + PW_PF, raw[(k + 1 + PW_PF) % 4]);
            uint32_t Hs[4];
            hsum(raw[(k + 1) % 4], Hs);
            const bool emit = d < yend && (int)(short)cur.y + 1 == r0 + s;
            // ((b0 * H0) >> 16) + ((b1 * H1) >> 16) + 2: the "+ 2" rides in the second product (+ 2 << 16, no carry
            // into it from below), the two ">> 16" are the SDWA word selects of one add, whose result lands in the low /
            // high half of a pair register; ">> 2" is then one packed shift per pixel pair
            const uint32_t b0 = cur.x & 0xFFFFu, b1 = cur.x >> 16;
            uint32_t pa[4], pb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pa[j] = __umul24(b0, Hp[j]);
                pb[j] = __umul24(b1, Hs[j]) + 0x20000u;
            }
            uint32_t t01, t23;
            asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(t01) : "v"(pa[0]), "v"(pb[0]));
            asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1" : "+v"(t01) : "v"(pa[1]), "v"(pb[1]));
            asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_1" : "=v"(t23) : "v"(pa[2]), "v"(pb[2]));
            asm("v_add_u32_sdwa %0, %1, %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:WORD_1" : "+v"(t23) : "v"(pa[3]), "v"(pb[3]));
            const uint32_t q01 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(orb_u2, t01) >> (orb_u2)(2));
            const uint32_t q23 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(orb_u2, t23) >> (orb_u2)(2));
            if (emit) {
                *park = __builtin_amdgcn_perm(q23, q01, 0x06040200u);
                park += 256;
                d += 1;
            }
            cur = s_yt[d];
#pragma unroll
            for (int j = 0; j < 4; ++j) Hp[j] = Hs[j];
        }
    }
    // burst store of the run (every lane reads back its own LDS column: no barrier)
    uint32_t oofs = __umul24((uint32_t)y0, (uint32_t)a.dpitch) + (uint32_t)dx0;
    const int nrows = yend - y0;
    for (int i0 = 0; i0 < a.rb; i0 += 8) {
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = s_out[min(i0 + i, a.rb - 1) * 256 + threadIdx.x];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i0 + i < nrows) *(uint32_t *)(dst + (oofs + (uint32_t)(i0 + i) * (uint32_t)a.dpitch)) = v[i];
    }
