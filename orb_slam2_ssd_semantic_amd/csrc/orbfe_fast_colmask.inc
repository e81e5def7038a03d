// orbfe_fast_colmask.inc -- the per-lane column masks of a FAST lane, included TEXTUALLY by the dense body (orbfe_fast_body.inc) and
// the lane-compacting body (orbfe_fast_body_c.inc).  Expects in scope: x (first pixel of the lane), ix0, ix1, wcell, ld, lane, wv.
// Leaves: ccj / mj (cell column and x in cell of the lane's four pixels), inside / lvalid / rvalid and their half-word masks
// in01 .. rv23, split01 / split23 / wave_split, out_lane.  The FM_LDS_CONSTS path (masks parked in LDS: s_lcm, s_lcr, s_lco of
// FM_LDS_DECLS) exists for the generic dense kernels only; the other kernels are compiled with the macro undefined (orbfe_fast.hip).
    // per-lane column masks: bit j = pixel j inside the interior / has a valid left / right neighbour in its cell
    // (cell column, x in cell) of the lane's four pixels from ONE division: pixel j + 1 is one step to the right of pixel j
    // (columns left of the interior count as its first column, as `ord` below wants them)
    int ccj[4], mj[4];
    {
        const int r0 = max(x - ix0, 0);
        int c = r0 / wcell, m = r0 - c * wcell;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j > 0 && x + j - ix0 >= 1) {
                ++m;
                if (m == wcell) { m = 0; ++c; }
            }
            ccj[j] = c;
            mj[j] = m;
        }
    }
    int inside = 0, lvalid = 0, rvalid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xx = x + j;
        if (xx >= ix0 && xx < ix1) {
            const int m = mj[j];
            inside |= 1 << j;
            if (m != 0) lvalid |= 1 << j;
            if (m != wcell - 1 && xx + 1 < ix1) rvalid |= 1 << j;
        }
    }
    auto halves = [](int bits, int j) -> uint32_t {
        return (((bits >> j) & 1) ? 0xFFFFu : 0u) | (((bits >> (j + 1)) & 1) ? 0xFFFF0000u : 0u);
    };
#ifdef FM_LDS_CONSTS
    s_lcm[wv][lane] = make_uint4(halves(inside, 0), halves(inside, 2), halves(lvalid, 0), halves(lvalid, 2));
    s_lcr[wv][lane] = make_uint2(halves(rvalid, 0), halves(rvalid, 2));
    // the address is laundered through an empty asm at every use, so the loads stay where they are written (a loop-invariant
    // load would be hoisted back into registers)
    uint32_t lc_m = (uint32_t)(uintptr_t)&s_lcm[wv][lane], lc_r = (uint32_t)(uintptr_t)&s_lcr[wv][lane], lc_o = (uint32_t)(uintptr_t)&s_lco[wv][lane];
    typedef uint32_t fm_v4 __attribute__((ext_vector_type(4)));
    typedef uint32_t fm_v2 __attribute__((ext_vector_type(2)));
#define FM_LC_LOAD(type, addr) ({ asm volatile("" : "+v"(addr)); *(const __attribute__((address_space(3))) type *)(uintptr_t)(addr); })
#else
    const uint32_t in01 = halves(inside, 0), in23 = halves(inside, 2);
    const uint32_t lv01 = halves(lvalid, 0), lv23 = halves(lvalid, 2);
    const uint32_t rv01 = halves(rvalid, 0), rv23 = halves(rvalid, 2);
#endif
    // a cell seam between the two pixels of a pair lets BOTH be NMS survivors; at most one pair of a lane has one
    const bool split01 = (inside & 3) == 3 && !(lvalid & 2), split23 = (inside & 12) == 12 && !(lvalid & 8);
    const bool wave_split = orb_ballot(split01 || split23) != 0ull;
    const bool out_lane = !(ld.flags & 1) && inside != 0;
