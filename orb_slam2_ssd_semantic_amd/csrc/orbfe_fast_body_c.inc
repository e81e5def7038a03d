// orbfe_fast_body_c.inc -- the FAST pass of one wave in its LANE-COMPACTING form (k_fast_map_c; VERDICT r4 next #4).
//
// Same results as the dense body (orbfe_fast_body.inc), other work distribution.  The dense form evaluates the 16 nine-arcs of
// EVERY pixel pair (the packed min / max network of fast_strength_pair).  Here every pair first takes the exact necessary test
// (15 operations: some opposite compass pair must both be brighter / darker than the centre by more than the threshold); a pair
// that passes -- 85 % on corner-saturated S frames, 19 % on camera-like S_tum frames -- leaves a ONE-DWORD TAG (lane, pair, row)
// in a wave-private LDS queue, and whenever 64 tags have gathered the 64 lanes of the wave evaluate one each: the seven rows of
// the pair's 12-byte window come from a wave-private LDS ring of the rows the lanes fetched (one dword per lane and row; the
// window of a lane is the dwords of lanes l - 1, l, l + 1), the network is the dense one unchanged (fast_strength_from), the
// strength goes to the (row, lane, pair) it belongs to in a 4-row LDS ring.  A pair that fails the test has strength 0 exactly
// (the test is necessary), which is what its slot is preset to.  The 3x3 suppression and the emission run FC_LAG rows behind the
// front, on the finished strength rows, as in the dense form.  An item never waits more than FC_LAG rows: a step first drains
// what the row FC_LAG steps back still has in the queue -- before its own row overwrites the oldest slot of the pixel ring.
//
// The lanes take their neighbours' pixels from the neighbouring LANES' dwords in that ring, not from memory: ONE dword load per
// lane and row instead of three, and no register ring of rows at all (the test reads the centre row with its two neighbour
// dwords and the row six steps back from the ring: 96 registers, five waves per SIMD -- the occupancy is worth more than the four
// LDS reads per step; A/B in DESIGN.md 11.4).  That
// needs the lane list of this form (build_plan: `clanes`): every piece of a strip inside a wave is closed by a halo lane on both
// sides -- at the image's side borders the 4-pixel column outside the detectable interior -- so every pixel whose strength is
// ever used has both neighbour dwords in the wave.  Pixels without them (the outer pixels of halo lanes) get strengths computed
// from zeros / a neighbouring piece's pixels: deterministic, masked or never read (the suppression reads column 3 of a left halo
// and column 0 of a right halo only, whose circles lie inside the piece).
// Expects in scope what the dense body expects, plus s_pix / s_q / s_srow.
    const int wvu = __builtin_amdgcn_readfirstlane(wv);   // the wave's index inside the workgroup is wave-uniform: LDS bases in SGPRs
    uint32_t *lflag = s_cf + wvu * cf_words;
    for (int i = lane; i < cf_words; i += 64) lflag[i] = 0u;  // wave-private: its own DS operations execute in order
    // Work is described per LANE: a 4-pixel column, a run of rows, "halo" (contributes neighbour strengths only).
    // The host packs the column strips of all row blocks of one level back to back into 64-lane waves, so narrow
    // levels do not leave lanes idle; neighbouring lanes are neighbouring columns inside one strip.
    const OrbLane ld = lanes[(int64_t)t * 64 + lane];
    const int level = __builtin_amdgcn_readfirstlane((int)(ld.flags >> 8));
    const OrbLevel &L = plan->lv[level];
    int pitch;
    const uint8_t *src = level_ptr(fs, L, level, b, &pitch);
    uint2 *slist = skeys + (int64_t)b * plan->keys_per_frame + L.key_off;
    int32_t *scnt = scount + (b * plan->nlevels + level) * ORBFE_NK_STRIDE;
    uint32_t *cflag = cflags + (int64_t)(b * plan->nlevels + level) * cf_words;
    const int ini_th = plan->ini_th;
    uint2 *sbuf = s_buf[wvu];
    int nbuf = 0;  // wave-uniform fill of sbuf
    int st_rows = 0, st_batches = 0;          // statistics of the sampled waves (wave-uniform)
    const int H = L.h, key_cap = L.key_cap;
    const int ix0 = ORBFE_EDGE, iy0 = ORBFE_EDGE, ix1 = L.ix1, iy1 = L.iy1;
    const int wcell = L.wcell, hcell = L.hcell;
    const int x = ld.x;                 // first pixel of this lane (16 <= x < ix1: the 12-byte row window is in the image)
    const int ys = ld.ys;
    int nsteps = ld.nrows;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nsteps = max(nsteps, __shfl_xor(nsteps, o, 64));
    nsteps = __builtin_amdgcn_readfirstlane(nsteps) + 8;  // wave-uniform, and the compiler knows it
    const int tz = max(plan->min_th, 1);

#include "orbfe_fast_colmask.inc"
    const int nrows_out = out_lane ? (int)ld.nrows : 0;
    // per-pixel part of `ord`, the rank key of the reference's candidate order (cell-row-major, raster inside a cell):
    // ord = (cell_row * ncc + cell_col) << 12 | y_in_cell << 6 | x_in_cell
    // (recomputed where a survivor is emitted -- rare on the frames this form is chosen for -- instead of living in four registers)
    auto ordx_of = [&](int j) -> uint32_t {
        const int rj = max(x + j - ix0, 0);
        const int c = rj / wcell;
        return ((uint32_t)c << 12) | (uint32_t)(rj - c * wcell);
    };
    int rmod = (ys - iy0) % hcell;                                  // y_in_cell of the next NMS row (per lane)
    uint32_t ordy = ((uint32_t)(((ys - iy0) / hcell) * L.ncc) << 12) | ((uint32_t)rmod << 6);
    const uint32_t ord_wrap = ((uint32_t)L.ncc << 12) - ((uint32_t)hcell << 6);  // added when a new cell row starts
    const uint32_t tzz = (uint32_t)tz * 0x00010001u;
    const uint32_t resp0 = (uint32_t)(tz - 1);
    const int ysrel = ys - 7 - iy0;                                 // strength row of step s, relative to iy0, minus s
    const uint32_t hrange = (uint32_t)(iy1 - iy0);
    // key of pixel 0 in the NMS row of step 0 (detection-window coordinates = level - 16, reference :831-832): at emission

    // Register ring, statically indexed under the 8-fold unroll (the pixel rows themselves live in the LDS ring only):
    uint32_t S01[8], S23[8];  // finished S of the pixel pairs (0,1), (2,3), ring slot = slot of the step that tested the row
#pragma unroll
    for (int k = 0; k < 8; ++k) S01[k] = S23[k] = 0u;
    // Image row of step s: ys - 4 + s.  Buffer addressing: the resource is the level of this frame with its exact extent, the lane's
    // offset is its first row and column, the step's row a scalar offset -- no address arithmetic per step.  A lane past its run
    // can ask for a row below the level: the range check answers 0 instead of reading (such rows never reach a result: their
    // strengths are computed against the impossible threshold of rows outside the interior).
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)src, 0, (H - 1) * pitch + L.w, 0x00020000);
    const int voff = (ys - 4) * pitch + x;
    auto fetch = [&](int s) -> uint32_t { return __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, s * pitch, 0); };
    uint32_t Raw = fetch(0);

    // ---- wave-private LDS ----------------------------------------------------------------------------------------------------
    // pixel ring: the row of step s lives in slots s % FC_PN and s % FC_PN + FC_PN (written twice, so that the seven rows of an
    // item are seven CONSECUTIVE slots from (s - 6) % FC_PN on, without a wrap); a slot is 64 dwords + one pad dword on both sides
    uint32_t *pix = s_pix[wvu];
    uint32_t *pixw = pix + 1 + lane;          // this lane's dword of slot 0
    if (lane < 2 * FC_PN) {                   // the pads, read by items of lanes 0 and 63 (results unused): defined once
        pix[lane * FC_PW] = 0u;
        pix[lane * FC_PW + FC_PW - 1] = 0u;
    }
    uint32_t *q = s_q[wvu];                   // the tag queue (ring of FC_QCAP dwords)
    uint32_t *srow = s_srow[wvu];             // [4][64] dwords = the strengths (<= 248: one byte each) of a lane's four pixels; slot of step s = s & 3
    int q_pushed = 0, q_popped = 0;           // wave-uniform, monotonic
    int snap[4] = {0, 0, 0, 0};               // q_pushed after the front half of the step that owns strength-row slot s & 3
    int ps = 0;                               // s % FC_PN of the step at hand (wave-uniform)
    const int nfront = nsteps;                // steps with a front half (a new image row)
    nsteps += FC_LAG;                         // the back half runs FC_LAG steps behind

    // 64 (or the last n) parked tags -> their strengths.  tag = lane | pair << 6 | (strength slot) << 7 | (first pixel slot) << 9
    // (The LDS traffic here is wave-private and crosses lanes: one lane's pixw / q / srow stores are read by other lanes.  The
    // hardware executes a wave's DS operations in order; the wave barriers below -- no instruction, a compiler fence -- keep the
    // compiler from moving a cross-lane read above the store it depends on.)
    auto batch = [&](int n) {                 // n wave-uniform, 1 .. 64
        __builtin_amdgcn_wave_barrier();
        if (lane < n) {
            const uint32_t tag = q[(q_popped + lane) & (FC_QCAP - 1)];
            const uint32_t il = tag & 63u, jb = (tag >> 6) & 1u;
            const uint32_t *pw = pix + (tag >> 9) * FC_PW + il;   // dwords of lanes il - 1, il, il + 1 of the item's first row
            // The pixel pair at window bytes (a, a + 1) of a row (byte i = pixel x - 4 + i of the item's lane) is one v_perm of the
            // dwords a >> 2 and (a >> 2) + 1; pair (2,3) of the lane sits two bytes further right: + 2 in both selector bytes
            // (a & 3 <= 3, so the selected bytes stay inside the two dwords).
            uint32_t wr[7][3];
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                wr[d][0] = pw[d * FC_PW];
                wr[d][1] = pw[d * FC_PW + 1];
                wr[d][2] = pw[d * FC_PW + 2];
            }
            const uint32_t dj = jb * 0x00020002u;
            auto pr = [&](int d, int a) -> uint32_t {
                return __builtin_amdgcn_perm(wr[d][(a >> 2) + 1], wr[d][a >> 2],
                                             (0x0c000c00u | ((uint32_t)((a & 3) + 1) << 16) | (uint32_t)(a & 3)) + dj);
            };
            // rows d = 0 .. 6 are image rows y - 3 .. y + 3; the circle in the order of fast_strength_pair<0> (window bytes 4, 5 = the pair)
            uint32_t c[16];
            c[0] = pr(6, 4);
            c[1] = pr(6, 5);
            c[2] = pr(5, 6);
            c[3] = pr(4, 7);
            c[4] = pr(3, 7);
            c[5] = pr(2, 7);
            c[6] = pr(1, 6);
            c[7] = pr(0, 5);
            c[8] = pr(0, 4);
            c[9] = pr(0, 3);
            c[10] = pr(1, 2);
            c[11] = pr(2, 1);
            c[12] = pr(3, 1);
            c[13] = pr(4, 1);
            c[14] = pr(5, 2);
            c[15] = pr(6, 3);
            const uint32_t v = pr(3, 4);
            const uint32_t sv = fast_strength_from(c, v, tzz);
            ((uint16_t *)srow)[(((tag >> 7) & 3u) * 64u + il) * 2u + jb] = (uint16_t)__builtin_amdgcn_perm(0u, sv, 0x0c0c0200u);
        }
        __builtin_amdgcn_wave_barrier();
        q_popped += n;
        st_batches++;
    };
    // the passing pairs of this row step -> queue
    auto park = [&](uint32_t p, uint32_t tag) {
        const unsigned long long bm = orb_ballot(p != 0u);
        if (bm == 0ull) return;               // wave-uniform
        if (q_pushed - q_popped > FC_QCAP - 64) batch(min(64, q_pushed - q_popped));   // room for up to 64 more
        if (p != 0u) q[(q_pushed + lanes_below(bm)) & (FC_QCAP - 1)] = tag;
        __builtin_amdgcn_wave_barrier();
        q_pushed += __popcll(bm);
        if (q_pushed - q_popped >= 64) batch(64);
    };

    for (int s0 = 0; s0 < nsteps; s0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k;
            if (s >= nsteps) break;    // wave-uniform
            // ================= what step s - FC_LAG parked is evaluated now, BEFORE this step's row overwrites the oldest slot of the
            // pixel ring (the first row of those items) ==========================================================================
            if (s - FC_LAG >= 6)
                while (q_popped < snap[(k + 8 - FC_LAG) & 3]) batch(min(64, q_pushed - q_popped));
            // ================= front half: image row of step s arrives, strength row rc = r - 3 is TESTED ====================
            if (s < nfront) {
                const uint32_t cur = Raw;
                Raw = fetch(s + 1);
                pixw[ps * FC_PW] = cur;
                pixw[(ps + FC_PN) * FC_PW] = cur;
                __builtin_amdgcn_wave_barrier();   // the neighbour lanes' dwords of this and earlier rows are read below
                if (s >= 6) {
                    // the centre row (3 steps old) with its left / right dwords (the neighbouring lanes'; lane 0 / 63: the pads) and
                    // the row 6 steps old, from the ring
                    const int ps3 = ps >= 3 ? ps - 3 : ps + FC_PN - 3, ps6 = ps >= 6 ? ps - 6 : ps + FC_PN - 6;
                    const uint32_t cl = pixw[ps3 * FC_PW - 1], cc = pixw[ps3 * FC_PW], cr = pixw[ps3 * FC_PW + 1];
                    const uint32_t c6 = pixw[ps6 * FC_PW];
                    const bool rowok = (uint32_t)(ysrel + s) < hrange;  // iy0 <= rc < iy1
                    const uint32_t tt = rowok ? tzz : 0x03FF03FFu;
                    // pair (0,1): pixels x-3, x-2 | x, x+1 | x+3, x+4;  pair (2,3): x-1, x | x+2, x+3 | x+5, x+6
                    const uint32_t p01 = fast_compass_from(__builtin_amdgcn_perm(0u, cur, 0x0c010c00u), __builtin_amdgcn_perm(0u, c6, 0x0c010c00u), __builtin_amdgcn_perm(cr, cc, 0x0c040c03u),
                                                           __builtin_amdgcn_perm(0u, cl, 0x0c020c01u), __builtin_amdgcn_perm(0u, cc, 0x0c010c00u), tt) & in01;
                    const uint32_t p23 = fast_compass_from(__builtin_amdgcn_perm(0u, cur, 0x0c030c02u), __builtin_amdgcn_perm(0u, c6, 0x0c030c02u), __builtin_amdgcn_perm(0u, cr, 0x0c020c01u),
                                                           __builtin_amdgcn_perm(cc, cl, 0x0c040c03u), __builtin_amdgcn_perm(0u, cc, 0x0c030c02u), tt) & in23;
                    srow[(k & 3) * 64 + lane] = 0u;   // a pair that fails the necessary test has strength 0
                    // first pixel slot of the items of this step: (s - 6) % FC_PN
                    const uint32_t tagrow = (uint32_t)lane | ((uint32_t)(k & 3) << 7) | ((uint32_t)ps6 << 9);
                    park(p01, tagrow);
                    park(p23, tagrow | 64u);
                    snap[k & 3] = q_pushed;
                    st_rows++;
                }
                ps = ps + 1 == FC_PN ? 0 : ps + 1;
            }
            // ================= back half: step sb = s - FC_LAG =================================================================
            const int sb = s - FC_LAG;
            const int kbq = (k + 8 - FC_LAG) & 3;                 // strength-row slot of step sb
            const int kb = (k + 8 - FC_LAG) % 8;                  // S register ring slot of step sb
            if (sb < 6) continue;
            {
                const uint32_t sv = srow[kbq * 64 + lane];
                S01[kb] = __builtin_amdgcn_perm(0u, sv, 0x0c010c00u) & in01;
                S23[kb] = __builtin_amdgcn_perm(0u, sv, 0x0c030c02u) & in23;
            }
            if (sb < 8) continue;
            // ---- 3x3 strict NMS of row rn = rc - 1 on packed pairs: rows U = S[kb-2], M = S[kb-1], D = S[kb] ----
            const int ku = (kb + 6) % 8, km = (kb + 7) % 8;
            const bool up_ok = rmod != 0;            // neighbours outside the own cell count as 0
            const bool dn_ok = rmod != hcell - 1;    // (the row at iy1 is already all zero)
            const uint32_t ord_row = ordy;
            {
                const bool wrap = rmod == hcell - 1;
                rmod = wrap ? 0 : rmod + 1;
                ordy += wrap ? 64u + ord_wrap : 64u;
            }
            if (orb_ballot((S01[km] | S23[km]) != 0u) == 0ull) continue;   // no strength in the row being suppressed (wave-uniform)
            const uint32_t u01 = up_ok ? S01[ku] : 0u, u23 = up_ok ? S23[ku] : 0u;
            const uint32_t d01 = dn_ok ? S01[kb] : 0u, d23 = dn_ok ? S23[kb] : 0u;
            const uint32_t m01 = S01[km], m23 = S23[km];
            const uint32_t v01 = pk_max_u16(u01, d01), v23 = pk_max_u16(u23, d23);   // vertical neighbours
            const uint32_t c01 = pk_max_u16(v01, m01), c23 = pk_max_u16(v23, m23);   // column maxima
            // neighbour lanes by DPP wave shifts (lane 0 / 63 read back 0: they have no such neighbour)
            const uint32_t cL = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c23, 0x138, 0xF, 0xF, true);  // wave_shr:1, .hi = column x-1
            const uint32_t cR = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c01, 0x130, 0xF, 0xF, true);  // wave_shl:1, .lo = column x+4
            const uint32_t l01 = __builtin_amdgcn_alignbit(c01, cL, 16) & lv01;      // columns (x-1, x)
            const uint32_t x12 = __builtin_amdgcn_alignbit(c23, c01, 16);            // columns (x+1, x+2)
            const uint32_t r23 = __builtin_amdgcn_alignbit(cR, c23, 16) & rv23;      // columns (x+3, x+4)
            const uint32_t n01 = pk_max3(l01, x12 & rv01, v01);
            const uint32_t n23 = pk_max3(x12 & lv23, r23, v23);
            const uint32_t g01 = pk_subsat_u16(m01, n01), g23 = pk_subsat_u16(m23, n23);  // != 0 <=> survivor
            const bool row_out = sb - 8 < nrows_out;  // per lane
            const unsigned long long brow = orb_ballot(row_out);
            const unsigned long long b01 = orb_ballot(g01 != 0u) & brow, b23 = orb_ballot(g23 != 0u) & brow;
            const bool has01 = row_out && g01 != 0u, has23 = row_out && g23 != 0u;
            if (b01 | b23) {
                const uint32_t keyrow = (uint32_t)(x - ORBFE_MINB) + ((uint32_t)(ys - 8 - ORBFE_MINB + sb) << 12);
                const uint32_t ordx[4] = {ordx_of(0), ordx_of(1), ordx_of(2), ordx_of(3)};
                const int p01n = __popcll(b01), p23n = __popcll(b23);
                if (nbuf + p01n + p23n + FC_SEAMS > FC_BUF) {   // room for this row (at most FC_SEAMS lanes straddle a cell seam)
                    fm_flush(slist, scnt, sbuf, nbuf, key_cap, lane, lflag, ini_th);
                    nbuf = 0;
                }
#include "orbfe_fast_emit.inc"
            }
        }
    }
    if (nbuf > 0) fm_flush(slist, scnt, sbuf, nbuf, key_cap, lane, lflag, ini_th);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (int i = lane; i < cf_words; i += 64) {
        const uint32_t v = lflag[i];
        if (v) atomicOr(&cflag[i], v);
    }
    // pass-rate statistics of a SAMPLE of the waves (every 16th, rotating with the frame): {row steps, batches, parked pairs};
    // parked / (128 * row steps) is the share of pixel pairs that pass the necessary test
    if (fstat && lane == 0 && ((t + b) & 15) == 0) {
        atomicAdd(&fstat[0], (unsigned long long)st_rows);
        atomicAdd(&fstat[1], (unsigned long long)st_batches);
        atomicAdd(&fstat[2], (unsigned long long)q_pushed);
    }
