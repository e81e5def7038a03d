// orbfe_fast_body.inc -- the body of the dense FAST pass of one wave (K2, see orbfe_fast.hip), included TEXTUALLY by k_fast_map
// and k_fast_map_u so that each compiles it in its own context (a shared __device__ function changed k_fast_map's
// register allocation: +1 % instructions).  Expects in scope: SPARSE, CELLROWS (constexpr bool, below), plan, fs, lanes, skeys,
// scount, cflags, cf_words, fstat, s_buf, s_cf and the wave-uniform t (index of the wave in the lane list), b (frame), lane, wv.
//
// CELLROWS = false is the generic form: any run of rows per lane.  CELLROWS = true is the CELL-ROW form:
// the reference runs cv::FAST once per 30-px cell (src/ORBextractor.cc:798-838): a corner's 3x3 suppression never looks across a
// cell boundary.  A wave of this form walks whole CELL ROWS: every lane is a 4-pixel column of a run of rows [ys, ys + nrows) that
// starts on a cell-row boundary and ends on one (or at the end of the detectable interior), and all runs of a wave have the same
// length: the lanes are at the same position inside their runs in every step.  Consequences, against the generic form:
//   * no strength row outside the run is ever needed (the row above its first row and the row below its last row count as zero):
//     nrows strength rows instead of nrows + 2, nrows + 7 steps instead of nrows + 8;
//   * everything that depends on the row only is the same in every lane and lives in SCALAR registers: the row's address (buffer
//     addressing: resource = the level, the lane's first row and column as its offset, the step's row as the scalar offset), the row's position in its cell (up / down
//     neighbours valid), the row part of the candidate order key `ord` and of the key's y coordinate, the loop bounds; every row
//     of the run is a detectable row, so the threshold needs no per-row validity select.
// Per row step that is ~20 vector instructions fewer of ~214, and 2 arc evaluations fewer per run.
//
// The row walk, both forms: blocks of eight steps under an 8-fold unroll (ring slots are compile-time constants), FM_PF raw rows
// in flight (orbfe_fast.hip; the row of step s + FM_PF is fetched in step s), no exit inside a block -- the steps a run lacks to
// a multiple of eight are padding steps in front of step 0 (below, at the loop).  tests/test_gpu_fast_prefetch.py walks every
// `nsteps mod 8` of both forms.
// Only the places that differ branch on CELLROWS; FM_LDS_CONSTS (orbfe_fast_colmask.inc) is an A/B path of the generic form.
    uint32_t *lflag = s_cf + wv * cf_words;
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
    uint2 *sbuf = s_buf[wv];
    int nbuf = 0;  // wave-uniform fill of sbuf
    int st_rows = 0, st_arc = 0, st_nms = 0;  // SPARSE statistics (wave-uniform)
    const int H = L.h, key_cap = L.key_cap;
    const int ix0 = ORBFE_EDGE, iy0 = ORBFE_EDGE, ix1 = L.ix1, iy1 = L.iy1;
    const int wcell = L.wcell, hcell = L.hcell;
    const int x = ld.x;                 // first pixel of this lane (16 <= x < ix1: the 12-byte row window is in the image)
    // the run of rows [ys, ys + nrows): every lane's run starts on a cell row and all runs of a wave have the same length (the host
    // packs it so; dead and halo lanes carry copies), so the POSITION INSIDE THE RUN is the same in every lane -- the first row
    // itself is a per-lane constant that only enters the lane's address, key and order constants
    const int ys = ld.ys;
    int nrows = ld.nrows;               // rows the wave walks: the common run length / the longest run of its lanes
    if (!CELLROWS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nrows = max(nrows, __shfl_xor(nrows, o, 64));
    }
    nrows = __builtin_amdgcn_readfirstlane(nrows);  // wave-uniform, and the compiler knows it
    // generic: pixel rows ys - 4 .. , the last suppression in step nrows + 7
    // cell rows: pixel rows ys - 3 .. ys + nrows + 2 in steps 0 .. nrows + 5, the last suppression in step nrows + 6
    const int nsteps = nrows + (CELLROWS ? 7 : 8);
    const int tz = max(plan->min_th, 1);

#include "orbfe_fast_colmask.inc"
    const int nrows_out = !CELLROWS && out_lane ? (int)ld.nrows : 0;   // generic: rows of the run the lane emits
    const unsigned long long bout = CELLROWS ? orb_ballot(out_lane) : 0ull;   // cell rows: lanes that emit (halo and dead lanes compute, never output)
    // per-pixel part of `ord`, the rank key of the reference's candidate order (cell-row-major, raster inside a cell):
    // ord = (cell_row * ncc + cell_col) << 12 | y_in_cell << 6 | x_in_cell
    // (cell rows: the cell row the lane's run starts in is part of the per-lane constant, what the rows walked add is scalar)
    uint32_t ordx[4];
    {
        const uint32_t row_part = CELLROWS ? (uint32_t)(((ys - iy0) / hcell) * L.ncc) << 12 : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) ordx[j] = row_part + (((uint32_t)ccj[j] << 12) | (uint32_t)mj[j]);
    }
#ifdef FM_LDS_CONSTS
    s_lco[wv][lane] = make_uint4(ordx[0], ordx[1], ordx[2], ordx[3]);
#endif
    int rmod = CELLROWS ? 0 : (ys - iy0) % hcell;                   // y_in_cell of the next NMS row (per lane; cell rows: runs start on a cell row)
    uint32_t ordy = CELLROWS ? 0u : ((uint32_t)(((ys - iy0) / hcell) * L.ncc) << 12) | ((uint32_t)rmod << 6);
    const uint32_t ord_wrap = ((uint32_t)L.ncc << 12) - ((uint32_t)hcell << 6);  // added when a new cell row starts
    const uint32_t tzz = (uint32_t)tz * 0x00010001u;
    const uint32_t resp0 = (uint32_t)(tz - 1);
    const int ysrel = ys - 7 - iy0;                                 // strength row of step s, relative to iy0, minus s
    const uint32_t hrange = (uint32_t)(iy1 - iy0);
    // key of pixel 0 in the NMS row of step 0 (detection-window coordinates = level - 16, reference :831-832): the row of step s
    // is ys - 8 + s, cell rows ys - 7 + s
    const uint32_t key00 = (uint32_t)(x - ORBFE_MINB) + ((uint32_t)(ys - (CELLROWS ? 7 : 8) - ORBFE_MINB) << 12);

    // 8-slot ring of unpacked rows (7 live), statically indexed under the 8-fold unroll; the raw row of step s + FM_PF is
    // fetched in step s: FM_PF rows in flight, FM_PF + 1 live 12-byte buffers in a ring of FM_RAW slots
    uint32_t R[8][FM_NE], Raw[FM_RAW][3];
    uint32_t S01[8], S23[8];  // S of the pixel pairs (0,1), (2,3) for the strength row computed in ring slot k
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        S01[k] = S23[k] = 0u;
#pragma unroll
        for (int i = 0; i < FM_NE; ++i) R[k][i] = 0u;
    }
    // generic: per-lane addresses (lanes past their run re-read a valid row).  Cell rows: buffer addressing, the step's row is a
    // scalar offset; rows ys - 3 .. ys + nrows + 4 all lie inside the level.
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)src, 0, -1, 0x00020000);
    const int voff = (ys - 3) * pitch + x - 4;
    typedef uint32_t fmu_v3 __attribute__((ext_vector_type(3)));
    auto fetch = [&](int s, uint32_t (&dst3)[3]) {
        if constexpr (CELLROWS) {   // (constexpr: the lambda captures what its live branch names, nothing of the other form)
            const fmu_v3 w = __builtin_amdgcn_raw_buffer_load_b96(rsrc, voff, s * pitch, 0);   // the step's row: a scalar offset
            dst3[0] = w.x;
            dst3[1] = w.y;
            dst3[2] = w.z;
        } else {
            const int r = ys - 4 + s;  // image row of step s (lanes past their run re-read a valid row)
            const uint8_t *row = src + (__umul24((uint32_t)min(r, H - 1), (uint32_t)pitch) + (uint32_t)x);
            dst3[0] = *(const uint32_t *)(row - 4);
            dst3[1] = *(const uint32_t *)(row);
            dst3[2] = *(const uint32_t *)(row + 4);
        }
    };
    // The walk is whole blocks of eight steps and no step of a block leaves the loop: the waitcnt pass merges conservatively where
    // control flow joins, and with a per-step exit (`if (s >= nsteps) break`) the wait in front of the unpack came out as
    // vmcnt(1) in steady state whatever the ring depth -- one row in flight.  So the steps a run lacks to a multiple of eight
    // come FIRST, as padding steps s = -pad .. -1: a padding step issues its fetch like any other step (the step is clamped on the
    // scalar side, so it asks for row 0 again) and does nothing else -- every path through a block has issued the same number of
    // loads, and the wait of every step is vmcnt(FM_PF).  The slot k of step s is (s + pad) % 8; only ring positions depend on it.
    // No fetch asks for a row past step nsteps (row ys + nrows + 4, what the one-row-ahead walk read last): the resource has no
    // bound of its own.
    const int pad = (8 - (nsteps & 7)) & 7;
    auto fetch_step = [&](int s, uint32_t (&dst3)[3]) { fetch(min(max(s, 0), nsteps), dst3); };   // rows of steps 0 .. nsteps, as before
#pragma unroll
    for (int i = 0; i < FM_PF; ++i) fetch_step(i - pad, Raw[i]);

    for (int s0 = -pad; s0 < nsteps; s0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = s0 + k;   // wave-uniform
            const bool have_row = !CELLROWS || s < nrows + 6;   // cell rows, scalar: the last step only suppresses
            // (the fetch is unconditional -- a conditional load is waited for where the branches join, i.e. at once; the rows past
            // the run that the last steps ask for, ys + nrows + 3 and + 4, still lie inside the level: iy1 + 4 <= h - 15)
            fetch_step(s + FM_PF, Raw[(k + FM_PF) % FM_RAW]);
            if (s < 0) continue;       // a padding step: nothing waits for its fetch
            fast_unpack_row(Raw[k % FM_RAW], R[k]);
            if (s < 6) continue;
            // ---- strength row rc = r - 3 (newest ring slot k is row rc+3, slot (k+2)%8 is row rc-3) ----
            if (have_row) {
                const uint32_t(&rm3)[FM_NE] = R[(k + 2) % 8];
                const uint32_t(&rm2)[FM_NE] = R[(k + 3) % 8];
                const uint32_t(&rm1)[FM_NE] = R[(k + 4) % 8];
                const uint32_t(&r0)[FM_NE] = R[(k + 5) % 8];
                const uint32_t(&rp1)[FM_NE] = R[(k + 6) % 8];
                const uint32_t(&rp2)[FM_NE] = R[(k + 7) % 8];
                const uint32_t(&rp3)[FM_NE] = R[k];
                const bool rowok = (uint32_t)(ysrel + s) < hrange;  // iy0 <= rc < iy1 (every row of a cell-row run is a detectable row)
                const uint32_t tt = CELLROWS || rowok ? tzz : 0x03FF03FFu;
                bool arcs = true;
#ifdef FM_LDS_CONSTS
                const fm_v4 lcm = FM_LC_LOAD(fm_v4, lc_m);
                const uint32_t in01 = lcm.x, in23 = lcm.y;
#endif
                if (SPARSE) {
                    const uint32_t p = (fast_compass_pair<0>(rm3, r0, rp3, tt) & in01) |
                                       (fast_compass_pair<2>(rm3, r0, rp3, tt) & in23);
                    arcs = orb_ballot(p != 0u) != 0ull;  // wave-uniform
#ifdef ORBFE_DEVELOPER
                    if (plan->dbg == 60) arcs = false;   // TIMING ONLY (wrong results): the pass without any arc evaluation
#endif
                    if (fstat) { st_rows++; st_arc += arcs ? 0 : 1; }
                }
                if (arcs) {
                    S01[k] = fast_strength_pair<0>(rm3, rm2, rm1, r0, rp1, rp2, rp3, tt) & in01;
                    S23[k] = fast_strength_pair<2>(rm3, rm2, rm1, r0, rp1, rp2, rp3, tt) & in23;
                } else {
                    S01[k] = S23[k] = 0u;
                }
            }
            if (s < (CELLROWS ? 7 : 8)) continue;
            // ---- 3x3 strict NMS of row rn = rc - 1 on packed pairs: rows U = S[k-2], M = S[k-1], D = S[k] ----
            const int ku = (k + 6) % 8, km = (k + 7) % 8;
            const bool up_ok = rmod != 0;            // neighbours outside the own cell count as 0
            const bool dn_ok = rmod != hcell - 1 && have_row;    // (generic: the row at iy1 is already all zero; cell rows: the last row has no row below it in the run)
            const uint32_t ord_row = ordy;
            {
                const bool wrap = rmod == hcell - 1;
                rmod = wrap ? 0 : rmod + 1;
                ordy += wrap ? 64u + ord_wrap : 64u;
            }
            if (SPARSE) {  // no strength in the row being suppressed -> nothing can survive (wave-uniform)
                if (orb_ballot((S01[km] | S23[km]) != 0u) == 0ull) {
                    if (fstat) st_nms++;
                    continue;
                }
            }
#ifdef FM_LDS_CONSTS
            const fm_v4 lcn = FM_LC_LOAD(fm_v4, lc_m);
            const fm_v2 lcr = FM_LC_LOAD(fm_v2, lc_r);
            const uint32_t lv01 = lcn.z, lv23 = lcn.w, rv01 = lcr.x, rv23 = lcr.y;
#endif
            const uint32_t u01 = up_ok ? S01[ku] : 0u, u23 = up_ok ? S23[ku] : 0u;
            const uint32_t d01 = dn_ok ? S01[k] : 0u, d23 = dn_ok ? S23[k] : 0u;
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
            // generic: per lane; cell rows: the lanes that emit, every row of the run
            const bool row_out = CELLROWS ? out_lane : s - 8 < nrows_out;
            // ballots of the plain compares, combined on the scalar side (a ballot of a combined predicate is lowered through a
            // VGPR: select 0 / 1, compare again)
            const unsigned long long brow = CELLROWS ? bout : orb_ballot(row_out);
            const unsigned long long b01 = orb_ballot(g01 != 0u) & brow, b23 = orb_ballot(g23 != 0u) & brow;
            const bool has01 = row_out && g01 != 0u, has23 = row_out && g23 != 0u;
            if (b01 | b23) {
#ifdef FM_LDS_CONSTS
                const fm_v4 lco = FM_LC_LOAD(fm_v4, lc_o);
                const uint32_t ordx[4] = {lco.x, lco.y, lco.z, lco.w};
#endif
                const uint32_t keyrow = key00 + ((uint32_t)s << 12);
                const int p01n = __popcll(b01), p23n = __popcll(b23);
#include "orbfe_fast_emit.inc"
                if (nbuf > FM_BUF - FM_ROW_MAX) {
                    fm_flush(slist, scnt, sbuf, nbuf, key_cap, lane, lflag, ini_th);
                    nbuf = 0;
                }
            }
        }
    }
    if (nbuf > 0) fm_flush(slist, scnt, sbuf, nbuf, key_cap, lane, lflag, ini_th);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (int i = lane; i < cf_words; i += 64) {
        const uint32_t v = lflag[i];
        if (v) atomicOr(&cflag[i], v);
    }
    if (SPARSE && fstat && lane == 0) {
        atomicAdd(&fstat[0], (unsigned long long)st_rows);
        atomicAdd(&fstat[1], (unsigned long long)st_arc);
        atomicAdd(&fstat[2], (unsigned long long)st_nms);
    }
