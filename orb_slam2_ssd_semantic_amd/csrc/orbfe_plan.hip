// orbfe_plan.hip -- the extractor's launch plan (csrc/orbfe_plan.h): constructor tables, level geometry and FAST cells, cv::resize
// tap tables, the FAST lane lists (dense and lane-compacting), the folded blur weights and the blur lane list.  The FAST, blur
// and pyramid kernels trust these tables blindly; tests/test_plan.py checks, without a GPU, what they rely on.
// No device code and no HIP runtime call here: the extension .hip only puts the file into the same build.
//
// Reference behaviour restated here (paths relative to /root/reference):
//   constructor tables            src/ORBextractor.cc:399-466
//   level sizes / pyramid layout  src/ORBextractor.cc:1117-1145
//   FAST cell grid + skip rules   src/ORBextractor.cc:771-816
//   quadtree roots                src/ORBextractor.cc:545-564
//   cv::resize coefficient tables OpenCV 3.2 imgwarp.cpp
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "orbfe_kernels.h"
#include "orbfe_plan.h"

// rows a FAST / blur wave walks down.  Measured on MI355X (256 x 640x480): 24..48 rows are equally fast and ~5 % faster
// than 64+ -- the 6..8 warm-up rows of a block are nearly free, while shorter waves balance the CUs better.
#define ORBFE_ROWS_PER_WAVE 40

static inline int cv_round_f(float v) { return (int)lrintf(v); }  // cvRound: half-to-even

// ---------------------------------------------------------------------------------------------------
// constructor tables
// ---------------------------------------------------------------------------------------------------
orbfe_status orb_ctor_tables(const orbfe_params *p, OrbPlanIn *in, float *sigma2, float *inv_sigma2)
{
    if (p->nlevels < 1 || p->nlevels > ORBFE_MAX_LEVELS || p->nfeatures < 0 || !(p->scale_factor > 1.0f) ||
        p->max_batch < 1 || p->max_width < 1 || p->max_height < 1 || p->max_width > 4096 || p->max_height > 4096) {
        orbfe_set_error("bad orbfe_params (nlevels 1..16, scale_factor > 1, max size <= 4096, max_batch >= 1)");
        return ORBFE_ERR_ARG;
    }
    memset(in, 0, sizeof(*in));
    // src/ORBextractor.cc:404-421
    const int nl = in->nlevels = p->nlevels;
    in->scale[0] = 1.0f;
    for (int i = 1; i < nl; ++i) in->scale[i] = in->scale[i - 1] * p->scale_factor;
    for (int i = 0; i < nl; ++i) {
        in->inv_scale[i] = 1.0f / in->scale[i];
        const float s2 = i == 0 ? 1.0f : in->scale[i] * in->scale[i];
        if (sigma2) sigma2[i] = s2;
        if (inv_sigma2) inv_sigma2[i] = 1.0f / s2;
    }
    // src/ORBextractor.cc:426-439
    const float factor = 1.0f / p->scale_factor;
    float desired = p->nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; ++l) {
        in->feat[l] = cv_round_f(desired);
        sum += in->feat[l];
        desired *= factor;
    }
    in->feat[nl - 1] = std::max(p->nfeatures - sum, 0);
    in->ini_th_fast = p->ini_th_fast;
    in->min_th_fast = p->min_th_fast;
    in->blur_rounding = p->blur_rounding;
    in->max_batch = p->max_batch;
    in->opt_blur_pieces = 1;
    in->opt_blur_updown = 1;
    return ORBFE_OK;
}

void orb_host_umax(int umax[16])
{
    // src/ORBextractor.cc:449-465
    int v, v0;
    const int vmax = (int)floorf(ORBFE_HALF_PATCH * sqrtf(2.f) / 2 + 1);
    const int vmin = (int)ceilf(ORBFE_HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = ORBFE_HALF_PATCH * ORBFE_HALF_PATCH;
    for (v = 0; v < 16; ++v) umax[v] = 0;
    for (v = 0; v <= vmax; ++v) umax[v] = (int)lrint(sqrt(hp2 - v * v));
    for (v = ORBFE_HALF_PATCH, v0 = 0; v >= vmin; --v) {
        while (umax[v0] == umax[v0 + 1]) ++v0;
        umax[v] = v0;
        ++v0;
    }
}

namespace
{
// a lane that computes along with its wave and outputs nothing (flag bit 0)
OrbLane dead_lane(int level, int x, int ys, int nrows, int flags = 0)
{
    return OrbLane{(uint16_t)x, (uint16_t)ys, (uint16_t)nrows, (uint16_t)((level << 8) | 1 | flags)};
}

// the tables inside `tabs` start on 4 entries: a lane reads the taps of its 4 pixels / 8 rows as 16-byte loads
int align_tabs(std::vector<OrbTab> &tabs)
{
    while (tabs.size() % 4) tabs.push_back(OrbTab{0, 0, 0, 0});
    return (int)tabs.size();
}

// cv::resize coefficient table of one axis
void resize_axis(int ssize, int dsize, bool is_x, OrbTab *out)
{
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1. / inv_scale;
    for (int d = 0; d < dsize; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= s;
        if (is_x) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        auto sat = [](int v) { return (int16_t)std::min(32767, std::max(-32768, v)); };
        out[d].s = (int16_t)s;
        out[d].c0 = sat(cv_round_f((1.f - f) * 2048));
        out[d].c1 = sat(cv_round_f(f * 2048));
        out[d].pad = 0;
    }
}

// running totals of the level loop
struct LevelSums {
    int64_t off = 0;
    int key_off = 0, sel_off = 0, cell_cap = 1, max_sel = 0;
};

// ---------------------------------------------------------------------------------------------------
// levels and cells
// ---------------------------------------------------------------------------------------------------
// FAST cells of level l (src/ORBextractor.cc:798-816); *key_cap = the worst-case number of candidates of the level
orbfe_status level_cells(int l, OrbLevel &L, std::vector<OrbCell> &cells, LevelSums &S, int *key_cap)
{
    const int minb = ORBFE_EDGE - 3;
    const int maxbx = L.w - ORBFE_EDGE + 3, maxby = L.h - ORBFE_EDGE + 3;
    L.cell0 = (int)cells.size();
    *key_cap = 0;
    for (int i = 0; i < L.nrows; ++i) {
        const float iniY = (float)(minb + i * L.hcell);
        float maxY = iniY + L.hcell + 6;
        if (iniY >= maxby - 3) continue;  // :803
        if (maxY > maxby) maxY = (float)maxby;
        for (int j = 0; j < L.ncols; ++j) {
            const float iniX = (float)(minb + j * L.wcell);
            float maxX = iniX + L.wcell + 6;
            if (iniX >= maxbx - 6) continue;  // :812
            if (maxX > maxbx) maxX = (float)maxbx;
            OrbCell c;
            c.level = (uint16_t)l;
            c.x0 = (uint16_t)iniX;
            c.y0 = (uint16_t)iniY;
            c.tw = (uint16_t)((int)maxX - (int)iniX);
            c.th = (uint16_t)((int)maxY - (int)iniY);
            c.ox = (uint16_t)(j * L.wcell);
            c.oy = (uint16_t)(i * L.hcell);
            c.pad = 0;
            if (c.tw > ORBFE_TILE_MAX || c.th > ORBFE_TILE_MAX) {
                orbfe_set_error("FAST tile %dx%d exceeds %d", c.tw, c.th, ORBFE_TILE_MAX);
                return ORBFE_ERR_SIZE;
            }
            // strict 3x3 NMS keeps at most one keypoint per 2x2 block of the detectable interior
            const int iw = std::max(0, (int)c.tw - 6), ih = std::max(0, (int)c.th - 6);
            const int worst = ((iw + 1) / 2) * ((ih + 1) / 2);
            S.cell_cap = std::max(S.cell_cap, worst);
            *key_cap += worst;
            cells.push_back(c);
        }
    }
    L.ncells = (int)cells.size() - L.cell0;
    {
        // non-skipped cells form a full (rows x cols) sub-grid (the skip rules depend on i or j alone)
        int ncc = 0;
        for (int k = L.cell0; k < (int)cells.size() && cells[k].y0 == cells[L.cell0].y0; ++k) ++ncc;
        L.ncc = ncc;
    }
    {
        const OrbCell &clast = cells.back();
        L.ix1 = L.ncells ? clast.x0 + clast.tw - 3 : ORBFE_EDGE;
        L.iy1 = L.ncells ? clast.y0 + clast.th - 3 : ORBFE_EDGE;
    }
    return ORBFE_OK;
}

// size, pyramid slice, FAST grid, quadtree roots and scratch slots of level l
orbfe_status plan_level(const OrbPlanIn &in, int l, int w, int ht, OrbPlanTables &T, LevelSums &S)
{
    OrbLevel &L = T.plan.lv[l];
    L.w = cv_round_f((float)w * in.inv_scale[l]);   // src/ORBextractor.cc:1122
    L.h = cv_round_f((float)ht * in.inv_scale[l]);
    L.pitch = orb_align_up(L.w, 64);
    L.off = (int32_t)S.off;
    S.off = orb_align_up64(S.off + (int64_t)L.pitch * L.h, 256);
    if (S.off > 0x7FFFFFFF) { orbfe_set_error("pyramid slice exceeds 2 GiB"); return ORBFE_ERR_SIZE; }
    // FAST grid (src/ORBextractor.cc:780-796)
    const int minb = ORBFE_EDGE - 3;
    const int maxbx = L.w - ORBFE_EDGE + 3, maxby = L.h - ORBFE_EDGE + 3;
    const float width = (float)(maxbx - minb), height = (float)(maxby - minb);
    const float W = 30;
    if (width < W || height < W) {
        orbfe_set_error("level %d (%dx%d) is smaller than one 30-px FAST cell plus borders", l, L.w, L.h);
        return ORBFE_ERR_SIZE;
    }
    L.ncols = (int)(width / W);
    L.nrows = (int)(height / W);
    L.wcell = (int)ceilf(width / L.ncols);
    L.hcell = (int)ceilf(height / L.nrows);
    int key_cap = 0;
    const orbfe_status s = level_cells(l, L, T.cells, S, &key_cap);
    if (s != ORBFE_OK) return s;
    L.nfeat = in.feat[l];
    // quadtree roots (src/ORBextractor.cc:545-559)
    L.nini = (int)roundf((float)(maxbx - minb) / (float)(maxby - minb));
    if (L.nini < 1 || L.nini > ORBFE_MAX_ROOTS) {  // 0 roots: the reference divides by zero (:547)
        orbfe_set_error("level %d aspect ratio gives %d quadtree roots (supported: 1..%d)", l, L.nini, ORBFE_MAX_ROOTS);
        return ORBFE_ERR_SIZE;
    }
    L.hx = (float)(maxbx - minb) / L.nini;
    for (int i = 0; i <= L.nini; ++i) L.root_x[i] = (int)(L.hx * (float)i);
    L.key_off = S.key_off;
    L.key_cap = key_cap;
    S.key_off += orb_align_up(std::max(key_cap, 1), 64);
    L.sel_cap = std::max(L.nfeat + 2, 4 * L.nini);
    L.sel_off = S.sel_off;
    S.sel_off += orb_align_up(L.sel_cap, 64);
    S.max_sel = std::max(S.max_sel, L.sel_cap);
    L.scale = in.scale[l];
    L.patch_size = (float)(int)(ORBFE_PATCH * in.scale[l]);  // :846
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// tap tables
// ---------------------------------------------------------------------------------------------------
// the cv::resize tables of level l (>= 1) from level l - 1
orbfe_status level_taps(int l, OrbPlan &P, std::vector<OrbTab> &tabs)
{
    OrbLevel &L = P.lv[l];
    const OrbLevel &S = P.lv[l - 1];
    if (S.w >= 2 * L.w) {  // k_pyr_walk: the 4 source pairs of a lane must fit one 8-byte window
        orbfe_set_error("scale factor too large: level %d is less than half as wide as level %d", l, l - 1);
        return ORBFE_ERR_ARG;
    }
    // tap tables, 4-entry aligned and padded by 8 (a lane reads the taps of its 4 pixels / 8 rows as
    // 16-byte loads; entries past the end repeat the last one)
    auto add_axis = [&](int ssize, int dsize, bool is_x) {
        const int at = align_tabs(tabs);
        tabs.resize(tabs.size() + dsize + 8);
        resize_axis(ssize, dsize, is_x, &tabs[at]);
        for (int i = 0; i < 8; ++i) tabs[at + dsize + i] = tabs[at + dsize - 1];
        return at;
    };
    L.xtab = add_axis(S.w, L.w, true);
    L.ytab = add_axis(S.h, L.h, false);
    // k_pyr_walk completes at most one destination row per source row: the source row index must grow strictly
    for (int d = 1; d < L.h; ++d)
        if (tabs[(size_t)L.ytab + d].s <= tabs[(size_t)L.ytab + d - 1].s) {
            orbfe_set_error("level %d: vertical resize taps are not strictly increasing", l);
            return ORBFE_ERR_ARG;
        }
    if (orbk_pyramid_lds_bytes(L.h) > 64 * 1024) {
        orbfe_set_error("level %d too tall for the pyramid kernel's LDS tap table", l);
        return ORBFE_ERR_SIZE;
    }
    return ORBFE_OK;
}

// what the level loop adds up to: scratch sizes per frame and the quadtree's node capacity
orbfe_status plan_totals(const LevelSums &S, OrbPlanTables &T)
{
    OrbPlan &P = T.plan;
    const int nl = P.nlevels;
    P.ncells = (int)T.cells.size();
    P.cell_cap = S.cell_cap;
    P.max_ncells = 1;
    for (int l = 0; l < nl; ++l) P.max_ncells = std::max(P.max_ncells, P.lv[l].ncells);
    P.keys_per_frame = S.key_off;
    P.sel_per_frame = S.sel_off;
    // node arrays: one slot more than the largest list, rounded to 64 (only the sort buffer inside is a power of two)
    const int M = orb_align_up(std::max(S.max_sel + 1, 64), 64);
    P.node_cap = M;
    P.max_nini = 1;
    for (int l = 0; l < nl; ++l) P.max_nini = std::max(P.max_nini, P.lv[l].nini);
    // Node arrays normally sit in LDS; a level asking for more nodes than fit (about 2400 features on ONE level) keeps them
    // in global scratch.  What remains is the width of the node index the keys of deep trees carry (14 bits).
    if (M > 16383) {
        orbfe_set_error("nfeatures too large: %d quadtree nodes on one level (at most 16383)", S.max_sel);
        return ORBFE_ERR_ARG;
    }
    for (int l = 0; l < nl; ++l)
        if (P.lv[l].ncells >= (1 << 16) || P.lv[l].wcell > 63 || P.lv[l].hcell > 63) {
            orbfe_set_error("level %d: %d FAST cells / cell size exceed the 16 + 6 + 6 bit candidate-order key", l, P.lv[l].ncells);
            return ORBFE_ERR_SIZE;
        }
    P.pyr_frame_bytes = S.off;
    if (T.tabs.empty()) T.tabs.resize(1);
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// FAST strips
// ---------------------------------------------------------------------------------------------------
// Per level and per run of rows, the 4-px columns x = 16, 20, ... < ix1 form a strip.  The run rule: balanced blocks of at most
// rows_fast rows, or (cellrows) k whole cell rows, k = rows_fast / hcell rounded (1 for the default 40 rows and the ~31-row
// cells of every shipped configuration).
std::vector<OrbLane> fast_strips(const OrbPlan &P, int rows_fast, bool cellrows)
{
    std::vector<OrbLane> stream;
    for (int l = 0; l < P.nlevels; ++l) {
        const OrbLevel &L = P.lv[l];
        const int rows = L.iy1 - ORBFE_EDGE, ncol = (L.ix1 - 16 + 3) / 4;
        if (rows <= 0 || ncol <= 0) continue;
        int rb;
        if (cellrows) {
            rb = std::max(1, (rows_fast + L.hcell / 2) / L.hcell) * L.hcell;
        } else {
            const int nblk = (rows + rows_fast - 1) / rows_fast;
            rb = (rows + nblk - 1) / nblk;
        }
        for (int ys = ORBFE_EDGE; ys < L.iy1; ys += rb) {
            const int nr = std::min(rb, L.iy1 - ys);
            for (int c = 0; c < ncol; ++c) stream.push_back(OrbLane{(uint16_t)(16 + 4 * c), (uint16_t)ys, (uint16_t)nr, (uint16_t)(l << 8)});
        }
    }
    return stream;
}

bool same_strip(const OrbLane &a, const OrbLane &b)
{
    return (a.flags >> 8) == (b.flags >> 8) && a.ys == b.ys && b.x == a.x + 4;
}

// FAST lane list: per level, per (balanced) row block of <= ORBFE_ROWS_PER_WAVE rows, the 4-px columns x = 16, 20, ... < ix1 form a
// strip; strips are packed back to back into single-level waves of 64 lanes.  Where a wave boundary falls inside a
// strip, each side gets one halo lane (computes neighbour strengths, outputs nothing).
void pack_dense(const std::vector<OrbLane> &dstream, bool cellrows, OrbPlanTables &T)
{
    OrbPlan &P = T.plan;
    std::vector<OrbLane> &flanes = T.flanes;
    size_t i = 0;
    for (int l = 0; l <= ORBFE_MAX_LEVELS; ++l) P.fwave_off[l] = -1;
    while (i < dstream.size()) {
        const int lvl = dstream[i].flags >> 8;
        const size_t w0 = flanes.size();
        const OrbLane first = dstream[i];
        // cell-row form: runs of ONE length per wave (every run starts on a cell row: the lanes are in step)
        auto fits = [&](const OrbLane &ln) { return !cellrows || ln.nrows == first.nrows; };
        if (P.fwave_off[lvl] < 0) P.fwave_off[lvl] = (int)(w0 / 64);
        if (i > 0 && same_strip(dstream[i - 1], dstream[i])) {  // continuing a cut strip: left halo first
            OrbLane hl = dstream[i - 1];
            hl.flags |= 1;
            flanes.push_back(hl);
        }
        while (i < dstream.size() && (dstream[i].flags >> 8) == lvl && fits(dstream[i]) && flanes.size() - w0 < 64) {
            const bool more = i + 1 < dstream.size() && same_strip(dstream[i], dstream[i + 1]);
            if (flanes.size() - w0 == 63 && more) {  // last slot and the strip goes on: right halo, lane moves on
                OrbLane hr = dstream[i];
                hr.flags |= 1;
                flanes.push_back(hr);
                break;
            }
            flanes.push_back(dstream[i]);
            ++i;
        }
        // dead lanes (cell-row form: they carry the wave's run, as its scalar row state wants)
        while (flanes.size() - w0 < 64) flanes.push_back(cellrows ? dead_lane(lvl, 16, first.ys, first.nrows) : dead_lane(lvl, 16, ORBFE_EDGE, 0));
    }
    const int nl = P.nlevels;
    P.nfwaves = (int)(flanes.size() / 64);
    P.fwave_off[nl] = P.nfwaves;
    for (int l = ORBFE_MAX_LEVELS; l > nl; --l) P.fwave_off[l] = P.nfwaves;
    for (int l = nl - 1; l >= 0; --l)
        if (P.fwave_off[l] < 0) P.fwave_off[l] = P.fwave_off[l + 1];   // a level without FAST rows
    T.fast_row_steps = 0;
    for (int wv = 0; wv < P.nfwaves; ++wv) {
        int mx = 0;
        for (int k = 0; k < 64; ++k) mx = std::max(mx, (int)flanes[(size_t)wv * 64 + k].nrows);
        T.fast_row_steps += mx + 8;
    }
}

// Lane list of the lane-compacting form (k_fast_map_c): the same strips, but EVERY piece of a strip inside a wave is closed by a halo
// lane on both sides (the 4-px column before / behind it, flag bit 0) -- its lanes take their left / right neighbour pixels from
// the neighbouring lanes, not from memory.  At the image's side borders the halo is the column outside the detectable interior
// (x = 12 / the column behind the last one: real pixels, nothing inside, nothing output).
void pack_compacting(const std::vector<OrbLane> &stream, OrbPlanTables &T)
{
    std::vector<OrbLane> &clanes = T.clanes;
    size_t i = 0;
    while (i < stream.size()) {
        const int lvl = stream[i].flags >> 8;
        const size_t w0 = clanes.size();
        while (i < stream.size() && (stream[i].flags >> 8) == lvl && 64 - (clanes.size() - w0) >= 3) {
            OrbLane hl = stream[i];
            hl.x = (uint16_t)(hl.x - 4);
            hl.flags |= 1;
            clanes.push_back(hl);
            size_t room = 64 - (clanes.size() - w0) - 1;   // the right halo takes the last slot
            OrbLane last = stream[i];
            while (room > 0) {
                last = stream[i];
                clanes.push_back(last);
                ++i;
                --room;
                if (!(i < stream.size() && same_strip(last, stream[i]))) break;
            }
            OrbLane hr = last;
            hr.x = (uint16_t)(hr.x + 4);
            hr.flags |= 1;
            clanes.push_back(hr);
        }
        while (clanes.size() - w0 < 64) clanes.push_back(dead_lane(lvl, 16, ORBFE_EDGE, 0));
    }
    T.plan.nfwaves_c = (int)(clanes.size() / 64);
}

void plan_fast_lanes(int rows_fast, OrbPlanTables &T)
{
    // The dense kernel of batch handles (k_fast_map_u) walks whole CELL ROWS: a run of rows starts on a cell-row boundary and
    // ends on one (or at the end of the detectable interior), and a wave holds runs of ONE length only -- the reference's FAST
    // never looks across a cell boundary (:798-838), so such a run needs no strength row of its neighbours, and everything that
    // depends on the position inside the run alone is scalar in the kernel.  k cell rows per run, k = rows_fast / hcell rounded (1 for the default
    // 40 rows and the ~31-row cells of every shipped configuration).  Handles made for a few frames per call (rows_fast < 24)
    // keep short balanced runs and the generic kernel: such a call is bound by the length of one wave's walk.
    const bool cellrows = rows_fast >= 24;
    T.plan.fast_cellrows = cellrows ? 1 : 0;
    const std::vector<OrbLane> stream = fast_strips(T.plan, rows_fast, false);
    pack_dense(cellrows ? fast_strips(T.plan, rows_fast, true) : stream, cellrows, T);
    pack_compacting(stream, T);
}

// ---------------------------------------------------------------------------------------------------
// blur weights
// ---------------------------------------------------------------------------------------------------
// k_blur7's border lanes: folded horizontal weights per (level, lane type) -- tap t of output pixel c sits on column
// reflect101(c - 3 + t), and taps that land on the same column add up (at most 49 + 49: a byte)
orbfe_status plan_blur_weights(OrbPlan &P)
{
    for (int l = 0; l < P.nlevels; ++l) {
        const OrbLevel &L = P.lv[l];
        if (L.w < 16) { orbfe_set_error("level %d too narrow for the blur kernel", l); return ORBFE_ERR_SIZE; }
        const int kern[7] = {18, 34, 49, 55, 49, 34, 18};
        const int xlast = ((L.w - 1) / 4) * 4;
        const int xs[4] = {4, 0, xlast - 4, xlast};   // a lane of every type
        for (int ty = 0; ty < 4; ++ty) {
            const int x = xs[ty], base = std::min(std::max(x - 4, 0), L.w - 12);
            for (int j = 0; j < 4; ++j) {
                const int c = std::min(x + j, L.w - 1);   // output pixels past the row's end are computed and not stored
                for (int t = 0; t < 7; ++t) {
                    int col = c - 3 + t;
                    if (col < 0) col = -col;
                    if (col >= L.w) col = 2 * L.w - 2 - col;
                    const int bi = col - base;
                    if (bi < 0 || bi > 11) { orbfe_set_error("level %d: blur window of column %d does not hold column %d", l, x, col); return ORBFE_ERR_SIZE; }
                    P.blur_wt[l][ty][3 * j + bi / 4] += (uint32_t)kern[t] << (8 * (bi % 4));
                }
            }
        }
    }
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// blur lanes
// ---------------------------------------------------------------------------------------------------
// blur lane list: every 4-px column of every (balanced, <= ORBFE_ROWS_PER_WAVE rows) row block, single-level waves, no
// halos.  Lanes do not talk to each other, so a wave can hold columns of different row blocks.  Columns whose 12-byte
// window [x - 4, x + 8) lies inside the row (flag bit 1: no reflected column) skip the byte rearrangement of the border
// path, so they get waves of their own.  Everything is laid out in 64-BYTE PIECES (16 lanes): the left and the right piece
// of a row block go to the border waves whole, the pieces between them to the interior waves -- every store instruction
// then writes whole 64-byte pieces.  (Border waves holding only the 2 - 3 reflected columns of 20-odd row blocks wrote a
// lone dword into 64 different lines per store: WRITE_SIZE was 1.19x the output, profiles/r04_ab_experiments.json;
// ORBFE_OPT_BLUR_PIECES = 0 brings that packing back for the A/B.)

// what the layouts of one level share
struct BlurLevel {
    const OrbPlanTables &T;
    int l;
    bool pieces;
    int ncol, nblk, rb;   // 4-px columns; row blocks and their (balanced) height
    int right0;           // first column of the 64-byte piece that holds the first column whose window reaches past the row's right end

    const OrbLevel &L() const { return T.plan.lv[l]; }
    int block_rows(int k) const { return std::min(rb, L().h - k * rb); }
    OrbLane lane(int c, int ys, int nr, bool interior, int flags = 0) const
    {
        return OrbLane{(uint16_t)(4 * c), (uint16_t)ys, (uint16_t)nr, (uint16_t)((l << 8) | (interior ? 2 : 0) | flags)};
    }
    // dead lanes shadow a column of the wave's kind
    OrbLane dead(bool interior_wave, int flags = 0) const { return dead_lane(l, interior_wave ? 4 : 0, 0, 0, (interior_wave ? 2 : 0) | flags); }
    bool is_interior(int c) const
    {
        const bool no_reflection = 4 * c >= 4 && 4 * c + 8 <= L().w;
        return pieces ? (no_reflection && c >= 16 && c < right0) : no_reflection;
    }
};

// One pass (0: interior waves, 1: border waves) of the layout, appended to ol.  nparity 2: the even row blocks' lanes first,
// then the odd blocks' with flag bit 3.
void blur_pass(const BlurLevel &B, int pass, int nparity, std::vector<OrbLane> &ol)
{
    for (int par = 0; par < nparity; ++par) {
        const int upflag = par ? 8 : 0;
        for (int k = 0; k < B.nblk; ++k) {
            if (nparity == 2 && (k & 1) != par) continue;
            const int ys = k * B.rb, nr = B.block_rows(k);
            if (nr <= 0) continue;
            for (int c = 0; c < B.ncol; ++c) {
                const bool interior = B.is_interior(c);
                if (interior != (pass == 0)) continue;
                ol.push_back(B.lane(c, ys, nr, interior, upflag));
                // the right piece is padded to its 16 slots, so that the next row block's left piece starts a piece again
                if (B.pieces && pass == 1 && c == B.ncol - 1)
                    while (ol.size() % 16) ol.push_back(B.dead(false, upflag));
            }
        }
        while (ol.size() % 64) ol.push_back(B.dead(pass == 0, upflag));
    }
}

// Odd row blocks walk UPWARDS (flag bit 3, wave-uniform: the even blocks' lanes come first, then the odd blocks'; the
// kernel is vertically symmetric).  Two neighbouring row blocks then read the rows around their common boundary at the
// same end of their walks -- both at the start or both at the end; all waves of a frame are in flight together -- and
// the second reader finds the halo rows in L2 instead of HBM: FETCH_SIZE of the kernel -18 % when every level does it.
// Keeping the two directions in waves of their own can cost a level one more (partly filled) wave, i.e. instructions,
// which is what the pipeline as a whole is bound by: a (level, pass) is split only where the wave count stays the same
// (ORBFE_OPT_BLUR_UPDOWN = 0: never, 2: always).
void blur_pass_updown(const BlurLevel &B, int pass, bool always, OrbPlanTables &T)
{
    std::vector<OrbLane> l1, l2;
    blur_pass(B, pass, 1, l1);
    blur_pass(B, pass, 2, l2);
    const bool split = always || l2.size() == l1.size();
    T.blanes.insert(T.blanes.end(), (split ? l2 : l1).begin(), (split ? l2 : l1).end());
}

void plan_blur_lanes(const OrbPlanIn &in, int rows_blur, OrbPlanTables &T)
{
    OrbPlan &P = T.plan;
    const int nl = P.nlevels;
    const int updown = std::max(0, std::min(2, in.opt_blur_updown));
    for (int l = 0; l < nl; ++l) {
        const OrbLevel &L = P.lv[l];
        BlurLevel B{T, l, in.opt_blur_pieces != 0};
        B.ncol = (L.w + 3) / 4;
        B.nblk = (L.h + rows_blur - 1) / rows_blur;
        B.rb = (L.h + B.nblk - 1) / B.nblk;
        B.right0 = (std::min(B.ncol - 1, std::max(0, (L.w - 8) / 4 + 1)) / 16) * 16;
        P.bwave_off[l] = (int)(T.blanes.size() / 64);
        for (int pass = 0; pass < 2; ++pass) {  // 0: interior waves, 1: border waves
            if (updown) blur_pass_updown(B, pass, updown == 2, T);
            else blur_pass(B, pass, 1, T.blanes);
        }
        P.bwave_off[l + 1] = (int)(T.blanes.size() / 64);
    }
    P.nbwaves = (int)(T.blanes.size() / 64);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------
orbfe_status orb_plan_build(const OrbPlanIn &in, int w, int ht, OrbPlanTables *out)
{
    OrbPlanTables &T = *out;
    T = OrbPlanTables();
    OrbPlan &P = T.plan;
    memset(&P, 0, sizeof(P));
    const int nl = P.nlevels = in.nlevels;
    P.w = w;
    P.h = ht;
    P.ini_th = std::min(255, std::max(0, in.ini_th_fast));
    P.min_th = std::min(255, std::max(0, in.min_th_fast));
    P.blur_rounding = in.blur_rounding;
    P.dbg = in.opt_debug;
    // Rows a FAST / blur wave walks.  Long runs amortise the 8 (FAST) / 6 (blur) halo rows -- right for batches, whose waves
    // fill the chip anyway.  A handle made for the online call (a frame or a few per call) is latency-bound instead: one wave's
    // walk IS the kernel's duration, so it takes short runs and more waves: single 640x480 frame, FAST 41 -> 25 -> 21 us and blur
    // 19 -> 11 -> 9 us with 40 -> 16 -> 8 rows (ORBFE_OPT_ROWS overrides, 8..512).
    int rows_per_wave = in.max_batch <= 2 ? 8 : (in.max_batch <= 8 ? 16 : ORBFE_ROWS_PER_WAVE);
    if (in.opt_rows >= 8 && in.opt_rows <= 512) rows_per_wave = in.opt_rows;
    // the FAST and the blur walk can take different run lengths (ORBFE_OPT_ROWS_FAST / ORBFE_OPT_ROWS_BLUR; A/B in
    // profiles/r04_ab_experiments.json): a longer run amortises the 8 (FAST) / 6 (blur) halo steps, a shorter one balances better
    int rows_fast = rows_per_wave, rows_blur = rows_per_wave;
    if (in.opt_rows_fast >= 8 && in.opt_rows_fast <= 512) rows_fast = in.opt_rows_fast;
    if (in.opt_rows_blur >= 8 && in.opt_rows_blur <= 512) rows_blur = in.opt_rows_blur;

    orbfe_status s;
    LevelSums S;
    for (int l = 0; l < nl; ++l) {
        if ((s = plan_level(in, l, w, ht, T, S)) != ORBFE_OK) return s;
        if (l >= 1 && (s = level_taps(l, P, T.tabs)) != ORBFE_OK) return s;
        if (P.lv[l].w > 4095 + 2 * ORBFE_MINB || P.lv[l].h > 4095 + 2 * ORBFE_MINB) {
            orbfe_set_error("level %d exceeds the 12-bit key coordinate range", l);
            return ORBFE_ERR_SIZE;
        }
    }
    if ((s = plan_totals(S, T)) != ORBFE_OK) return s;
    plan_fast_lanes(rows_fast, T);
    if ((s = plan_blur_weights(P)) != ORBFE_OK) return s;
    plan_blur_lanes(in, rows_blur, T);
    if (P.ini_th < P.min_th) {
        orbfe_set_error("iniThFAST (%d) must be >= minThFAST (%d)", P.ini_th, P.min_th);
        return ORBFE_ERR_ARG;
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_internal_plan_table(const orbfe_params *p, const int32_t knobs[6], int32_t w, int32_t h, int32_t which,
                                                  void *dst, size_t cap, size_t *bytes)
{
    if (!p || !knobs || !bytes || w < 1 || h < 1 || w > 4096 || h > 4096 || which < 0 || which > 6) {
        orbfe_set_error("bad argument to orbfe_internal_plan_table");
        return ORBFE_ERR_ARG;
    }
    OrbPlanIn in;
    orbfe_status s = orb_ctor_tables(p, &in, nullptr, nullptr);
    if (s != ORBFE_OK) return s;
    in.opt_rows = knobs[0]; in.opt_rows_fast = knobs[1]; in.opt_rows_blur = knobs[2];
    in.opt_blur_pieces = knobs[3]; in.opt_blur_updown = knobs[4]; in.opt_debug = knobs[5];
    OrbPlanTables T;
    if ((s = orb_plan_build(in, w, h, &T)) != ORBFE_OK) return s;
    const struct { const void *p; size_t n; } tables[7] = {
        {&T.plan, sizeof(OrbPlan)},
        {T.cells.data(), T.cells.size() * sizeof(OrbCell)},
        {T.tabs.data(), T.tabs.size() * sizeof(OrbTab)},
        {T.flanes.data(), T.flanes.size() * sizeof(OrbLane)},
        {T.clanes.data(), T.clanes.size() * sizeof(OrbLane)},
        {T.blanes.data(), T.blanes.size() * sizeof(OrbLane)},
        {&T.fast_row_steps, sizeof(T.fast_row_steps)}};
    *bytes = tables[which].n;
    if (!dst) return ORBFE_OK;   // sizing call
    if (cap < *bytes) { orbfe_set_error("orbfe_internal_plan_table: %zu bytes needed, %zu given", *bytes, cap); return ORBFE_ERR_CAP; }
    if (*bytes) memcpy(dst, tables[which].p, *bytes);
    return ORBFE_OK;
}
