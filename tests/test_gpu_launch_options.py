"""Every result-neutral launch option of the extractor (include/orbfe.h, orbfe_set_option) against the CPU oracle.

The header promises byte-identical results for every setting but ORBFE_OPT_BLUR_ROUNDING, and bench.py's A/B flags rely on it.
The options move run and workgroup boundaries: FAST row runs and their packing into waves (ROWS / ROWS_FAST), blur row blocks
and lane packing (ROWS_BLUR, BLUR_PIECES, BLUR_UPDOWN), pyramid lane runs (PYR_ROWS), quadtree workgroup sizes (QT_THREADS_*)
and the blur's stream (OVERLAP).  Each case compares, per level, the pyramid, the FAST candidates (survivors and order), the
quadtree selection and the blurred level, then keypoint bit patterns and descriptors.

The frame shapes are chosen in SHAPES below; test_shape_table_covers_the_run_boundaries (no GPU) checks that their levels
really reach the boundaries the sweep is about, with a short mirror of the planner's run split written here."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame
from test_gpu_extract import assert_same_output, cand_array

EDGE = 19   # EDGE_THRESHOLD: first detectable row / column of a level

# name: (width, height, nlevels, scale factor, nfeatures)
SHAPES = {
    "vga": (640, 480, 8, 1.2, 1000),      # the shipped configuration; hcell 31..34
    "odd": (517, 389, 8, 1.2, 700),       # odd sizes; level 7 has 2 cell rows of 39
    "strip": (1203, 301, 5, 1.35, 800),   # 4 to 6 quadtree roots per level; level 4 is ONE cell row of 59 rows
    "tiny": (209, 155, 6, 1.2, 300),      # level 5 is 84 x 62: one 30-row cell, the smallest level the FAST grid allows
    "narrow": (107, 127, 4, 1.2, 150),    # level 3 is 62 x 73: one 30-column cell, 16 blur columns
}

ROWS_FAST = (8, 9, 13, 23, 24, 25, 40, 48, 64, 100, 257, 512)
ROWS_BLUR = (8, 9, 15, 17, 41, 97, 512)
QT_THREADS = (64, 128, 192, 256, 320, 384, 448, 512)
BATCH = 9        # frames of a batched call: more than 8 (the pyramid's long runs, rows 40 by default)


# ---- level geometry and the planner's run split, mirrored on the host -------------------------------------------------------
@lru_cache(maxsize=None)
def level_geometry(shape):
    """per level: (w, h, hcell, ix1, iy1, roots) -- the FAST grid of src/ORBextractor.cc:780-838 from the oracle's cell_grid;
    ix1 / iy1 = one past the last detectable column / row"""
    from oracle import oracle_ffi as O
    w, h, nl, sf, nf = SHAPES[shape]
    lw, lh = O.OracleExtractor(nf, sf, nl, 20, 7).level_sizes(w, h)
    out = []
    for W, H in zip(lw.tolist(), lh.tolist()):
        ok, ncols, nrows, wcell, hcell = O.cell_grid(W, H)
        assert ok, (shape, W, H)
        minb, maxbx, maxby = EDGE - 3, W - EDGE + 3, H - EDGE + 3
        ys = [minb + i * hcell for i in range(nrows) if minb + i * hcell < maxby - 3]
        xs = [minb + j * wcell for j in range(ncols) if minb + j * wcell < maxbx - 6]
        iy1 = min(ys[-1] + hcell + 6, maxby) - 3
        ix1 = min(xs[-1] + wcell + 6, maxbx) - 3
        roots = int(np.float32(maxbx - minb) / np.float32(maxby - minb) + np.float32(0.5))   # round() of :547
        out.append(dict(w=W, h=H, hcell=hcell, ix1=ix1, iy1=iy1, roots=roots))
    return out


def fast_runs(L, rows_fast):
    """(first row, rows) of the FAST runs of one level: cell-row runs of kc whole cell rows (rows_fast >= 24, the dense kernel
    k_fast_map_u) or balanced blocks of at most rows_fast rows (k_fast_map and the lane-compacting kernel)"""
    rows = L["iy1"] - EDGE
    if rows_fast >= 24:
        kc = max(1, (rows_fast + L["hcell"] // 2) // L["hcell"])
        rb = kc * L["hcell"]
        return [(ys, min(rb, L["iy1"] - ys)) for ys in range(EDGE, L["iy1"], rb)]
    nblk = -(-rows // rows_fast)
    rb = -(-rows // nblk)
    return [(EDGE + k * rb, min(rb, L["iy1"] - EDGE - k * rb)) for k in range(nblk) if L["iy1"] - EDGE - k * rb > 0]


def fast_work(shape, rows_fast):
    """(row steps, waves) per frame of the dense FAST lane list -- orbfe_get_work_counts: strips of 4-px columns per run, packed
    into single-level waves of 64 lanes, a halo lane on each side of a strip cut by a wave boundary, and in the cell-row form
    runs of one length per wave"""
    cellrows = rows_fast >= 24
    stream = []
    for lvl, L in enumerate(level_geometry(shape)):
        ncol = (L["ix1"] - 16 + 3) // 4
        for ys, nr in fast_runs(L, rows_fast):
            stream += [(lvl, 16 + 4 * c, ys, nr) for c in range(ncol)]

    def same_strip(a, b):
        return a[0] == b[0] and a[2] == b[2] and b[1] == a[1] + 4

    i, steps, waves = 0, 0, 0
    while i < len(stream):
        first = stream[i]
        lanes = [stream[i - 1][3]] if i > 0 and same_strip(stream[i - 1], stream[i]) else []
        while i < len(stream) and stream[i][0] == first[0] and (not cellrows or stream[i][3] == first[3]) and len(lanes) < 64:
            if len(lanes) == 63 and i + 1 < len(stream) and same_strip(stream[i], stream[i + 1]):
                lanes.append(stream[i][3])
                break
            lanes.append(stream[i][3])
            i += 1
        steps += max(lanes + [first[3] if cellrows else 0]) + 8
        waves += 1
    return steps, waves


def default_rows(max_batch):
    return 8 if max_batch <= 2 else (16 if max_batch <= 8 else 40)


# ---- frames and the oracle's answers (computed once per module) ---------------------------------------------------------------
@lru_cache(maxsize=None)
def frame(shape, i):
    w, h = SHAPES[shape][:2]
    return synth_frame(7000 + 50 * list(SHAPES).index(shape) + i, h, w, sparse=(i % 3 == 2))


def clustered_frame(k):
    """all corners inside one box (tests/test_gpu_extract.py::test_clustered_corners_deep_quadtree): near-empty and deep trees"""
    x0, y0, bw, bh = ((200, 150, 96, 96), (19, 19, 60, 60), (500, 380, 120, 80), (300, 30, 40, 400))[k]
    img = np.full((480, 640), 128, np.uint8)
    img[y0:y0 + bh, x0:x0 + bw] = synth_frame(900 + k)[y0:y0 + bh, x0:x0 + bw]
    return img


class Ref:
    """what the oracle computes for one frame: output and every per-level tap"""

    def __init__(self, oracle, shape, img, blur_mode):
        w, h, nl, sf, nf = SHAPES[shape]
        oe = oracle.OracleExtractor(nf, sf, nl, 20, 7)
        oe.set_blur_mode(blur_mode)
        self.kps, self.desc = oe(img, cap=nf + 16 * nl + 64)
        self.levels = [oe.level(l) for l in range(nl)]
        self.cands = [cand_array(oe.candidates(l)) for l in range(nl)]
        self.sel = [cand_array(oe.selected(l)) for l in range(nl)]
        self.blurred = [oe.blurred(l) if len(self.sel[l]) else None for l in range(nl)]


_REFS = {}


def ref(oracle, shape, i, blur_mode=0):
    """i: frame index (int) or ('clustered', k)"""
    key = (shape, i, blur_mode)
    if key not in _REFS:
        img = clustered_frame(i[1]) if isinstance(i, tuple) else frame(shape, i)
        _REFS[key] = Ref(oracle, shape, img, blur_mode)
    return _REFS[key]


def check_frame(e, f, r, label, stages=("level", "cand", "sel", "blur")):
    for l in range(len(r.levels)):
        if "level" in stages:
            assert np.array_equal(e.pyramid_level(l, f), r.levels[l]), (label, "pyramid", l)
        if "cand" in stages:
            assert np.array_equal(e.candidates(l, f), r.cands[l]), (label, "FAST candidates", l)
        if "sel" in stages:
            assert np.array_equal(e.selected(l, f), r.sel[l]), (label, "quadtree", l)
        if "blur" in stages and r.blurred[l] is not None:
            assert np.array_equal(e.blurred_level(l, f), r.blurred[l]), (label, "blurred", l)


def extractor(shape, max_batch=1, **kw):
    from orb_slam2_ssd_semantic_amd import ORBextractor
    w, h, nl, sf, nf = SHAPES[shape]
    return ORBextractor(nf, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=max_batch, **kw)


class DeviceBatch:
    """one orbfe_extract_batch_device call on HBM-resident frames; the output blocks start as 0xA5 garbage so the
    zero-filled padding is checked too.  The input stays alive with the object (level 0 is read in place by the taps)."""

    def __init__(self, e, frames):
        import torch
        B, h, w = frames.shape
        cap = e.capacity()
        self.dg = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        dk = torch.full((B, cap * 28), 0xA5, dtype=torch.uint8, device="cuda")
        dd = torch.full((B, cap, 32), 0xA5, dtype=torch.uint8, device="cuda")
        dn = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        e.extract_batch_device(self.dg.data_ptr(), B, w, h, w, w * h, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.overflow() == 0
        self.n, self.kraw, self.desc = dn.cpu().numpy(), dk.cpu().numpy(), dd.cpu().numpy()

    def output(self, b):
        from orb_slam2_ssd_semantic_amd import KP_DTYPE
        n = int(self.n[b])
        assert not self.kraw[b, n * 28:].any() and not self.desc[b, n:].any(), ("padding not zero-filled", b)
        return self.kraw[b, :n * 28].copy().view(KP_DTYPE), self.desc[b, :n]


# ---- the shape table, checked without a GPU ---------------------------------------------------------------------------------
def test_shape_table_covers_the_run_boundaries(oracle):
    """The sweep's shapes reach the boundaries the options move (a sweep over easy shapes would pass vacuously)."""
    lv = [(s, l, L) for s in SHAPES for l, L in enumerate(level_geometry(s))]
    rows = [L["iy1"] - EDGE for _, _, L in lv]
    # balanced FAST blocks: a level whose detectable rows split exactly, leave one row, or leave one row short, for every
    # run length of the generic form
    for r in ROWS_FAST:
        if r < 24:
            assert {0, 1, r - 1} <= {n % r for n in rows}, r
    # cell-row FAST runs: at least three run lengths put 2+ cell rows into one run on level 0 of every shape (interior cell
    # seams inside a run: up_ok / dn_ok / ord_wrap of orbfe_fast_body.inc with CELLROWS), and runs are cut short at the end of a level
    for s in SHAPES:
        L0 = level_geometry(s)[0]
        kcs = [max(1, (r + L0["hcell"] // 2) // L0["hcell"]) for r in ROWS_FAST if r >= 24]
        assert sum(k >= 2 for k in kcs) >= 3, s
    assert any(len(fast_runs(L, r)) >= 2 and fast_runs(L, r)[-1][1] < fast_runs(L, r)[0][1]
               for _, _, L in lv for r in ROWS_FAST if r >= 48)
    hcells = {L["hcell"] for _, _, L in lv}
    assert len(hcells) >= 5 and max(hcells) >= 50, sorted(hcells)
    assert {L["w"] % 4 for _, _, L in lv} == {0, 1, 2, 3}
    # blur: columns of 4 px in 64-byte pieces of 16 columns: column counts at 16k - 1, 16k and 16k + 1
    assert {15, 0, 1} <= {((L["w"] + 3) // 4) % 16 for _, _, L in lv}
    assert max(L["roots"] for _, _, L in lv) >= 4
    # the one-cell minimum of the FAST grid: 30 px plus 2 x 16 border (62 px), in height and in width
    assert min(L["h"] for _, _, L in lv) <= 64 and min(L["w"] for _, _, L in lv) <= 64
    # pyramid: widths that are not a multiple of 256 px (waves of mixed row runs)
    assert any(L["w"] % 256 for _, _, L in lv)
    # the mirror agrees with itself where the planner must not change: 24 / 25 / 40 rows make the same cell-row plan wherever
    # every cell is 31..34 rows high, and the generic form differs from the cell-row form
    assert fast_work("vga", 24) == fast_work("vga", 40) != fast_work("vga", 23)


# ---- FAST runs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows_fast", ROWS_FAST)
def test_fast_run_length(oracle, rows_fast):
    """ROWS_FAST on a single-frame handle (default 8 rows) and a 9-frame device batch (default 40 rows), dense FAST (0, 1: the
    cell-row kernel k_fast_map_u from 24 rows on) and lane-compacting FAST (2).  The work counts of the plan must be those of
    the mirror, so the option provably took effect."""
    changed = 0
    for shape in SHAPES:
        single = extractor(shape, 1, options={"rows_fast": rows_fast})
        batch = extractor(shape, BATCH, options={"rows_fast": rows_fast})
        frames = np.stack([frame(shape, i) for i in range(BATCH)])
        refs = [ref(oracle, shape, i) for i in range(BATCH)]
        for mode in (0, 1, 2):
            label = (shape, rows_fast, mode)
            single.set_fast_mode(mode)
            batch.set_fast_mode(mode)
            gk, gd = single(frames[0])
            check_frame(single, 0, refs[0], label + ("single",))
            assert_same_output(gk, gd, refs[0].kps, refs[0].desc)
            db = DeviceBatch(batch, frames)
            for b in range(BATCH):
                assert_same_output(*db.output(b), refs[b].kps, refs[b].desc)
            for b in (0, BATCH - 1):
                check_frame(batch, b, refs[b], label + ("batch", b))
        for e, mb in ((single, 1), (batch, BATCH)):
            got = e.work_counts()
            want = fast_work(shape, rows_fast)
            assert (got["fast_row_steps_per_frame"], got["fast_waves_per_frame"]) == want, (shape, mb, got, want)
            changed += want != fast_work(shape, default_rows(mb))
    # the option moved the plan away from the handle's default: on every shape for at least one of the two handles (8 rows is
    # the single-frame default; 24 / 25 / 40 rows make the batch default's one-cell-row runs on 31..34-row cells)
    assert changed >= len(SHAPES), changed


# ---- blur row blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rows_blur", ROWS_BLUR)
def test_blur_row_blocks(oracle, rows_blur):
    """ROWS_BLUR x BLUR_UPDOWN {0, 1, 2} x BLUR_PIECES {0, 1} x BLUR_ROUNDING {0, 1} on every shape of the table (every
    width % 4, column counts 16k - 1 / 16k / 16k + 1), two frames per call: blurred levels and output."""
    for shape in SHAPES:
        e = extractor(shape, 2, options={"rows_blur": rows_blur})
        frames = np.stack([frame(shape, i) for i in range(2)])
        for rounding in (0, 1):
            e.set_option("blur_rounding", rounding)
            refs = [ref(oracle, shape, i, rounding) for i in range(2)]
            for updown in (0, 1, 2):
                for pieces in (0, 1):
                    e.set_option("blur_updown", updown)
                    e.set_option("blur_pieces", pieces)
                    res = e.extract_batch(frames)
                    for b in range(2):
                        label = (shape, rows_blur, rounding, updown, pieces, b)
                        check_frame(e, b, refs[b], label, stages=("blur",))
                        assert_same_output(*res[b], refs[b].kps, refs[b].desc)


# ---- pyramid runs -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pyr_rows", range(2, 17))
def test_pyramid_run_length(oracle, pyr_rows):
    """PYR_ROWS (k_pyr_walk's destination rows per lane run) on 1-frame and 9-frame calls (defaults 2 and 16), odd sizes,
    scale factors 1.2 and 1.35: every pyramid level and the output."""
    for shape in SHAPES:
        e = extractor(shape, BATCH, options={"pyr_rows": pyr_rows})
        frames = np.stack([frame(shape, i) for i in range(BATCH)])
        refs = [ref(oracle, shape, i) for i in range(BATCH)]
        gk, gd = e(frames[1])
        check_frame(e, 0, refs[1], (shape, pyr_rows, "single"), stages=("level",))
        assert_same_output(gk, gd, refs[1].kps, refs[1].desc)
        db = DeviceBatch(e, frames)
        for b in range(BATCH):
            assert_same_output(*db.output(b), refs[b].kps, refs[b].desc)
        for b in (0, 4, BATCH - 1):
            check_frame(e, b, refs[b], (shape, pyr_rows, "batch", b), stages=("level",))


# ---- quadtree workgroups ------------------------------------------------------------------------------------------------------
QT_FRAMES = [0, 1, ("clustered", 0), ("clustered", 1), ("clustered", 2), ("clustered", 3)]


def qt_frame(i):
    return clustered_frame(i[1]) if isinstance(i, tuple) else frame("vga", i)


@pytest.mark.gpu
@pytest.mark.parametrize("qt", QT_THREADS)
def test_quadtree_workgroup_size(oracle, qt):
    """QT_THREADS_0 on the ungrouped path (fewer than 128 frames: one k_octree launch for all levels with that many threads,
    including 64 and the sizes that are not powers of two), dense-corner and clustered-box frames, DEBUG 0 / 50 (streaming key
    passes only) / 51 (generic node passes only), plus the 4..6-root strip.  Not covered here: k_octree<true> (node arrays in
    global scratch, nfeatures beyond ~2400 on one level) always launches QT_MAX = 512 threads whatever the option says."""
    e = extractor("vga", len(QT_FRAMES), options={"qt_threads_0": qt})
    s = extractor("strip", 1, options={"qt_threads_0": qt})
    frames = np.stack([qt_frame(i) for i in QT_FRAMES])
    refs = [ref(oracle, "vga", i) for i in QT_FRAMES]
    for debug in (0, 50, 51):
        e.set_option("debug", debug)
        s.set_option("debug", debug)
        res = e.extract_batch(frames)
        for b, r in enumerate(refs):
            check_frame(e, b, r, (qt, debug, QT_FRAMES[b]), stages=("cand", "sel"))
            assert_same_output(*res[b], r.kps, r.desc)
        rs = ref(oracle, "strip", 0)
        gk, gd = s(frame("strip", 0))
        check_frame(s, 0, rs, (qt, debug, "strip"), stages=("sel",))
        assert_same_output(gk, gd, rs.kps, rs.desc)


GROUP_FRAMES = QT_FRAMES + [2, 3]   # 8 distinct frames, 16 times over: one call of 128 frames


def group_batch():
    return np.stack([qt_frame(GROUP_FRAMES[i % len(GROUP_FRAMES)]) for i in range(128)])


@pytest.mark.gpu
@pytest.mark.parametrize("qts", [(64, 64, 64), (192, 320, 448), (512, 512, 512)])
def test_grouped_quadtree_workgroup_sizes(oracle, qts):
    """128 frames: the quadtree launches once per level group with QT_THREADS_0 / 1 / 2 threads each."""
    e = extractor("vga", 128, options={f"qt_threads_{i}": v for i, v in enumerate(qts)})
    refs = [ref(oracle, "vga", i) for i in GROUP_FRAMES]
    db = DeviceBatch(e, group_batch())
    for b in range(128):
        r = refs[b % len(refs)]
        assert_same_output(*db.output(b), r.kps, r.desc)
    for b in range(len(refs)):
        check_frame(e, b, refs[b], (qts, b), stages=("sel",))


# ---- blur stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [-1, 0, 1, 2])
def test_overlap(oracle, overlap):
    """OVERLAP (blur inline / on the side stream from before FAST / beside the quadtree / by batch size) on 1, 9 and 128
    frames."""
    e = extractor("vga", 128, options={"overlap": overlap})
    refs = [ref(oracle, "vga", i) for i in GROUP_FRAMES]
    gk, gd = e(qt_frame(GROUP_FRAMES[0]))
    check_frame(e, 0, refs[0], (overlap, 1), stages=("blur",))
    assert_same_output(gk, gd, refs[0].kps, refs[0].desc)
    frames = group_batch()
    for B in (9, 128):
        db = DeviceBatch(e, frames[:B])
        for b in range(B):
            r = refs[b % len(refs)]
            assert_same_output(*db.output(b), r.kps, r.desc)
        for b in (0, 7):
            check_frame(e, b, refs[b], (overlap, B, b), stages=("blur",))


# ---- options changed on a live handle -----------------------------------------------------------------------------------------
LIVE = [  # (option, non-default value, default)
    ("overlap", 2, -1), ("rows", 48, 0), ("rows_fast", 100, 0), ("rows_blur", 17, 0), ("blur_pieces", 0, 1),
    ("blur_updown", 2, 1), ("pyr_rows", 5, 0), ("qt_threads_0", 192, 0), ("qt_threads_1", 320, 0), ("qt_threads_2", 448, 0),
    ("debug", 50, 0), ("blur_rounding", 1, 0),
]


@pytest.mark.gpu
def test_options_changed_between_calls_and_reset(oracle):
    """One handle: every option set to a non-default value between calls, one more per call, then set back one by one; each
    call equals the oracle (the plan is rebuilt where an option needs it).  After the reset, the padded output blocks equal
    those of a fresh default handle byte for byte, zero-filled slots included."""
    e = extractor("vga", BATCH)
    frames = np.stack([frame("vga", i) for i in range(BATCH)])
    state = {name: default for name, _, default in LIVE}

    def call(label):
        db = DeviceBatch(e, frames)
        mode = state["blur_rounding"]
        refs = [ref(oracle, "vga", i, mode) for i in range(BATCH)]
        for b in range(BATCH):
            assert_same_output(*db.output(b), refs[b].kps, refs[b].desc)
        check_frame(e, 0, refs[0], label)
        rf = state["rows_fast"] or state["rows"] or default_rows(BATCH)
        got = e.work_counts()
        assert (got["fast_row_steps_per_frame"], got["fast_waves_per_frame"]) == fast_work("vga", rf), (label, got)
        return db

    call("default")
    for name, value, _ in LIVE:
        e.set_option(name, value)
        state[name] = value
        call(("set", name))
    for name, _, default in LIVE:
        e.set_option(name, default)
        state[name] = default
        db = call(("reset", name))
    fresh = DeviceBatch(extractor("vga", BATCH), frames)
    assert np.array_equal(db.n, fresh.n)
    assert np.array_equal(db.kraw, fresh.kraw) and np.array_equal(db.desc, fresh.desc)


# ---- through the pipeline bench.py times -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_with_bench_options(oracle):
    """FramePipeline of 2 pipes x 8-frame sub-batches, 18 frames (3 sub-batches) with rows_fast / rows_blur / overlap set on its
    extractors as bench.py's A/B flags do: keypoints, descriptors and matches to the previous frame equal the oracle's."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, FramePipeline
    w, h, nl, sf, nf = SHAPES["vga"]
    N = 18
    frames = np.stack([frame("vga", i) for i in range(N)])
    refs = [ref(oracle, "vga", i) for i in range(N)]
    pl = FramePipeline(nf, sf, nl, 20, 7, max_width=w, max_height=h, sub_batch=8, npipes=2)
    for ex in pl.extractors:
        ex.set_option("rows_fast", 64)
        ex.set_option("rows_blur", 41)
        ex.set_option("overlap", 2)
    cap = pl.capacity()
    dg = torch.from_numpy(frames).cuda()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    dk, dd, dn = z((N, cap, 7), torch.int32), z((N, cap, 32), torch.uint8), z(N, torch.int32)
    dm, dnm = z((N, cap), torch.int32), z(N, torch.int32)
    pl.extract_match_device(dg.data_ptr(), N, w, h, w, w * h, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(), dm.data_ptr(),
                            dnm.data_ptr(), flags=0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert pl.overflow() == 0
    n, kps, desc, match, nm = (t.cpu().numpy() for t in (dn, dk, dd, dm, dnm))
    for k, r in enumerate(refs):
        nk = int(n[k])
        assert_same_output(kps[k, :nk].copy().view(KP_DTYPE).reshape(-1), desc[k, :nk], r.kps, r.desc)
        if k == 0:
            assert int(nm[k]) == 0 and np.all(match[k, :nk] == -1)
            continue
        p = refs[k - 1]
        rm, _, _, rn = oracle.match_bf(r.desc, p.desc, r.kps["angle"], p.kps["angle"], 0.9, 100, True)
        assert int(nm[k]) == rn and np.array_equal(match[k, :nk], rm), k
        assert np.all(match[k, nk:] == -1), k


# ---- rejected values -----------------------------------------------------------------------------------------------------------
REJECTED = [("rows", 7), ("rows", 513), ("rows", -1), ("rows_fast", 7), ("rows_fast", 513), ("rows_fast", -1),
            ("rows_blur", 7), ("rows_blur", 513), ("rows_blur", -1), ("pyr_rows", 1), ("pyr_rows", 17)] + \
           [(f"qt_threads_{i}", v) for i in range(3) for v in (32, 96, 576, -64)] + \
           [("blur_pieces", 2), ("blur_updown", 3), ("overlap", -2), ("overlap", 3)]


@pytest.mark.gpu
def test_rejected_values_leave_the_handle_as_it_was(oracle):
    """Out-of-range values answer ORBFE_ERR_ARG and change nothing: the next call still equals the oracle and keeps the
    default plan."""
    from orb_slam2_ssd_semantic_amd import _ffi
    e = extractor("tiny", 1)
    L = _ffi.lib()
    r = ref(oracle, "tiny", 0)
    for name, value in REJECTED:
        assert L.orbfe_set_option(e.handle, _ffi.OPTIONS[name], C.c_int32(value)) == _ffi.ORBFE_ERR_ARG, (name, value)
        gk, gd = e(frame("tiny", 0))
        check_frame(e, 0, r, (name, value))
        assert_same_output(gk, gd, r.kps, r.desc)
        got = e.work_counts()
        assert (got["fast_row_steps_per_frame"], got["fast_waves_per_frame"]) == fast_work("tiny", default_rows(1)), (name, value)
