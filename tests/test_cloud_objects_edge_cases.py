"""tests/cloud_edge_cases.py and tests/objects_edge_cases.py checked on the CPU, on the oracles and the planner's port alone, so
that tests/test_gpu_cloud_edges.py and tests/test_gpu_objects_edges.py cannot go blind when someone edits a case: every case
reaches the seam it is there for.  The seams: entry 1024 of k_cloud_scan (item 262 144 of the kernels that feed it), the second
grid-stride trip of k_cloud_minmax, the three breaks of knn_plan, the AUTO mode's switch at 2048 finite points, the voxel grid's
overflow, the paint's chunks of 256 candidates."""
import numpy as np
import pytest

import cloud_cases as CC
import cloud_edge_cases as CE
import cloud_oracle as CO
import objects_cases as OC
import objects_edge_cases as OE
import objects_oracle as OO

F = np.float32


def past_the_seam(segments):
    """the compaction has more than 1024 entries, the counts behind entry 1024 differ from one another, the placement is the
    ordered one, and a scan that lost its carry at entry 1024 would place the items elsewhere"""
    segs = segments if isinstance(segments, list) else [segments]
    counts = np.concatenate([CE.block_counts(s) for s in segs])
    assert len(counts) > CE.SCAN
    assert len(set(counts[CE.SCAN:].tolist())) > 1 or len(counts) == CE.SCAN + 1
    good, bad = CE.placement(segs), CE.placement(segs, reset_at=CE.SCAN)
    assert good.tolist() == list(range(len(good)))
    assert good.tolist() != bad.tolist()
    return counts


# ---- the scan model itself ---------------------------------------------------------------------------------------------------------
def test_scan_model():
    counts = np.arange(2500) % 7
    want = np.cumsum(counts) - counts
    assert CE.exclusive_scan(counts).tolist() == want.tolist()
    broken = CE.exclusive_scan(counts, reset_at=1024)
    assert broken[:1024].tolist() == want[:1024].tolist() and broken[1024] == 0 and broken[2048] == counts[1024:2048].sum()
    assert CE.SEAM == 262144 and CE.blocks_of(CE.SEAM) == 1024 and CE.blocks_of(CE.SEAM + 1) == 1025


# ---- A: past 1024 workgroups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "rows"])
def test_big_frame_passes_the_seam(kind):
    f = CE.big_frame(kind)
    flags = CE.kept_flags(f)
    counts = past_the_seam(flags)
    assert len(counts) == 1026 and counts[CE.SCAN:].tolist() != [256, 256]
    got = CO.generate_point_cloud(*f)
    assert len(got) == int(flags.sum()) == int(counts.sum())
    if kind == "mixed":
        assert len(got) == 262649
    else:
        assert len(set(counts.tolist())) >= 8 and (counts == 0).any() and 0 < len(got) < 262649


def test_three_frames_straddle_entry_1024():
    w, h, B = CE.STRADDLE
    assert CE.blocks_of(w * h) == 352 and 2 * 352 < CE.SCAN < 3 * 352
    flags = [CE.kept_flags(f) for f in CE.batch(w, h, B, 400)]
    past_the_seam(flags)
    assert len(set(int(f.sum()) for f in flags)) == B           # the per-keyframe counts tell the keyframes apart


@pytest.mark.parametrize("total", sorted(CE.BATCH_TOTALS))
def test_batch_totals(total):
    w, h, B = CE.BATCH_TOTALS[total]
    assert CE.blocks_of(w * h) * B == total and (w * h) % CE.WG != 0     # the last workgroup of every keyframe is partial
    counts = np.concatenate([CE.block_counts(CE.kept_flags(f)) for f in CE.batch(w, h, B, 500 + total)])
    assert len(counts) == total and len(set(counts.tolist())) > 8


@pytest.fixture(scope="module")
def voxel_clouds():
    return {nf: CE.voxel_cloud(nf) for nf in (False, True)}


@pytest.mark.parametrize("not_finite", [False, True])
@pytest.mark.parametrize("leaf,voxels", [(0.05, 8001), (0.25, 65)])
def test_voxel_cloud_passes_the_seam(voxel_clouds, leaf, voxels, not_finite):
    pts = voxel_clouds[not_finite]
    heads = CE.head_flags(pts, leaf)
    counts = past_the_seam(heads)
    assert len(pts) == 262400 and len(counts) == 1025 and counts[1024] >= 1 and int(heads.sum()) == voxels
    nfin = CE.bounds(pts)[2]
    if not_finite:
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
        bad = np.nonzero(~np.isfinite(xyz).all(1))[0]
        assert 40 <= len(bad) <= 51 and (bad < CE.SEAM).sum() > 10 and (bad >= CE.SEAM).sum() > 10
        assert CE.SEAM < nfin == len(pts) - len(bad)
    else:
        assert nfin == len(pts)


def test_second_trip_holds_every_extreme():
    pts = CE.second_trip_cloud()
    assert len(pts) == CE.SEAM + CE.TAIL and CE.blocks_of(len(pts)) == 1026
    mn, mx, nfin = CE.bounds(pts)
    mn1, mx1, nfin1 = CE.bounds(pts[:CE.SEAM])
    assert (mn < mn1).all() and (mx > mx1).all()                 # all six sides come from the second trip
    assert nfin == len(pts) - 2 and nfin1 == CE.SEAM
    assert CO.voxel_plan(pts, 0.25) != CO.voxel_plan(pts[:CE.SEAM], 0.25)
    assert len(CO.voxel_grid(pts, 0.25)[0]) != len(CO.voxel_grid(pts[:CE.SEAM], 0.25)[0])
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
    fin = np.isfinite(xyz).all(1)
    lo, hi = np.where(fin[:, None], xyz, np.inf), np.where(fin[:, None], xyz, -np.inf)
    assert {int(i) // CE.WG for i in np.r_[lo.argmin(0), hi.argmax(0)]} == {1024, 1025}      # both workgroups of the second trip bring one
    mirror = CE.second_trip_cloud(mirror=True)
    m = CE.bounds(mirror)
    m1 = CE.bounds(mirror[:CE.WG])
    assert m[0].tobytes() == m1[0].tobytes() == mn.tobytes() and m[1].tobytes() == m1[1].tobytes() == mx.tobytes()
    assert CO.voxel_plan(mirror, 0.25) == CO.voxel_plan(pts, 0.25)


def test_big_inserts_cross_the_seam():
    om = CO.Map(CE.INSERT_LEAF)
    first, second = CE.big_inserts()
    c1 = om.insert(first)
    n1 = len(om.pts)
    c2 = CO.generate_point_cloud(*second[0])
    assert n1 < CE.SEAM < n1 + len(c2) and c1[0] > CE.SEAM       # the append of the second insert crosses item 262 144
    assert not om.overflow and n1 > 1024


# ---- B: overflow -------------------------------------------------------------------------------------------------------------------
def test_overflow_plan():
    om = CO.Map(CE.OVERFLOW_LEAF)
    total = 0
    for frames in CE.overflow_inserts():
        cloud = CO.generate_point_cloud(*frames[0])
        assert CO.voxel_plan(np.concatenate([om.pts, cloud]), CE.OVERFLOW_LEAF) == "overflow"
        counts = om.insert(frames)
        total += counts[0]
        assert om.overflow and len(om.pts) == total and om.pts[-counts[0]:].tobytes() == cloud.tobytes()
    assert CO.voxel_plan(om.pts, 0.05) != "overflow"             # the depths are ordinary: it is the leaf that overflows


# ---- C: paint ----------------------------------------------------------------------------------------------------------------------
def test_paint_chunk_counts():
    d, bgr = CE.constant_plane()
    for box, n in CE.CHUNK_BOXES.items():
        idx = CO.paint_box(d, bgr.copy(), box, (1, 2, 3))[0]
        assert len(idx) == n == CE.paint_need([box])
    assert [n % CE.WG for n in CE.CHUNK_BOXES.values()] == [0, 0, 8]


def test_paint_boxes_that_produce_nothing():
    d, bgr = CC.paint_frame(CE.PAINT_W, CE.PAINT_H, 7)
    for box in CE.NOTHING_BOXES:
        img = bgr.copy()
        boxes = [CE.ORDINARY_BOXES[0], box, CE.ORDINARY_BOXES[1]]
        idx = CO.paint_boxes(d, img, boxes, [(1, 2, 3), (4, 5, 6), (7, 8, 9)])
        assert len(idx[0]) > 0 and len(idx[1]) == 0 and len(idx[2]) > 0 and CE.paint_need([box]) == 0
        alone = bgr.copy()
        CO.paint_boxes(d, alone, [boxes[0], boxes[2]], [(1, 2, 3), (7, 8, 9)])
        assert np.array_equal(img, alone)                        # no pixel changed by the box in the middle


def test_paint_box_over_the_right_edge():
    d, bgr = CC.paint_frame(CE.PAINT_W, CE.PAINT_H, CE.EDGE_SEED)
    idx = CO.paint_box(d, bgr.copy(), CE.EDGE_BOX, (1, 2, 3))[0]
    cols = set((idx % CE.PAINT_W).tolist())
    assert len(idx) == 97 and {0, 1, 2} <= cols and max(cols) >= 49
    assert CE.EDGE_BOX[0] - 1 + CE.EDGE_BOX[2] - 2 > CE.PAINT_W  # the painted columns run past the plane's width


# ---- D: the planner ----------------------------------------------------------------------------------------------------------------
def test_every_older_case_takes_the_density_break():
    sets = [p for p, _, _ in OC.CASES.values()] + [OC.border_base(1), OC.blobs(20000, 77, outliers=0.02)]
    assert [OE.plan_of(p)[0]["brk"] for p in sets] == ["density"] * len(sets)
    assert OE.plan_of(OC.CASES["far_point"][0])[0]["dims"] == [109, 1, 1]


@pytest.mark.parametrize("name", ["line", "far_point_4100"])
def test_axis_limit_is_reached(name):
    plan, nfin = OE.plan_of(OE.GRID_CASES[name][0])
    assert plan["brk"] == "maxdim" and plan["dims"] == [808, 1, 1] and plan["cells"] * 4 < nfin
    extent = float(np.ptp(OE.GRID_CASES[name][0][:, 0]))
    assert 798 < extent * float(plan["inv_cell"]) < OE.KNN_MAX_DIM - 2      # what the stop rule's proof rests on
    res = OO.statistical_outlier_removal(OC.rec(OE.GRID_CASES[name][0]), 50, 1.0)
    if name == "far_point_4100":
        assert res["keep"].tolist() == [True] * 4100 + [False]   # exactly the far point goes
    else:
        OC.vacuity(res)


def test_zero_extents():
    for name, dims in (("flat_sheet", [15, 15, 1]), ("flat_line", [265, 1, 1])):
        pts, ks = OE.GRID_CASES[name]
        plan, _ = OE.plan_of(pts)
        assert plan["brk"] == "density" and plan["dims"] == dims and ks == (50, 6)
        assert [float(np.ptp(pts[:, k])) == 0 for k in range(3)] == [d == 1 for d in dims]
        for k in ks:
            OC.vacuity(OO.statistical_outlier_removal(OC.rec(pts), k, 1.0))


def test_planner_port_other_exits():
    assert OE.knn_plan([0, 0, 0], [0, 0, 0], 100)["brk"] == "one_cell"
    assert OE.knn_plan([0, 0, 0], [np.inf, 1, 1], 100) is None
    assert OE.knn_plan([-3e38, 0, 0], [3e38, 1, 1], 100) is None                  # the extent is not finite
    big = OE.knn_plan([0, 0, 0], [1, 1, 1], 1 << 30)
    assert big["brk"] == "maxcells" and big["cells"] <= OE.KNN_MAX_CELLS and max(big["dims"]) < OE.KNN_MAX_DIM - 2
    assert OE.plan_of(OC.coincident(80))[0]["brk"] == "one_cell"


def test_exactly_64_finite_points():
    pts = OE.exactly_64()
    res = OO.statistical_outlier_removal(OC.rec(pts), 63, 1.0)
    assert len(pts) == 67 and res["n_finite"] == 64 and res["status"] == OO.OK
    assert OO.statistical_outlier_removal(OC.rec(pts[:-2]), 63, 1.0)["status"] == OO.TOO_FEW      # one finite point fewer
    OC.vacuity(res)


def test_auto_switch_counts():
    for nfin in (2048, 2049):
        pts = OE.auto_switch(nfin)
        assert len(pts) == nfin + 3 and int(np.isfinite(pts).all(1).sum()) == nfin
    assert OE.KNN_AUTO_BRUTE == 2048


def test_grid_sets_differ_in_size_and_plan():
    sets = OE.grid_sets()
    assert [len(s) for s in sets] == [100, 3000, 4096, 80, 0, 60]
    cells = [OE.plan_of(s)[0]["cells"] for s in sets if len(s)]
    assert cells[0] < cells[1] < cells[2] and cells[3] == 1 and cells[4] < cells[0]          # the scratch grows, then shrinks in use
    assert OO.statistical_outlier_removal(OC.rec(sets[4]), 50, 1.0)["status"] == OO.EMPTY


def test_stddev_mul_kept_counts():
    pts = OC.rec(OE.stddev_points())
    kept = [int(OO.statistical_outlier_removal(pts, 50, mul)["keep"].sum()) for mul in OE.STDDEV_MULS]
    assert tuple(kept) == OE.STDDEV_KEPT == (280, 300, 0, 0)
    thr = [OO.statistical_outlier_removal(pts, 50, mul)["threshold"] for mul in OE.STDDEV_MULS]
    assert thr[1] == np.inf and thr[3] == -np.inf and thr[2] < 0 < thr[0]


def test_stddev_frame_objects():
    d, bgr, K, T, lists = OE.stddev_frame()
    objs = OO.frame_objects(d, bgr, K, T, lists, 0.05, 50, OE.SM_MUL)
    assert [o["status"] for o in objs] == [OO.EMPTY, OO.TOO_FEW, OO.OK]
    assert (objs[0]["n_kept"], objs[0]["n_voxels"]) == (0, 0) and objs[0]["threshold"] < 0
    assert objs[1]["n_kept"] == objs[1]["n_in"] == 32
    assert 0 < objs[2]["n_voxels"] <= objs[2]["n_kept"] < objs[2]["n_in"]


# ---- E: compaction past 1024 workgroups, indices outside the plane -----------------------------------------------------------------
def test_outside_objects_pass_the_seam():
    objs, lists = OE.outside_objects()
    assert [len(ix) for ix in lists] == [OE.E_NAN_INDICES, 1200, 33] and OE.E_NAN_INDICES > CE.SEAM
    assert [o["status"] for o in objs] == [OO.TOO_FEW, OO.OK, OO.TOO_FEW]
    d, bgr, K, T, _ = OE.outside_frame()
    cloud = OO.organised_cloud(d, bgr, K, T)
    assert not np.isfinite(cloud["z"][lists[0]]).any()           # object 0: no finite point, no neighbour search
    assert objs[0]["n_kept"] == OE.E_NAN_INDICES and objs[2]["n_kept"] == 33
    assert 0 < objs[1]["n_kept"] < 1200 and objs[1]["n_voxels"] > 0
    assert sorted(set(lists[2].tolist()) - set(lists[1].tolist())) == [-1, OE.E_W * OE.E_H, OE.INT32_MAX]
    past_the_seam(OE.kept_flags(objs))
