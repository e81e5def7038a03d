"""tests/geometry_oracle.py against hand-worked cases of DynaSLAM::Geometry (perfect/src/Geometry.cc), and the library's host-only
entry points against the oracle.  No GPU."""
import math
import struct

import numpy as np
import pytest

import geometry_cases as GC
import geometry_oracle as GO

F = np.float32


def pixels(J):
    return sorted((int(x), int(y)) for y, x in np.argwhere(J))


def test_ring_of_25_inserts():
    """InsertFrame2DB (:532-550): mNumElem stops at 19, slot 19 is never written, inserts 19..24 overwrite slots 0..5, and
    GetRefFrames reads slots 0..18"""
    db = GO.DataBase()
    for i in range(25):
        db.insert(i)
        assert db.num == min(i + 1, 19)
    assert db.num == 19 and (db.ini, db.fin) == (6, 5)
    assert db.slots == [19, 20, 21, 22, 23, 24] + list(range(6, 19)) + [None]
    assert db.slots[:db.num] == [19, 20, 21, 22, 23, 24] + list(range(6, 19))


def test_pose_read_through_at_double():
    """rotm2euler reads the CV_32F pose through at<double>: "R(i, j)" is the double made of the floats at flat positions
    4 i + 2 j and 4 i + 2 j + 1 of the pose, so the angles are not the rotation's"""
    T = GC.pose(0.1, 0.2, 0.3, 0.5, -0.4, 0.3)
    flat = T.reshape(16)

    def pun(i, j):
        return struct.unpack("<d", struct.pack("<ff", flat[4 * i + 2 * j], flat[4 * i + 2 * j + 1]))[0]

    assert GO.pose_as_double(T, 1, 0) == pun(1, 0) and GO.pose_as_double(T, 2, 2) == pun(2, 2) == 0.0   # (2, 2) is the pose's last row
    sy = F(math.sqrt(pun(0, 0) ** 2 + pun(1, 0) ** 2))
    want = [float(F(math.atan2(pun(2, 1), pun(2, 2)))), float(F(math.atan2(-pun(2, 0), float(sy)))),
            float(F(math.atan2(pun(1, 0), pun(0, 0))))]
    assert GO.rotm2euler(T) == want
    meant = GO.rotm2euler(T, punned=False)
    assert np.allclose(meant, [0.1, 0.2, 0.3], atol=1e-6)
    assert max(abs(a - b) for a, b in zip(want, meant)) > 1.0


def test_region_growing_threshold_pixel_and_frontier():
    """two pixels of 1 in a plane of 5, seed on the left one.  Step 1 takes the right one (entry 1, distance 0); step 2 finds
    only distances of 4, takes entry 0 all the same (the pixel that crosses the threshold is still added) and stops without
    looking at its neighbours.  J = both pixels and their six neighbours: the frontier is in the result."""
    trace = []
    J = GO.region_growing(GC.plane9([(4, 4), (5, 4)]), 4, 4, trace=trace)
    assert trace == [(1, 5, 4, 0.0), (0, 3, 4, 4.0)]
    assert pixels(J) == sorted([(4, 4), (5, 4), (3, 4), (4, 3), (4, 5), (6, 4), (5, 3), (5, 5)])


def test_region_growing_last_entry_is_no_candidate():
    """the equal pixel lies BELOW the seed, so it is the fourth and last entry of the list, which the scan `i < neg_pos` never
    reaches: the growth takes entry 0 at distance 4 and ends"""
    trace = []
    J = GO.region_growing(GC.plane9([(4, 4), (4, 5)]), 4, 4, trace=trace)
    assert trace == [(0, 3, 4, 4.0)]
    assert pixels(J) == sorted([(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)])


def test_region_growing_swap_remove_on_a_plateau():
    """all distances equal: entry 0 wins every time and the last entry takes its place.  By hand: (3,4) goes, (4,5) moves to
    0; its neighbours (2,4) (3,3) (3,5) are appended, (4,5) goes and (3,5) moves to 0; (5,5) (4,6) are appended, (3,5) goes."""
    trace = []
    J = GO.region_growing(GC.plane9(), 4, 4, trace=trace)
    assert trace[:3] == [(0, 3, 4, 0.0), (0, 4, 5, 0.0), (0, 3, 5, 0.0)]
    assert J.all() and len(trace) == 79


def test_constant_plane_ends_one_short_of_reg_size():
    """A constant 48 x 46 plane: every pixel ends in J.  The list's last entry is never a candidate, so the growth stops with
    one entry left, after w*h - 2 steps (reg_size = w*h - 1): `reg_size < total` is still true when minMaxLoc finds nothing."""
    trace = []
    J = GO.region_growing(np.full((46, 48), 2.0, F), 10, 10, trace=trace)
    assert J.all() and len(trace) == 48 * 46 - 2 and all(t[3] == 0.0 for t in trace)


def test_region_growing_seed_on_the_border():
    """seed in the corner: two of its neighbours are outside.  (1,0) is entry 0 and the only candidate; then (0,1) at 4."""
    trace = []
    J = GO.region_growing(GC.plane9([(0, 0), (1, 0)]), 0, 0, trace=trace)
    assert trace == [(0, 1, 0, 0.0), (0, 0, 1, 4.0)]
    assert pixels(J) == sorted([(0, 0), (1, 0), (0, 1), (2, 0), (1, 1)])


def test_seed_order_changes_the_union():
    im, A, B = GC.staircase()
    _, acc_ab, u_ab, _ = GO.depth_region_growing([A, B], im)
    _, acc_ba, u_ba, _ = GO.depth_region_growing([B, A], im)
    assert acc_ab.tolist() == [1, 0] and acc_ba.tolist() == [1, 1]
    assert u_ab.sum() < u_ba.sum() and not u_ab[20, 45] and u_ba[20, 45]


@pytest.mark.parametrize("r", [10, 15, 1, 0])
def test_ellipse_half_widths(r):
    """getStructuringElement's dx = cvRound(r sqrt((r^2 - dy^2) / r^2)) against round(sqrt(r^2 - dy^2)) in integers"""
    want = [(math.isqrt(4 * (r * r - (i - r) ** 2)) + 1) // 2 for i in range(2 * r + 1)]
    assert GO.ellipse_half_widths(r) == want
    if r == 10:   # the 21x21 table of csrc/orbfe_flow.hip
        assert sorted(set(want)) == [0, 4, 6, 7, 8, 9, 10]
    from orb_slam2_ssd_semantic_amd import geometry
    assert geometry.ellipse_half_widths(r) == want


def test_dilate_is_the_ellipse():
    u = np.zeros((50, 60), np.uint8)
    u[25, 30] = 1
    d = GO.dilate_ellipse(u)
    hw = GO.ellipse_half_widths(15)
    for i, w in enumerate(hw):
        row = d[25 - 15 + i]
        assert row[30 - w:30 + w + 1].all() and row.sum() == 2 * w + 1
    u[:] = 0
    u[0, 0] = 1   # zeros outside the image
    assert GO.dilate_ellipse(u).sum() == sum(w + 1 for w in hw[15:])


def test_acos_known_answers():
    """the canonical acos: exact at the ends, NaN outside, and within one unit in the last place of the host's"""
    assert GO.geo_acos(1.0) == 0.0 and GO.geo_acos(-1.0) == math.pi and GO.geo_acos(0.0) == math.pi / 2
    assert math.isnan(GO.geo_acos(1.0000000000000002)) and math.isnan(GO.geo_acos(-1.5)) and math.isnan(GO.geo_acos(math.nan))
    assert GO.geo_acos(0.5) == 1.0471975511965979 and GO.geo_acos(1e-20) == math.pi / 2
    xs = np.concatenate([np.linspace(-1, 1, 4001), 1 - np.logspace(-16, -1, 200), np.logspace(-16, -1, 200) - 1,
                         [math.cos(math.radians(30)), np.nextafter(math.cos(math.radians(30)), 2)]])
    for x in xs:
        got, ref = GO.geo_acos(float(x)), math.acos(float(x))
        assert abs(got - ref) <= np.spacing(ref), x


def test_select_ref_frames_host():
    """the library's GetRefFrames (host only) against the oracle, on 19, 7, 5 and 3 poses"""
    from orb_slam2_ssd_semantic_amd import geometry
    for n, seed in ((19, 1), (7, 2), (5, 3), (3, 4)):
        db = GC.key_poses(n, seed, rot=0.2, trans=0.5)
        for cur in (GC.pose(0.01, 0.02, -0.03, 0.1, 0.0, -0.1), GC.pose(0.3, -0.2, 0.1, -0.4, 0.2, 0.3), db[0]):
            want = GO.select_ref_frames(cur, db)
            assert len(want) == min(5, n) and geometry.select_ref_frames(cur, db) == want


def test_scene_stages_are_all_exercised():
    """the box scene of the GPU tests: every filter of ExtractDynPoints drops something, only the first dynamic point is
    grown, and the union is the box and its border up to the ring pixels behind a box pixel that stayed the list's last entry"""
    sc = GC.box_scene()
    mask, done, t = GC.oracle_run(sc)
    c = t["counts"]
    assert done == 1 and c["depth7"] > c["in_frame"] > c["found"] > c["gate"] > c["dyn"] > 1
    assert t["accepted"].tolist() == [1] + [0] * (c["dyn"] - 1)
    x0, y0, bw, bh = sc["box"]
    full = GC.box_union(160, 120, sc["box"])
    assert t["union"][y0:y0 + bh, x0:x0 + bw].all() and not (t["union"] & ~full).any() and (full - t["union"]).sum() <= 4
    assert np.array_equal(mask, 1 - GO.dilate_ellipse(t["union"]))
    assert GC.oracle_run(sc, nkf=4)[:2][1] == 0 and GC.oracle_run(sc, nkf=4)[0].all()


def test_edge_scenes_sit_on_their_edges():
    """what the GPU edge tests rely on, shown with the oracle first"""
    assert [GC.oracle_run(GC.window_scene(n))[2]["counts"]["dyn"] for n in range(5)] == [0, 1, 1, 1, 0]
    assert GC.oracle_run(GC.window_scene(0))[2]["counts"]["found"] == 0 and GC.oracle_run(GC.window_scene(4))[2]["counts"]["gate"] == 1
    assert [GC.oracle_run(GC.count_scene(n))[2]["stages"]["mode"] for n in (1, 4, 16, 17)] == [2, 1, 0, 0]
    t = GC.oracle_run(GC.nan_scene())[2]
    nan = int(np.isnan(t["stages"]["angles"]).sum())
    assert 0 < nan < 16 and t["counts"]["parallax"] == 16 - nan
    a = np.array(GC.oracle_run(GC.parallax_scene())[2]["stages"]["angles"])
    assert (a < 26).sum() >= 4 and (a > 34).sum() >= 4
    sc = GC.depth7_scene()
    assert np.nextafter(sc["flip"][0], F(9)) == sc["flip"][1]
    c = GC.oracle_run(sc)[2]["counts"]
    assert (c["parallax"], c["depth7"]) == (2, 1)
    for r in (0, 1, 2, 3, 4):
        t = GC.oracle_run(GC.rank_scene(r))[2]
        assert t["counts"]["dyn"] == 12 and set(t["dyn"][:, 2]) == {r}
