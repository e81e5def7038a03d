"""DynaSLAM::Geometry on the GPU at its edges, each against tests/geometry_oracle.py bit for bit: the gates of ExtractDynPoints, the
shapes OpenCV's gemm treats differently, empty references, the seed order and the passes of DepthRegionGrowing, the smallest
image.  tests/test_geometry_oracle.py shows with the oracle that each scene sits on its edge."""
import numpy as np
import pytest

import geometry_cases as GC
import geometry_oracle as GO
from geometry_checks import check_scene
from orb_slam2_ssd_semantic_amd import Geometry
from orb_slam2_ssd_semantic_amd import geometry as GE

pytestmark = pytest.mark.gpu
F = np.float32


def test_key_point_depth_either_side_of_6():
    kf = GC.plane(3.0)
    below = np.nextafter(F(6), F(0))
    kf[30, 20], kf[30, 40], kf[30, 60], kf[50, 20] = below, 6.0, 0.0, np.nextafter(F(0), F(1))
    keys = [(20.5, 30.5), (40.5, 30.5), (60.5, 30.5), (20.5, 50.5)]
    _, taps = check_scene(GC.single_ref_scene(keys, kf, GC.plane(2.3)))
    assert taps["counts"]["read"] == 4 and taps["counts"]["depth"] == 2


def test_projected_depth_either_side_of_7():
    _, taps = check_scene(GC.depth7_scene())
    assert (taps["counts"]["parallax"], taps["counts"]["depth7"]) == (2, 1)


def test_parallax_either_side_of_30_degrees():
    _, taps = check_scene(GC.parallax_scene())
    assert 0 < taps["counts"]["parallax"] < taps["counts"]["depth"]


def test_equal_translations_drop_the_nan_angles():
    _, taps = check_scene(GC.nan_scene())
    assert taps["counts"]["parallax"] == 16 - int(np.isnan(taps["stages"]["angles"]).sum()) < 16


@pytest.mark.parametrize("side", ["left", "right", "top", "bottom"])
def test_projection_at_the_border(side):
    """the re-projected pixel is ceil(x), and IsInFrame wants 21 < x < w - 21: columns 21 | 22 and w - 22 | w - 21, rows likewise"""
    w, h = GC.W1, GC.H1
    keys = {"left": [(20.4, 40.5), (21.4, 40.5)], "right": [(w - 22.6, 40.5), (w - 21.6, 40.5)],
            "top": [(48.5, 20.4), (48.5, 21.4)], "bottom": [(48.5, h - 22.6), (48.5, h - 21.6)]}[side]
    _, taps = check_scene(GC.single_ref_scene(keys, GC.plane(3.0), GC.plane(2.3)))
    px = [(x, y) for x, y, _ in taps["stages"]["projected"]]
    assert px == {"left": [(22, 41)], "right": [(w - 22, 41)], "top": [(49, 22)], "bottom": [(49, h - 22)]}[side]
    assert taps["counts"]["depth7"] == 2 and taps["counts"]["in_frame"] == 1


def test_current_depth_zero_under_the_projection():
    cur = GC.plane(2.3)
    cur[41, 49] = 0.0
    _, taps = check_scene(GC.single_ref_scene([(48.5, 40.5), (60.5, 40.5)], GC.plane(3.0), cur))
    assert taps["counts"]["depth7"] == 2 and taps["counts"]["in_frame"] == 1


@pytest.mark.parametrize("n_near", [0, 1, 2, 3, 4])
def test_window_and_variance(n_near):
    """0: no neighbour below the projected depth (the point is dropped); 2, 3: neighbours of equal difference, the first in scan
    order wins; 3 | 4: the patch variance either side of 0.001"""
    _, taps = check_scene(GC.window_scene(n_near))
    c = taps["counts"]
    assert (c["found"], c["gate"], c["dyn"]) == [(0, 0, 0), (1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 0)][n_near]


@pytest.mark.parametrize("n", [1, 4, 16, 17])
def test_survivor_counts_that_change_the_gemm(n):
    _, taps = check_scene(GC.count_scene(n))
    assert taps["counts"]["parallax"] == taps["counts"]["depth7"] == taps["counts"]["dyn"] == n


@pytest.mark.parametrize("rank", [0, 1, 2, 3, 4])
def test_references_without_survivors(rank):
    """four of the five references have no keypoint: before, around and after the one that has"""
    _, taps = check_scene(GC.rank_scene(rank))
    assert set(taps["dyn"][:, 2]) == {rank}


def test_no_survivor_anywhere():
    sc = GC.single_ref_scene(np.zeros((0, 2), F), GC.plane(3.0), GC.plane(2.3))
    g, taps = check_scene(sc)
    mask, computed = g.correct(sc["cur_depth"], sc["cur_T"], *sc["K"])
    assert computed == 1 and mask.all() and taps["counts"]["read"] == 0


def _regions(im, seeds, max_seeds):
    g = Geometry(im.shape[1], im.shape[0], max(1, (len(seeds) + 4) // 5), max_seeds)
    want, acc, union, regions = GO.depth_region_growing(seeds, im)
    mask, got_acc, got_union = GE.depth_region_growing(g, seeds, im)
    assert np.array_equal(mask, want) and np.array_equal(got_acc, acc) and np.array_equal(got_union, union)
    return g, acc, regions


def test_two_seeds_in_one_region_and_seed_order():
    im, A, B = GC.staircase()
    _, acc, _ = _regions(im, [A, B], 8)
    assert acc.tolist() == [1, 0]   # B lies in A's region: skipped
    _, acc, _ = _regions(im, [B, A], 8)
    assert acc.tolist() == [1, 1]   # the other order grows both, and the union differs (tests/test_geometry_oracle.py)
    _regions(im, [B, A], 1)         # the same through two passes that carry the union
    _regions(im, [A, B, A, (2, 2), B], 2)


@pytest.mark.parametrize("n", [8, 9, 16, 17, 30])
def test_more_seeds_than_max_seeds(n):
    """max_seeds = 8: n seeds at, one past and several times the capacity, a covered and a zero-depth seed among them"""
    im, seeds = GC.seed_grid(n)
    seeds[3] = (seeds[2][0] + 1, seeds[2][1])   # on seed 2's frontier
    im[seeds[5][1], seeds[5][0]] = 0.0
    g, acc, regions = _regions(im, seeds, 8)
    assert acc.sum() == n - 2 and not acc[3] and not acc[5]
    last = (n - 1) // 8 * 8
    for i in range(last, n):   # the regions of the last pass
        J = g.tap(GE.TAP_REGION, index=i - last, shape=im.shape)
        assert np.array_equal(J, regions.get(i, np.zeros_like(J))), i


@pytest.mark.parametrize("case", ["threshold", "last_entry", "plateau", "corner"])
def test_region_growing_hand_cases(case):
    """the hand-worked planes of tests/test_geometry_oracle.py; the corner seed on a 47 x 45 plane of its own"""
    if case == "corner":
        im = np.full((45, 47), 5.0, F)
        im[0, 0] = im[0, 1] = 1.0
        x, y = 0, 0
    else:
        spots = {"threshold": [(4, 4), (5, 4)], "last_entry": [(4, 4), (4, 5)], "plateau": []}[case]
        im, x0, y0 = GC.embed(GC.plane9(spots) if spots else np.full((9, 9), 5.0, F))
        x, y = x0 + 4, y0 + 4
    g = Geometry(47, 45, 1, 1)
    assert np.array_equal(GE.region_growing(g, im, x, y), GO.region_growing(im, x, y))


def test_constant_plane_and_smallest_image():
    """a constant 48 x 46 plane (the growth ends with one list entry left) and a 45 x 45 scene"""
    im = np.full((46, 48), 2.0, F)
    g = Geometry(48, 46, 1, 1)
    J = GE.region_growing(g, im, 10, 10)
    assert J.all() and np.array_equal(J, GO.region_growing(im, 10, 10))
    K = GC.intrinsics(45, 45)
    T = GC.ACTIVE_T
    cur_T = T.copy()
    cur_T[0, 3] += F(0.002)
    none = np.zeros((0, 2), F)
    frames = [dict(Tcw=P, depth=np.full((45, 45), 3.0, F), keys=none, keys_un=none) for P in GC.key_poses(4, 31, rot=0.03, trans=0.3)]
    keys = np.array([(21.5, 21.5), (20.5, 21.5), (23.5, 21.5), (21.5, 23.5)], F)   # pixels (22, 22) | (21, 22) (24, 22) (22, 24)
    frames.append(dict(Tcw=T, depth=np.full((45, 45), 3.0, F), keys=keys, keys_un=keys))
    cur = np.full((45, 45), 2.3, F)
    _, taps = check_scene(dict(K=K, key_frames=frames, cur_T=cur_T, cur_depth=cur))
    assert taps["counts"]["in_frame"] == 1 and taps["dyn"].tolist() == [[22, 22, taps["refs"].index(4)]]
    with pytest.raises(Exception):
        Geometry(44, 45, 1, 1)
