"""Known answers, worked out by hand, for tests/cloud_oracle.py (the unpinned restatement of the reference's point-cloud map) and
for the host-only orbfe_cloud_pose_matrix.  No GPU."""
import ctypes as C
import math

import numpy as np

import cloud_oracle as CO

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_generate_2x2_identity():
    # fx = fy = 1, cx = cy = 0.5: x = (c - 0.5) * d, y = (r - 0.5) * d
    depth = np.array([[1, 2], [0, np.nan]], F)
    bgr = np.array([[[1, 2, 3], [4, 5, 6]], [[7, 8, 9], [10, 11, 12]]], np.uint8)
    out = CO.generate_point_cloud(depth, bgr, (1, 1, 0.5, 0.5), np.eye(4))
    assert len(out) == 3                                     # the NaN pixel is dropped, the zero-depth one is kept
    assert out["x"].tolist() == [-0.5, 1.0, 0.0] and out["y"].tolist() == [-0.5, -1.0, 0.0] and out["z"].tolist() == [1.0, 2.0, 0.0]
    assert bits(out["x"])[2] == 0                            # (-0.0 + 0.0 + 0.0) + 0.0 in the transform is +0.0
    assert out["rgba"].tolist() == [0xff030201, 0xff060504, 0xff090807]


def test_generate_overflow_in_x_and_in_the_transform():
    depth = np.array([[3e38, 1e38]], F)
    bgr = np.zeros((1, 2, 3), np.uint8)
    T = np.eye(4)
    assert len(CO.generate_point_cloud(depth, bgr, (1, 1, 2, 0), T)) == 1       # (0 - 2) * 3e38 is -inf; (1 - 2) * 1e38 is finite
    T[2, 2] = 4.0                                                                # z = 4e38 does not fit a float
    assert len(CO.generate_point_cloud(depth, bgr, (1, 1, 2, 0), T)) == 0
    T[2, 2], T[0, 3] = 1.0, 5.0
    out = CO.generate_point_cloud(np.array([[2.0]], F), np.zeros((1, 1, 3), np.uint8), (2, 2, 1, 1), T)
    assert (out["x"][0], out["y"][0], out["z"][0]) == (4.0, -1.0, 2.0)          # (0 - 1) * 2 / 2 = -1, plus 5


def test_voxel_exact_multiples_of_the_leaf():
    # leaf 0.5, inverse exactly 2: floor(-1.5) = -2 but (int)-1.5 = -1, floor(-0.5) = -1 but (int)-0.5 = 0
    x = [-1.0, -0.5, 0.0, 0.5, 1.0, -0.75, -0.25]
    red = [10, 20, 30, 40, 50, 13, 21]
    pts = CO.records([[v, 0, 0] for v in x], [0xff000000 | (r << 16) for r in red])
    plan = CO.voxel_plan(pts, 0.5)
    assert plan == (F(2), [-2, 0, 0], [1, 5, 5])
    assert CO.voxel_keys(pts, plan).tolist() == [0, 1, 2, 3, 4, 0, 1]
    out, ovf = CO.voxel_grid(pts, 0.5)
    assert not ovf and out["x"].tolist() == [-0.875, -0.375, 0.0, 0.5, 1.0]
    assert [(c >> 16) & 255 for c in out["rgba"].tolist()] == [11, 20, 30, 40, 50]   # (10 + 13) / 2 = 11.5 -> 11, (20 + 21) / 2 -> 20
    assert all(c >> 24 == 255 for c in out["rgba"].tolist())


def test_voxel_leaf_one_centimetre():
    # 1.0f / 0.01f rounds to exactly 100.0f (0.01f is 0.00999999977..., its reciprocal 100.0000022 is nearer 100 than the next
    # float, 100.0000076); what shows is the float product p * inverse_leaf: 0.29f = 0.28999999165 times 100 is 28.99999917,
    # which rounds to the float 29.0, so the point lies in cell 29 and not in cell 28 where real arithmetic puts it
    assert F(1) / F(0.01) == F(100) and float(F(0.01)) != 0.01
    assert float(F(0.29)) * 100.0 < 29.0 and F(0.29) * F(100) == F(29)
    pts = CO.records([[0, 0, 0], [0.29, 0, 0], [0.2850, 0, 0]], [0xff000000] * 3)
    plan = CO.voxel_plan(pts, 0.01)
    assert plan == (F(100), [0, 0, 0], [1, 30, 30])
    assert CO.voxel_keys(pts, plan).tolist() == [0, 29, 28]
    out, _ = CO.voxel_grid(pts, 0.01)
    assert out["x"].tolist() == [0.0, float(F(0.285)), float(F(0.29))]              # ascending idx, not input order


def test_voxel_more_cells_than_int_max():
    far = CO.records([[0, 0, 0], [1e6, 1e6, 0]], [1, 2])      # (1e8 + 1)^2 cells
    out, ovf = CO.voxel_grid(far, 0.01)
    assert ovf and out.tobytes() == far.tobytes()
    line = CO.records([[0, 0, 0], [1e6, 0, 0]], [1, 2])       # 1e6 m apart along one axis: 1e8 + 1 cells, below INT_MAX
    out, ovf = CO.voxel_grid(line, 0.01)
    assert not ovf and len(out) == 2
    out, ovf = CO.voxel_grid(CO.records([[0, 0, 0], [3e38, 0, 0]], [1, 2]), 0.01)   # 3e40 does not fit a float, let alone an int64
    assert ovf and len(out) == 2


def test_voxel_empty_and_not_finite():
    out, ovf = CO.voxel_grid(np.zeros(0, CO.REC_DTYPE), 0.05)
    assert len(out) == 0 and not ovf
    pts = CO.records([[np.nan, 0, 0], [0.01, 0.01, 0.01], [0, np.inf, 0]], [1, 0xff112233, 3])
    out, ovf = CO.voxel_grid(pts, 0.05)
    assert len(out) == 1 and out["rgba"][0] == 0xff112233 and out["x"][0] == F(0.01)
    assert len(CO.voxel_grid(pts[[0, 2]], 0.05)[0]) == 0


def test_voxel_sum_order_is_the_stable_one():
    # one voxel (leaf 2^26): 2^24 + 1 rounds back to 2^24 (ties to even), so front to back the sum is 2^24; back to front it
    # is (1 + 1) + 2^24 = 2^24 + 2
    pts = CO.records([[16777216, 0, 0], [1, 0, 0], [1, 0, 0]], [0xff000000] * 3)
    stable, _ = CO.voxel_grid(pts, 2.0 ** 26)
    rev, _ = CO.voxel_grid(pts, 2.0 ** 26, order="reversed")
    assert len(stable) == 1 and len(rev) == 1
    assert stable["x"][0] == F(16777216) / F(3) == F(5592405.5)
    assert rev["x"][0] == F(16777218) / F(3) == F(5592406)
    assert stable["x"][0] != rev["x"][0]
    # 255 * n passes 2^24 at n = 65794: from there on a float colour sum no longer moves by 255 exactly
    white = CO.records(np.zeros((3, 3)), [0xffffffff] * 3)
    assert CO.centroid(white)[3] == 0xffffffff


def _box_frame():
    # 16 x 12, box (4, 3, 10, 10): beg = 4 + 2 * 16 - 1 = 35; the mean window is rows k = 3 .. 6 (10 * 0.3 and 10 * 0.7
    # are exactly 3.0 and 7.0 in double) and columns 3 .. 6 of each; the paint covers rows 0 .. 8, columns 0 .. 7
    depth = np.full((12, 16), 2.0, F)
    bgr = np.zeros((12, 16, 3), np.uint8)
    return depth, bgr, (4.0, 3.0, 10.0, 10.0), 35


def test_box_mean_includes_half_a_metre_and_six():
    depth, bgr, box, beg = _box_frame()
    assert 10 * 0.7 == 7 and 10 * 0.3 == 3
    win = [beg + k * 16 + j for k in range(3, 7) for j in range(3, 7)]
    assert CO.box_touched(box, 16, 12) == (beg, beg + 8 * 16 + 7)
    flat = depth.reshape(-1)
    flat[win[0]], flat[win[1]], flat[win[2]], flat[win[3]] = 0.5, 6.0, np.nextafter(F(0.5), F(0)), np.nextafter(F(6), F(7))
    flat[beg + 2 * 16 + 3] = 100.0      # the row above the window
    flat[beg + 7 * 16 + 3] = 100.0      # the row below it
    flat[beg + 3 * 16 + 7] = 100.0      # the column right of it
    flat[beg + 3 * 16 + 2] = 100.0      # the column left of it
    _, mean = CO.paint_box(depth, bgr, box, (1, 2, 3))
    assert mean == F(30.5) / F(14)      # 12 x 2.0 + 0.5 + 6.0 over 14 pixels: both bounds are inside, their neighbours outside
    flat[win] = 0.0
    idx, mean = CO.paint_box(depth, bgr, box, (1, 2, 3))
    assert mean == 0 and set(idx.tolist()) == set(win)     # nothing in range: the mean is 0 and |d| < 0.4 still paints


def test_box_paint_at_the_edge_of_forty_centimetres():
    depth, bgr, box, beg = _box_frame()
    flat = depth.reshape(-1)
    hi, lo = F(2.4), F(1.6)
    assert float(hi - F(2)) >= 0.4 and float(F(2) - lo) < 0.4     # 2.4f - 2 = 0.4000001, 2 - 1.6f = 0.39999998
    flat[beg:beg + 4] = [hi, np.nextafter(hi, F(0)), lo, np.nextafter(lo, F(0))]
    idx, mean = CO.paint_box(depth, bgr, box, (9, 8, 7))
    assert mean == 2.0
    region = [beg + k * 16 + j for k in range(9) for j in range(8)]
    assert idx.tolist() == [j for j in region if j not in (beg, beg + 3)]
    painted = np.zeros(12 * 16, bool)
    painted[idx] = True
    assert (bgr.reshape(-1, 3)[painted] == (9, 8, 7)).all() and not bgr.reshape(-1, 3)[~painted].any()


def test_box_outside_the_image():
    depth, bgr, _, _ = _box_frame()
    for box in ((0, 1, 10, 5), (4, 0, 10, 10), (4, 3, 10, 12), (8, 3, 16, 11)):
        t = CO.box_touched(box, 16, 12)
        assert t[0] < 0 or t[1] >= 16 * 12, box
    assert CO.box_touched((4, 3, 10, 11.9), 16, 12)[1] < 16 * 12      # (int)11.9 = 11 rows still fit
    assert CO.box_touched((0, 3, 10, 10), 16, 12)[0] == 31          # x = 0 reaches into the row above: flat indices, defined
    assert CO.box_touched((0, 0, 5, 0), 16, 12) is None      # no rows: touches nothing, not an error


# ---- orbfe_cloud_pose_matrix (host only) ---------------------------------------------------------------------------------------
def test_pose_matrix_normalises_the_quaternion():
    from orb_slam2_ssd_semantic_amd import pose_matrix
    # R = 2 I: trace 6, w = sqrt(7) / 2, x = y = z = 0; normalised w = 1, so the rotation that comes back is I, not 2 I
    T = np.eye(4, dtype=F)
    T[:3, :3] *= 2
    T[:3, 3] = [1, 2, 3]
    want = np.eye(4)
    want[:3, 3] = [-1, -2, -3]
    for f in (CO.pose_matrix, pose_matrix):
        assert np.array_equal(f(T), want)
    # 3 x a quarter turn about z: trace 3, w = 1, z = (3 + 3) / 4 = 1.5; normalised by sqrt(3.25): cos = (1 - 2.25) / 3.25
    T = np.eye(4, dtype=F)
    T[:3, :3] = [[0, -3, 0], [3, 0, 0], [0, 0, 3]]
    T[:3, 3] = [1, 0, 0]
    got = pose_matrix(T)
    assert got.tobytes() == CO.pose_matrix(T).tobytes()
    c, s = -1.25 / 3.25, 2 * 1.5 / 3.25
    assert np.allclose(got[:3, :3], [[c, s, 0], [-s, c, 0], [0, 0, 1]], atol=1e-15)      # the transpose of the rotation
    assert np.allclose(got[:3, 3], [-c, s, 0], atol=1e-15)


def test_pose_matrix_bits_over_random_poses():
    from orb_slam2_ssd_semantic_amd import pose_matrix
    import cloud_cases as CC
    rng = np.random.default_rng(5)
    for k in range(200):
        T = CC.pose_tcw(k)
        if k % 4 == 1:                    # trace <= 0: each of the three largest-diagonal branches
            i = (k // 4) % 3
            D = -np.ones(3)
            D[i] = 1
            T[:3, :3] = (np.diag(D) @ T[:3, :3].astype(np.float64)).astype(F)
        if k % 4 == 2:
            T[:3, :3] += rng.normal(scale=1e-3, size=(3, 3)).astype(F)       # a pose that drifted off the rotations
        a, b = pose_matrix(T), CO.pose_matrix(T)
        assert a.tobytes() == b.tobytes(), k
        assert np.allclose(a[:3, :3] @ a[:3, :3].T, np.eye(3), atol=1e-12)


def test_cloud_needs_a_device(have_gpu):
    from orb_slam2_ssd_semantic_amd import PointCloudMap, OrbfeError, _ffi
    L = _ffi.lib()
    h = C.c_void_p()
    assert L.orbfe_cloud_create(-1, 0.0, 100, 1, 8, 8, C.byref(h)) == _ffi.ORBFE_ERR_ARG       # no leaf
    assert L.orbfe_cloud_create(-1, 0.01, 0, 1, 8, 8, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_cloud_size(None) == 0
    assert L.orbfe_cloud_pose_matrix(None, None) == _ffi.ORBFE_ERR_ARG
    if have_gpu:
        return
    try:
        PointCloudMap(0.01, 8, 8, max_points=100)
    except OrbfeError as err:
        assert err.status == _ffi.ORBFE_ERR_NODEVICE
    else:
        raise AssertionError("constructed without a HIP device")
