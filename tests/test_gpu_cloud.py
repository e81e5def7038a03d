"""The dense point-cloud map on the GPU (csrc/orbfe_cloud.hip) against tests/cloud_oracle.py, bit for bit: positions as uint32
views, colours, counts, order and the per-box index lists.  The shapes sit on the kernels' seams (a wave of 64, a workgroup of
256, the last partial workgroup), not on the workload's size."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_cases as CC
import cloud_oracle as CO
from orb_slam2_ssd_semantic_amd import OrbfeError, PointCloudMap, _ffi
from orb_slam2_ssd_semantic_amd import cloud as CL

F = np.float32


def same(got, want):
    """records equal as bytes (no NaN can be in either: both sides drop them)"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def stack(frames):
    return (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), [f[3] for f in frames], [f[2] for f in frames])


# ---- generate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(37, 23), (64, 8)])
@pytest.mark.parametrize("B", [1, 3])
def test_generate(w, h, B):
    frames = [CC.frame(w, h, 10 * B + b) for b in range(B)]
    want = [CO.generate_point_cloud(*f) for f in frames]
    assert all(0 < len(x) < w * h for x in want)
    with PointCloudMap(0.05, w, h, max_points=16, max_frames=3) as m:
        cloud, counts = m.generate(*stack(frames))
        assert counts.tolist() == [len(x) for x in want]
        assert same(CL.to_records(cloud), np.concatenate(want))
        # one record short: the need is reported and nothing is written
        total = sum(len(x) for x in want)
        out = torch.zeros((total, 4), dtype=torch.int32, device="cuda")
        d, c, T, K = stack(frames)
        dd, cc, nb, Ka, Ta = m._frames(d, c, T, K)
        n = C.c_int32()
        st = m._L.orbfe_cloud_generate_device(m.h, *m._plane_args(dd, cc), nb, _ffi.ptr(Ka), _ffi.ptr(Ta), _ffi.tensor_ptr(out), total - 1, None,
                                              C.byref(n), None)
        assert st == _ffi.ORBFE_ERR_CAP and n.value == total and not out.any()


@pytest.mark.gpu
def test_generate_all_invalid_and_all_valid_frames():
    w, h = 37, 23
    frames = [CC.frame(w, h, 1, "invalid"), CC.frame(w, h, 2, "clean"), CC.frame(w, h, 3, "invalid")]
    want = [CO.generate_point_cloud(*f) for f in frames]
    assert [len(x) for x in want] == [0, w * h, 0]
    with PointCloudMap(0.05, w, h, max_points=16, max_frames=3) as m:
        cloud, counts = m.generate(*stack(frames))
        assert counts.tolist() == [0, w * h, 0] and same(CL.to_records(cloud), want[1])
        cloud, counts = m.generate(*stack(frames[:1]))
        assert counts.tolist() == [0] and cloud.shape[0] == 0


@pytest.mark.gpu
def test_generate_pitched_planes():
    """rows and frames further apart than they are long"""
    w, h, B = 37, 23, 2
    frames = [CC.frame(w, h, 40 + b) for b in range(B)]
    want = np.concatenate([CO.generate_point_cloud(*f) for f in frames])
    dp, cp = 48, 120   # floats / bytes per row
    d = torch.full((B, h + 1, dp), float("nan"), dtype=torch.float32, device="cuda")
    c = torch.zeros((B, h + 2, cp), dtype=torch.uint8, device="cuda")
    for b, f in enumerate(frames):
        d[b, :h, :w] = torch.from_numpy(f[0]).cuda()
        c[b, :h, :3 * w] = torch.from_numpy(f[1].reshape(h, 3 * w)).cuda()
    K = np.stack([f[2] for f in frames])
    T = np.stack([f[3] for f in frames])
    with PointCloudMap(0.05, w, h, max_points=16, max_frames=B) as m:
        out = torch.zeros((B * w * h, 4), dtype=torch.int32, device="cuda")
        n = C.c_int32()
        counts = np.zeros(B, np.int32)
        _ffi.check(m._L.orbfe_cloud_generate_device(m.h, _ffi.tensor_ptr(d), dp * 4, (h + 1) * dp * 4, _ffi.tensor_ptr(c), cp, (h + 2) * cp, B,
                                                    _ffi.ptr(K), _ffi.ptr(T), _ffi.tensor_ptr(out), B * w * h, _ffi.ptr(counts), C.byref(n), None), "generate")
        assert n.value == len(want) and same(CL.to_records(out[:n.value]), want)


# ---- voxel filter --------------------------------------------------------------------------------------------------------------
def check_voxels(pts, leaf, cap=None):
    want, wovf = CO.voxel_grid(pts, leaf)
    with PointCloudMap(leaf, 1, 1, max_points=max(len(pts), 1), max_frames=1) as m:
        got, ovf = m.voxel_filter(pts, cap=cap)
    got = CL.to_records(got)
    assert ovf == wovf and len(got) == len(want)
    assert same(got, want)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_voxel_random_cube(n):
    out = check_voxels(CC.random_cloud(n, n), 0.05)
    assert len(out) <= n and (n < 5000 or len(out) < n)


@pytest.mark.gpu
def test_voxel_many_points_in_one_voxel():
    out = check_voxels(CC.one_voxel_cloud(300, 1), 0.05)       # the voxel's points span two workgroups of the sort and the heads
    assert len(out) == 2


@pytest.mark.gpu
def test_voxel_colour_sums_past_2_24():
    pts = CC.one_voxel_cloud(70000, 2, white=True)               # 255 * 70000 > 2^24: the float colour sums depend on the order
    out = check_voxels(pts, 0.05)
    assert len(out) == 2
    rev = CO.centroid(pts[1:][::-1])
    assert (float(out["x"][1]), float(out["y"][1]), float(out["z"][1])) != tuple(float(v) for v in rev[:3])   # the test can tell the orders apart


@pytest.mark.gpu
def test_voxel_negative_coordinates_and_not_finite_points():
    pts = CC.random_cloud(700, 7, -0.6, 0.4)
    check_voxels(pts, 0.05)
    pts["x"][[0, 64, 699]] = np.nan
    pts["z"][[5, 255]] = np.inf
    out = check_voxels(pts, 0.05)
    assert len(out) > 0


@pytest.mark.gpu
def test_voxel_empty_overflow_and_cap():
    assert len(check_voxels(np.zeros(0, CO.REC_DTYPE), 0.05)) == 0
    assert len(check_voxels(CO.records([[np.nan, 0, 0]], [1]), 0.05)) == 0
    far = CO.records([[0, 0, 0], [1e6, 1e6, 0], [0.001, 0, 0]], [1, 2, 3])
    assert len(check_voxels(far, 0.01)) == 3                     # more than INT_MAX cells: the flag, and the input copied through
    assert len(check_voxels(CO.records([[0, 0, 0], [1e6, 0, 0]], [1, 2]), 0.01)) == 2      # 1e8 + 1 cells in a line: filtered
    pts = CC.random_cloud(257, 257)
    need = len(CO.voxel_grid(pts, 0.05)[0])
    with PointCloudMap(0.05, 1, 1, max_points=257, max_frames=1) as m:
        with pytest.raises(OrbfeError) as e:
            m.voxel_filter(pts, cap=need - 1)
        assert e.value.status == _ffi.ORBFE_ERR_CAP
        with pytest.raises(OrbfeError) as e:
            m.voxel_filter(far, cap=2)                           # the copy-through needs room for the input
        assert e.value.status == _ffi.ORBFE_ERR_CAP


@pytest.mark.gpu
def test_voxel_filtering_twice():
    pts = CC.random_cloud(5000, 9)
    once = check_voxels(pts, 0.05)
    twice = check_voxels(once, 0.05)
    assert len(twice) == len(once)


# ---- paint ---------------------------------------------------------------------------------------------------------------------
def check_paint(depth, bgr, boxes, colors):
    want_img = bgr.copy()
    want_idx = CO.paint_boxes(depth, want_img, boxes, colors)
    with PointCloudMap(0.05, depth.shape[1], depth.shape[0], max_points=16, max_frames=1) as m:
        img, idx = m.paint_boxes(depth, bgr, boxes, colors)
    assert len(idx) == len(want_idx)
    for g, w_ in zip(idx, want_idx):
        assert g.dtype == np.int32 and g.tolist() == w_.tolist()
    assert np.array_equal(img.cpu().numpy(), want_img)
    return want_idx


@pytest.mark.gpu
def test_paint_one_box_inside():
    depth, bgr = CC.paint_frame(64, 48, 1)
    idx = check_paint(depth, bgr, [(14.7, 10.2, 36.9, 29.5)], [(255, 0, 128)])
    assert 100 < len(idx[0]) < 35 * 28


@pytest.mark.gpu
def test_paint_overlapping_boxes_in_list_order():
    depth, bgr = CC.paint_frame(64, 48, 2)
    boxes = [(10, 8, 30, 30), (20, 12, 40, 30), (10, 8, 30, 30)]
    idx = check_paint(depth, bgr, boxes, [(1, 2, 3), (4, 5, 6), (7, 8, 9)])
    assert len(set(idx[0].tolist()) & set(idx[1].tolist())) > 50 and idx[0].tolist() == idx[2].tolist()


@pytest.mark.gpu
def test_paint_no_depth_in_range():
    depth, bgr = CC.paint_frame(64, 48, 3)
    depth[12:36, 16:48] = np.where(np.arange(24 * 32).reshape(24, 32) % 3 == 0, F(0.3), F(7.0))   # the mean stays 0
    idx = check_paint(depth, bgr, [(10, 8, 44, 32)], [(200, 100, 50)])
    assert len(idx[0]) > 200          # |0.3 - 0| < 0.4 and the zero-depth pixels


@pytest.mark.gpu
def test_paint_mean_row_longer_than_one_staging_pass():
    rng = np.random.default_rng(11)
    depth = rng.uniform(0.3, 7.0, (6, 2700)).astype(F)       # the mean window is 1076 pixels wide, staged 1024 at a time
    bgr = rng.integers(0, 256, (6, 2700, 3), dtype=np.uint8)
    idx = check_paint(depth, bgr, [(1, 1, 2690, 5)], [(3, 2, 1)])
    assert len(idx[0]) > 100


@pytest.mark.gpu
def test_paint_whole_plane_and_edges():
    """a box that spans the plane, and the 0.5 / 6 / 0.4 edges of the hand-worked CPU cases"""
    depth, bgr = CC.paint_frame(64, 48, 4)
    check_paint(depth, bgr, [(1, 2, 64, 46)], [(9, 9, 9)])
    d = np.full((12, 16), 2.0, F)
    flat = d.reshape(-1)
    flat[35:39] = [F(2.4), np.nextafter(F(2.4), F(0)), F(1.6), np.nextafter(F(1.6), F(0))]
    idx = check_paint(d, np.zeros((12, 16, 3), np.uint8), [(4, 3, 10, 10)], [(9, 8, 7)])[0].tolist()      # the mean is 2.0
    assert 36 in idx and 37 in idx and 35 not in idx and 38 not in idx
    flat[35 + 3 * 16 + 3], flat[35 + 3 * 16 + 4] = 0.5, 6.0                                                # both enter the mean
    check_paint(d, np.zeros((12, 16, 3), np.uint8), [(4, 3, 10, 10)], [(9, 8, 7)])


@pytest.mark.gpu
def test_paint_box_outside_the_image():
    depth, bgr = CC.paint_frame(64, 48, 5)
    dep = torch.from_numpy(depth).cuda()
    with PointCloudMap(0.05, 64, 48, max_points=16, max_frames=1) as m:
        for bad in ((10, 0, 20, 20), (10, 31, 20, 20), (np.nan, 3, 5, 5), (10, 8, 70, 20)):
            img = torch.from_numpy(bgr).cuda()
            idx = torch.full((4096,), -7, dtype=torch.int32, device="cuda")
            counts = np.full(2, -7, np.int32)
            n = C.c_int32(-7)
            bx = np.array([(12, 10, 20, 20), bad], F)      # the good box before it is not painted either
            col = np.array([(1, 2, 3), (4, 5, 6)], np.uint8)
            st = m._L.orbfe_cloud_paint_boxes_device(m.h, _ffi.tensor_ptr(dep), 64 * 4, _ffi.tensor_ptr(img), 64 * 3,
                                                     _ffi.ptr(bx), _ffi.ptr(col), 2, _ffi.tensor_ptr(idx), 4096, _ffi.ptr(counts), C.byref(n), None)
            assert st == _ffi.ORBFE_ERR_ARG, bad
            assert np.array_equal(img.cpu().numpy(), bgr) and bool((idx == -7).all()) and counts.tolist() == [-7, -7]
        with pytest.raises(OrbfeError) as e:
            m.paint_boxes(depth, bgr, [(10, 0, 20, 20)], [(1, 2, 3)])
        assert e.value.status == _ffi.ORBFE_ERR_ARG


# ---- insert --------------------------------------------------------------------------------------------------------------------
def three_inserts():
    return [[CC.frame(37, 23, 100 + 2 * k + b) for b in range(2)] for k in range(3)]


@pytest.fixture(scope="module")
def running_map():
    """the oracle's map after each of the three inserts"""
    om = CO.Map(0.05)
    states = []
    for frames in three_inserts():
        counts = om.insert(frames)
        states.append((counts, om.pts.copy()))
    return states


@pytest.mark.gpu
def test_insert_three_times(running_map):
    most = max(len(s[1]) for s in running_map) + 2 * 37 * 23
    n = C.c_int32()
    ovf = C.c_int32()
    L = _ffi.lib()
    h = C.c_void_p()
    _ffi.check(L.orbfe_cloud_create(0, 0.05, most, 2, 37, 23, C.byref(h)), "create")
    try:
        for frames, (counts, want) in zip(three_inserts(), running_map):
            d = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
            c = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
            K = np.stack([f[2] for f in frames])
            T = np.stack([f[3] for f in frames])
            got_counts = np.zeros(2, np.int32)
            _ffi.check(L.orbfe_cloud_insert_device(h, _ffi.tensor_ptr(d), 37 * 4, 37 * 23 * 4, _ffi.tensor_ptr(c), 37 * 3, 37 * 23 * 3, 2, _ffi.ptr(K),
                                                   _ffi.ptr(T), _ffi.ptr(got_counts), C.byref(n), C.byref(ovf), None), "insert")
            assert got_counts.tolist() == counts and n.value == len(want) == L.orbfe_cloud_size(h) and ovf.value == 0
            got = np.zeros(n.value, CO.REC_DTYPE)
            _ffi.check(L.orbfe_cloud_download(h, _ffi.ptr(got), len(got), C.byref(n)), "download")
            assert same(got, want)
        assert L.orbfe_cloud_download(h, _ffi.ptr(got), len(got) - 1, C.byref(n)) == _ffi.ORBFE_ERR_CAP and n.value == len(got)
    finally:
        L.orbfe_cloud_destroy(h)


@pytest.mark.gpu
def test_insert_capacity_one_short(running_map):
    frames = three_inserts()
    first, second = running_map[0], running_map[1]
    need = len(first[1]) + sum(second[0])           # the map after insert 1 plus the new points of insert 2, before the filter
    assert need > sum(first[0])                      # so it is the second insert that does not fit
    with PointCloudMap(0.05, 37, 23, max_points=need - 1, max_frames=2) as m:
        assert m.insert(*stack(frames[0])) == len(first[1])
        with pytest.raises(OrbfeError) as e:
            m.insert(*stack(frames[1]))
        assert e.value.status == _ffi.ORBFE_ERR_CAP and str(need) in str(e.value)
        assert same(m.records(), first[1])           # the map is as it was
    with PointCloudMap(0.05, 37, 23, max_points=need, max_frames=2) as m:
        m.insert(*stack(frames[0]))
        assert m.insert(*stack(frames[1])) == len(second[1])


@pytest.mark.gpu
def test_point_cloud_map_class(running_map):
    with PointCloudMap(0.05, 37, 23, max_points=1 << 14, max_frames=2) as m:
        for frames, (counts, want) in zip(three_inserts(), running_map):
            assert m.insert(*stack(frames)) == len(want) == len(m)
            assert m.last_counts.tolist() == counts and not m.overflow
            assert same(m.records(), want)
        assert np.array_equal(m.points().view(np.uint32), np.stack([want["x"], want["y"], want["z"]], 1).view(np.uint32))
        rgba = want["rgba"]
        assert np.array_equal(m.colors(), np.stack([(rgba >> 16) & 255, (rgba >> 8) & 255, rgba & 255, rgba >> 24], 1).astype(np.uint8))
        assert m.voxel_filter() == len(want) and same(m.records(), want)        # the map is a fixed point of its own filter
        m.clear()
        assert len(m) == 0 and len(m.records()) == 0


@pytest.mark.gpu
def test_insert_with_a_float_pose_and_boxes():
    """a float32 Tcw goes through pose_matrix; the boxes are painted before the cloud is generated"""
    w, h = 64, 48
    depth, bgr = CC.paint_frame(w, h, 6)
    Tcw = CC.pose_tcw(6)
    K = CC.intrinsics(w, h, 6)
    boxes, colors = [(14, 10, 36, 29)], [(0, 255, 0)]
    img = bgr.copy()
    want_idx = CO.paint_boxes(depth, img, boxes, colors)
    om = CO.Map(0.05)
    om.insert([(depth, img, K, CO.pose_matrix(Tcw))])
    with PointCloudMap(0.05, w, h, max_points=2 * w * h, max_frames=1) as m:
        assert m.insert(depth, bgr, Tcw, K, boxes=boxes, colors=colors) == len(om.pts)
        assert m.last_indices[0].tolist() == want_idx[0].tolist()
        assert same(m.records(), om.pts)


@pytest.mark.gpu
def test_free_functions():
    from orb_slam2_ssd_semantic_amd import generate_point_cloud, paint_boxes, voxel_grid
    f = CC.frame(37, 23, 77)
    assert same(generate_point_cloud(f[0], f[1], f[3], f[2]), CO.generate_point_cloud(*f))
    pts = CC.random_cloud(65, 3)
    got, ovf = voxel_grid(pts, 0.05)
    assert not ovf and same(got, CO.voxel_grid(pts, 0.05)[0])
    depth, bgr = CC.paint_frame(64, 48, 8)
    img = bgr.copy()
    want = CO.paint_boxes(depth, img, [(10, 8, 30, 30)], [(5, 6, 7)])
    got_img, idx = paint_boxes(depth, bgr, [(10, 8, 30, 30)], [(5, 6, 7)])
    assert np.array_equal(got_img, img) and idx[0].tolist() == want[0].tolist()


@pytest.mark.gpu
def test_host_insert_of_one_keyframe():
    f = CC.frame(37, 23, 55)
    om = CO.Map(0.05)
    om.insert([f])
    with PointCloudMap(0.05, 37, 23, max_points=2048, max_frames=1) as m:
        n, ovf = C.c_int32(), C.c_int32()
        _ffi.check(m._L.orbfe_cloud_insert(m.h, _ffi.ptr(np.ascontiguousarray(f[0])), _ffi.ptr(np.ascontiguousarray(f[1])), _ffi.ptr(f[2]),
                                           _ffi.ptr(np.ascontiguousarray(f[3])), C.byref(n), C.byref(ovf)), "orbfe_cloud_insert")
        assert n.value == len(om.pts) and same(m.records(), om.pts)
