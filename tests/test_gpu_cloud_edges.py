"""The dense point-cloud map on the GPU (csrc/orbfe_cloud.hip, csrc/orbfe_cloud_dev.h) at the size of the real workload, against
tests/cloud_oracle.py, bit for bit: records as bytes (positions as their uint32 bits), counts and index lists.  The cases
(tests/cloud_edge_cases.py; tests/test_cloud_objects_edge_cases.py shows on the CPU that each reaches its seam) sit past entry 1024
of k_cloud_scan -- item 262 144 of k_cloud_generate, k_cloud_heads and the per-keyframe counts --, on the second grid-stride trip of
k_cloud_minmax, on the overflow branch of the insert and on the chunk loop of the paint."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_cases as CC
import cloud_edge_cases as CE
import cloud_oracle as CO
from orb_slam2_ssd_semantic_amd import OrbfeError, PointCloudMap, _ffi
from orb_slam2_ssd_semantic_amd import cloud as CL

F = np.float32


def same(got, want):
    """records equal as bytes (no NaN can be in either: both sides drop them)"""
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def stack(frames):
    return (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), [f[3] for f in frames], [f[2] for f in frames])


def check_generate(frames, w, h, one_short=False):
    want = [CO.generate_point_cloud(*f) for f in frames]
    total = sum(len(x) for x in want)
    with PointCloudMap(0.05, w, h, max_points=16, max_frames=len(frames)) as m:
        cloud, counts = m.generate(*stack(frames))
        print("generate", w, h, len(frames), "counts", counts.tolist(), [len(x) for x in want])
        assert counts.tolist() == [len(x) for x in want] and cloud.shape[0] == total
        assert same(CL.to_records(cloud), np.concatenate(want))
        if one_short:                                            # the need is reported and nothing is written
            out = torch.zeros((total, 4), dtype=torch.int32, device="cuda")
            dd, cc, nb, Ka, Ta = m._frames(*stack(frames))
            n = C.c_int32()
            st = m._L.orbfe_cloud_generate_device(m.h, *m._plane_args(dd, cc), nb, _ffi.ptr(Ka), _ffi.ptr(Ta), _ffi.tensor_ptr(out), total - 1, None,
                                                  C.byref(n), None)
            assert st == _ffi.ORBFE_ERR_CAP and n.value == total and not out.any()


# ---- A1, A2: generate --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixed", "rows"])
def test_generate_one_frame_of_1026_workgroups(kind):
    check_generate([CE.big_frame(kind)], CE.BIG_W, CE.BIG_H, one_short=True)


@pytest.mark.gpu
def test_generate_third_keyframe_straddles_entry_1024():
    w, h, B = CE.STRADDLE
    check_generate(CE.batch(w, h, B, 400), w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("total", sorted(CE.BATCH_TOTALS))
def test_generate_batch_of_total_entries(total):
    w, h, B = CE.BATCH_TOTALS[total]
    check_generate(CE.batch(w, h, B, 500 + total), w, h)


# ---- A3, A4: voxel filter ----------------------------------------------------------------------------------------------------------
def check_voxels(pts, leaf):
    want, wovf = CO.voxel_grid(pts, leaf)
    with PointCloudMap(leaf, 1, 1, max_points=len(pts), max_frames=1) as m:
        got, ovf = m.voxel_filter(pts)
    got = CL.to_records(got)
    print("voxels", len(pts), leaf, "->", len(got), len(want), "overflow", ovf, wovf)
    assert ovf == wovf and len(got) == len(want)
    assert same(got, want)
    return got


@pytest.fixture(scope="module")
def voxel_clouds():
    return {nf: CE.voxel_cloud(nf) for nf in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("not_finite", [False, True])
@pytest.mark.parametrize("leaf,voxels", [(0.05, 8001), (0.25, 65)])
def test_voxel_heads_scan_of_1025_entries(voxel_clouds, leaf, voxels, not_finite):
    assert len(check_voxels(voxel_clouds[not_finite], leaf)) == voxels


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
def test_voxel_bounds_from_the_second_trip(mirror):
    pts = CE.second_trip_cloud(mirror)
    out = check_voxels(pts, 0.25)
    assert len(out) > 4 ** 3                                     # [0.1, 0.9]^3 is 4^3 voxels: those of the extremes are there too


# ---- A5: insert at real size -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_insert_twice_at_real_size():
    om = CO.Map(CE.INSERT_LEAF)
    inserts = CE.big_inserts()
    states = []
    for frames in inserts:
        counts = om.insert(frames)
        states.append((counts, om.pts.copy()))
    need = len(states[0][1]) + states[1][0][0]                   # the map after insert 1 plus the new points of insert 2
    assert len(states[0][1]) < CE.SEAM < need
    with PointCloudMap(CE.INSERT_LEAF, CE.BIG_W, CE.BIG_H, max_points=need, max_frames=1) as m:
        for frames, (counts, want) in zip(inserts, states):
            assert m.insert(*stack(frames)) == len(want) == len(m)
            assert m.last_counts.tolist() == counts and not m.overflow
            assert same(m.records(), want)


# ---- B: insert overflow ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_insert_overflow_leaves_the_appended_map():
    om = CO.Map(CE.OVERFLOW_LEAF)
    inserts = CE.overflow_inserts()
    third = len(CO.generate_point_cloud(*inserts[2][0]))
    with PointCloudMap(CE.OVERFLOW_LEAF, 37, 23, max_points=3 * 37 * 23, max_frames=1) as m:
        for frames in inserts[:2]:
            counts = om.insert(frames)
            assert om.overflow
            assert m.insert(*stack(frames)) == len(om.pts) == len(m)             # the size is the appended count
            assert m.overflow and m.last_counts.tolist() == counts
            assert same(m.records(), om.pts)                                     # the unfiltered append
    need = len(om.pts) + third
    with PointCloudMap(CE.OVERFLOW_LEAF, 37, 23, max_points=need - 1, max_frames=1) as m:
        for frames in inserts[:2]:
            m.insert(*stack(frames))
        with pytest.raises(OrbfeError) as e:
            m.insert(*stack(inserts[2]))
        assert e.value.status == _ffi.ORBFE_ERR_CAP and str(need) in str(e.value)
        assert len(m) == len(om.pts) and same(m.records(), om.pts)               # the map is as it was


# ---- C: paint ----------------------------------------------------------------------------------------------------------------------
def paint_call(m, depth, bgr, boxes, colors, idx_cap):
    """the device call as it is -> (status, painted plane, index buffer, counts, n_out)"""
    dep = torch.from_numpy(depth).cuda()
    img = torch.from_numpy(bgr).cuda()
    idx = torch.full((max(idx_cap, 1) + 8,), -7, dtype=torch.int32, device="cuda")
    counts = np.full(len(boxes), -7, np.int32)
    n = C.c_int32(-7)
    bx, col = np.array(boxes, F), np.array(colors, np.uint8)
    w = depth.shape[1]
    st = m._L.orbfe_cloud_paint_boxes_device(m.h, _ffi.tensor_ptr(dep), w * 4, _ffi.tensor_ptr(img), w * 3, _ffi.ptr(bx), _ffi.ptr(col), len(boxes),
                                             _ffi.tensor_ptr(idx), idx_cap, _ffi.ptr(counts), C.byref(n), None)
    return st, img.cpu().numpy(), idx.cpu().numpy(), counts, n.value


def check_paint(depth, bgr, boxes, colors):
    """at idx_cap = the need exactly: image, index list, counts and total against the oracle; one less: ORBFE_ERR_CAP, nothing done"""
    want_img = bgr.copy()
    want_idx = CO.paint_boxes(depth, want_img, boxes, colors)
    need = CE.paint_need(boxes)
    flat = np.concatenate(want_idx) if want_idx else np.zeros(0, np.int32)
    with PointCloudMap(0.05, depth.shape[1], depth.shape[0], max_points=16, max_frames=1) as m:
        st, img, idx, counts, n = paint_call(m, depth, bgr, boxes, colors, need)
        print("paint", boxes, "counts", counts.tolist(), [len(x) for x in want_idx], "need", need)
        assert st == _ffi.ORBFE_OK and counts.tolist() == [len(x) for x in want_idx] and n == len(flat)
        assert idx[:n].tolist() == flat.tolist() and (idx[n:] == -7).all()       # every box's indices behind the previous box's
        assert np.array_equal(img, want_img)
        if need > 0:
            st, img, idx, counts, n = paint_call(m, depth, bgr, boxes, colors, need - 1)
            assert st == _ffi.ORBFE_ERR_CAP and n == need
            assert np.array_equal(img, bgr) and (idx == -7).all() and counts.tolist() == [-7] * len(boxes)
    return want_idx


@pytest.mark.gpu
@pytest.mark.parametrize("box", sorted(CE.CHUNK_BOXES))
def test_paint_exact_chunk_counts(box):
    d, bgr = CE.constant_plane()
    idx = check_paint(d, bgr, [box], [(255, 0, 128)])
    assert len(idx[0]) == CE.CHUNK_BOXES[box] == CE.paint_need([box])            # every candidate recorded: the buffer is full


@pytest.mark.gpu
@pytest.mark.parametrize("box", CE.NOTHING_BOXES)
def test_paint_box_that_produces_nothing(box):
    d, bgr = CC.paint_frame(CE.PAINT_W, CE.PAINT_H, 7)
    idx = check_paint(d, bgr, [CE.ORDINARY_BOXES[0], box, CE.ORDINARY_BOXES[1]], [(1, 2, 3), (4, 5, 6), (7, 8, 9)])
    assert len(idx[0]) > 0 and len(idx[1]) == 0 and len(idx[2]) > 0
    check_paint(d, bgr, [box], [(4, 5, 6)])                                      # alone: nothing at all, idx_cap 0


@pytest.mark.gpu
def test_paint_box_over_the_right_edge():
    d, bgr = CC.paint_frame(CE.PAINT_W, CE.PAINT_H, CE.EDGE_SEED)
    idx = check_paint(d, bgr, [CE.EDGE_BOX], [(9, 8, 7)])[0]
    assert len(idx) == 97 and {0, 1, 2} <= set((idx % CE.PAINT_W).tolist())
    with PointCloudMap(0.05, CE.PAINT_W, CE.PAINT_H, max_points=16, max_frames=1) as m:       # and through the class
        img, got = m.paint_boxes(d, bgr, [CE.EDGE_BOX], [(9, 8, 7)])
        want_img = bgr.copy()
        CO.paint_boxes(d, want_img, [CE.EDGE_BOX], [(9, 8, 7)])
        assert got[0].tolist() == idx.tolist() and np.array_equal(img.cpu().numpy(), want_img)
