"""The outlier filter and the 3-D objects on the GPU (csrc/orbfe_objects.hip) against tests/objects_oracle.py, bit for bit:
distances as uint32, threshold / mean / stddev as uint64, masks, counts, centroids, bounds and voxel records as bytes.  The sizes
sit on the kernels' seams (mean_k + 1, a wave of 64, a tile of 256), the adversarial sets on the grid's."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_cases as CC
import cloud_oracle as CO
import objects_cases as OC
import objects_oracle as OO
from orb_slam2_ssd_semantic_amd import ObjectDatabase, PointCloudMap, _ffi, statistical_outlier_removal
from orb_slam2_ssd_semantic_amd import cloud as CL

F = np.float32
BRUTE, GRID = CL.KNN_BRUTE, CL.KNN_GRID
_ORACLE = {}


def oracle(key, pts, mean_k, mul):
    """computed once per case, shared by the modes"""
    if key not in _ORACLE:
        _ORACLE[key] = OO.statistical_outlier_removal(OC.rec(pts), mean_k, mul)
    return _ORACLE[key]


def u64(v):
    return np.array([v], np.float64).view(np.uint64)[0]


def run_filter(m, pts, mean_k, mul, mode, offsets=None):
    dist, keep, stats, plans = m.outlier_filter(OC.rec(pts), offsets, mean_k, mul, mode)
    return dist.cpu().numpy(), keep.cpu().numpy(), stats, plans


def check_filter(key, pts, mean_k, mul, mode, m=None):
    want = oracle(key, pts, mean_k, mul)
    own = m is None
    m = m or PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1)
    try:
        dist, keep, stats, plans = run_filter(m, pts, mean_k, mul, mode)
    finally:
        if own:
            m.close()
    s = stats[0]
    print(key, mode, "status", s["status"], want["status"], "kept", s["n_kept"], int(want["keep"].sum()), "threshold", s["threshold"], want["threshold"])
    assert s["status"] == want["status"] and s["n_in"] == len(pts) and s["n_finite"] == want["n_finite"]
    assert dist.view(np.uint32).tolist() == want["distances"].view(np.uint32).tolist()
    assert (u64(s["threshold"]), u64(s["mean"]), u64(s["stddev"])) == (u64(want["threshold"]), u64(want["mean"]), u64(want["stddev"]))
    assert keep.astype(bool).tolist() == want["keep"].tolist() and s["n_kept"] == int(want["keep"].sum())
    if want["status"] == OO.OK:
        assert plans[0]["used"] == (GRID if mode == GRID else BRUTE)
    return plans[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [BRUTE, GRID])
@pytest.mark.parametrize("n", [50, 51, 64, 65, 256, 257, 1500])
def test_filter_sizes(n, mode):
    check_filter(("size", n), OC.blobs(n, n), 50, 1.0, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [BRUTE, GRID])
@pytest.mark.parametrize("mean_k", [1, 8, 50, 63])
def test_filter_mean_k(mean_k, mode):
    check_filter(("k", mean_k), OC.blobs(700, 20), mean_k, 1.0, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice16", "coincident_plus", "far_point", "sheet", "not_finite", "collinear3"])
def test_filter_adversarial_grid(name):
    pts, k, mul = OC.CASES[name]
    check_filter(("case", name), pts, k, mul, GRID)
    if name == "lattice16":
        check_filter(("case", name, 50), pts, 50, 1.0, GRID)


@pytest.mark.gpu
def test_filter_points_on_cell_borders():
    base = OC.border_base(1)
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        _, _, _, plans = run_filter(m, base, 50, 1.0, GRID)
        p = plans[0]
        assert p["used"] == GRID and p["cells"] > 64 and min(p["dims"]) > 2
        pts = OC.on_borders(base, p["dims"], p["origin"], p["inv_cell"], 1)
        cell = ((pts[:, 0] - p["origin"][0]) * p["inv_cell"]).astype(F)
        assert (np.abs(cell - np.round(cell)) < 1e-5).sum() > 100            # they do sit on the borders
        q = check_filter(("border", 1), pts, 50, 1.0, GRID, m)
        assert q.tobytes() == p.tobytes()                                     # the same bounds and count: the same grid


@pytest.mark.gpu
def test_grid_equals_brute_force_at_20000():
    pts = OC.blobs(20000, 77, outliers=0.02)
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        a = run_filter(m, pts, 50, 1.0, BRUTE)
        b = run_filter(m, pts, 50, 1.0, GRID)
        c = run_filter(m, pts, 50, 1.0, CL.KNN_AUTO)
    assert a[3][0]["used"] == BRUTE and b[3][0]["used"] == GRID and c[3][0]["used"] == GRID
    assert 0 < a[2][0]["n_kept"] < 20000
    for x in (b, c):
        assert a[0].tobytes() == x[0].tobytes() and a[1].tobytes() == x[1].tobytes() and a[2].tobytes() == x[2].tobytes()


@pytest.mark.gpu
def test_filter_several_sets_in_one_call():
    sets = [OC.blobs(300, 31), OC.blobs(40, 32), np.zeros((0, 3), F), OC.CASES["not_finite"][0]]
    off = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        dist, keep, stats, _ = run_filter(m, np.concatenate(sets), 50, 1.0, CL.KNN_AUTO, off)
    assert stats["status"].tolist() == [OO.OK, OO.TOO_FEW, OO.EMPTY, OO.OK]
    for o, s in enumerate(sets):
        want = OO.statistical_outlier_removal(OC.rec(s), 50, 1.0)
        assert dist[off[o]:off[o + 1]].view(np.uint32).tolist() == want["distances"].view(np.uint32).tolist()
        assert keep[off[o]:off[o + 1]].astype(bool).tolist() == want["keep"].tolist()
        assert u64(stats[o]["threshold"]) == u64(want["threshold"])


@pytest.mark.gpu
def test_statistical_outlier_removal_function():
    pts = OC.blobs(300, 31)
    keep, dist, st = statistical_outlier_removal(pts)
    want = OO.statistical_outlier_removal(OC.rec(pts))
    assert keep.tolist() == want["keep"].tolist() and dist.tobytes() == want["distances"].tobytes() and st["status"] == OO.OK


@pytest.mark.gpu
def test_filter_argument_errors():
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        off = np.array([0, 0], np.int32)
        st = np.zeros(1, CL.FILTER_DTYPE)
        for k, mode in ((0, 0), (64, 0), (50, 3), (50, -1)):
            assert m._L.orbfe_cloud_outlier_filter_device(m.h, None, _ffi.ptr(off), 1, k, 1.0, mode, None, None, _ffi.ptr(st), None,
                                                          None) == _ffi.ORBFE_ERR_ARG
        assert m.objects_scratch_bytes() == 0                                 # decided before anything was allocated


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def oracle_chain(frames):
    """paint, objects and database of the oracle over the keyframes -> (per-frame object lists, the database)"""
    boxes, colors, probs, classes = OC.e2e_boxes()
    sel = np.nonzero(probs.astype(np.float64) > OO.PROB_GATE)[0]
    db, out = OO.ObjectDatabase(), []
    for d, bgr, K, T in frames:
        img = bgr.copy()
        idx = CO.paint_boxes(d, img, boxes[sel], colors[sel])
        objs = OO.frame_objects(d, img, K, T, idx, 0.05)
        for o, k in zip(objs, sel):
            if o["status"] == OO.OK:
                db.merge(classes[k], probs[k], o["centroid"], o["min"], o["max"])
        out.append((objs, idx))
    return out, db, sel


def same_object(got, want):
    assert (got["status"], got["n_in"], got["n_kept"], got["n_voxels"]) == (want["status"], want["n_in"], want["n_kept"], want["n_voxels"])
    for name in ("centroid", "min", "max"):
        assert got[name].tobytes() == np.asarray(want[name], F).tobytes(), name
    for name in ("threshold", "mean", "stddev"):
        assert u64(got[name]) == u64(want[name]), name


@pytest.mark.gpu
def test_end_to_end_two_keyframes():
    frames = [OC.e2e_frame(3), OC.e2e_frame(3, shift=0.05)]
    want, wdb, wsel = oracle_chain(frames)
    assert [o["status"] for o in want[0][0]] == [OO.OK, OO.TOO_FEW, OO.OK]
    assert want[0][0][2]["n_voxels"] == 1 and not want[0][0][2]["distances"].any()      # the zero-depth patch: one place
    assert 0 < want[0][0][0]["n_kept"] < want[0][0][0]["n_in"]
    assert len(wdb.clusters) == 2                                                        # the second keyframe's objects merged
    boxes, colors, probs, classes = OC.e2e_boxes()
    db = ObjectDatabase()
    with PointCloudMap(0.05, OC.E2E_W, OC.E2E_H, max_points=16, max_frames=1) as m:
        for (d, bgr, K, T), (wobjs, widx) in zip(frames, want):
            objs, sel, painted = m.objects(d, bgr, T, K, boxes, colors, probs, classes, db=db)
            assert sel.tolist() == wsel.tolist() and len(objs) == 3
            for g, w in zip(objs, wobjs):
                same_object(g, w)
            # the same objects with their kept indices and voxels, every search mode
            _, idx = m.paint_boxes(d, bgr, boxes[sel], colors[sel])
            for mode in (CL.KNN_AUTO, BRUTE, GRID):
                o2, kept, vox = m.build_objects(d, painted, T, K, idx, mode=mode, want_kept=True, want_voxels=True)
                assert o2.tobytes() == objs.tobytes()
                for b, w in enumerate(wobjs):
                    assert kept[b].tolist() == np.asarray(widx[b])[w["keep"]].tolist()
                    assert vox[b].tobytes() == (w["voxels"] if w["status"] == OO.OK else np.zeros(0, CO.REC_DTYPE)).tobytes()
    assert db.records().tobytes() == wdb.records().tobytes()


def device_call(m, d, c, dstride, cstride, K, T, idx, counts, kept_cap, vox_cap, kept, vox):
    objs = np.zeros(len(counts), CL.OBJECT_DTYPE)
    nk, nv = C.c_int32(), C.c_int32()
    st = m._L.orbfe_cloud_objects_device(m.h, _ffi.tensor_ptr(d), dstride, _ffi.tensor_ptr(c), cstride, _ffi.ptr(K), _ffi.ptr(T), _ffi.tensor_ptr(idx),
                                         _ffi.ptr(counts), len(counts), 50, 1.0, 0, _ffi.ptr(objs), _ffi.tensor_ptr(kept), kept_cap,
                                         _ffi.tensor_ptr(vox), vox_cap, C.byref(nk), C.byref(nv), None)
    return st, objs, nk.value, nv.value


@pytest.mark.gpu
def test_capacities_and_pitched_planes():
    d, bgr, K, T = OC.e2e_frame(4)
    (wobjs, widx), = oracle_chain([(d, bgr, K, T)])[0]
    w, h = OC.E2E_W, OC.E2E_H
    img = bgr.copy()
    CO.paint_boxes(d, img, OC.E2E_BOXES, OC.E2E_COLORS)
    counts = np.array([len(ix) for ix in widx], np.int32)
    idx = torch.from_numpy(np.concatenate(widx).astype(np.int32)).cuda()
    need_k = sum(o["n_kept"] for o in wobjs)
    need_v = sum(o["n_voxels"] for o in wobjs if o["status"] == OO.OK)
    dp, cp = 80, 200   # floats / bytes per row
    dd = torch.full((h + 1, dp), float("nan"), dtype=torch.float32, device="cuda")
    cc = torch.zeros((h + 2, cp), dtype=torch.uint8, device="cuda")
    dd[:h, :w] = torch.from_numpy(d).cuda()
    cc[:h, :3 * w] = torch.from_numpy(img.reshape(h, 3 * w)).cuda()
    K, T = np.ascontiguousarray(K, F), np.ascontiguousarray(T, np.float64)
    with PointCloudMap(0.05, w, h, max_points=16, max_frames=1) as m:
        kept = torch.zeros(need_k, dtype=torch.int32, device="cuda")
        vox = torch.zeros((need_v, 4), dtype=torch.int32, device="cuda")
        for kc, vc in ((need_k - 1, need_v), (need_k, need_v - 1)):            # one short: the need, nothing written
            st, objs, nk, nv = device_call(m, dd, cc, dp * 4, cp, K, T, idx, counts, kc, vc, kept, vox)
            assert st == _ffi.ORBFE_ERR_CAP and (nk, nv) == (need_k, need_v)
            assert not kept.any() and not vox.any() and not objs.tobytes().strip(b"\0")
        st, objs, nk, nv = device_call(m, dd, cc, dp * 4, cp, K, T, idx, counts, need_k, need_v, kept, vox)
        assert st == _ffi.ORBFE_OK and (nk, nv) == (need_k, need_v)
        for g, wo in zip(objs, wobjs):
            same_object(g, wo)
        assert kept.cpu().numpy().tolist() == np.concatenate([np.asarray(ix)[o["keep"]] for ix, o in zip(widx, wobjs)]).tolist()
        assert CL.to_records(vox).tobytes() == np.concatenate([o["voxels"] for o in wobjs if o["status"] == OO.OK]).tobytes()


@pytest.mark.gpu
def test_host_convenience_and_scratch_on_first_use():
    d, bgr, K, T = OC.e2e_frame(5)
    (wobjs, _), = oracle_chain([(d, bgr, K, T)])[0]
    want_img = bgr.copy()
    CO.paint_boxes(d, want_img, OC.E2E_BOXES, OC.E2E_COLORS)
    with PointCloudMap(0.05, OC.E2E_W, OC.E2E_H, max_points=OC.E2E_W * OC.E2E_H, max_frames=1) as m:
        m.insert(d, bgr, T, K, boxes=OC.E2E_BOXES, colors=OC.E2E_COLORS)
        m.voxel_filter()
        assert m.objects_scratch_bytes() == 0                                 # a handle that only maps holds nothing of the objects
        objs = np.zeros(3, CL.OBJECT_DTYPE)
        img = bgr.copy()
        dc, Kc, Tc = np.ascontiguousarray(d, F), np.ascontiguousarray(K, F), np.ascontiguousarray(T, np.float64)
        _ffi.check(m._L.orbfe_cloud_objects(m.h, _ffi.ptr(dc), _ffi.ptr(img), _ffi.ptr(Kc), _ffi.ptr(Tc), _ffi.ptr(OC.E2E_BOXES), _ffi.ptr(OC.E2E_COLORS), 3,
                                            50, 1.0, 0, _ffi.ptr(objs)), "orbfe_cloud_objects")
        assert m.objects_scratch_bytes() > 0
        assert img.tobytes() == want_img.tobytes()
        for g, w in zip(objs, wobjs):
            same_object(g, w)
