"""The outlier filter and the 3-D objects on the GPU (csrc/orbfe_objects.hip) at the edges of the kNN grid's plan and past 1024
workgroups of the compaction, against tests/objects_oracle.py, bit for bit: distances as uint32, threshold / mean / stddev as uint64,
masks, counts, index lists and voxel records as bytes; every returned orbfe_knn_plan against the planner's port in
tests/objects_edge_cases.py.  tests/test_cloud_objects_edge_cases.py shows on the CPU that each case reaches its edge: the axis
limit of knn_plan, extents of exactly 0, mean_k + 1 finite points, the AUTO switch at 2048, stddev_mul other than 1, and item
262 144 of k_obj_compact."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_edge_cases as CE
import cloud_oracle as CO
import objects_cases as OC
import objects_edge_cases as OE
import objects_oracle as OO
from orb_slam2_ssd_semantic_amd import OrbfeError, PointCloudMap, _ffi
from orb_slam2_ssd_semantic_amd import cloud as CL

F = np.float32
AUTO, BRUTE, GRID = CL.KNN_AUTO, CL.KNN_BRUTE, CL.KNN_GRID
_ORACLE = {}


def oracle(key, pts, mean_k, mul=1.0):
    """computed once per case, shared by the modes and the tests"""
    key = (key, mean_k, mul)
    if key not in _ORACLE:
        _ORACLE[key] = OO.statistical_outlier_removal(OC.rec(pts), mean_k, mul)
    return _ORACLE[key]


def u64(v):
    return np.array([v], np.float64).view(np.uint64)[0]


def u32(v):
    return np.asarray(v, F).view(np.uint32).tolist()


def same_plan(p, pts):
    """the returned plan against the port: dims, cells, the finite count, origin and inv_cell as bits"""
    want, nfin = OE.plan_of(pts)
    print("  plan", p["dims"].tolist(), p["cells"], p["n_finite"], "port", want["dims"], want["cells"], nfin, want["brk"])
    assert p["used"] == GRID and p["n_finite"] == nfin
    assert p["dims"].tolist() == want["dims"] and p["cells"] == want["cells"]
    assert u32(p["origin"]) == u32(want["origin"]) and u32(p["inv_cell"]) == u32(want["inv_cell"])
    return want


def same_filter(want, n, dist, keep, s):
    assert s["status"] == want["status"] and s["n_in"] == n and s["n_finite"] == want["n_finite"]
    assert dist.view(np.uint32).tolist() == want["distances"].view(np.uint32).tolist()
    assert (u64(s["threshold"]), u64(s["mean"]), u64(s["stddev"])) == (u64(want["threshold"]), u64(want["mean"]), u64(want["stddev"]))
    assert keep.astype(bool).tolist() == want["keep"].tolist() and s["n_kept"] == int(want["keep"].sum())


def check_filter(key, pts, mean_k, mode, mul=1.0, m=None):
    want = oracle(key, pts, mean_k, mul)
    own = m is None
    m = m or PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1)
    try:
        dist, keep, stats, plans = m.outlier_filter(OC.rec(pts), None, mean_k, mul, mode)
        dist, keep = dist.cpu().numpy(), keep.cpu().numpy()
    finally:
        if own:
            m.close()
    s = stats[0]
    print(key, mean_k, mul, mode, "status", s["status"], want["status"], "kept", s["n_kept"], int(want["keep"].sum()), "threshold", s["threshold"],
          want["threshold"])
    same_filter(want, len(pts), dist, keep, s)
    return plans[0]


# ---- D1 - D3: the planner's axis limit, extents of exactly 0 ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["line", "far_point_4100"])
def test_grid_at_the_axis_limit(name):
    pts, ks = OE.GRID_CASES[name]
    p = check_filter(name, pts, ks[0], GRID)
    want = same_plan(p, pts)
    assert want["brk"] == "maxdim" and p["dims"].tolist() == [808, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("mean_k", [50, 6])
@pytest.mark.parametrize("name", ["flat_sheet", "flat_line"])
def test_grid_with_zero_extents(name, mean_k):
    pts, _ = OE.GRID_CASES[name]
    p = check_filter(name, pts, mean_k, GRID)
    same_plan(p, pts)
    assert sorted(p["dims"].tolist())[0] == 1


# ---- D4, D5: mean_k + 1 finite points, the AUTO switch ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [BRUTE, GRID])
def test_mean_k_63_with_exactly_64_finite_points(mode):
    pts = OE.exactly_64()
    p = check_filter("exactly_64", pts, 63, mode)
    assert p["n_finite"] == 64 and p["used"] == mode
    if mode == GRID:
        same_plan(p, pts)


@pytest.mark.gpu
@pytest.mark.parametrize("nfin,used", [(2048, BRUTE), (2049, GRID)])
def test_auto_switches_behind_2048_finite_points(nfin, used):
    pts = OE.auto_switch(nfin)
    p = check_filter(("auto", nfin), pts, 50, AUTO)
    assert p["used"] == used and p["n_finite"] == nfin and len(pts) == nfin + 3
    if used == GRID:
        same_plan(p, pts)


# ---- D6: several sets, one GRID call ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_grid_scratch_across_sets_of_different_size(order):
    named = list(enumerate(OE.grid_sets()))
    if order == "reversed":
        named = named[::-1]
    sets = [s for _, s in named]
    off = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        dist, keep, stats, plans = m.outlier_filter(OC.rec(np.concatenate(sets)), off, 50, 1.0, GRID)
        dist, keep = dist.cpu().numpy(), keep.cpu().numpy()
    for o, (k, s) in enumerate(named):
        want = oracle(("set", k), s, 50)
        print("set", k, len(s), "status", stats[o]["status"], want["status"], "kept", stats[o]["n_kept"], int(want["keep"].sum()))
        same_filter(want, len(s), dist[off[o]:off[o + 1]], keep[off[o]:off[o + 1]], stats[o])
        if want["status"] == OO.OK:
            same_plan(plans[o], s)
    assert sorted(stats["status"].tolist()) == [OO.OK] * 5 + [OO.EMPTY]


# ---- D7: stddev_mul ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mul,kept", list(zip(OE.STDDEV_MULS, OE.STDDEV_KEPT)))
def test_stddev_mul(mul, kept):
    pts = OE.stddev_points()
    for mode in (BRUTE, GRID):
        check_filter("stddev", pts, 50, mode, mul)
    assert int(oracle("stddev", pts, 50, mul)["keep"].sum()) == kept


@pytest.mark.gpu
def test_stddev_mul_nan_stays_refused():
    with PointCloudMap(0.05, 1, 1, max_points=1, max_frames=1) as m:
        with pytest.raises(OrbfeError) as e:
            m.outlier_filter(OC.rec(OE.stddev_points()), None, 50, float("nan"), AUTO)
        assert e.value.status == _ffi.ORBFE_ERR_ARG
    d, bgr, K, T, lists = OE.stddev_frame()
    with PointCloudMap(0.05, OE.SM_W, OE.SM_H, max_points=16, max_frames=1) as m:
        with pytest.raises(OrbfeError) as e:
            m.build_objects(d, bgr, T, K, lists, 50, float("nan"))
        assert e.value.status == _ffi.ORBFE_ERR_ARG


def same_object(got, want):
    assert (got["status"], got["n_in"], got["n_kept"], got["n_voxels"]) == (want["status"], want["n_in"], want["n_kept"], want["n_voxels"])
    for name in ("centroid", "min", "max"):
        assert got[name].tobytes() == np.asarray(want[name], F).tobytes(), name
    for name in ("threshold", "mean", "stddev"):
        assert u64(got[name]) == u64(want[name]), name


def same_objects(objs, kept, vox, want, lists):
    for b, (g, w) in enumerate(zip(objs, want)):
        print("object", b, "status", g["status"], w["status"], "kept", g["n_kept"], w["n_kept"], "voxels", g["n_voxels"], w["n_voxels"])
        same_object(g, w)
        assert kept[b].tolist() == np.asarray(lists[b])[w["keep"]].tolist()
        assert vox[b].tobytes() == (w["voxels"] if w["status"] == OO.OK else np.zeros(0, CO.REC_DTYPE)).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [AUTO, GRID])
def test_object_whose_filter_keeps_nothing_and_the_one_behind_it(mode):
    d, bgr, K, T, lists = OE.stddev_frame()
    want = OO.frame_objects(d, bgr, K, T, lists, 0.05, 50, OE.SM_MUL)
    assert [w["status"] for w in want] == [OO.EMPTY, OO.TOO_FEW, OO.OK]
    with PointCloudMap(0.05, OE.SM_W, OE.SM_H, max_points=16, max_frames=1) as m:
        objs, kept, vox = m.build_objects(d, bgr, T, K, lists, 50, OE.SM_MUL, mode, want_kept=True, want_voxels=True)
    same_objects(objs, kept, vox, want, lists)
    assert (objs[0]["status"], objs[0]["n_kept"], objs[0]["n_voxels"]) == (CL.OBJECT_EMPTY, 0, 0)
    assert len(kept[2]) == want[2]["n_kept"] > 0 and len(vox[2]) == want[2]["n_voxels"] > 0


# ---- E: compaction past 1024 workgroups, indices outside the plane ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def outside():
    return OE.outside_objects()


@pytest.mark.gpu
def test_objects_compaction_past_1024_workgroups(outside):
    want, lists = outside
    d, bgr, K, T, _ = OE.outside_frame()
    with PointCloudMap(0.05, OE.E_W, OE.E_H, max_points=16, max_frames=1) as m:
        objs, kept, vox = m.build_objects(d, bgr, T, K, lists, want_kept=True, want_voxels=True)
    same_objects(objs, kept, vox, want, lists)
    assert objs["status"].tolist() == [CL.OBJECT_TOO_FEW, CL.OBJECT_OK, CL.OBJECT_TOO_FEW]
    assert sum(len(k) for k in kept[:1]) > CE.SEAM                               # object 1's kept indices lie behind workgroup 1024
    assert kept[2].tolist() == lists[2].tolist() and {-1, OE.E_W * OE.E_H, OE.INT32_MAX} <= set(kept[2].tolist())


@pytest.mark.gpu
def test_objects_capacity_one_short_past_1024_workgroups(outside):
    want, lists = outside
    d, bgr, K, T, _ = OE.outside_frame()
    need_k = sum(w["n_kept"] for w in want)
    need_v = sum(w["n_voxels"] for w in want if w["status"] == OO.OK)
    counts = np.array([len(ix) for ix in lists], np.int32)
    K, T = np.ascontiguousarray(K, F), np.ascontiguousarray(T, np.float64)
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(bgr).cuda()
    idx = torch.from_numpy(np.concatenate(lists).astype(np.int32)).cuda()
    kept = torch.zeros(need_k, dtype=torch.int32, device="cuda")
    vox = torch.zeros((need_v, 4), dtype=torch.int32, device="cuda")

    def call(m, kc, vc):
        objs = np.zeros(len(counts), CL.OBJECT_DTYPE)
        nk, nv = C.c_int32(), C.c_int32()
        st = m._L.orbfe_cloud_objects_device(m.h, _ffi.tensor_ptr(dd), OE.E_W * 4, _ffi.tensor_ptr(cc), OE.E_W * 3, _ffi.ptr(K), _ffi.ptr(T),
                                             _ffi.tensor_ptr(idx), _ffi.ptr(counts), len(counts), 50, 1.0, 0, _ffi.ptr(objs), _ffi.tensor_ptr(kept), kc,
                                             _ffi.tensor_ptr(vox), vc, C.byref(nk), C.byref(nv), None)
        return st, objs, nk.value, nv.value

    with PointCloudMap(0.05, OE.E_W, OE.E_H, max_points=16, max_frames=1) as m:
        for kc, vc in ((need_k - 1, need_v), (need_k, need_v - 1)):              # one short: the need, nothing written
            st, objs, nk, nv = call(m, kc, vc)
            assert st == _ffi.ORBFE_ERR_CAP and (nk, nv) == (need_k, need_v)
            assert not kept.any() and not vox.any() and not objs.tobytes().strip(b"\0")
        st, objs, nk, nv = call(m, need_k, need_v)
        assert st == _ffi.ORBFE_OK and (nk, nv) == (need_k, need_v)
        for g, w in zip(objs, want):
            same_object(g, w)
        assert kept.cpu().numpy().tolist() == np.concatenate([np.asarray(ix)[w["keep"]] for ix, w in zip(lists, want)]).tolist()
        assert CL.to_records(vox).tobytes() == want[1]["voxels"].tobytes()
