"""tests/objects_oracle.py against cases checked by hand, and the host-only cluster database (orbfe_objects_*, sem_merge) against
the oracle, record by record as bytes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cloud_oracle as CO
import objects_cases as OC
import objects_oracle as OO
from orb_slam2_ssd_semantic_amd import ObjectDatabase, _ffi
from orb_slam2_ssd_semantic_amd import cloud as CL

F = np.float32
D = np.float64


# ---- the filter ------------------------------------------------------------------------------------------------------------------
def test_three_collinear_points():
    pts, k, mul = OC.CASES["collinear3"]
    r = OO.statistical_outlier_removal(OC.rec(pts), k, mul)
    assert r["distances"].tolist() == [2.0, 1.5, 2.5]
    assert (r["mean"], r["stddev"], r["threshold"]) == (2.0, 0.5, 2.25)
    assert r["keep"].tolist() == [True, True, False]
    assert OO.statistical_outlier_removal(OC.rec(pts), k, 1.0)["keep"].all()   # 2.5 > 2.5 is false: the comparison is strict


def test_lattice_interior_in_closed_form():
    pts, k, mul = OC.CASES["lattice16"]
    r = OO.statistical_outlier_removal(OC.rec(pts), k, mul)
    OC.vacuity(r)
    ijk = np.round(pts / F(0.25)).astype(int)
    interior = ((ijk > 0) & (ijk < 15)).all(1)
    assert (r["distances"][interior] == F(0.25)).all()             # six neighbours at one step
    corner = (ijk == 0).all(1)
    want = (3 * 0.25 + 3 * np.sqrt(D(F(0.125)))) / 6.0             # three at a step, three at a face diagonal
    assert r["distances"][corner][0] == F(want)
    assert r["keep"][interior].all() and not r["keep"][corner].any()


def test_coincident_points_are_all_kept():
    r = OO.statistical_outlier_removal(OC.rec(OC.coincident(80)), 50, 1.0)
    assert r["status"] == OO.OK and not r["distances"].any() and r["stddev"] == 0 and r["threshold"] == 0 and r["keep"].all()


@pytest.mark.parametrize("name", [n for n in OC.CASES if n != "collinear3"])
def test_cases_are_not_vacuous(name):
    pts, k, mul = OC.CASES[name]
    OC.vacuity(OO.statistical_outlier_removal(OC.rec(pts), k, mul))


def test_too_few_and_empty():
    r = OO.statistical_outlier_removal(OC.rec(OC.blobs(50, 3)), 50, 1.0)
    assert r["status"] == OO.TOO_FEW and r["keep"].all() and not r["distances"].any()
    p = OC.blobs(51, 3)
    p[7] = np.nan                                                  # 51 records, 50 of them finite
    assert OO.statistical_outlier_removal(OC.rec(p), 50, 1.0)["status"] == OO.TOO_FEW
    assert OO.statistical_outlier_removal(OC.rec(np.zeros((0, 3), F)), 50, 1.0)["status"] == OO.EMPTY
    o = OO.build_object(OC.rec(OC.blobs(50, 3)), 0.05)
    assert o["status"] == OO.TOO_FEW and o["n_kept"] == 50 and o["n_voxels"] == 0


@pytest.mark.parametrize("name", ["lattice16", "coincident_plus", "not_finite"])
def test_result_does_not_depend_on_the_order(name):
    """what ties must not break: permute the input, un-permute the result"""
    pts, k, mul = OC.CASES[name]
    a = OO.statistical_outlier_removal(OC.rec(pts), k, mul)
    perm = np.random.default_rng(5).permutation(len(pts))
    b = OO.statistical_outlier_removal(OC.rec(pts[perm]), k, mul)
    inv = np.argsort(perm)
    assert a["distances"].view(np.uint32).tolist() == b["distances"][inv].view(np.uint32).tolist()
    # the serial sums run in another order, so the threshold may move in its last bits; no point sits that close to it
    assert a["keep"].tolist() == b["keep"][inv].tolist()


def test_sqrt_modes_differ():
    pts = OC.blobs(300, 9)
    a, _ = OO.knn_mean_distances(OC.rec(pts), 50, "double")
    b, _ = OO.knn_mean_distances(OC.rec(pts), 50, "float")
    assert (a.view(np.uint32) != b.view(np.uint32)).any()
    assert np.allclose(a, b, rtol=1e-6)


def test_not_finite_points_keep_distance_zero():
    pts, k, mul = OC.CASES["not_finite"]
    r = OO.statistical_outlier_removal(OC.rec(pts), k, mul)
    bad = ~np.isfinite(pts).all(1)
    assert bad.sum() == 4 and r["n_finite"] == len(pts) - 4
    assert not r["distances"][bad].any() and r["keep"][bad].all()


def test_object_of_one_voxel_row():
    o = OO.build_object(OC.rec(OC.CASES["blobs1500"][0]), 0.05)
    assert o["status"] == OO.OK and 1 < o["n_voxels"] < o["n_kept"] < o["n_in"]
    assert (o["min"] <= o["centroid"]).all() and (o["centroid"] <= o["max"]).all()


# ---- sem_merge through the C-ABI -------------------------------------------------------------------------------------------------
def both(obj_size=None):
    return ObjectDatabase(obj_size), OO.ObjectDatabase(obj_size)


def merge_both(dbs, class_id, prob, c, mn, mx):
    got = dbs[0].merge(class_id, prob, c, mn, mx)
    want = dbs[1].merge(class_id, prob, c, mn, mx)
    assert got == want
    assert dbs[0].records().tobytes() == dbs[1].records().tobytes()
    return got


def test_cluster_layout():
    assert CL.CLUSTER_DTYPE == OO.CLUSTER_DTYPE


def test_merge_first_insert_and_other_class():
    dbs = both()
    assert merge_both(dbs, 9, 0.9, [0, 0, 1], [-1, -1, 0], [1, 1, 2]) == 0
    assert merge_both(dbs, 15, 0.8, [0, 0, 1], [-1, -1, 0], [1, 1, 2]) == 1      # the same place, another class
    assert len(dbs[0]) == 2


def test_merge_takes_the_nearest_of_several():
    dbs = both()
    for x in (0.0, 2.0, 4.0):
        merge_both(dbs, 9, 0.9, [x, 0, 0], [x - 1, -1, -1], [x + 1, 1, 1])
    assert merge_both(dbs, 9, 0.7, [2.2, 0, 0], [1, -1, -1], [3, 1, 1]) == 1
    r = dbs[0].records()
    assert len(r) == 3 and r["centroid"][1, 0] == F(F(2.0) + F(2.2)) / F(2) and r["prob"][1] == F(D(F(0.9) + F(0.7)) / 2.0)


def test_merge_is_strict_at_obj_size():
    size = np.full(21, 0.5, F)
    dbs = both(size)
    merge_both(dbs, 3, 0.9, [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert merge_both(dbs, 3, 0.9, [0.5, 0, 0], [0, 0, 0], [0, 0, 0]) == 1       # dist == obj_size: appended
    assert merge_both(dbs, 3, 0.9, [-0.49999997, 0, 0], [0, 0, 0], [0, 0, 0]) == 0


def test_merge_never_reaches_100_metres():
    size = np.full(21, 1000.0, F)
    dbs = both(size)
    merge_both(dbs, 3, 0.9, [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert merge_both(dbs, 3, 0.9, [100, 0, 0], [0, 0, 0], [0, 0, 0]) == 1       # dist < 100 is false
    assert merge_both(dbs, 3, 0.9, [-99.99999, 0, 0], [0, 0, 0], [0, 0, 0]) == 0


def test_merge_shrinks_max():
    dbs = both()
    merge_both(dbs, 9, 0.9, [0, 0, 0], [-1, -1, -1], [1, 1, 1])
    merge_both(dbs, 9, 0.9, [0.1, 0, 0], [-2, -0.5, -1], [0.5, 2, 1])
    r = dbs[0].records()[0]
    assert r["min"].tolist() == [-2, -1, -1] and r["max"].tolist() == [0.5, 1, 1]   # the smaller maximum


def test_merge_default_table():
    dbs = both()
    merge_both(dbs, 5, 0.9, [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert merge_both(dbs, 5, 0.9, [0.07, 0, 0], [0, 0, 0], [0, 0, 0]) == 1      # a bottle: 0.06
    merge_both(dbs, 1, 0.9, [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert merge_both(dbs, 1, 0.9, [0.59, 0, 0], [0, 0, 0], [0, 0, 0]) == 2      # anything else: 0.6


def test_forty_random_merges():
    rng = np.random.default_rng(11)
    dbs = both()
    for _ in range(40):
        c = rng.uniform(-1, 1, 3).astype(F)
        e = rng.uniform(0.05, 0.5, 3).astype(F)
        merge_both(dbs, int(rng.choice([5, 9, 15, 20])), F(rng.uniform(0.55, 1.0)), c, c - e, c + e)
    assert 1 < len(dbs[0]) < 40
    dbs[0].clear()
    assert len(dbs[0]) == 0


# ---- arguments decided before any launch -----------------------------------------------------------------------------------------
def test_argument_errors():
    L = _ffi.lib()
    z = np.zeros(3, F)
    db = ObjectDatabase()
    for cid in (-1, 21):
        assert L.orbfe_objects_merge(db.h, cid, 0.9, _ffi.ptr(z), _ffi.ptr(z), _ffi.ptr(z), None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_objects_merge(db.h, 3, 0.9, None, _ffi.ptr(z), _ffi.ptr(z), None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_objects_merge(None, 3, 0.9, _ffi.ptr(z), _ffi.ptr(z), _ffi.ptr(z), None) == _ffi.ORBFE_ERR_ARG
    out = np.zeros(1, CL.CLUSTER_DTYPE)
    assert L.orbfe_objects_get(db.h, 0, _ffi.ptr(out)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_objects_create(None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_objects_size(None) == 0
    off = np.zeros(2, np.int32)
    st = np.zeros(1, CL.FILTER_DTYPE)
    assert L.orbfe_cloud_outlier_filter_device(None, None, _ffi.ptr(off), 1, 50, 1.0, 0, None, None, _ffi.ptr(st), None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_cloud_objects_device(None, None, 0, None, 0, None, None, None, None, 0, 50, 1.0, 0, None, None, 0, None, 0, None, None,
                                        None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_cloud_objects(None, None, None, None, None, None, None, 0, 50, 1.0, 0, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_cloud_objects_scratch_bytes(None) == 0
