"""Seeded inputs for the 3-D object tests (tests/test_objects_oracle.py, tests/test_gpu_objects.py).  Every point set is a
float32 [n, 3] array; `vacuity` asserts on the oracle's result alone that a case removes something and keeps something."""
import numpy as np

import cloud_cases as CC
import cloud_oracle as CO
import objects_oracle as OO

F = np.float32


def rec(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return CO.records(xyz, np.full(len(xyz), 0xff808080, np.uint32))


def collinear3():
    return np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F)


def lattice(m=16, h=0.25):
    g = np.arange(m, dtype=F) * F(h)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)


def coincident(n):
    return np.tile(np.array([[0.5, -1.25, 2.0]], F), (n, 1))


def blobs(n, seed, outliers=0.05):
    """three Gaussian blobs and a few points scattered over the room"""
    rng = np.random.default_rng(7000 + seed)
    centres = np.array([[0, 0, 2], [1.5, 0.2, 2.5], [-1, 0.5, 3]], F)
    k = rng.integers(0, 3, n)
    p = centres[k] + rng.normal(scale=0.08, size=(n, 3))
    far = rng.random(n) < outliers
    p[far] = rng.uniform(-3, 3, (int(far.sum()), 3)) + [0, 0, 3]
    return p.astype(F)


def coincident_plus(seed):
    """300 points in one place and 60 distinct ones around it"""
    rng = np.random.default_rng(7100 + seed)
    return np.concatenate([coincident(300), (np.array([0.5, -1.25, 2.0]) + rng.normal(scale=0.3, size=(60, 3))).astype(F)])


def far_point(seed):
    """a tight blob and one point 50 m away: its shells run out"""
    rng = np.random.default_rng(7200 + seed)
    return np.concatenate([rng.normal(scale=0.02, size=(400, 3)).astype(F), np.array([[50, 0, 0]], F)])


def sheet(seed):
    """a plane z = 2 exactly, a few points off it"""
    rng = np.random.default_rng(7300 + seed)
    p = rng.uniform(-1, 1, (900, 3))
    p[:, 2] = 2.0
    p[:12, 2] += rng.uniform(0.3, 1.0, 12)
    return p.astype(F)


def with_not_finite(seed):
    p = blobs(700, 50 + seed)
    p[5] = [np.nan, 0, 0]
    p[64] = [0, np.inf, 1]
    p[300] = [1, 2, -np.inf]
    p[699] = [np.nan, np.nan, np.nan]
    return p


def border_base(seed, n=2000):
    """random points in the unit cube; the first two pin the bounds"""
    rng = np.random.default_rng(7400 + seed)
    p = rng.uniform(0.05, 0.95, (n, 3)).astype(F)
    p[0], p[1] = [0, 0, 0], [1, 1, 1]
    return p


def on_borders(base, dims, origin, inv_cell, seed, count=600):
    """base with `count` of its points moved next to cell borders of the planned grid: on an axis the float at which the cell
    (int)((x - origin) * inv_cell) changes, and its neighbours one and two ulps to either side"""
    rng = np.random.default_rng(7500 + seed)
    p = base.copy()
    inv, origin = F(inv_cell), np.asarray(origin, F)
    for e in range(count):
        i = 2 + e
        ax = e % 3
        b = int(rng.integers(1, max(2, int(dims[ax]))))
        x = F(origin[ax] + F(b) / inv)
        for _ in range(int(rng.integers(0, 3))):
            x = np.nextafter(x, F(-np.inf) if e % 2 else F(np.inf))
        p[i, ax] = min(max(x, F(0)), F(1))
    return p


CASES = {   # name -> (points, mean_k, stddev_mul)
    "collinear3": (collinear3(), 2, 0.5),
    "lattice16": (lattice(16), 6, 1.0),
    "blobs1500": (blobs(1500, 1), 50, 1.0),
    "coincident_plus": (coincident_plus(1), 50, 1.0),
    "far_point": (far_point(1), 50, 1.0),
    "sheet": (sheet(1), 50, 1.0),
    "not_finite": (with_not_finite(1), 50, 1.0),
}


def vacuity(res):
    """the filter did something: a point removed, a point kept"""
    assert res["status"] == OO.OK
    assert 0 < int(res["keep"].sum()) < len(res["keep"])


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E_W, E2E_H = 64, 48
E2E_BOXES = np.array([[18, 14, 28, 20], [22, 18, 8, 6], [3, 3, 14, 9]], F)   # ordinary; fewer than 51 indices; the zero-depth patch
E2E_COLORS = np.array([[255, 0, 0], [0, 0, 255], [0, 255, 0]], np.uint8)
E2E_PROBS = np.array([0.9, 0.8, 0.7, 0.5], F)   # the fourth detection fails the 0.54 gate
E2E_CLASSES = np.array([9, 15, 20, 5], np.int32)


def e2e_frame(seed, shift=0.0):
    """cloud_cases.paint_frame with a zero-depth patch (its inner window holds nothing else, so the mean is 0 and the zeros are the
    box's points: one place, every distance 0) and a NaN inside that box.  `shift` moves the camera along x."""
    d, bgr = CC.paint_frame(E2E_W, E2E_H, seed)
    d[1:12, 1:18] = 0
    d[3, 5] = np.nan
    K = CC.intrinsics(E2E_W, E2E_H, seed)
    T = CO.pose_matrix(CC.pose_tcw(seed))
    T[0, 3] += shift
    return d, bgr, K, T


def e2e_boxes():
    """the detections of a frame: boxes, colours, probabilities, classes (one more box than passes the gate)"""
    return np.concatenate([E2E_BOXES, np.array([[30, 30, 10, 8]], F)]), np.concatenate([E2E_COLORS, np.array([[9, 9, 9]], np.uint8)]), E2E_PROBS, E2E_CLASSES
