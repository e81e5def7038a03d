"""Seeded inputs for the outlier filter and the 3-D objects at the edges of the kNN grid's plan and past 1024 workgroups of the
compaction (tests/test_cloud_objects_edge_cases.py checks on the CPU that every case reaches its edge, tests/test_gpu_objects_edges.py
runs them on the device), and a port of the host planner knn_plan of csrc/orbfe_objects.hip that also says which of its three
breaks ended the shrinking.  Numpy only.  Test support only."""
import numpy as np

import cloud_edge_cases as CE
import cloud_oracle as CO
import objects_cases as OC
import objects_oracle as OO

F = np.float32
KNN_AUTO_BRUTE = 2048
KNN_MAX_DIM = 1000
KNN_MAX_CELLS = 1 << 22
INT32_MAX = 2 ** 31 - 1


# ---- knn_plan, step for step: double where the C++ has double, float where it has float ---------------------------------------------
def _isnormal(v):
    v = F(v)
    return bool(np.isfinite(v)) and abs(float(v)) >= float(np.finfo(F).tiny)


def knn_plan(mn, mx, nfin):
    """-> None (no grid can serve) or dict(dims, cells, origin float32 [3], inv_cell float32, brk): brk is "one_cell" (no extent),
    "maxdim" (an axis would reach KNN_MAX_DIM - 2 cells), "maxcells", "density" (about four points per cell) or "iterations\""""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    with np.errstate(all="ignore"):
        e = (mx - mn).astype(F)
    if not np.isfinite(e).all():
        return None
    emax = F(0)
    for k in range(3):
        if e[k] > emax:
            emax = e[k]
    plan = dict(dims=[1, 1, 1], cells=1, origin=mn.copy(), inv_cell=F(0), brk="one_cell")
    if not emax > 0:
        return plan
    s = float(emax)
    brk = "iterations"
    for _ in range(64):
        t = s * 0.8
        if float(emax) / t >= float(KNN_MAX_DIM - 2):
            brk = "maxdim"
            break
        c = 1
        for k in range(3):
            c *= int(float(e[k]) / t) + 1
        if c > KNN_MAX_CELLS:
            brk = "maxcells"
            break
        s = t
        if c * 4 >= nfin:
            brk = "density"
            break
    inv = F(1.0 / s)
    if not np.isfinite(inv) or not inv > 0 or not _isnormal(inv) or not _isnormal(F(s)):
        return None
    cells = 1
    for k in range(3):
        plan["dims"][k] = int(F(e[k] * inv)) + 1
        if plan["dims"][k] > KNN_MAX_DIM + 8:
            return None
        cells *= plan["dims"][k]
    plan.update(cells=cells, inv_cell=inv, brk=brk)
    return plan


def plan_of(pts):
    """the plan of a float32 [n, 3] point set: bounds and count over its finite points (no set here holds both +0 and -0 on an axis,
    where a minimum depends on the order)"""
    p = np.asarray(pts, F).reshape(-1, 3)
    fin = np.isfinite(p).all(1)
    if not fin.any():
        return None, 0
    return knn_plan(p[fin].min(0), p[fin].max(0), int(fin.sum())), int(fin.sum())


# ---- D: point sets --------------------------------------------------------------------------------------------------------------------
def line(seed=1):
    """D1: 4100 points on a line: no density can be reached before the axis limit"""
    rng = np.random.default_rng(9000 + seed)
    p = np.zeros((4100, 3), F)
    p[:, 0] = rng.uniform(-2, 2, 4100).astype(F)
    p[:, 1], p[:, 2] = 0.5, 2.0
    return p


def far_point_4100(seed=1):
    """D2: a millimetre blob and one point 50 m away: the axis limit, and a walk that runs every shell to rmax"""
    rng = np.random.default_rng(9100 + seed)
    return np.concatenate([rng.normal(scale=0.001, size=(4100, 3)).astype(F), np.array([[50, 0, 0]], F)])


def flat_sheet(seed=1, line_too=False):
    """D3: 900 points in [-1, 1]^2 at z = 2 exactly (one cell along z); line_too: y = 0.5 as well (one cell along y and z)"""
    rng = np.random.default_rng(9200 + seed)
    p = rng.uniform(-1, 1, (900, 3)).astype(F)
    p[:, 2] = 2.0
    if line_too:
        p[:, 1] = 0.5
    return p


NOT_FINITE = np.array([[np.nan, 0, 0], [0, np.inf, 1], [1, 2, -np.inf]], F)


def with_three_not_finite(p, at):
    """p with the three records inserted before positions at[0] < at[1] < at[2] of the result"""
    out = list(np.asarray(p, F))
    for a, r in zip(at, NOT_FINITE):
        out.insert(a, r)
    return np.asarray(out, F)


def exactly_64():
    """D4: mean_k = 63 needs 64 finite points: every finite point is every other's neighbour"""
    return with_three_not_finite(OC.blobs(64, 63), (0, 40, 66))


def auto_switch(nfin):
    """D5: nfin finite points (2048: the last brute-force size of AUTO, 2049: the first grid) and three that are not finite"""
    return with_three_not_finite(OC.blobs(nfin, nfin, outliers=0.02), (5, 1000, nfin + 2))


def grid_sets():
    """D6: sets of very different size for one GRID call"""
    return [OC.blobs(100, 41), OC.blobs(3000, 42), OC.lattice(16), OC.coincident(80), np.zeros((0, 3), F), OC.blobs(60, 43)]


GRID_CASES = {   # name -> (points, mean_k values)
    "line": (line(), (50,)),
    "far_point_4100": (far_point_4100(), (50,)),
    "flat_sheet": (flat_sheet(), (50, 6)),
    "flat_line": (flat_sheet(line_too=True), (50, 6)),
}

STDDEV_MULS = (0.0, np.inf, -1.0, -np.inf)
STDDEV_KEPT = (280, 300, 0, 0)       # on blobs(300, 31)


def stddev_points():
    return OC.blobs(300, 31)


# ---- D7 through build_objects: an object whose filter keeps nothing, and the object behind it -----------------------------------------
SM_W, SM_H = 64, 48
SM_MUL = -1.0


def stddev_frame():
    """Three patches of a 64 x 48 plane as index lists.  With stddev_mul = -1 the threshold is mean - stddev: object 0 (a flat wall
    and a few pixels metres behind it: stddev > mean) keeps nothing, object 1 (too few points) keeps all, object 2 (depths spread
    evenly: stddev < mean) keeps some.  -> (depth, bgr, K, T, index lists)"""
    import cloud_cases as CC
    rng = np.random.default_rng(9300)
    d = rng.uniform(1.0, 6.0, (SM_H, SM_W)).astype(F)
    d[4:20, 4:28] = rng.uniform(2.0, 2.004, (16, 24)).astype(F)
    for r, c in ((5, 6), (9, 20), (15, 11), (18, 25), (12, 5)):
        d[r, c] = 6.9
    bgr = rng.integers(0, 256, (SM_H, SM_W, 3), dtype=np.uint8)
    flat = np.arange(SM_W * SM_H, dtype=np.int32).reshape(SM_H, SM_W)
    lists = [flat[4:20, 4:28].reshape(-1), flat[30:34, 2:10].reshape(-1), flat[22:46, 34:62].reshape(-1)]
    return d, bgr, CC.intrinsics(SM_W, SM_H, 7), CO.pose_matrix(CC.pose_tcw(7)), lists


# ---- E: compaction past 1024 workgroups, indices outside the plane ---------------------------------------------------------------------
E_W, E_H = 512, 520
E_PATCH = (480, 460, 30, 40)          # top row, left column, rows, columns: 1200 pixels of ordinary depth near the bottom right
E_NAN_INDICES = 262300                # > 262 144: object 1's kept indices start behind workgroup 1024 of k_obj_compact
NAN_REC = (np.nan, np.nan, np.nan, 0xff000000)   # what k_obj_gather writes for an index outside the plane


def outside_frame():
    """-> (depth, bgr, K, T, index lists of the three objects)"""
    import cloud_cases as CC
    rng = np.random.default_rng(9400)
    r0, c0, nr, nc = E_PATCH
    d = np.full((E_H, E_W), np.nan, F)
    d[r0:r0 + nr, c0:c0 + nc] = rng.uniform(1.8, 2.6, (nr, nc)).astype(F)
    d[r0 + 3, c0 + 5] = d[r0 + 20, c0 + 33] = 6.5
    bgr = rng.integers(0, 256, (E_H, E_W, 3), dtype=np.uint8)
    flat = np.arange(E_W * E_H, dtype=np.int32).reshape(E_H, E_W)
    patch = flat[r0:r0 + nr, c0:c0 + nc].reshape(-1)
    nan_pixels = np.setdiff1d(flat.reshape(-1), patch)[:E_NAN_INDICES].astype(np.int32)
    third = np.concatenate([patch[:10], [-1], patch[600:610], [E_W * E_H], patch[1190:], [INT32_MAX]]).astype(np.int32)
    return d, bgr, CC.intrinsics(E_W, E_H, 8), CO.pose_matrix(CC.pose_tcw(8)), [nan_pixels, patch.astype(np.int32), third]


def outside_objects(leaf=0.05, mean_k=50, mul=1.0):
    """the oracle's objects for outside_frame: object 2's records are built by hand (frame_objects would wrap a negative index)
    -> (list of build_object results, index lists)"""
    d, bgr, K, T, lists = outside_frame()
    cloud = OO.organised_cloud(d, bgr, K, T)
    out = []
    for ix in lists:
        ix = np.asarray(ix, np.int64)
        inside = (ix >= 0) & (ix < E_W * E_H)
        before = np.zeros(len(ix), CO.REC_DTYPE)
        before[:] = NAN_REC
        before[inside] = cloud[ix[inside]]
        out.append(OO.build_object(before, leaf, mean_k, mul))
    return out, lists


def kept_flags(objs):
    """the keep flags of all objects of a call, in order: what k_obj_compact compacts"""
    return np.concatenate([o["keep"] for o in objs])


placement = CE.placement
