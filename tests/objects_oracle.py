"""CPU oracle of the fork's 3-D object loop (reference src/pointcloudmapping.cc:441-479 and sem_merge, :246-322): ExtractIndices,
pcl::StatisticalOutlierRemoval, pcl::VoxelGrid, compute3DCentroid, getMinMax3D and the cluster database.  Numpy, float32 where
the C++ has float and float64 where it has double, sums in the C++ order.  generate, voxel_grid and paint_boxes come from
cloud_oracle.py.

UNPINNED, as cloud_oracle.py is: PCL, FLANN and Eigen are on no machine this project builds on.  What is restated is PCL 1.8.1
(statistical_outlier_removal.hpp, extract_indices.hpp, centroid.hpp, common.hpp), FLANN 1.8's L2_Simple and the reference's own
sem_merge as the author knows them.  The assumptions that decide a bit, continuing cloud_oracle's P1 .. P16:

O1   ExtractIndices runs on the ORGANISED cloud generatePointCloud returned and transformPointCloud moved, before
     removeNaNFromPointCloud: index j is pixel j, its colour the painted plane's.  A point that is not finite stays in `before`.
O2   The kd-tree holds only the finite points (PCL's KdTreeFLANN drops the others when is_dense is false).  The distance is
     FLANN's L2_Simple<float>: result = 0; result += diff * diff per axis, in float, no FMA: ((dx*dx) + dy*dy) + dz*dz.
O3   applyFilterIndices: a point that is not finite gets distances[i] = 0 and is not counted as valid.  Any other point gets
     the mean_k + 1 smallest squared distances in ascending order; element 0 (the query or a coincident twin) is skipped;
     dist_sum is a serial double sum of the square roots of elements 1 .. mean_k; distances[i] = (float)(dist_sum / mean_k).
     Ties at the k-th distance change which neighbour FLANN returns, not its distance: the multiset of the mean_k + 1
     smallest distances is unique, so a brute-force sort gives what the kd-tree gives.
O4   sqrt(nn_dists[k]) is ambiguous across PCL builds: with the C <math.h> it is the double square root of the widened float
     (sqrt="double"); where libstdc++'s <math.h> wrapper puts std::sqrt(float) in scope it is the float square root, widened
     afterwards (sqrt="float").  THE LIBRARY'S DECISION is "double".
O5   The threshold: sum += d and sq_sum += d * d are serial double sums over ALL entries of `distances` in index order (the
     zeros of the points that are not finite included); d * d is a float product, widened afterwards.  mean = sum / valid;
     variance = (sq_sum - sum * sum / valid) / (valid - 1); stddev = sqrt(variance); threshold = mean + stddev_mul * stddev.
O6   A point is removed when (double)distances[i] > threshold (negative_ is false).  A NaN threshold keeps everything; the
     points that are not finite have distance 0 and are kept unless the threshold is negative.
O7   Fewer than mean_k + 1 finite points: the reference reads past the end of nn_dists (undefined).  THE LIBRARY'S DECISION:
     the object has status TOO_FEW, is not filtered (every point kept, every distance 0, threshold = mean = stddev = 0) and
     yields no cluster.
O8   An object with no index, or one whose kept points leave no voxel (none kept, or none of them finite): status EMPTY, no
     cluster (the reference would hand sem_merge an uninitialised centroid).  THE LIBRARY'S DECISION.
O9   VoxelGrid is cloud_oracle.voxel_grid with the map's leaf over the kept points, in order; on its overflow the kept points
     pass through.
O10  compute3DCentroid on the voxels takes the dense path: three serial float sums in voxel order (Vector4f +=), each divided by
     (float)n with a true division.
O11  getMinMax3D: the per-axis minimum and maximum over the voxels whose coordinates are finite.
O12  sem_merge as written.  The name is a function of class_id, so the search by name is a search by class.  Of the same-class
     entries the nearest centroid is taken: dist = sqrtf((dx*dx + dy*dy) + dz*dz) (Eigen's Vector3f norm), compared strictly,
     dist < center_distance, starting from 100.0f -- an entry 100 m away or more is never `best_close`.  It merges when
     center_distance < obj_size[class_id] (float): prob = (float)((double)(p0 + p1) / 2.0), the sum in float; centroid =
     (c0 + c1) / 2 per component in float; minPt the per-axis minimum; maxPt takes the SMALLER of the two maxima (:308-310,
     kept as the reference has it).  Otherwise the cluster is appended.  obj_size defaults to the reference's table (:63-70).
"""
import numpy as np

import cloud_oracle as CO

F = np.float32
D = np.float64
OK, TOO_FEW, EMPTY = 0, 1, 2
PROB_GATE = 0.54

OBJ_SIZE = np.full(21, 0.6, F)
OBJ_SIZE[5], OBJ_SIZE[9], OBJ_SIZE[15], OBJ_SIZE[20] = 0.06, 0.5, 0.35, 0.25

CLUSTER_DTYPE = np.dtype([("class_id", "<i4"), ("prob", "<f4"), ("centroid", "<f4", 3), ("min", "<f4", 3), ("max", "<f4", 3)])
assert CLUSTER_DTYPE.itemsize == 44


def xyz_of(pts):
    if pts.dtype == CO.REC_DTYPE:
        return np.stack([pts["x"], pts["y"], pts["z"]], 1)
    return np.asarray(pts, F).reshape(-1, 3)


# ---- ExtractIndices (O1) ---------------------------------------------------------------------------------------------------------
def organised_cloud(depth, bgr, K, T):
    """every pixel's record, the ones that are not finite included (cloud_oracle's P2, P3 without P4)"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T, D).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = np.arange(w, dtype=np.int32).astype(F)[None, :]
        r = np.arange(h, dtype=np.int32).astype(F)[:, None]
        x = ((c - cx) * depth / fx).astype(F)
        y = ((r - cy) * depth / fy).astype(F)
        z = depth.copy()
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        xd, yd, zd = x.astype(D), y.astype(D), z.astype(D)
        out = []
        for k, src in enumerate((x, y, z)):
            v = (((T[k, 0] * xd + T[k, 1] * yd) + T[k, 2] * zd) + T[k, 3]).astype(F)
            out.append(np.where(fin, v, src))
    bgr = np.asarray(bgr, np.uint8).reshape(h, w, 3).astype(np.uint32)
    rgba = (np.uint32(255) << np.uint32(24)) | (bgr[..., 2] << np.uint32(16)) | (bgr[..., 1] << np.uint32(8)) | bgr[..., 0]
    return CO.records(np.stack([o.reshape(-1) for o in out], 1), rgba.reshape(-1))


# ---- StatisticalOutlierRemoval (O2 - O7) ------------------------------------------------------------------------------------------
def knn_mean_distances(pts, mean_k, sqrt="double"):
    """-> (distances float32 [n], finite mask).  Brute force: a float distance matrix, np.sort per row."""
    xyz = xyz_of(pts)
    n = len(xyz)
    fin = np.isfinite(xyz).all(1)
    dist = np.zeros(n, F)
    q = xyz[fin]
    if len(q) < mean_k + 1:
        return None, fin
    out = np.zeros(len(q), F)
    step = max(1, (1 << 22) // max(len(q), 1))
    with np.errstate(all="ignore"):
        for a in range(0, len(q), step):
            d = (q[a:a + step, None, :] - q[None, :, :]).astype(F)
            d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)
            near = np.sort(d2, axis=1)[:, 1:mean_k + 1]
            roots = np.sqrt(near.astype(D)) if sqrt == "double" else np.sqrt(near).astype(D)
            s = np.zeros(len(near), D)
            for k in range(mean_k):   # serial, ascending
                s = s + roots[:, k]
            out[a:a + step] = (s / D(mean_k)).astype(F)
    dist[fin] = out
    return dist, fin


def statistical_outlier_removal(pts, mean_k=50, stddev_mul=1.0, sqrt="double"):
    """-> dict(status, distances float32 [n], keep bool [n], threshold, mean, stddev (float64), n_finite)"""
    n = len(pts)
    res = dict(status=OK, distances=np.zeros(n, F), keep=np.ones(n, bool), threshold=D(0), mean=D(0), stddev=D(0), n_finite=0)
    if n == 0:
        res["status"] = EMPTY
        return res
    dist, fin = knn_mean_distances(pts, mean_k, sqrt)
    res["n_finite"] = int(fin.sum())
    if dist is None:
        res["status"] = TOO_FEW
        return res
    s = sq = D(0)
    for d in dist:
        s = s + D(d)
        sq = sq + D(F(d * d))
    valid = D(res["n_finite"])
    with np.errstate(all="ignore"):
        mean = s / valid
        var = (sq - s * s / valid) / (valid - D(1))
        std = np.sqrt(var)
        thr = mean + D(stddev_mul) * std
    res.update(distances=dist, keep=~(dist.astype(D) > thr), threshold=thr, mean=mean, stddev=std)
    return res


# ---- one object: filter, VoxelGrid, centroid, bounds (O8 - O11) -------------------------------------------------------------------
def centroid3(vox):
    s = [F(0), F(0), F(0)]
    for x, y, z in zip(vox["x"], vox["y"], vox["z"]):
        s = [F(s[0] + x), F(s[1] + y), F(s[2] + z)]
    n = F(len(vox))
    return np.array([s[0] / n, s[1] / n, s[2] / n], F)


def build_object(before, leaf, mean_k=50, stddev_mul=1.0):
    """before: REC_DTYPE records of one box.  -> dict(status, n_in, n_kept, n_voxels, centroid, min, max, threshold, mean, stddev,
    keep, distances, voxels)"""
    f = statistical_outlier_removal(before, mean_k, stddev_mul)
    out = dict(status=f["status"], n_in=len(before), n_kept=int(f["keep"].sum()), n_voxels=0, centroid=np.zeros(3, F), min=np.zeros(3, F),
               max=np.zeros(3, F), threshold=f["threshold"], mean=f["mean"], stddev=f["stddev"], keep=f["keep"], distances=f["distances"],
               voxels=np.zeros(0, CO.REC_DTYPE))
    if f["status"] != OK:
        return out
    vox, _ = CO.voxel_grid(before[f["keep"]], leaf)
    out["voxels"], out["n_voxels"] = vox, len(vox)
    if len(vox) == 0:
        out["status"] = EMPTY
        return out
    with np.errstate(all="ignore"):
        out["centroid"] = centroid3(vox)
    xyz = xyz_of(vox)
    fin = np.isfinite(xyz).all(1)
    if fin.any():
        out["min"], out["max"] = xyz[fin].min(0), xyz[fin].max(0)
    return out


def frame_objects(depth, painted_bgr, K, T, index_lists, leaf, mean_k=50, stddev_mul=1.0):
    cloud = organised_cloud(depth, painted_bgr, K, T)
    return [build_object(cloud[np.asarray(ix, np.int64)], leaf, mean_k, stddev_mul) for ix in index_lists]


# ---- sem_merge (O12) -------------------------------------------------------------------------------------------------------------
class ObjectDatabase:
    def __init__(self, obj_size=None):
        self.obj_size = OBJ_SIZE.copy() if obj_size is None else np.asarray(obj_size, F).reshape(21).copy()
        self.clusters = []   # dicts of class_id, prob, centroid, min, max

    def merge(self, class_id, prob, centroid, mn, mx):
        """-> the index of the entry that took the cluster"""
        new = dict(class_id=int(class_id), prob=F(prob), centroid=np.asarray(centroid, F).copy(), min=np.asarray(mn, F).copy(),
                   max=np.asarray(mx, F).copy())
        best, center_distance = -1, F(100)
        with np.errstate(all="ignore"):
            for i, c in enumerate(self.clusters):
                if c["class_id"] != new["class_id"]:
                    continue
                d = (new["centroid"] - c["centroid"]).astype(F)
                dist = np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                if dist < center_distance:
                    center_distance, best = dist, i
            if best >= 0 and center_distance < self.obj_size[new["class_id"]]:
                c = self.clusters[best]
                c["prob"] = F(D(F(c["prob"] + new["prob"])) / D(2.0))
                c["centroid"] = ((c["centroid"] + new["centroid"]).astype(F) / F(2)).astype(F)
                c["min"] = np.where(c["min"] > new["min"], new["min"], c["min"]).astype(F)
                c["max"] = np.where(c["max"] > new["max"], new["max"], c["max"]).astype(F)
                return best
        self.clusters.append(new)
        return len(self.clusters) - 1

    def records(self):
        out = np.zeros(len(self.clusters), CLUSTER_DTYPE)
        for i, c in enumerate(self.clusters):
            out[i] = (c["class_id"], c["prob"], c["centroid"], c["min"], c["max"])
        return out
