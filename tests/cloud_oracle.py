"""CPU oracle of the fork's dense point-cloud map (reference src/pointcloudmapping.cc): draw_rect_with_depth_threshold,
generatePointCloud + pcl::transformPointCloud, removeNaNFromPointCloud, the append and pcl::VoxelGrid.  Numpy, float32 where
the C++ has float and float64 where it has double, sums in the C++ order, one loop per voxel.

UNPINNED: PCL, Eigen and g2o are on no machine this project builds on, so nothing here was run against them.  What is
restated is PCL 1.8.1 (voxel_grid.hpp, centroid.hpp / accumulators.hpp, transforms.hpp, filter.hpp), Eigen 3.2 and g2o's
SE3Quat as the author knows them.  Every place where that knowledge decides a bit is an assumption, numbered here:

P1   PointXYZRGBA is 16 bytes of payload: float x, y, z and one uint32 `rgba` = a << 24 | r << 16 | g << 8 | b; a new point
     has a = 255.  generatePointCloud sets r, g, b and leaves a.
P2   generatePointCloud is evaluated as written, in float: x = ((float)c - cx) * d / fx (product first, then a true division),
     y likewise with r, cy, fy; z = d.
P3   pcl::transformPointCloud(in, out, Matrix4d) on a cloud with is_dense == false copies every point, leaves one whose x, y or
     z is not finite as it is, and writes the others as (float)(((m00 * x + m01 * y) + m02 * z) + m03) per row, the products
     and sums in double, no fused multiply-add.
P4   removeNaNFromPointCloud keeps, in order, the points whose x, y and z are all finite AFTER the transform (a finite input
     can overflow in the conversion to float).
P5   VoxelGrid: inverse_leaf = 1.0f / leaf in float; leaf = (float)resolution on the three axes.
P6   getMinMax3D runs over the finite points; points that are not finite are skipped by the filter as well (the is_dense ==
     false path; the map itself never holds one).  No finite point: the output is empty.
P7   dx = (int64)((max - min) * inverse_leaf) + 1 per axis, the product in float.  dx * dy * dz > INT_MAX: PCL warns and
     returns the input unchanged (`overflow`).  Where PCL's own arithmetic would leave defined behaviour -- a float beyond
     int64, an int64 product that wraps, or div_b0 * div_b1 * div_b2 > INT_MAX while dx * dy * dz is not -- the oracle also
     reports `overflow` and passes the input through.
P8   min_b = (int)floor(min * inverse_leaf), max_b likewise, the product in float; div_b = max_b - min_b + 1; divb_mul =
     (1, div_b0, div_b0 * div_b1).
P9   per point ijk = (int)(floor(p * inverse_leaf) - (float)min_b), product, floor and difference in float (`floor` resolves
     to the float overload); idx = ijk0 * divb_mul0 + ijk1 * divb_mul1 + ijk2 * divb_mul2.
P10  The points are sorted by idx.  std::sort leaves the order of equal keys open; THE LIBRARY'S DECISION is ascending input
     position inside a voxel (a stable sort).  `order="reversed"` gives another order std::sort would be allowed to produce, for
     the test that tells the two apart.
P11  min_points_per_voxel_ = 0, downsample_all_data_ = true: every voxel is one pcl::CentroidPoint.  xyz is accumulated as
     Vector3f += in sorted order and divided by (float)n with a true division (Eigen 3.2 scalar_quotient1_op, not a product
     with the reciprocal); r, g, b, a are accumulated as float sums of (float)channel and each stored as (uint32)(sum / (float)n).
P12  Output voxels are in ascending idx.
P13  draw_rect_with_depth_threshold: `(int)rect.height*0.3` is ((int)rect.height) * 0.3 in double; an `int` initialised or
     compared with it truncates / promotes as C++ says: k starts at (int)(H * 0.3) and runs while (double)k < H * 0.7; a row's
     columns run from (int)((double)start + W * 0.3) while j < (int)((double)start + W * 0.7).  `abs` is the float overload; its
     result is promoted to double for `< 0.4`.  A NaN depth passes `d < 0.5 || d > 6` and enters the sum.  mean = sum / (float)count.
P14  scalar.val[] (double) stored into a uchar is the colour byte itself for the 0 .. 255 values the fork's table holds.
P15  Converter::toSE3Quat: the float Tcw widened to double; g2o::SE3Quat(R, t) builds an Eigen::Quaterniond from R (Eigen's
     trace / largest-diagonal branches), flips it if w < 0 and normalises it: coeffs / sqrt(squaredNorm), squaredNorm summed as
     (x*x + z*z) + (y*y + w*w) (Eigen's SSE2 packet reduction of a Vector4d), each coefficient divided (true division).  The
     Isometry3d gets toRotationMatrix() of that quaternion and t unchanged.
P16  Isometry3d::inverse(): R^T and -(R^T) t, every row as (r0 * t0 + r1 * t1) + r2 * t2; the matrix is handed over row-major.
"""
import math

import numpy as np

F = np.float32
REC_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
INT_MAX = 2 ** 31 - 1


def records(xyz, rgba):
    out = np.zeros(len(rgba), REC_DTYPE)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["rgba"] = rgba
    return out


# ---- generatePointCloud .. removeNaNFromPointCloud (P1 - P4) ------------------------------------------------------------------
def generate_point_cloud(depth, bgr, K, T):
    """depth float32 [h, w], bgr uint8 [h, w, 3], K = (fx, fy, cx, cy), T float64 [4, 4] (T.inverse().matrix()).
    -> REC_DTYPE [count], the finite points in pixel order"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = np.arange(w, dtype=np.int32).astype(F)[None, :]
        r = np.arange(h, dtype=np.int32).astype(F)[:, None]
        x = ((c - cx) * depth / fx).astype(F)
        y = ((r - cy) * depth / fy).astype(F)
        z = depth.copy()
        fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        out = []
        for k, src in enumerate((x, y, z)):
            v = (((T[k, 0] * xd + T[k, 1] * yd) + T[k, 2] * zd) + T[k, 3]).astype(F)
            out.append(np.where(fin, v, src))
    bgr = np.asarray(bgr, np.uint8).reshape(h, w, 3).astype(np.uint32)
    rgba = (np.uint32(255) << np.uint32(24)) | (bgr[..., 2] << np.uint32(16)) | (bgr[..., 1] << np.uint32(8)) | bgr[..., 0]
    keep = (np.isfinite(out[0]) & np.isfinite(out[1]) & np.isfinite(out[2])).reshape(-1)
    xyz = np.stack([o.reshape(-1) for o in out], 1)
    return records(xyz[keep], rgba.reshape(-1)[keep])


# ---- pcl::VoxelGrid (P5 - P12) ----------------------------------------------------------------------------------------------
def _to_int64(v):
    """(int64)float, or None where C++ leaves the conversion undefined"""
    v = float(v)
    if not math.isfinite(v) or v >= 2.0 ** 63 or v < -2.0 ** 63:
        return None
    return int(v)


def voxel_plan(pts, leaf):
    """pts REC_DTYPE.  -> None (no finite point), "overflow", or (inverse_leaf, min_b int [3], divb_mul int [3])"""
    leaf = F(leaf)
    inv = F(1.0) / leaf
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
    fin = np.isfinite(xyz).all(1)
    if not fin.any():
        return None
    mn, mx = xyz[fin].min(0), xyz[fin].max(0)
    with np.errstate(all="ignore"):
        d = [_to_int64((mx[k] - mn[k]) * inv) for k in range(3)]
        lo = [_to_int64(np.floor(mn[k] * inv)) for k in range(3)]
        hi = [_to_int64(np.floor(mx[k] * inv)) for k in range(3)]
    if any(v is None for v in d + lo + hi):
        return "overflow"
    d = [v + 1 for v in d]
    if d[0] * d[1] * d[2] > INT_MAX or any(abs(v) > INT_MAX for v in lo + hi):
        return "overflow"
    div = [hi[k] - lo[k] + 1 for k in range(3)]
    if div[0] * div[1] * div[2] > INT_MAX:
        return "overflow"
    return inv, lo, [1, div[0], div[0] * div[1]]


def voxel_keys(pts, plan):
    """idx of every point (int64; -1 for a point that is not finite)"""
    inv, min_b, mul = plan
    idx = np.zeros(len(pts), np.int64)
    fin = np.ones(len(pts), bool)
    with np.errstate(all="ignore"):
        for k, name in enumerate("xyz"):
            p = pts[name]
            fin &= np.isfinite(p)
            ijk = (np.floor(p * inv) - F(min_b[k])).astype(F)
            idx += np.where(np.isfinite(ijk), ijk, 0).astype(np.int64) * mul[k]
    idx[~fin] = -1
    return idx


def centroid(pts):
    """pcl::CentroidPoint over pts in the given order (P11)"""
    sx = sy = sz = F(0)
    sr = sg = sb = sa = F(0)
    c = pts["rgba"]
    cols = [pts["x"], pts["y"], pts["z"], (c >> 24).astype(F), ((c >> 16) & 255).astype(F), ((c >> 8) & 255).astype(F), (c & 255).astype(F)]
    for x, y, z, a, r, g, b in zip(*cols):
        sx, sy, sz = sx + x, sy + y, sz + z
        sa, sr, sg, sb = sa + a, sr + r, sg + g, sb + b
    n = F(len(pts))
    rgba = (int(sa / n) << 24) | (int(sr / n) << 16) | (int(sg / n) << 8) | int(sb / n)
    return (sx / n, sy / n, sz / n, rgba)


def voxel_grid(pts, leaf, order="stable"):
    """-> (REC_DTYPE [voxels], overflow flag)"""
    pts = np.asarray(pts, REC_DTYPE)
    plan = voxel_plan(pts, leaf)
    if plan is None:
        return np.zeros(0, REC_DTYPE), False
    if isinstance(plan, str):
        return pts.copy(), True
    idx = voxel_keys(pts, plan)
    pos = np.nonzero(idx >= 0)[0]
    pos = pos[np.argsort(idx[pos], kind="stable")]
    keys = idx[pos]
    heads = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0]
    ends = np.r_[heads[1:], len(pos)]
    out = np.zeros(len(heads), REC_DTYPE)
    for v, (a, b) in enumerate(zip(heads, ends)):
        members = pos[a:b]
        if order == "reversed":
            members = members[::-1]
        out[v] = centroid(pts[members])
    return out, False


class Map:
    """viewer()'s globalMap: insert() takes the keyframes one wake-up of the thread finds"""

    def __init__(self, resolution):
        self.leaf = F(resolution)
        self.pts = np.zeros(0, REC_DTYPE)
        self.overflow = False

    def insert(self, frames):
        """frames: (depth, bgr, K, T) each"""
        clouds = [generate_point_cloud(*f) for f in frames]
        self.pts = np.concatenate([self.pts] + clouds)
        self.pts, self.overflow = voxel_grid(self.pts, self.leaf)
        return [len(c) for c in clouds]


# ---- draw_rect_with_depth_threshold (P13, P14) ---------------------------------------------------------------------------------
def box_touched(box, w, h):
    """(lowest, highest) flat index the reference reads or writes for the box, or None when it touches nothing"""
    X, Y, W, H = (int(v) for v in box)
    beg = X + (Y - 1) * w - 1
    lo, hi = None, None

    def see(a, b):   # [a, b)
        nonlocal lo, hi
        if b > a:
            lo = a if lo is None else min(lo, a)
            hi = b - 1 if hi is None else max(hi, b - 1)
    k = int(H * 0.3)
    while k < H * 0.7:
        start = beg + k * w
        see(int(start + W * 0.3), int(start + W * 0.7))
        k += 1
    for k in range(0, H - 1):
        start = beg + k * w
        see(start, start + W - 1 - 1)
    return None if lo is None else (lo, hi)


def paint_box(depth, bgr, box, color):
    """One call of draw_rect_with_depth_threshold on depth float32 [h, w] and bgr uint8 [h, w, 3] (painted in place).
    -> (indices int32 ascending, mean float32)"""
    h, w = depth.shape
    dep = depth.reshape(-1)
    col = bgr.reshape(-1, 3)
    X, Y, W, H = (int(v) for v in box)
    t = box_touched(box, w, h)
    if t is not None and (t[0] < 0 or t[1] >= w * h):
        raise IndexError("the box reaches outside the image")
    beg = X + (Y - 1) * w - 1
    count, s = 0, F(0)
    k = int(H * 0.3)
    with np.errstate(all="ignore"):
        while k < H * 0.7:
            start = beg + k * w
            for j in range(int(start + W * 0.3), int(start + W * 0.7)):
                d = dep[j]
                if float(d) < 0.5 or float(d) > 6:
                    continue
                s = F(s + d)
                count += 1
            k += 1
        mean = F(0.0)
        if count > 0:
            mean = F(s / F(count))
        idx = []
        for k in range(0, H - 1):
            start = beg + k * w
            for j in range(start, start + W - 1 - 1):
                if float(np.abs(F(dep[j] - mean))) < 0.4:
                    idx.append(j)
                    col[j] = color
    return np.asarray(idx, np.int32), mean


def paint_boxes(depth, bgr, boxes, colors):
    """the boxes of one frame in list order -> list of index arrays"""
    return [paint_box(depth, bgr, b, c)[0] for b, c in zip(boxes, colors)]


# ---- Converter::toSE3Quat + Isometry3d::inverse (P15, P16) --------------------------------------------------------------------
def pose_matrix(Tcw):
    """Tcw float32 [4, 4] -> T.inverse().matrix() float64 [4, 4]"""
    m = np.asarray(Tcw, F).reshape(4, 4).astype(np.float64)
    R, t = m[:3, :3], m[:3, 3]
    q = [0.0] * 4   # x, y, z, w
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[2, 1] - R[1, 2]) * s
        q[1] = (R[0, 2] - R[2, 0]) * s
        q[2] = (R[1, 0] - R[0, 1]) * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = math.sqrt(((R[i, i] - R[j, j]) - R[k, k]) + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    if q[3] < 0:
        q = [v * -1.0 for v in q]
    x, y, z, w = q
    nrm = math.sqrt((x * x + z * z) + (y * y + w * w))
    x, y, z, w = x / nrm, y / nrm, z / nrm, w / nrm
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    Rn = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                   [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                   [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    out = np.zeros((4, 4))
    out[:3, :3] = Rn.T
    for r in range(3):
        a = Rn.T[r]
        out[r, 3] = -((a[0] * t[0] + a[1] * t[1]) + a[2] * t[2])
    out[3, 3] = 1.0
    return out
