"""The fork's dense coloured point-cloud map (reference src/pointcloudmapping.cc) on the GPU, through the C-ABI of
csrc/orbfe_cloud.hip: the box paint, generatePointCloud + transformPointCloud + removeNaNFromPointCloud, the append to the
global map and pcl::VoxelGrid.  Planes are torch device tensors (numpy arrays are uploaded first); a cloud on the device is an
int32 [n, 4] tensor holding the bits of (x, y, z, rgba).  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import Handle, stream_arg, tensor_ptr

ABI, dtype = _ffi.ABI, _ffi.dtype
REC_DTYPE, OBJECT_DTYPE, FILTER_DTYPE = dtype("orbfe_cloud_point"), dtype("orbfe_object"), dtype("orbfe_filter_stat")
PLAN_DTYPE, CLUSTER_DTYPE = dtype("orbfe_knn_plan"), dtype("orbfe_cluster")
OBJECT_OK, OBJECT_TOO_FEW, OBJECT_EMPTY = ABI.ORBFE_OBJECT_OK, ABI.ORBFE_OBJECT_TOO_FEW, ABI.ORBFE_OBJECT_EMPTY
KNN_AUTO, KNN_BRUTE, KNN_GRID = ABI.ORBFE_KNN_AUTO, ABI.ORBFE_KNN_BRUTE, ABI.ORBFE_KNN_GRID
PROB_GATE = 0.54   # the reference merges a detection only when prob > 0.54


def pose_matrix(Tcw):
    """Converter::toSE3Quat(Tcw) then Isometry3d::inverse().matrix(): Tcw float32 [4, 4] -> float64 [4, 4] (host only)"""
    t = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    out = np.zeros((4, 4), np.float64)
    _ffi.check(_ffi.lib().orbfe_cloud_pose_matrix(_ffi.ptr(t), _ffi.ptr(out)), "orbfe_cloud_pose_matrix")
    return out


def _intrinsics(camera):
    """(fx, fy, cx, cy), or anything with a 3 x 3 `K` (Camera)"""
    K = getattr(camera, "K", None)
    if K is not None:
        K = np.asarray(K, np.float32).reshape(3, 3)
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    return np.ascontiguousarray(camera, np.float32).reshape(4)


def _matrix(pose):
    """float64 [4, 4] = T.inverse().matrix() as it is; float32 [4, 4] = Tcw, through pose_matrix"""
    a = np.asarray(pose)
    if a.dtype == np.float64:
        return np.ascontiguousarray(a).reshape(4, 4)
    if a.dtype == np.float32:
        return pose_matrix(a)
    raise ValueError("a pose is a float32 Tcw or a float64 Twc matrix")


def to_records(t):
    """a device cloud (int32 [n, 4]) -> REC_DTYPE [n] on the host"""
    return t.cpu().numpy().view(REC_DTYPE).reshape(-1).copy()


class PointCloudMap(Handle):
    """globalMap of the reference's PointCloudMapping: a device-resident voxel-filtered cloud of at most max_points records
    (the points of an insert before its filter pass included), fed max_frames keyframes of w x h at a time."""

    _HANDLE, _DESTROY = "h", "orbfe_cloud_destroy"

    def __init__(self, resolution, w, h, max_points=1 << 22, max_frames=4, device=0):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(self._L.orbfe_cloud_create(device, float(resolution), max_points, max_frames, w, h, C.byref(self.h)), "orbfe_cloud_create")
        self.device, self.w, self.ht = device, w, h
        self.max_points, self.max_frames = max_points, max_frames
        self.overflow = False

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _planes(self, depth, bgr):
        import torch
        d = torch.as_tensor(depth).to(self._dev())
        c = torch.as_tensor(bgr).to(self._dev())
        if d.dtype != torch.float32 or c.dtype != torch.uint8:
            raise ValueError("depth must be float32 (Camera.depth_to_float), bgr uint8")
        d = d.reshape(-1, self.ht, self.w).contiguous()
        c = c.reshape(-1, self.ht, self.w, 3).contiguous()
        if d.shape[0] != c.shape[0]:
            raise ValueError("one colour plane per depth plane")
        return d, c

    def _frames(self, depth, bgr, pose, camera):
        d, c = self._planes(depth, bgr)
        B = d.shape[0]
        poses = [pose] if np.asarray(pose).ndim == 2 else list(pose)
        cams = camera if isinstance(camera, (list, tuple)) and len(camera) == B and np.ndim(camera[0]) > 0 else [camera] * B
        if len(poses) != B:
            raise ValueError("one pose per keyframe")
        K = np.ascontiguousarray(np.stack([_intrinsics(k) for k in cams]), np.float32)
        T = np.ascontiguousarray(np.stack([_matrix(p) for p in poses]), np.float64)
        return d, c, B, K, T

    def _plane_args(self, d, c):
        return (tensor_ptr(d), self.w * 4, self.w * self.ht * 4, tensor_ptr(c), self.w * 3, self.w * self.ht * 3)

    def paint_boxes(self, depth, bgr, boxes, colors, stream=None):
        """draw_rect_with_depth_threshold for the boxes (x, y, width, height) of one frame, in list order, with their colours
        (the three bytes stored per painted pixel).  bgr (a contiguous uint8 device tensor) is painted in place; a host array is
        copied first.  -> (bgr device tensor, list of int32 index arrays, one per box)"""
        import torch
        d, c = self._planes(depth, bgr)
        if d.shape[0] != 1:
            raise ValueError("one frame at a time")
        bx = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        if len(col) != len(bx):
            raise ValueError("one colour per box")
        most = int(sum(max(int(b[2]) - 2, 0) * max(int(b[3]) - 1, 0) for b in bx if np.isfinite(b).all() and np.abs(b).max() < 2 ** 20))
        idx = torch.zeros(max(most, 1), dtype=torch.int32, device=self._dev())
        counts = np.zeros(max(len(bx), 1), np.int32)
        n = C.c_int32()
        _ffi.check(self._L.orbfe_cloud_paint_boxes_device(self.h, tensor_ptr(d), self.w * 4, tensor_ptr(c), self.w * 3, _ffi.ptr(bx), _ffi.ptr(col),
                                                          len(bx), tensor_ptr(idx), most, _ffi.ptr(counts), C.byref(n),
                                                          stream_arg(self._dev(), stream)), "orbfe_cloud_paint_boxes_device")
        flat = idx[:n.value].cpu().numpy()
        ends = np.cumsum(counts[:len(bx)])
        return c[0], [flat[e - k:e].copy() for e, k in zip(ends, counts[:len(bx)])]

    def generate(self, depth, bgr, pose, camera, cap=None, stream=None):
        """The finite, transformed points of one keyframe or a batch ([B, h, w] planes, B poses, one camera or B of them), in
        order.  -> (device cloud int32 [n, 4], counts int32 [B])"""
        import torch
        d, c, B, K, T = self._frames(depth, bgr, pose, camera)
        cap = B * self.w * self.ht if cap is None else int(cap)
        out = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=self._dev())
        counts = np.zeros(max(B, 1), np.int32)
        n = C.c_int32()
        _ffi.check(self._L.orbfe_cloud_generate_device(self.h, *self._plane_args(d, c), B, _ffi.ptr(K), _ffi.ptr(T), tensor_ptr(out), cap,
                                                       _ffi.ptr(counts), C.byref(n), stream_arg(self._dev(), stream)), "orbfe_cloud_generate_device")
        return out[:n.value], counts[:B]

    def insert(self, depth, bgr, pose, camera, boxes=None, colors=None, stream=None):
        """What the mapping thread does for the keyframes it wakes up to: (paint the boxes of a single keyframe,) generate,
        append, one voxel-filter pass.  pose: a float32 Tcw (through pose_matrix) or a float64 T.inverse().matrix() per
        keyframe.  -> the map's size (per-keyframe counts in self.last_counts, the box indices in self.last_indices)"""
        d, c, B, K, T = self._frames(depth, bgr, pose, camera)
        self.last_indices = None
        if boxes is not None and len(boxes):
            if B != 1:
                raise ValueError("boxes go with a single keyframe")
            _, self.last_indices = self.paint_boxes(d, c, boxes, colors, stream)
        counts = np.zeros(max(B, 1), np.int32)
        n, ovf = C.c_int32(), C.c_int32()
        _ffi.check(self._L.orbfe_cloud_insert_device(self.h, *self._plane_args(d, c), B, _ffi.ptr(K), _ffi.ptr(T), _ffi.ptr(counts), C.byref(n),
                                                     C.byref(ovf), stream_arg(self._dev(), stream)), "orbfe_cloud_insert_device")
        self.last_counts = counts[:B]
        self.overflow = bool(ovf.value)
        return n.value

    def voxel_filter(self, points=None, cap=None, stream=None):
        """pcl::VoxelGrid with the map's leaf.  points = None: over the map itself, in place (an insert already ends with one,
        so this changes nothing unless the map was loaded) -> its size.  Else over any cloud (device int32 [n, 4] or REC_DTYPE
        host records) -> (device cloud, overflow)"""
        import torch
        own = points is None
        if own:
            n_in = len(self)
            src = self.device_cloud().clone()
        else:
            if isinstance(points, np.ndarray):
                points = torch.from_numpy(np.ascontiguousarray(points, REC_DTYPE).view(np.int32).reshape(-1, 4))
            src = points.to(self._dev()).contiguous()
            if src.dtype != torch.int32 or src.ndim != 2 or src.shape[1] != 4:
                raise ValueError("a cloud is an int32 [n, 4] tensor")
            n_in = src.shape[0]
        cap = n_in if cap is None else int(cap)
        out = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=self._dev())
        n, ovf = C.c_int32(), C.c_int32()
        _ffi.check(self._L.orbfe_cloud_voxel_filter_device(self.h, tensor_ptr(src) if n_in else None, n_in, tensor_ptr(out), cap, C.byref(n),
                                                           C.byref(ovf), stream_arg(self._dev(), stream)), "orbfe_cloud_voxel_filter_device")
        if own:
            self.overflow = bool(ovf.value)
            self.load(out[:n.value], stream)
            return n.value
        return out[:n.value], bool(ovf.value)

    def outlier_filter(self, points, offsets=None, mean_k=50, stddev_mul=1.0, mode=KNN_AUTO, stream=None):
        """pcl::StatisticalOutlierRemoval over one point set or several (offsets: CSR, len(sets) + 1 entries from 0): a device
        cloud (int32 [n, 4]) or REC_DTYPE host records.  -> (distances float32 device tensor [n], keep uint8 device tensor [n],
        FILTER_DTYPE stats [sets], PLAN_DTYPE plans [sets])"""
        import torch
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(np.ascontiguousarray(points, REC_DTYPE).view(np.int32).reshape(-1, 4))
        src = points.to(self._dev()).contiguous()
        if src.dtype != torch.int32 or src.ndim != 2 or src.shape[1] != 4:
            raise ValueError("a cloud is an int32 [n, 4] tensor")
        n = src.shape[0]
        off = np.array([0, n], np.int32) if offsets is None else np.ascontiguousarray(offsets, np.int32)
        if off.ndim != 1 or len(off) < 1 or (len(off) > 0 and off[-1] != n):
            raise ValueError("offsets run from 0 to the number of points")
        nobj = len(off) - 1
        dist = torch.zeros(max(n, 1), dtype=torch.float32, device=self._dev())
        keep = torch.zeros(max(n, 1), dtype=torch.uint8, device=self._dev())
        stats = np.zeros(max(nobj, 1), FILTER_DTYPE)
        plans = np.zeros(max(nobj, 1), PLAN_DTYPE)
        _ffi.check(self._L.orbfe_cloud_outlier_filter_device(self.h, tensor_ptr(src) if n else None, _ffi.ptr(off), nobj, int(mean_k),
                                                             float(stddev_mul), int(mode), tensor_ptr(dist), tensor_ptr(keep), _ffi.ptr(stats),
                                                             _ffi.ptr(plans), stream_arg(self._dev(), stream)),
                   "orbfe_cloud_outlier_filter_device")
        return dist[:n], keep[:n], stats[:nobj], plans[:nobj]

    def build_objects(self, depth, bgr, pose, camera, indices, mean_k=50, stddev_mul=1.0, mode=KNN_AUTO, want_kept=False, want_voxels=False,
                      stream=None):
        """The objects of one keyframe from the index lists paint_boxes returned (bgr: the painted plane).  -> OBJECT_DTYPE [boxes],
        and, when asked for, the list of kept-index arrays and the list of REC_DTYPE voxel arrays"""
        import torch
        d, c, B, K, T = self._frames(depth, bgr, pose, camera)
        if B != 1:
            raise ValueError("one keyframe at a time")
        counts = np.array([len(ix) for ix in indices], np.int32)
        nb, total = len(counts), int(counts.sum())
        flat = np.concatenate([np.asarray(ix, np.int32) for ix in indices]) if total else np.zeros(0, np.int32)
        idx = torch.from_numpy(np.ascontiguousarray(flat)).to(self._dev()) if total else None
        objs = np.zeros(max(nb, 1), OBJECT_DTYPE)
        kept = torch.zeros(max(total, 1), dtype=torch.int32, device=self._dev()) if want_kept else None
        vox = torch.zeros((max(total, 1), 4), dtype=torch.int32, device=self._dev()) if want_voxels else None
        nk, nv = C.c_int32(), C.c_int32()
        _ffi.check(self._L.orbfe_cloud_objects_device(self.h, tensor_ptr(d), self.w * 4, tensor_ptr(c), self.w * 3, _ffi.ptr(K), _ffi.ptr(T),
                                                      tensor_ptr(idx) if total else None, _ffi.ptr(counts) if nb else None, nb, int(mean_k),
                                                      float(stddev_mul), int(mode), _ffi.ptr(objs), tensor_ptr(kept) if want_kept else None, total,
                                                      tensor_ptr(vox) if want_voxels else None, total, C.byref(nk), C.byref(nv),
                                                      stream_arg(self._dev(), stream)), "orbfe_cloud_objects_device")
        objs = objs[:nb]
        out = [objs]
        if want_kept:
            flatk = kept[:nk.value].cpu().numpy()
            ends = np.cumsum(objs["n_kept"])
            out.append([flatk[e - k:e].copy() for e, k in zip(ends, objs["n_kept"])])
        if want_voxels:
            flatv = to_records(vox[:nv.value])
            nvs = np.where(objs["status"] == OBJECT_OK, objs["n_voxels"], 0)
            ends = np.cumsum(nvs)
            out.append([flatv[e - k:e].copy() for e, k in zip(ends, nvs)])
        return out[0] if len(out) == 1 else tuple(out)

    def objects(self, depth, bgr, pose, camera, boxes, colors, probs, class_ids, db=None, mean_k=50, stddev_mul=1.0, mode=KNN_AUTO, stream=None):
        """What viewer() does with the detections of one keyframe: the reference's prob > 0.54 gate, the box paint, then per box
        the outlier filter, the voxel grid, the centroid and the bounds; with `db` (an ObjectDatabase) every object whose status
        is OBJECT_OK is merged into it.  -> (OBJECT_DTYPE records of the boxes that passed the gate, their positions in `boxes`,
        the painted bgr device tensor)"""
        bx = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        col = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        pr = np.ascontiguousarray(probs, np.float32).reshape(-1)
        cid = np.ascontiguousarray(class_ids, np.int32).reshape(-1)
        if not (len(bx) == len(col) == len(pr) == len(cid)):
            raise ValueError("one colour, probability and class per box")
        sel = np.nonzero(pr.astype(np.float64) > PROB_GATE)[0]
        d, c = self._planes(depth, bgr)
        painted, indices = self.paint_boxes(d, c, bx[sel], col[sel], stream)
        objs = self.build_objects(d, c, pose, camera, indices, mean_k, stddev_mul, mode, stream=stream)
        if db is not None:
            for o, k in zip(objs, sel):
                if o["status"] == OBJECT_OK:
                    db.merge(int(cid[k]), pr[k], o["centroid"], o["min"], o["max"])
        return objs, sel, painted

    def objects_scratch_bytes(self):
        """device bytes the outlier filter and the objects have allocated on this handle (0 until they are first used)"""
        return int(self._L.orbfe_cloud_objects_scratch_bytes(self.h))

    def load(self, points, stream=None):
        """replace the map by a device cloud (int32 [n, 4]); an empty one clears it"""
        p = points.contiguous()
        _ffi.check(self._L.orbfe_cloud_upload_device(self.h, tensor_ptr(p) if p.shape[0] else None, p.shape[0], stream_arg(self._dev(), stream)),
                   "orbfe_cloud_upload_device")

    def clear(self):
        _ffi.check(self._L.orbfe_cloud_upload_device(self.h, None, 0, None), "orbfe_cloud_upload_device")

    def __len__(self):
        return int(self._L.orbfe_cloud_size(self.h))

    def device_cloud(self):
        """a copy of the map on the device (int32 [n, 4])"""
        import torch
        n = len(self)
        out = torch.empty((n, 4), dtype=torch.int32, device=self._dev())
        if n:
            rec = self.records()
            out.copy_(torch.from_numpy(rec.view(np.int32).reshape(-1, 4)))
        return out

    def records(self):
        """the map on the host, REC_DTYPE [n]"""
        out = np.zeros(len(self), REC_DTYPE)
        n = C.c_int32()
        _ffi.check(self._L.orbfe_cloud_download(self.h, _ffi.ptr(out) if len(out) else None, len(out), C.byref(n)), "orbfe_cloud_download")
        return out

    def points(self):
        """float32 [n, 3]"""
        r = self.records()
        return np.stack([r["x"], r["y"], r["z"]], 1)

    def colors(self):
        """uint8 [n, 4]: r, g, b, a"""
        c = self.records()["rgba"]
        return np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255, c >> 24], 1).astype(np.uint8)


def generate_point_cloud(depth, bgr, pose, camera, device=0):
    """One keyframe -> REC_DTYPE records on the host (a throw-away handle; keep a PointCloudMap for repeated use)"""
    d = np.asarray(depth) if not hasattr(depth, "shape") else depth
    with PointCloudMap(1.0, int(d.shape[-1]), int(d.shape[-2]), max_points=1, max_frames=1, device=device) as m:
        cloud, _ = m.generate(depth, bgr, pose, camera)
        return to_records(cloud)


def voxel_grid(points, leaf, device=0):
    """pcl::VoxelGrid at `leaf` over REC_DTYPE records (or a device cloud) -> (REC_DTYPE records, overflow)"""
    n = len(points)
    with PointCloudMap(leaf, 1, 1, max_points=max(n, 1), max_frames=1, device=device) as m:
        out, ovf = m.voxel_filter(points)
        return to_records(out), ovf


def paint_boxes(depth, bgr, boxes, colors, device=0):
    """draw_rect_with_depth_threshold for the boxes of one frame -> (painted bgr uint8 [h, w, 3] on the host, index arrays)"""
    d = np.asarray(depth) if not hasattr(depth, "shape") else depth
    with PointCloudMap(1.0, int(d.shape[-1]), int(d.shape[-2]), max_points=1, max_frames=1, device=device) as m:
        img, idx = m.paint_boxes(depth, bgr, boxes, colors)
        return img.cpu().numpy(), idx


class ObjectDatabase(Handle):
    """The reference's `clusters` vector with sem_merge (host only, no device needed).  obj_size: 21 floats, the distance below
    which two centroids of a class are one object; None = the reference's table."""

    _HANDLE, _DESTROY = "h", "orbfe_objects_destroy"

    def __init__(self, obj_size=None):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        sizes = None if obj_size is None else np.ascontiguousarray(obj_size, np.float32).reshape(21)
        _ffi.check(self._L.orbfe_objects_create(_ffi.ptr(sizes), C.byref(self.h)), "orbfe_objects_create")

    def merge(self, class_id, prob, centroid, min_pt, max_pt):
        """-> the index of the entry that took the cluster"""
        v = [np.ascontiguousarray(a, np.float32).reshape(3) for a in (centroid, min_pt, max_pt)]
        i = C.c_int32()
        _ffi.check(self._L.orbfe_objects_merge(self.h, int(class_id), float(np.float32(prob)), _ffi.ptr(v[0]), _ffi.ptr(v[1]), _ffi.ptr(v[2]),
                                               C.byref(i)), "orbfe_objects_merge")
        return i.value

    def __len__(self):
        return int(self._L.orbfe_objects_size(self.h))

    def records(self):
        """CLUSTER_DTYPE [len(self)]"""
        out = np.zeros(len(self), CLUSTER_DTYPE)
        for i in range(len(out)):
            _ffi.check(self._L.orbfe_objects_get(self.h, i, C.c_void_p(out[i:i + 1].ctypes.data)), "orbfe_objects_get")
        return out

    def clear(self):
        self._L.orbfe_objects_clear(self.h)


def statistical_outlier_removal(points, mean_k=50, stddev_mul=1.0, mode=KNN_AUTO, device=0):
    """pcl::StatisticalOutlierRemoval over REC_DTYPE records, a float32 [n, 3] array or a device cloud -> (keep bool [n],
    distances float32 [n], the FILTER_DTYPE record) on the host"""
    if isinstance(points, np.ndarray) and points.dtype != REC_DTYPE:
        xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        rec = np.zeros(len(xyz), REC_DTYPE)
        rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        points = rec
    with PointCloudMap(1.0, 1, 1, max_points=1, max_frames=1, device=device) as m:
        dist, keep, stats, _ = m.outlier_filter(points, None, mean_k, stddev_mul, mode)
        return keep.cpu().numpy().astype(bool), dist.cpu().numpy(), stats[0]
