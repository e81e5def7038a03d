"""DynaSLAM::Geometry on the GPU: the fork's multi-view geometry dynamic-point mask (perfect/src/Geometry.cc), the third producer
of the mask the masked Frame consumes, through the C-ABI of csrc/orbfe_geometry.hip.  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import KP_DTYPE, Handle, stream_arg, tensor_ptr

TAP_COUNTS, TAP_DYN, TAP_SEEDS, TAP_UNION, TAP_REGION = (
    _ffi.ABI.constants["ORBFE_GEOMETRY_TAP_" + k] for k in ("COUNTS", "DYN", "SEEDS", "UNION", "REGION"))
DB_SIZE, REF_FRAMES = _ffi.ABI.constants["ORBFE_GEOMETRY_DB_SIZE"], _ffi.ABI.constants["ORBFE_GEOMETRY_REF_FRAMES"]
COUNT_NAMES = ("read", "depth", "parallax", "depth7", "in_frame", "found", "gate", "dyn")


def _pose(Tcw):
    T = np.ascontiguousarray(Tcw, np.float32)
    if T.size != 16:
        raise ValueError("a pose is a 4x4 float32 mTcw")
    return T.reshape(16)


def _keys(k):
    """keypoints as orbfe_keypoint records: a KP_DTYPE array as the extractor returns it, or [n][2] (x, y)"""
    k = np.asarray(k)
    if k.dtype == KP_DTYPE:
        return np.ascontiguousarray(k)
    xy = np.ascontiguousarray(k, np.float32).reshape(-1, 2)
    out = np.zeros(len(xy), KP_DTYPE)
    out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def select_ref_frames(cur_Tcw, db_Tcw):
    """GetRefFrames on the host (no device needed): the indices of the min(5, n) most distant of the n <= 20 poses db_Tcw"""
    db = np.ascontiguousarray(db_Tcw, np.float32).reshape(-1, 16)
    idx = np.zeros(REF_FRAMES, np.int32)
    n = C.c_int32()
    _ffi.check(_ffi.lib().orbfe_geometry_select_ref_frames(_ffi.ptr(_pose(cur_Tcw)), _ffi.ptr(db), len(db), _ffi.ptr(idx), C.byref(n)),
               "orbfe_geometry_select_ref_frames")
    return [int(i) for i in idx[:n.value]]


def ellipse_half_widths(r):
    hw = np.zeros(2 * r + 1, np.int32)
    _ffi.check(_ffi.lib().orbfe_geometry_ellipse(r, _ffi.ptr(hw)), "orbfe_geometry_ellipse")
    return [int(v) for v in hw]


def acos_kat(x):
    """the library's canonical acos on the device, float64 in and out"""
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    _ffi.check(_ffi.lib().orbfe_geometry_kat(_ffi.ABI.constants["ORBFE_GEOMETRY_KAT_ACOS"], x.size, _ffi.ptr(x), _ffi.ptr(out)),
               "orbfe_geometry_kat")
    return out


class Geometry(Handle):
    """One DynaSLAM::Geometry: the key-frame ring lives on the device.  update_db() is GeometricModelUpdateDB for a key frame,
    correct() GeometricModelCorrection on one host depth plane, correct_batch_device() the same for device-resident frames
    against the ring as it stands, in the layout flow.mask_keypoints reads."""

    _HANDLE, _DESTROY = "h", "orbfe_geometry_destroy"

    def __init__(self, max_width=640, max_height=480, max_keypoints=2000, max_seeds=256, device=0):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(self._L.orbfe_geometry_create(device, max_width, max_height, max_keypoints, max_seeds, C.byref(self.h)),
                   "orbfe_geometry_create")
        self.device, self.max_seeds = device, max_seeds

    @property
    def stream(self):
        return self._L.orbfe_geometry_get_stream(self.h)

    @property
    def chunk(self):
        return self._L.orbfe_geometry_chunk(self.h)

    def reset(self):
        _ffi.check(self._L.orbfe_geometry_reset(self.h), "orbfe_geometry_reset")

    def db_state(self):
        """(mNumElem, mIni, mFin, per slot the number of inserts before the one it holds or -1)"""
        n, i, f = C.c_int32(), C.c_int32(), C.c_int32()
        slots = np.zeros(DB_SIZE, np.int32)
        _ffi.check(self._L.orbfe_geometry_db_state(self.h, C.byref(n), C.byref(i), C.byref(f), _ffi.ptr(slots)), "orbfe_geometry_db_state")
        return n.value, i.value, f.value, [int(s) for s in slots]

    def update_db(self, Tcw, depth, keys, keys_un):
        """depth: float32 [h, w] (numpy, or a torch tensor on the device together with keys / keys_un as KP_DTYPE byte blocks)"""
        T = _pose(Tcw)
        if isinstance(depth, np.ndarray):
            depth = np.ascontiguousarray(depth, np.float32)
            k, u = _keys(keys), _keys(keys_un)
            if len(k) != len(u):
                raise ValueError("keys and keys_un differ in length")
            h, w = depth.shape
            _ffi.check(self._L.orbfe_geometry_insert_keyframe(self.h, _ffi.ptr(depth), w, h, w * 4, _ffi.ptr(k), _ffi.ptr(u), len(k), _ffi.ptr(T),
                                                              0), "orbfe_geometry_insert_keyframe")
            return
        import torch
        assert depth.dtype == torch.float32 and depth.is_cuda and depth.stride(1) == 1
        h, w = depth.shape
        n = keys.numel() * keys.element_size() // KP_DTYPE.itemsize
        torch.cuda.current_stream(depth.device).synchronize()   # the insert runs on the handle's stream
        _ffi.check(self._L.orbfe_geometry_insert_keyframe(self.h, tensor_ptr(depth), w, h, depth.stride(0) * 4, tensor_ptr(keys),
                                                          tensor_ptr(keys_un), n, _ffi.ptr(T), 1), "orbfe_geometry_insert_keyframe")

    def correct(self, depth, Tcw, fx, fy, cx, cy):
        """(mask uint8 [h, w] of 1 = static / 0 = dynamic, computed): computed is 0, and the mask all ones, with fewer than 5 key
        frames or Tcw None"""
        depth = np.ascontiguousarray(depth, np.float32)
        h, w = depth.shape
        mask = np.empty((h, w), np.uint8)
        done = C.c_int32()
        T = None if Tcw is None else _pose(Tcw)
        _ffi.check(self._L.orbfe_geometry_correct(self.h, _ffi.ptr(depth), w, h, w * 4, _ffi.ptr(T), fx, fy, cx, cy, _ffi.ptr(mask), w,
                                                  C.byref(done)), "orbfe_geometry_correct")
        return mask, done.value

    def correct_batch_device(self, depth, Tcw, fx, fy, cx, cy, masks=None, ones=None, stream=None):
        """depth: torch float32 [n, h, w] on the device; Tcw: host [n, 4, 4].  Returns (masks uint8 [n, h, w], ones int32 [n]) on
        the device and the host computed flags [n].  Enqueued on `stream` (default: torch's current stream), no synchronisation."""
        import torch
        n, h, w = depth.shape
        assert depth.dtype == torch.float32 and depth.is_cuda and depth.stride(2) == 1
        T = np.ascontiguousarray(Tcw, np.float32).reshape(n, 16)
        if masks is None:
            masks = torch.empty((n, h, w), dtype=torch.uint8, device=depth.device)
        if ones is None:
            ones = torch.empty(n, dtype=torch.int32, device=depth.device)
        done = np.zeros(n, np.int32)
        _ffi.check(self._L.orbfe_geometry_correct_batch_device(self.h, tensor_ptr(depth), n, w, h, depth.stride(1) * 4, depth.stride(0) * 4,
                                                               _ffi.ptr(T), fx, fy, cx, cy, tensor_ptr(masks), masks.stride(1), masks.stride(0),
                                                               tensor_ptr(ones), _ffi.ptr(done), stream_arg(depth.device, stream)),
                   "orbfe_geometry_correct_batch_device")
        return masks, ones, done

    def depth_region_growing(self, seeds, depth):
        """DepthRegionGrowing alone: seeds [(x, y)] in order on one host depth plane -> mask; the taps then describe frame 0"""
        depth = np.ascontiguousarray(depth, np.float32)
        h, w = depth.shape
        s = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
        mask = np.empty((h, w), np.uint8)
        _ffi.check(self._L.orbfe_geometry_depth_region_growing(self.h, _ffi.ptr(depth), w, h, w * 4, _ffi.ptr(s), len(s), _ffi.ptr(mask), w),
                   "orbfe_geometry_depth_region_growing")
        return mask

    def tap(self, stage, frame=0, index=0, shape=None):
        """a stage of the last call: see orbfe_geometry_tap.  shape = (h, w) of the call's planes for TAP_UNION / TAP_REGION"""
        if stage == TAP_COUNTS:
            buf = np.zeros(8, np.int32)
        elif stage == TAP_DYN:
            buf = np.zeros((self.counts(frame)["dyn"], 3), np.int32)
        elif stage == TAP_SEEDS:
            buf = np.zeros(self.counts(frame)["dyn"], np.uint8)
        else:
            buf = np.zeros(shape, np.uint8)
        n = C.c_int32()
        _ffi.check(self._L.orbfe_geometry_tap(self.h, frame, stage, index, _ffi.ptr(buf), buf.nbytes, C.byref(n)), "orbfe_geometry_tap")
        return buf

    def counts(self, frame=0):
        return dict(zip(COUNT_NAMES, (int(v) for v in self.tap(TAP_COUNTS, frame))))


def extract_dyn_points(geometry, depth, Tcw, fx, fy, cx, cy):
    """ExtractDynPoints against geometry's ring: (dyn int32 [m][3] of (x, y, label), counts by COUNT_NAMES)"""
    _, done = geometry.correct(depth, Tcw, fx, fy, cx, cy)
    if not done:
        return np.zeros((0, 3), np.int32), dict.fromkeys(COUNT_NAMES, 0)
    return geometry.tap(TAP_DYN), geometry.counts()


def region_growing(geometry, depth, x, y):
    """RegionGrowing(im, x, y, 0.20f): J uint8 [h, w], the region and its frontier"""
    geometry.depth_region_growing([(x, y)], depth)
    return geometry.tap(TAP_REGION, index=0, shape=np.asarray(depth).shape)


def depth_region_growing(geometry, seeds, depth):
    """(mask, accepted flags uint8 [n], union before the dilation)"""
    mask = geometry.depth_region_growing(seeds, depth)
    shape = np.asarray(depth).shape
    return mask, geometry.tap(TAP_SEEDS), geometry.tap(TAP_UNION, shape=shape)
