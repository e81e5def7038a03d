"""The RGB-D Frame's per-frame geometry on the GPU: cv::undistortPoints (OpenCV 3.2) as Frame::UndistortKeyPoints calls it
(perfect/src/Frame.cc:750-781), Frame::ComputeImageBounds (:784-815), Frame::ComputeStereoFromRGBD (:1041-1062) and Tracking's
depth convertTo (perfect/src/Tracking.cc:681-682), through the C-ABI of csrc/orbfe_frame.hip.  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import DEPTH_F32, DEPTH_U16  # noqa: F401
from ._ffi import Handle, stream_arg, tensor_ptr


def _depth_format(d):
    """ORBFE_DEPTH_* of a [nframes, h, w] device tensor: float32, or 16-bit integers read as u16 (torch.int16 holds the bits)"""
    if not d.is_cuda or d.stride(2) != 1:
        raise ValueError("depth must be a device tensor with contiguous rows")
    if d.is_floating_point():
        if d.element_size() != 4:
            raise ValueError("a float depth plane must be float32")
        return DEPTH_F32
    if d.element_size() != 2:
        raise ValueError("an integer depth plane must hold 16-bit values")
    return DEPTH_U16


def _mat3(a, name):
    a = np.asarray(a, np.float32)
    if a.shape != (3, 3):
        raise ValueError(f"{name} must be 3x3")
    return a


class Camera(Handle):
    """mK, mDistCoef and mbf of a Frame.  K: 3x3 (converted to float32, as the settings file's CV_32F mK); dist: 0, 4, 5, 8 or 12
    coefficients k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]; P: the new camera matrix of undistortPoints -- "K" (the Frame's
    call, the default), None (normalised coordinates) or a 3x3 matrix."""

    _HANDLE, _DESTROY = "_m", "orbfe_matcher_destroy"   # the matcher whose stream and scratch the calls use, made on first use

    def __init__(self, K, dist=(), bf=0.0, P="K", device=0):
        self._L = _ffi.lib()
        K = _mat3(K, "K")
        d = np.asarray(dist, np.float32).ravel()
        c = _ffi.OrbfeCamera()
        c.K[:] = K.ravel().tolist()
        if isinstance(P, str):
            if P != "K":
                raise ValueError('P must be "K", None or a 3x3 matrix')
            P = K
        if P is not None:
            c.P[:] = _mat3(P, "P").ravel().tolist()
            c.has_P = 1
        if len(d) > 12:
            raise ValueError("at most 12 distortion coefficients (the tilted model is not built)")
        c.dist[:len(d)] = d.tolist()
        c.ndist = len(d)
        c.bf = float(bf)
        self.cam = c
        self.K, self.dist, self.bf = K, d, np.float32(bf)
        self.device = device
        self._m = None

    def _matcher(self):
        if self._m is None:
            m = C.c_void_p()
            _ffi.check(self._L.orbfe_matcher_create(self.device, C.byref(m)), "orbfe_matcher_create")
            self._m = m
        return self._m

    def undistort_points(self, xy):
        """cv::undistortPoints(src, dst, K, D, noArray(), P) on host points: float32 [n, 2] (no k1 shortcut)."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.empty_like(xy)
        _ffi.check(self._L.orbfe_undistort_points(self._matcher(), _ffi.ptr(xy), len(xy), C.byref(self.cam), _ffi.ptr(out)),
                   "orbfe_undistort_points")
        return out

    def image_bounds(self, w, h):
        """Frame::ComputeImageBounds for a w x h image: (minX, maxX, minY, maxY, gw_inv, gh_inv) as float32 -- minX, minY, gw_inv and
        gh_inv are the arguments of the grid calls."""
        out = np.zeros(6, np.float32)
        _ffi.check(self._L.orbfe_image_bounds(C.byref(self.cam), int(w), int(h), _ffi.ptr(out)), "orbfe_image_bounds")
        return tuple(out.tolist())

    def frame_geometry(self, kps, n, cap, depth=None, scale=1.0, stream=None, kps_un=None, depth_out=None, uright=None):
        """UndistortKeyPoints + ComputeStereoFromRGBD for every frame of an extractor output block, on torch device tensors:
        kps (nframes * cap orbfe_keypoint records, any dtype), n int32 [nframes]; depth None or a uint16 / float32 tensor
        [nframes, h, w] (rows contiguous), scale = the float 1 / DepthMapFactor.  Returns (kps_un like kps, depth float32
        [nframes, cap], uright float32 [nframes, cap]); enqueued on `stream` (default: torch's current stream)."""
        import torch
        nframes = n.numel()
        if kps_un is None:
            kps_un = torch.empty_like(kps)
        if depth_out is None:
            depth_out = torch.empty((nframes, cap), dtype=torch.float32, device=kps.device)
        if uright is None:
            uright = torch.empty((nframes, cap), dtype=torch.float32, device=kps.device)
        if kps.numel() * kps.element_size() < nframes * cap * 28 or not kps.is_contiguous():
            raise ValueError("kps must be a contiguous block of nframes * cap keypoint records")
        dp, dw, dh, fmt, ds, dfs = None, 0, 0, DEPTH_U16, 0, 0
        if depth is not None:
            if depth.dim() == 2:
                depth = depth.unsqueeze(0)
            fmt = _depth_format(depth)
            es = depth.element_size()
            dp, dh, dw, ds, dfs = tensor_ptr(depth), depth.shape[1], depth.shape[2], depth.stride(1) * es, depth.stride(0) * es
        st = stream_arg(kps.device, stream)
        _ffi.check(self._L.orbfe_frame_geometry_batch_device(self._matcher(), tensor_ptr(kps), tensor_ptr(n), int(cap), nframes, C.byref(self.cam), dp,
                                                             dw, dh, fmt, ds, dfs, float(scale), tensor_ptr(kps_un), tensor_ptr(depth_out),
                                                             tensor_ptr(uright), st), "orbfe_frame_geometry_batch_device")
        return kps_un, depth_out, uright

    @staticmethod
    def depth_to_float(depth, scale, out=None, stream=None):
        """mImDepth.convertTo(CV_32F, scale) on a uint16 (or int16 holding u16 bits) / float32 torch tensor [nframes, h, w] or
        [h, w] on the device: float32 of the same shape.  Enqueued on `stream` (default: torch's current stream)."""
        import torch
        d = depth.unsqueeze(0) if depth.dim() == 2 else depth
        nf, h, w = d.shape
        fmt = _depth_format(d)
        if out is None:
            out = torch.empty(depth.shape, dtype=torch.float32, device=depth.device)
        o = out.unsqueeze(0) if out.dim() == 2 else out
        es = d.element_size()
        st = stream_arg(depth.device, stream)
        _ffi.check(_ffi.lib().orbfe_depth_to_float_device(tensor_ptr(d), fmt, nf, w, h, d.stride(1) * es, d.stride(0) * es, float(scale), tensor_ptr(o),
                                                          o.stride(1) * 4, o.stride(0) * 4, st), "orbfe_depth_to_float_device")
        return out
