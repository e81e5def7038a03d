"""FlowSLAM::Flow on the GPU: the fork's optical-flow dynamic-point mask (perfect/src/Flow.cc:15-52), its homography-compensated
form (:73-80, warpPerspective first) and the masked-Frame keypoint rule (perfect/src/Frame.cc:360-377), through the C-ABI of
csrc/orbfe_flow.hip.  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi, _ransac
from ._ffi import Handle, stream_arg, tensor_ptr

TAP_HALF, TAP_FLOW, TAP_FLOW2, TAP_PRE, TAP_MASK, TAP_POLY, TAP_WARP = (
    _ffi.ABI.constants["ORBFE_FLOW_TAP_" + k] for k in ("HALF", "FLOW", "FLOW2", "PRE", "MASK", "POLY", "WARP"))


def plan(w, h):
    """The Farneback level plan of a w x h frame's half-size image, level 0 first: [(lw, lh, ksize, blur taps)]."""
    L = _ffi.lib()
    n = C.c_int32()
    lw, lh, ks = (np.zeros(4, np.int32) for _ in range(3))
    taps = np.zeros((4, 19), np.float32)
    _ffi.check(L.orbfe_flow_plan(w, h, C.byref(n), _ffi.ptr(lw), _ffi.ptr(lh), _ffi.ptr(ks), _ffi.ptr(taps)), "orbfe_flow_plan")
    return [(int(lw[i]), int(lh[i]), int(ks[i]), taps[i, :ks[i]].copy()) for i in range(n.value)]


def poly_constants():
    """FarnebackPrepareGaussian(5, 1.2) as the library computes it: (g, xg, xxg) float32 [11] each, (ig11, ig03, ig33, ig55)."""
    g = np.zeros(33, np.float32)
    ig = np.zeros(4, np.float64)
    _ffi.check(_ffi.lib().orbfe_flow_poly_constants(_ffi.ptr(g), _ffi.ptr(ig)), "orbfe_flow_poly_constants")
    return g[:11], g[11:22], g[22:], tuple(float(v) for v in ig)


class Flow(Handle):
    """One FlowSLAM::Flow: its previous half-size frame lives on the device.  compute_mask() is Flow::ComputeMask on one host
    frame; compute_masks() the same over a device-resident sequence; mask_keypoints() the masked-Frame rule on the padded
    device blocks of ORBextractor.extract_batch_device-style outputs."""

    _HANDLE, _DESTROY = "h", "orbfe_flow_destroy"

    def __init__(self, max_width=640, max_height=480, max_batch=1, device=0):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(self._L.orbfe_flow_create(device, max_width, max_height, max_batch, C.byref(self.h)), "orbfe_flow_create")
        self.device = device

    @property
    def stream(self):
        return self._L.orbfe_flow_get_stream(self.h)

    def reset(self):
        _ffi.check(self._L.orbfe_flow_reset(self.h), "orbfe_flow_reset")

    def compute_mask(self, gray, threshold, homography=None):
        """Flow::ComputeMask(GrayImg, mask, threshold): uint8 [h, w] of 0 / 1.  With a 3x3 homography (float32 or float64, as
        findHomography returns it, not inverted): Flow::ComputeMask(GrayImg, Homo, mask, threshold), the frame warped first."""
        gray = np.ascontiguousarray(gray, np.uint8)
        h, w = gray.shape
        mask = np.empty((h, w), np.uint8)
        if homography is None:
            _ffi.check(self._L.orbfe_flow_compute_mask(self.h, _ffi.ptr(gray), w, h, w, float(threshold), _ffi.ptr(mask), w),
                       "orbfe_flow_compute_mask")
            return mask
        H = np.asarray(homography)
        if H.shape != (3, 3) or H.dtype not in (np.float32, np.float64):
            raise ValueError("homography must be a 3x3 float32 / float64 matrix")
        H = np.ascontiguousarray(H, np.float64)   # Mat::convertTo(CV_64F): exact for float32
        _ffi.check(self._L.orbfe_flow_compute_mask_homo(self.h, _ffi.ptr(gray), w, h, w, _ffi.ptr(H), float(threshold), _ffi.ptr(mask),
                                                        w), "orbfe_flow_compute_mask_homo")
        return mask

    def compute_masks(self, frames, threshold, masks=None, ones=None, stream=None, homographies=None, use=None):
        """frames: torch uint8 [n, h, w] on the device.  Returns (masks uint8 [n, h, w], ones int32 [n]) on the device; mask i
        comes from frames i-1 and i (mask 0 from the previous call's last frame).  Enqueued on `stream` (default: torch's
        current stream), no synchronisation.  homographies: torch float64 [n, 3, 3] on the device; frame i is warped by
        homographies[i] first when use is None or use[i] != 0 (use: torch int32 [n] on the device)."""
        import torch
        n, h, w = frames.shape
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.stride(2) == 1 and frames.stride(1) == w
        if masks is None:
            masks = torch.empty((n, h, w), dtype=torch.uint8, device=frames.device)
        if ones is None:
            ones = torch.empty(n, dtype=torch.int32, device=frames.device)
        st = stream_arg(frames.device, stream)
        if homographies is None:
            if use is not None:
                raise ValueError("use without homographies")
            _ffi.check(self._L.orbfe_flow_compute_masks_device(self.h, tensor_ptr(frames), n, w, h, w, frames.stride(0), float(threshold),
                                                               tensor_ptr(masks), w, masks.stride(0), tensor_ptr(ones), st),
                       "orbfe_flow_compute_masks_device")
            return masks, ones
        H = homographies
        _ransac.check_tensor(H, torch.float64, "homographies", "float64 [n, 3, 3]", (n, 3, 3))
        if use is not None:
            _ransac.check_tensor(use, torch.int32, "use", "int32 [n]", (n,))
        _ffi.check(self._L.orbfe_flow_compute_masks_homo_device(self.h, tensor_ptr(frames), n, w, h, w, frames.stride(0), tensor_ptr(H),
                                                                None if use is None else tensor_ptr(use), float(threshold), tensor_ptr(masks), w,
                                                                masks.stride(0), tensor_ptr(ones), st),
                   "orbfe_flow_compute_masks_homo_device")
        return masks, ones

    def tap(self, frame, stage, level=0):
        """A stage of the last call (frame index within it): see orbfe_flow_tap."""
        per = {TAP_HALF: (np.uint8, 1), TAP_FLOW: (np.float32, 2), TAP_FLOW2: (np.float32, 2), TAP_PRE: (np.uint8, 1),
               TAP_MASK: (np.uint8, 1), TAP_POLY: (np.float32, 5), TAP_WARP: (np.uint8, 1)}
        dt, ch = per[stage]
        cap = 4096 * 4096 * 20
        buf = np.empty(cap, np.uint8)
        w, h = C.c_int32(), C.c_int32()
        _ffi.check(self._L.orbfe_flow_tap(self.h, frame, stage, level, _ffi.ptr(buf), cap, C.byref(w), C.byref(h)), "orbfe_flow_tap")
        n = w.value * h.value * ch * np.dtype(dt).itemsize
        a = buf[:n].view(dt).reshape(h.value, w.value, ch)
        return a[:, :, 0].copy() if ch == 1 else a.copy()


def mask_keypoints(masks, ones, kps, desc, n, cap, stream=None):
    """perfect/src/Frame.cc:360-377 in place on device blocks: masks uint8 [b, h, w], ones int32 [b], kps [b*cap*28] bytes
    (orbfe_keypoint), desc uint8 [b*cap*32], n int32 [b] -- all torch tensors on the device.  masks may be pitched
    (stride(1) >= w, stride(2) == 1).  ones[i] is the sum of mask i's values (what compute_masks returns); frame i is filtered
    when it exceeds h*w*0.65.  A keypoint is in the plane iff x > -1 and x < w and y > -1 and y < h, decided in float before
    the truncation (a NaN is out); a keypoint outside the plane, or on a mask value other than 1, is dropped."""
    import torch
    b, h, w = masks.shape
    assert masks.dtype == torch.uint8 and masks.stride(2) == 1
    st = stream_arg(masks.device, stream)
    _ffi.check(_ffi.lib().orbfe_mask_keypoints_device(tensor_ptr(masks), w, h, masks.stride(1), masks.stride(0), tensor_ptr(ones), b, tensor_ptr(kps), tensor_ptr(desc),
                                                      tensor_ptr(n), cap, st), "orbfe_mask_keypoints_device")
