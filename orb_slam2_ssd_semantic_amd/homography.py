"""cv::findHomography on the GPU: the RANSAC estimate the fork's Tracking::TrackHomo (perfect/src/Tracking.cc:1331-1399) feeds
to the homography-compensated flow mask, and method 0 (least squares over all points), through the C-ABI of
csrc/orbfe_homography.hip.  No CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi, _ransac
from ._ffi import Handle, stream_arg, tensor_ptr

ABI = _ffi.ABI
RANSAC = ABI.ORBFE_HOMOGRAPHY_RANSAC
TAP_RANSAC, TAP_INFO, TAP_REFIT = ABI.ORBFE_HOMO_TAP_RANSAC, ABI.ORBFE_HOMO_TAP_INFO, ABI.ORBFE_HOMO_TAP_REFIT
KAT_RNG, KAT_HYPOT, KAT_NUMITERS, KAT_JACOBI9, KAT_JACOBI8 = (ABI.ORBFE_HOMO_KAT_RNG, ABI.ORBFE_HOMO_KAT_HYPOT, ABI.ORBFE_HOMO_KAT_NUMITERS,
                                                              ABI.ORBFE_HOMO_KAT_JACOBI9, ABI.ORBFE_HOMO_KAT_JACOBI8)


def _pairs(a, n=None):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 2)   # cv::Mat::convertTo(CV_32F)
    if n is not None and len(a) != n:
        raise ValueError("src and dst must hold the same number of points")
    return a


class Homography(Handle):
    """Device scratch for findHomography calls of at most max_pairs point pairs (host form) and batches of at most max_sets
    point sets (device form)."""

    _HANDLE, _DESTROY = "h", "orbfe_homography_destroy"

    def __init__(self, max_pairs=4096, max_sets=64, device=0):
        self._L = _ffi.lib()
        self.h = C.c_void_p()
        _ffi.check(self._L.orbfe_homography_create(device, max_pairs, max_sets, C.byref(self.h)), "orbfe_homography_create")
        self.device = device
        self.max_pairs = max_pairs
        self.max_sets = max_sets

    @property
    def stream(self):
        return self._L.orbfe_homography_get_stream(self.h)

    def find(self, src, dst, method=RANSAC, threshold=3.0, max_iters=2000, confidence=0.995):
        """cv::findHomography(src, dst, method, threshold, mask, max_iters, confidence) on host points: (H float64 [3, 3] or
        None, mask uint8 [n])."""
        s = _pairs(src)
        d = _pairs(dst, len(s))
        n = len(s)
        H = np.zeros(9, np.float64)
        mask = np.zeros(n, np.uint8)
        ok = C.c_int32()
        _ffi.check(self._L.orbfe_find_homography(self.h, _ffi.ptr(s), _ffi.ptr(d), n, int(method), float(threshold), int(max_iters),
                                                 float(confidence), _ffi.ptr(H), _ffi.ptr(mask) if n else None, C.byref(ok)),
                   "orbfe_find_homography")
        return (H.reshape(3, 3) if ok.value else None), mask

    def find_batch(self, offsets, src, dst, method=RANSAC, threshold=3.0, max_iters=2000, confidence=0.995, min_pairs=-1,
                   H=None, ok=None, mask=None, stream=None):
        """The batched form on torch device tensors: offsets int32 [nsets + 1] (CSR), src / dst float32 [N, 2].  Returns
        (H float64 [nsets, 3, 3], ok int32 [nsets], mask uint8 [N]) on the device; ok = result and n_i > min_pairs.  Enqueued
        on `stream` (default: torch's current stream), no synchronisation."""
        import torch
        _ransac.check_tensors((offsets, torch.int32, "offsets"), (src, torch.float32, "src"), (dst, torch.float32, "dst"))
        nsets = offsets.numel() - 1
        dev = offsets.device
        if H is None:
            H = torch.empty((nsets, 3, 3), dtype=torch.float64, device=dev)
        if ok is None:
            ok = torch.empty(nsets, dtype=torch.int32, device=dev)
        if mask is None:
            mask = torch.empty(max(src.shape[0], 1), dtype=torch.uint8, device=dev)
        st = stream_arg(dev, stream)
        _ffi.check(self._L.orbfe_find_homographies_device(self.h, tensor_ptr(offsets), tensor_ptr(src), tensor_ptr(dst), nsets, int(method),
                                                          float(threshold), int(max_iters), float(confidence), int(min_pairs),
                                                          tensor_ptr(H), tensor_ptr(ok), tensor_ptr(mask), st),
                   "orbfe_find_homographies_device")
        return H, ok, mask[:src.shape[0]]

    def tap(self, set_index, stage):
        """A stage of the last call: TAP_RANSAC / TAP_REFIT float64 [9], TAP_INFO int32 [4] (RANSAC result, iterations run,
        final niters, refit accepted)."""
        out = np.zeros(4, np.int32) if stage == TAP_INFO else np.zeros(9, np.float64)
        _ffi.check(self._L.orbfe_homography_tap(self.h, set_index, stage, _ffi.ptr(out), out.nbytes), "orbfe_homography_tap")
        return out


_default = {}


def find_homography(src, dst, method=RANSAC, threshold=3.0, max_iters=2000, confidence=0.995, device=0):
    """cv::findHomography(src, dst, method, threshold, mask, max_iters, confidence): (H float64 [3, 3] or None, mask uint8 [n]).
    method is RANSAC (8) or 0.  One cached handle per device, grown to the largest point count seen."""
    n = len(_pairs(src))
    return _ransac.default_handle(_default, Homography, "max_pairs", device, n).find(src, dst, method, threshold, max_iters, confidence)


def kat(what, data, n=None):
    """Runs a device primitive on host data (orbfe_homography_kat): KAT_RNG (data: the uint64 initial state, n draws) ->
    uint32 [n]; KAT_HYPOT (float64 [n, 2]) -> float64 [n]; KAT_NUMITERS (float64 [n, 3] of p, ep, max_iters) -> int32 [n];
    KAT_JACOBI9 / KAT_JACOBI8 (float64 [n, k, k]) -> (W float64 [n, k], V float64 [n, k, k])."""
    L = _ffi.lib()
    if what == KAT_RNG:
        inp = np.array([data], np.uint64)
        out = np.zeros(n, np.uint32)
    elif what == KAT_HYPOT:
        inp = np.ascontiguousarray(data, np.float64).reshape(-1, 2)
        n = len(inp)
        out = np.zeros(n, np.float64)
    elif what == KAT_NUMITERS:
        inp = np.ascontiguousarray(data, np.float64).reshape(-1, 3)
        n = len(inp)
        out = np.zeros(n, np.int32)
    else:
        k = 9 if what == KAT_JACOBI9 else 8
        inp = np.ascontiguousarray(data, np.float64).reshape(-1, k, k).copy()
        n = len(inp)
        out = np.zeros((n, k + k * k), np.float64)
    _ffi.check(L.orbfe_homography_kat(what, n, _ffi.ptr(inp), _ffi.ptr(out)), "orbfe_homography_kat")
    if what in (KAT_JACOBI9, KAT_JACOBI8):
        return out[:, :k].copy(), out[:, k:].reshape(n, k, k).copy()
    return out
