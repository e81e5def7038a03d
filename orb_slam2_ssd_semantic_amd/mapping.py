"""LocalMapping's keyframe-rate matcher, batched and device-resident (csrc/orbfe_tri_search.hip; include/orbfe.h
"SearchForTriangulation, batched"): the neighbour loop of LocalMapping::CreateNewMapPoints up to vMatchedPairs -- the baseline
gate, ComputeF12 and the epipole of every (keyframe, neighbour) pair, then ORBmatcher::SearchForTriangulation for all pairs in
one call.  The triangulation of the pairs and KeyFrame::ComputeSceneMedianDepth stay with the caller.

The *_batch_device methods are thin: device pointers (ints) and the structs of _ffi, asynchronous on `stream`.
search_for_triangulation_device() takes torch tensors and allocates the results.  compute_f12(), tri_search_scratch_bytes() and
tri_search_info() need no GPU."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import TriKeyframes, TriOut, check, ptr, stream_arg
from .tracking import TH_LOW, camera  # noqa: F401  (camera(): the orbfe_track_camera both keyframes share)

_INFO = {k[len("ORBFE_TRI_INFO_"):].lower(): v for k, v in _ffi.ABI.constants.items() if k.startswith("ORBFE_TRI_INFO_")}


def _dp(t):
    return None if t is None else t.data_ptr()


def compute_f12(Tcw1, Tcw2, cam):
    """LocalMapping::ComputeF12 on the host (orbfe_compute_f12, the function the pair kernel runs): F12 (3, 3) float32"""
    T1 = np.ascontiguousarray(np.asarray(Tcw1, np.float32).reshape(-1)[:12])
    T2 = np.ascontiguousarray(np.asarray(Tcw2, np.float32).reshape(-1)[:12])
    F = np.zeros(9, np.float32)
    check(_ffi.lib().orbfe_compute_f12(ptr(T1), ptr(T2), C.byref(cam), ptr(F)), "orbfe_compute_f12")
    return F.reshape(3, 3)


def tri_search_scratch_bytes(npairs, cap):
    """bytes of matcher scratch SearchForTriangulation_batch_device takes (orbfe_tri_search_scratch_bytes); no GPU needed"""
    n = _ffi.lib().orbfe_tri_search_scratch_bytes(int(npairs), int(cap))
    if n < 0:
        raise ValueError("outside the limits of the batched search: 1 <= cap <= 8192, npairs * cap < 2^25")
    return int(n)


def tri_search_info():
    """the search kernel's constants by name: lanes, tile, queries_per_pass, node_workgroups, max_cap (orbfe_tri_search_info)"""
    return {k: int(_ffi.lib().orbfe_tri_search_info(v)) for k, v in _INFO.items()}


def keyframes_struct(d_kps, d_desc, d_n, cap, nframes, d_fv_node, d_fv_off, d_fv_idx, d_counts, d_uright=None, d_has_mp=None):
    """orbfe_tri_keyframes from torch tensors (the caller keeps them alive)"""
    return TriKeyframes(_dp(d_kps), _dp(d_desc), _dp(d_n), int(cap), int(nframes), _dp(d_uright), _dp(d_has_mp), _dp(d_fv_node),
                        _dp(d_fv_off), _dp(d_fv_idx), _dp(d_counts))


class LocalMapper:
    """The device-resident LocalMapping calls on a matcher's scratch: LocalMapper(ORBmatcher(...))"""

    compute_f12 = staticmethod(compute_f12)
    tri_search_scratch_bytes = staticmethod(tri_search_scratch_bytes)
    tri_search_info = staticmethod(tri_search_info)

    def __init__(self, matcher):
        self._mt = matcher
        self._L = matcher._L

    def set_triangulation_kernel(self, kernel):
        """0 = LDS tiles, a group of lanes per feature (default), 1 = one thread per feature: same results"""
        check(self._L.orbfe_matcher_set_triangulation_kernel(self._mt._m, int(kernel)), "orbfe_matcher_set_triangulation_kernel")

    def TriangulationPairs_batch_device(self, d_Tcw, d_Ow, nframes, cam, mb, mono, d_median_depth, d_kf1, d_kf2, npairs, d_F12, d_epi,
                                        d_pair_skip, stream=None):
        check(self._L.orbfe_triangulation_pairs_batch_device(self._mt._m, d_Tcw, d_Ow, int(nframes), C.byref(cam), float(mb), int(mono),
                                                             d_median_depth, d_kf1, d_kf2, int(npairs), d_F12, d_epi, d_pair_skip, stream),
              "orbfe_triangulation_pairs_batch_device")

    def SearchForTriangulation_batch_device(self, kf, d_kf1, d_kf2, npairs, d_F12, d_epi, d_pair_skip, scale_factors, level_sigma2, out,
                                            th_low=TH_LOW, only_stereo=False, check_ori=True, stream=None):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        if len(sf) != len(s2):
            raise ValueError("scale_factors and level_sigma2 have one entry per level each")
        check(self._L.orbfe_search_for_triangulation_batch_device(self._mt._m, C.byref(kf), d_kf1, d_kf2, int(npairs), d_F12, d_epi,
                                                                  d_pair_skip, ptr(sf), ptr(s2), len(sf), int(th_low), int(only_stereo),
                                                                  int(check_ori), C.byref(out), stream),
              "orbfe_search_for_triangulation_batch_device")

    def search_for_triangulation_device(self, kf, kf1, kf2, F12, epi, scale_factors, level_sigma2, pair_skip=None, th_low=TH_LOW,
                                        only_stereo=False, check_ori=True, stream=None):
        """SearchForTriangulation_batch_device on torch tensors: kf an orbfe_tri_keyframes (keyframes_struct), kf1 / kf2 int32 [P],
        F12 float32 [P][9], epi float32 [P][2], pair_skip uint8 [P] or None.  Allocates and returns (match12 [P][cap], nmatches
        [P], pairs [P][cap][2], npairs [P]) on the device of kf1; nothing is read back."""
        import torch
        P, dev = int(kf1.numel()), kf1.device
        match12 = torch.empty((P, kf.cap), dtype=torch.int32, device=dev)
        nmatches = torch.zeros((P,), dtype=torch.int32, device=dev)
        pairs = torch.full((P, kf.cap, 2), -1, dtype=torch.int32, device=dev)
        npairs = torch.zeros((P,), dtype=torch.int32, device=dev)
        out = TriOut(_dp(match12), _dp(nmatches), _dp(pairs), _dp(npairs))
        self.SearchForTriangulation_batch_device(kf, _dp(kf1), _dp(kf2), P, _dp(F12), _dp(epi), _dp(pair_skip), scale_factors, level_sigma2,
                                                 out, th_low, only_stereo, check_ori, stream_arg(dev, stream))
        return match12, nmatches, pairs, npairs
