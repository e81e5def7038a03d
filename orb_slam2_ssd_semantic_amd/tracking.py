"""The tracker's two projection searches, batched and device-resident (csrc/orbfe_track.hip; include/orbfe.h "Tracker"):
SearchByProjection(CurrentFrame, LastFrame, th, bMono) of TrackWithMotionModel / TrackHomo and SearchByProjection(F,
vpMapPoints, th) of SearchLocalPoints, with Frame::UnprojectStereo, UpdateLastFrame's close-point rule, isInFrustum and
PredictScale on the device.

The *_batch_device methods are thin: device pointers (ints) and the structs of _ffi, asynchronous on `stream`.
track_last_frame() takes torch tensors, allocates the results and handles the entry-buffer retry.  frustum_points() and
scratch_bytes() need no GPU."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import TRACK_PROJ_DTYPE, InitSearchFirst, InitSearchOut, TrackCamera, TrackFrames, TrackLast, TrackMap, TrackOut, check, ptr, stream_arg

TH_HIGH, TH_LOW = _ffi.ABI.ORBFE_TH_HIGH, _ffi.ABI.ORBFE_TH_LOW   # src/ORBmatcher.cc:39-40


def camera(fx, fy, cx, cy, bf, minx, maxx, miny, maxy):
    return TrackCamera(*[float(v) for v in (fx, fy, cx, cy, bf, minx, maxx, miny, maxy)])


def _levels(scale_factors):
    sf = np.ascontiguousarray(scale_factors, np.float32)
    return sf, len(sf)


def scratch_bytes(nframes, qcap, ent_cap):
    """bytes of matcher scratch the batched search takes (orbfe_track_scratch_bytes); no GPU needed"""
    n = _ffi.lib().orbfe_track_scratch_bytes(int(nframes), int(qcap), int(ent_cap))
    if n < 0:
        raise ValueError("outside the limits of the batched search: nframes * qcap < 2^25, ent_cap < 2^32")
    return int(n)


def frustum_points(Tcw, cam, log_scale_factor, nlevels, world_pos, normal, min_dist, max_dist, seen=None, bad=None):
    """Frame::isInFrustum + PredictScale on the host for the points of one frame (orbfe_frustum_points): (proj, in_view) with
    proj a TRACK_PROJ_DTYPE array (level -1 where not in view)"""
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
    wp = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    mn, mx = np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32)
    sn = None if seen is None else np.ascontiguousarray(seen, np.uint8)
    bd = None if bad is None else np.ascontiguousarray(bad, np.uint8)
    n = len(wp)
    proj, in_view = np.zeros(n, TRACK_PROJ_DTYPE), np.zeros(n, np.uint8)
    check(_ffi.lib().orbfe_frustum_points(ptr(T), C.byref(cam), float(log_scale_factor), int(nlevels), n, ptr(wp), ptr(nm), ptr(mn), ptr(mx),
                                          ptr(sn), ptr(bd), ptr(proj), ptr(in_view)), "orbfe_frustum_points")
    return proj, in_view


def _dp(t):
    return None if t is None else t.data_ptr()


def frames_struct(d_kps, d_desc, d_n, cap, d_cell_off, d_cell_idx, minx, miny, gw_inv, gh_inv, d_uright=None, d_slot=None):
    """orbfe_track_frames from torch tensors (the caller keeps them alive)"""
    return TrackFrames(_dp(d_kps), _dp(d_desc), _dp(d_n), int(cap), _dp(d_cell_off), _dp(d_cell_idx), float(minx), float(miny), float(gw_inv),
                       float(gh_inv), _dp(d_uright), _dp(d_slot))


def init_search_structs(d_kps1, d_desc1, d_n1, cap1, d_matches12, d_nmatches, d_status, d_prev_out=None, d_offsets1=None, d_offsets2=None,
                        d_matches12_csr=None, d_keys1_xy=None, d_keys2_xy=None):
    """(orbfe_init_search_first, orbfe_init_search_out) from torch tensors (the caller keeps them alive)"""
    return (InitSearchFirst(_dp(d_kps1), _dp(d_desc1), _dp(d_n1), int(cap1)),
            InitSearchOut(_dp(d_matches12), _dp(d_nmatches), _dp(d_prev_out), _dp(d_offsets1), _dp(d_offsets2), _dp(d_matches12_csr),
                          _dp(d_keys1_xy), _dp(d_keys2_xy), _dp(d_status)))


def init_search_scratch_bytes(npairs, cap1, ent_cap):
    """bytes of matcher scratch SearchForInitialization_batch_device takes (orbfe_init_search_scratch_bytes); no GPU needed"""
    n = _ffi.lib().orbfe_init_search_scratch_bytes(int(npairs), int(cap1), int(ent_cap))
    if n < 0:
        raise ValueError("outside the limits of the batched search: cap <= 15360, npairs * cap < 2^25, ent_cap < 2^32")
    return int(n)


def init_search_ent_cap(npairs):
    """the first guess for the entry buffer of SearchForInitialization_batch_device: a 100 px window over 2000 features holds
    about 150 candidates per level-0 query; d_status[0] tells the exact need when it is short"""
    return max(int(npairs), 1) * 256 * 1024


class Tracker:
    """The device-resident tracking calls on a matcher's scratch: Tracker(ORBmatcher(...))"""

    def __init__(self, matcher):
        self._mt = matcher
        self._L = matcher._L

    def UnprojectSelect_batch_device(self, d_kps, d_depth, d_n, cap, nframes, d_Tcw, cam, th_depth, d_keeps, d_world_pos, d_created,
                                     stream=None):
        check(self._L.orbfe_unproject_select_batch_device(self._mt._m, d_kps, d_depth, d_n, int(cap), int(nframes), d_Tcw, C.byref(cam),
                                                          float(th_depth), d_keeps, d_world_pos, d_created, stream),
              "orbfe_unproject_select_batch_device")

    def GateLastFrame_batch_device(self, d_Tcw_cur, last, cam, mb, mono, th, scale_factors, nframes, d_q, d_qsrc, d_nq, qcap, stream=None):
        sf, nl = _levels(scale_factors)
        check(self._L.orbfe_gate_last_frame_batch_device(self._mt._m, d_Tcw_cur, C.byref(last), C.byref(cam), float(mb), int(mono), float(th),
                                                         ptr(sf), nl, int(nframes), d_q, d_qsrc, d_nq, int(qcap), stream),
              "orbfe_gate_last_frame_batch_device")

    def GateLocalMap_batch_device(self, d_Tcw, cam, th, scale_factors, log_scale_factor, tmap, d_list_off, d_list_idx, d_seen, nentries,
                                  nframes, d_q, d_qsrc, d_nq, qcap, d_visible=None, d_proj=None, stream=None):
        sf, nl = _levels(scale_factors)
        check(self._L.orbfe_gate_local_map_batch_device(self._mt._m, d_Tcw, C.byref(cam), float(th), ptr(sf), nl, float(log_scale_factor),
                                                        C.byref(tmap), d_list_off, d_list_idx, d_seen, int(nentries), int(nframes), d_q,
                                                        d_qsrc, d_nq, int(qcap), d_visible, d_proj, stream),
              "orbfe_gate_local_map_batch_device")

    def SearchByProjection_batch_device(self, frames, nframes, d_q, d_qsrc, d_nq, qcap, d_qpool, pool_rows, pool_frame_rows, th, nnratio,
                                        ratio_rule, ent_cap, d_match, d_best, d_second, d_status, inv_level_sigma2=None, stream=None):
        is2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        check(self._L.orbfe_search_by_projection_batch_device(self._mt._m, C.byref(frames), int(nframes), d_q, d_qsrc, d_nq, int(qcap), d_qpool,
                                                              int(pool_rows), int(pool_frame_rows), ptr(is2), 0 if is2 is None else len(is2),
                                                              int(th), float(nnratio), int(ratio_rule), int(ent_cap), d_match, d_best,
                                                              d_second, d_status, stream),
              "orbfe_search_by_projection_batch_device")

    def Replay_batch_device(self, frames, nframes, d_match, d_qsrc, d_nq, qcap, d_last_kps, cap_last, check_ori, d_assigned, d_nmatches,
                            d_pairs=None, d_npairs=None, stream=None):
        check(self._L.orbfe_track_replay_batch_device(self._mt._m, C.byref(frames), int(nframes), d_match, d_qsrc, d_nq, int(qcap), d_last_kps,
                                                      int(cap_last), int(check_ori), d_assigned, d_nmatches, d_pairs, d_npairs, stream),
              "orbfe_track_replay_batch_device")

    def TrackLastFrame_batch_device(self, cur, d_Tcw_cur, last, cam, mb, mono, th, scale_factors, th_high, check_ori, ent_cap, nframes, out,
                                    stream=None):
        sf, nl = _levels(scale_factors)
        check(self._L.orbfe_track_last_frame_batch_device(self._mt._m, C.byref(cur), d_Tcw_cur, C.byref(last), C.byref(cam), float(mb),
                                                          int(mono), float(th), ptr(sf), nl, int(th_high), int(check_ori), int(ent_cap),
                                                          int(nframes), C.byref(out), stream),
              "orbfe_track_last_frame_batch_device")

    def TrackLocalMap_batch_device(self, cur, d_Tcw, cam, th, scale_factors, log_scale_factor, tmap, d_list_off, d_list_idx, d_seen, nentries,
                                   th_high, nnratio, ent_cap, nframes, out, d_visible=None, d_proj=None, stream=None):
        sf, nl = _levels(scale_factors)
        check(self._L.orbfe_track_local_map_batch_device(self._mt._m, C.byref(cur), d_Tcw, C.byref(cam), float(th), ptr(sf), nl,
                                                         float(log_scale_factor), C.byref(tmap), d_list_off, d_list_idx, d_seen, int(nentries),
                                                         int(th_high), float(nnratio), int(ent_cap), int(nframes), C.byref(out), d_visible,
                                                         d_proj, stream),
              "orbfe_track_local_map_batch_device")

    def SearchForInitialization_batch_device(self, first, second, npairs, d_prev_in, window, out, th_low=TH_LOW, nnratio=0.9,
                                             check_ori=True, min_matches=0, ent_cap=None, stream=None):
        """ORBmatcher::SearchForInitialization for npairs frame pairs (orbfe_search_for_initialization_batch_device): first /
        out from init_search_structs, second from frames_struct, d_prev_in a device pointer (int) or None; asynchronous on
        `stream`.  out.d_status[0] != 0 afterwards: the entry buffer was short, call again with that ent_cap."""
        if ent_cap is None:
            ent_cap = init_search_ent_cap(npairs)
        check(self._L.orbfe_search_for_initialization_batch_device(self._mt._m, C.byref(first), C.byref(second), int(npairs), d_prev_in,
                                                                   int(window), int(th_low), float(nnratio), int(bool(check_ori)),
                                                                   int(min_matches), int(ent_cap), C.byref(out), stream),
              "orbfe_search_for_initialization_batch_device")

    # ---- torch layer -------------------------------------------------------------------------------------------------
    @staticmethod
    def alloc_out(nframes, cap, qcap, device="cuda"):
        """the result tensors of a chain call and the orbfe_track_out that points at them: (tensors, struct)"""
        import torch
        i32 = dict(dtype=torch.int32, device=device)
        t = dict(q=torch.zeros((nframes, qcap, 8), **i32), qsrc=torch.zeros((nframes, qcap), **i32), nq=torch.zeros((nframes,), **i32),
                 match=torch.full((nframes, qcap), -1, **i32), best=torch.zeros((nframes, qcap), **i32),
                 second=torch.zeros((nframes, qcap), **i32), status=torch.zeros((2,), **i32), assigned=torch.zeros((nframes, cap), **i32),
                 nmatches=torch.zeros((nframes,), **i32), pairs=torch.zeros((nframes, qcap, 2), **i32), npairs=torch.zeros((nframes,), **i32))
        out = TrackOut(t["q"].data_ptr(), t["qsrc"].data_ptr(), t["nq"].data_ptr(), int(qcap), t["match"].data_ptr(), t["best"].data_ptr(),
                       t["second"].data_ptr(), t["status"].data_ptr(), t["assigned"].data_ptr(), t["nmatches"].data_ptr(),
                       t["pairs"].data_ptr(), t["npairs"].data_ptr())
        return t, out

    def track_last_frame(self, cur, d_Tcw_cur, last, cam, mb, mono, th, scale_factors, nframes, th_high=TH_HIGH, check_ori=True,
                         ent_cap=None, out=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) for nframes pairs on torch's current stream.  cur / last are
        the structs (frames_struct, _ffi.TrackLast) over tensors the caller holds.  Reads the status back and, when the entry
        buffer was too small, calls once more with the exact need.  Returns the dict of result tensors (plus "ent_cap")."""
        qcap = int(last.cap)
        if out is None:
            out = self.alloc_out(nframes, int(cur.cap), qcap)
        t, o = out
        if ent_cap is None:
            ent_cap = max(nframes * qcap * 96, 1 << 16)   # the host path's first guess per query
        st = stream_arg(None, None)
        for attempt in range(2):
            self.TrackLastFrame_batch_device(cur, d_Tcw_cur, last, cam, mb, mono, th, scale_factors, th_high, check_ori, ent_cap, nframes, o, st)
            need = int(t["status"][0].item())   # the one wait of the call
            if need == 0:
                t["ent_cap"] = ent_cap   # what sufficed (a plain int): a caller that repeats the call passes it again
                return t
            ent_cap = need
        raise _ffi.OrbfeError(_ffi.ORBFE_ERR_NOMEM, "track_last_frame: candidate scratch still too small (%d entries)" % need)
