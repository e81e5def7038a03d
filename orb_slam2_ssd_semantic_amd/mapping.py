"""LocalMapping::CreateNewMapPoints, batched and device-resident (csrc/orbfe_tri_search.hip, csrc/orbfe_newpoints.hip; include/orbfe.h
"SearchForTriangulation, batched" and "CreateNewMapPoints, device-resident"): the baseline gate, ComputeF12 and the epipole of every
(keyframe, neighbour) pair, ORBmatcher::SearchForTriangulation for all pairs in one call, the triangulation and the gates of every
match up to `new MapPoint(x3D, ...)`, KeyFrame::ComputeSceneMedianDepth, and the neighbour loop with the slot state carried from
one round of pairs to the next.  The triangulation's oracle is tests/newpoints_oracle.py, a numpy restatement that no compiled
reference pins.  And the next statement of LocalMapping::Run, SearchInNeighbors, with LoopClosing::SearchAndFuse: ORBmatcher::Fuse in
both overloads for a batch of (keyframe, list) pairs (csrc/orbfe_fuse.hip; include/orbfe.h "Fuse, batched"): Fuse_batch_device,
FuseSearch_batch_device, fuse_candidates_device (vpFuseCandidates), the numpy convenience fuse_device; fuse_gate_points(),
sim3_pose() and fuse_scratch_bytes() need no GPU.

The *_batch_device methods are thin: device pointers (ints) and the structs of _ffi, asynchronous on `stream`.
search_for_triangulation_device() and create_new_map_points_device() take torch tensors and allocate the results.  compute_f12(),
triangulate_match(), plan_rounds(), the *_scratch_bytes() and tri_search_info() need no GPU."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import NEWPT_KEY_DTYPE, NewptGeom, NewptOut, NewptState, TriKeyframes, TriOut, check, ptr, stream_arg
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


NEWPT = {k[len("ORBFE_NEWPT_"):]: v for k, v in _ffi.ABI.constants.items() if k.startswith("ORBFE_NEWPT_")}   # verdict by name


def newpt_key(ux, uy, octave, depth=-1.0, uright=-1.0, rx=None, ry=None):
    """one orbfe_newpt_key record: mvKeysUn (ux, uy, octave), mvKeys (rx, ry; default the same), mvDepth, mvuRight"""
    k = np.zeros(1, NEWPT_KEY_DTYPE)
    k["ux"], k["uy"], k["rx"], k["ry"] = ux, uy, ux if rx is None else rx, uy if ry is None else ry
    k["depth"], k["uright"], k["octave"] = depth, uright, octave
    return k


def triangulate_match(Tcw1, Ow1, Tcw2, Ow2, cam, mb, k1, k2, scale_factors, level_sigma2, scale_factor):
    """the loop body of CreateNewMapPoints for one match on the host (orbfe_triangulate_match, the function the kernel runs):
    -> (verdict, x3D float32 [3]); k1 / k2 from newpt_key()"""
    a = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)[:n]) for v, n in ((Tcw1, 12), (Ow1, 3), (Tcw2, 12), (Ow2, 3))]
    sf, s2 = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
    x = np.zeros(3, np.float32)
    v = _ffi.lib().orbfe_triangulate_match(ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), C.byref(cam), float(mb), ptr(k1), ptr(k2), ptr(sf),
                                           ptr(s2), min(len(sf), len(s2)), float(scale_factor), ptr(x))
    if v < 0:
        raise ValueError("orbfe_triangulate_match: " + _ffi.last_error())
    return int(v), x


def plan_rounds(kf1, kf2):
    """orbfe_newpoints_plan_rounds: -> (round_of [P], order [P], round_off [nrounds + 1]) int32; pair order[j] stands at position j"""
    k1, k2 = np.ascontiguousarray(kf1, np.int32).reshape(-1), np.ascontiguousarray(kf2, np.int32).reshape(-1)
    if len(k1) != len(k2):
        raise ValueError("kf1 and kf2 have one entry per pair each")
    P = len(k1)
    round_of, order, off = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P + 1, np.int32)
    nr = _ffi.lib().orbfe_newpoints_plan_rounds(ptr(k1), ptr(k2), P, ptr(round_of), ptr(order), ptr(off))
    if nr < 0:
        raise ValueError("orbfe_newpoints_plan_rounds: " + _ffi.last_error())
    return round_of, order, off[:nr + 1].copy()


def newpoints_scratch_bytes(npairs, cap, nframes):
    """bytes of matcher scratch the triangulation and the neighbour loop take beside the search's; no GPU needed"""
    n = _ffi.lib().orbfe_newpoints_scratch_bytes(int(npairs), int(cap), int(nframes))
    if n < 0:
        raise ValueError("outside the limits: 1 <= cap <= 8192, npairs * cap < 2^25, nframes >= 0")
    return int(n)


def geometry_struct(d_Tcw, d_Ow, cam, mb, scale_factor, d_depth=None, d_kps_raw=None):
    """orbfe_newpt_geom from torch tensors (the caller keeps them alive)"""
    return NewptGeom(_dp(d_kps_raw), _dp(d_depth), _dp(d_Tcw), _dp(d_Ow), cam, float(mb), float(scale_factor))


def keyframes_struct(d_kps, d_desc, d_n, cap, nframes, d_fv_node, d_fv_off, d_fv_idx, d_counts, d_uright=None, d_has_mp=None):
    """orbfe_tri_keyframes from torch tensors (the caller keeps them alive)"""
    return TriKeyframes(_dp(d_kps), _dp(d_desc), _dp(d_n), int(cap), int(nframes), _dp(d_uright), _dp(d_has_mp), _dp(d_fv_node),
                        _dp(d_fv_off), _dp(d_fv_idx), _dp(d_counts))


FUSE_PLAIN, FUSE_SIM3 = _ffi.ABI.ORBFE_FUSE_PLAIN, _ffi.ABI.ORBFE_FUSE_SIM3
# d_action by name: NONE, ADD, REPLACE_SLOT, REPLACE_POINT, COUNTED, DEFERRED, REPLACE_CANDIDATE
FUSE = {k[len("ORBFE_FUSE_"):]: v for k, v in _ffi.ABI.constants.items() if k.startswith("ORBFE_FUSE_") and k[11:] not in ("PLAIN", "SIM3")}


def fuse_scratch_bytes(npoints, ntargets, cap):
    """bytes of matcher scratch fuse_candidates_device takes (the search and the replay take none); no GPU needed"""
    n = _ffi.lib().orbfe_fuse_scratch_bytes(int(npoints), int(ntargets), int(cap))
    if n < 0:
        raise ValueError("outside the limits: 1 <= cap <= 15360, ntargets * cap < 2^25")
    return int(n)


def fuse_gate_points(Tcw, Ow, cam, th, scale_factors, log_scale_factor, world_pos, normal, min_dist, max_dist, mode=FUSE_PLAIN):
    """the gating of ORBmatcher::Fuse for the points of one (keyframe, list) pair on the host (orbfe_fuse_gate_points, the function
    the search kernel runs): (q PROJ_QUERY_DTYPE [n], level int32 [n], ok uint8 [n])"""
    T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(-1)[:12])
    O3 = np.ascontiguousarray(np.asarray(Ow, np.float32).reshape(-1)[:3])
    sf = np.ascontiguousarray(scale_factors, np.float32)
    wp = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    mn, mx = np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32)
    n = len(wp)
    q, level, ok = np.zeros(n, _ffi.PROJ_QUERY_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    check(_ffi.lib().orbfe_fuse_gate_points(ptr(T), ptr(O3), C.byref(cam), float(th), ptr(sf), float(log_scale_factor), len(sf), int(mode), n,
                                            ptr(wp), ptr(nm), ptr(mn), ptr(mx), ptr(q), ptr(level), ptr(ok)), "orbfe_fuse_gate_points")
    return q, level, ok


def sim3_pose(Scw):
    """the pose-level expressions of Fuse's Sim3 overload (src/ORBmatcher.cc:1209-1213), the caller's by the library's rule: scw =
    (float)sqrt(row 0 . row 0 in double), Rcw = sRcw / scw and tcw = Scw.col(3) / scw element by element in double rounded to float,
    Ow = -Rcw.t() * tcw accumulated left to right in float.  -> (Tcw float32 [12], Ow float32 [3])"""
    S = np.asarray(Scw, np.float32).reshape(4, 4)
    r0 = S[0, :3].astype(np.float64)
    scw = np.float32(np.sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]))
    T = (S[:3, :4].astype(np.float64) / np.float64(scw)).astype(np.float32)
    Ow = np.zeros(3, np.float32)
    for k in range(3):
        acc = np.float32(-T[0, k]) * T[0, 3]
        acc = np.float32(acc + np.float32(-T[1, k]) * T[1, 3])
        Ow[k] = np.float32(acc + np.float32(-T[2, k]) * T[2, 3])
    return np.ascontiguousarray(T.reshape(12)), Ow


def fuse_lists_struct(d_pair_kf, d_Tcw, d_Ow, d_list_off, d_list_idx, nentries, npairs, d_list_skip=None):
    """orbfe_fuse_lists from torch tensors (the caller keeps them alive)"""
    return _ffi.FuseLists(_dp(d_pair_kf), _dp(d_Tcw), _dp(d_Ow), _dp(d_list_off), _dp(d_list_idx), _dp(d_list_skip), int(nentries), int(npairs))


class LocalMapper:
    """The device-resident LocalMapping calls on a matcher's scratch: LocalMapper(ORBmatcher(...))"""

    fuse_scratch_bytes = staticmethod(fuse_scratch_bytes)
    fuse_gate_points = staticmethod(fuse_gate_points)
    sim3_pose = staticmethod(sim3_pose)
    compute_f12 = staticmethod(compute_f12)
    triangulate_match = staticmethod(triangulate_match)
    plan_rounds = staticmethod(plan_rounds)
    newpoints_scratch_bytes = staticmethod(newpoints_scratch_bytes)
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

    @staticmethod
    def _levels(scale_factors, level_sigma2):
        sf, s2 = np.ascontiguousarray(scale_factors, np.float32), np.ascontiguousarray(level_sigma2, np.float32)
        if len(sf) != len(s2):
            raise ValueError("scale_factors and level_sigma2 have one entry per level each")
        return sf, s2

    def TriangulatePairs_batch_device(self, kf, geom, d_kf1, d_kf2, npairs, d_pairs, d_npairs, scale_factors, level_sigma2, out, stream=None):
        sf, s2 = self._levels(scale_factors, level_sigma2)
        check(self._L.orbfe_triangulate_pairs_batch_device(self._mt._m, C.byref(kf), C.byref(geom), d_kf1, d_kf2, int(npairs), d_pairs, d_npairs,
                                                           ptr(sf), ptr(s2), len(sf), C.byref(out), stream),
              "orbfe_triangulate_pairs_batch_device")

    def SceneMedianDepth_batch_device(self, d_Tcw, d_has_mp, d_mp_xyz, d_n, nframes, cap, q, d_median, stream=None):
        check(self._L.orbfe_scene_median_depth_batch_device(self._mt._m, d_Tcw, d_has_mp, d_mp_xyz, d_n, int(nframes), int(cap), int(q),
                                                            d_median, stream), "orbfe_scene_median_depth_batch_device")

    def CreateNewMapPoints_batch_device(self, kf, geom, state, mono, d_kf1, d_kf2, npairs, round_off, scale_factors, level_sigma2, tri_out,
                                        out, th_low=TH_LOW, only_stereo=False, check_ori=True, id_base=0, d_pair_skip=None, stream=None):
        """round_off: the HOST array of nrounds + 1 offsets into the pairs, which stand in round order"""
        sf, s2 = self._levels(scale_factors, level_sigma2)
        ro = np.ascontiguousarray(round_off, np.int32).reshape(-1)
        if len(ro) < 1:
            raise ValueError("round_off has nrounds + 1 entries")
        check(self._L.orbfe_create_new_map_points_batch_device(self._mt._m, C.byref(kf), C.byref(geom), C.byref(state), int(mono), d_kf1, d_kf2,
                                                               int(npairs), ptr(ro), len(ro) - 1, ptr(sf), ptr(s2), len(sf), int(th_low),
                                                               int(only_stereo), int(check_ori), int(id_base), d_pair_skip, C.byref(tri_out),
                                                               C.byref(out), stream), "orbfe_create_new_map_points_batch_device")

    def create_new_map_points_device(self, kf, geom, has_mp, mp_xyz, mp_id, kf1, kf2, scale_factors, level_sigma2, mono=False, th_low=TH_LOW,
                                     only_stereo=False, check_ori=True, id_base=0, round_off=None, stream=None):
        """The neighbour loop on torch tensors.  kf / geom: keyframes_struct() / geometry_struct(); has_mp uint8 [B][cap], mp_xyz
        float32 [B][cap][3], mp_id int32 [B][cap] are UPDATED in place; kf1 / kf2: the pairs in the reference's loop order (any
        int sequence).  Plans the rounds (plan_rounds) unless round_off is given (then the pairs are taken as they stand), allocates
        the outputs and returns a dict: order (position -> the caller's pair), round_off, and per POSITION new_idx [P][cap][2],
        new_xyz [P][cap][3], nnew [P], verdict [P][cap], match12 [P][cap], nmatches [P], pairs [P][cap][2], npairs [P], pair_skip
        [P].  Nothing is read back."""
        import torch
        k1, k2 = np.asarray(kf1, np.int32).reshape(-1), np.asarray(kf2, np.int32).reshape(-1)
        if round_off is None:
            _, order, round_off = plan_rounds(k1, k2)
        else:
            order = np.arange(len(k1), dtype=np.int32)
        P, cap, dev = len(k1), kf.cap, has_mp.device
        d1, d2 = (torch.from_numpy(np.ascontiguousarray(k[order])).to(dev) for k in (k1, k2))
        i32 = dict(dtype=torch.int32, device=dev)
        r = dict(order=order, round_off=np.asarray(round_off, np.int32), new_idx=torch.full((P, cap, 2), -1, **i32),
                 new_xyz=torch.zeros((P, cap, 3), dtype=torch.float32, device=dev), nnew=torch.zeros((P,), **i32),
                 verdict=torch.full((P, cap), 255, dtype=torch.uint8, device=dev), match12=torch.full((P, cap), -1, **i32),
                 nmatches=torch.zeros((P,), **i32), pairs=torch.full((P, cap, 2), -1, **i32), npairs=torch.zeros((P,), **i32),
                 pair_skip=torch.zeros((P,), dtype=torch.uint8, device=dev))
        self.CreateNewMapPoints_batch_device(kf, geom, NewptState(_dp(has_mp), _dp(mp_xyz), _dp(mp_id)), mono, _dp(d1), _dp(d2), P, round_off,
                                             scale_factors, level_sigma2, TriOut(_dp(r["match12"]), _dp(r["nmatches"]), _dp(r["pairs"]), _dp(r["npairs"])),
                                             NewptOut(_dp(r["verdict"]), _dp(r["new_idx"]), _dp(r["new_xyz"]), _dp(r["nnew"])), th_low, only_stereo,
                                             check_ori, id_base, _dp(r["pair_skip"]), stream_arg(dev, stream))
        r["kf1"], r["kf2"] = d1, d2
        return r

    # ---- Fuse, batched (include/orbfe.h "Fuse, batched") ------------------------------------------------
    def FuseSearch_batch_device(self, frames, nkf, lists, cam, tmap, th, scale_factors, inv_level_sigma2, log_scale_factor, d_match, d_dist,
                                mode=FUSE_PLAIN, th_low=TH_LOW, stream=None):
        """the gate and the window search alone (orbfe_fuse_search_batch_device): frames from tracking.frames_struct, lists from
        fuse_lists_struct, tmap an orbfe_track_map; d_match / d_dist device pointers (ints) of nentries int32 each"""
        sf, s2 = self._levels(scale_factors, inv_level_sigma2)
        check(self._L.orbfe_fuse_search_batch_device(self._mt._m, C.byref(frames), int(nkf), C.byref(lists), C.byref(cam), C.byref(tmap), float(th),
                                                     ptr(sf), ptr(s2), len(sf), float(log_scale_factor), int(th_low), int(mode), d_match, d_dist,
                                                     stream), "orbfe_fuse_search_batch_device")

    def Fuse_batch_device(self, frames, nkf, lists, cam, tmap, d_nobs, d_slot_mp, th, scale_factors, inv_level_sigma2, log_scale_factor, out,
                          mode=FUSE_PLAIN, th_low=TH_LOW, stream=None):
        """ORBmatcher::Fuse for a batch of (keyframe, list) pairs, search + replay (orbfe_fuse_batch_device): d_nobs / d_slot_mp device
        pointers (ints) or None, out an orbfe_fuse_out (_ffi.FuseOut); asynchronous on `stream`, nothing is read back"""
        sf, s2 = self._levels(scale_factors, inv_level_sigma2)
        check(self._L.orbfe_fuse_batch_device(self._mt._m, C.byref(frames), int(nkf), C.byref(lists), C.byref(cam), C.byref(tmap), d_nobs, d_slot_mp,
                                              float(th), ptr(sf), ptr(s2), len(sf), float(log_scale_factor), int(th_low), int(mode),
                                              C.byref(out), stream), "orbfe_fuse_batch_device")

    @staticmethod
    def alloc_fuse_out(nentries, npairs, cap, device="cuda", first=False):
        """the result tensors of Fuse_batch_device and the orbfe_fuse_out that points at them: (tensors, struct)"""
        import torch
        i32 = dict(dtype=torch.int32, device=device)
        t = dict(match=torch.full((nentries,), -1, **i32), dist=torch.full((nentries,), 256, **i32),
                 action=torch.zeros((nentries,), dtype=torch.uint8, device=device), other=torch.full((nentries,), -1, **i32),
                 nfused=torch.zeros((npairs,), **i32), first=torch.full((npairs, cap), -1, **i32) if first else None)
        return t, _ffi.FuseOut(_dp(t["match"]), _dp(t["dist"]), _dp(t["action"]), _dp(t["other"]), _dp(t["nfused"]), _dp(t["first"]))

    def FuseCandidates_device(self, d_slot_mp, d_n, nkf, cap, d_targets, ntargets, cur_kf, d_bad, npoints, d_cand, d_cand_skip, cand_cap,
                              d_ncand, stream=None):
        check(self._L.orbfe_fuse_candidates_device(self._mt._m, d_slot_mp, d_n, int(nkf), int(cap), d_targets, int(ntargets), int(cur_kf), d_bad,
                                                   int(npoints), d_cand, d_cand_skip, int(cand_cap), d_ncand, stream),
              "orbfe_fuse_candidates_device")

    def fuse_candidates_device(self, slot_mp, n, targets, bad, cur_kf=-1, cand_cap=None, stream=None):
        """vpFuseCandidates of SearchInNeighbors on torch tensors: slot_mp int32 [nkf][cap], n int32 [nkf], targets int32 [T] (keyframe
        rows), bad uint8 [npoints].  Allocates and returns (cand int32 [cand_cap], skip uint8 [cand_cap], ncand int32 [2] = written,
        full count) on the device of slot_mp; nothing is read back.  cand_cap defaults to min(T * cap, npoints), which always suffices."""
        import torch
        nkf, cap = int(slot_mp.shape[0]), int(slot_mp.shape[1])
        T, npoints, dev = int(targets.numel()), int(bad.numel()), slot_mp.device
        if cand_cap is None:
            cand_cap = max(min(T * cap, npoints), 1)
        cand = torch.full((cand_cap,), -1, dtype=torch.int32, device=dev)
        skip = torch.zeros((cand_cap,), dtype=torch.uint8, device=dev)
        ncand = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.FuseCandidates_device(_dp(slot_mp), _dp(n), nkf, cap, _dp(targets), T, cur_kf, _dp(bad), npoints, _dp(cand), _dp(skip), cand_cap,
                                   _dp(ncand), stream_arg(dev, stream))
        return cand, skip, ncand

    def fuse_device(self, kf, mps, th, mode=FUSE_PLAIN, Scw=None, th_low=TH_LOW):
        """One Fuse call on numpy data, for tests and tools: kf / mps in the dict layout of the test cases (kf: desc, xy, octave,
        uRight, state (0 none, 1 good, 2 bad), obs, Rcw, tcw, Ow, K = (fx, fy, cx, cy, mbf), bounds, gw_inv, gh_inv, scale_factors,
        inv_sigma2, log_scale; mps: null, bad, in_kf (optional), world_pos, normal, max_dist, min_dist, mpdesc, obs (optional)).  The map
        table is the list's points followed by the keyframe's own: the point of feature i has index len(mps) + i.  With
        FUSE_SIM3 the pose comes from Scw (4x4) through sim3_pose().  Uploads, runs grid -> Fuse_batch_device on torch's current
        stream, downloads: (match, dist, action, other, nfused)."""
        import torch
        from . import KP_DTYPE
        from .tracking import frames_struct
        f32, i32, u8 = np.float32, np.int32, np.uint8
        nKF, nmp = len(np.asarray(kf["octave"])), len(np.asarray(mps["bad"]))
        cap = max(nKF, 1)
        blk = np.zeros((1, cap), KP_DTYPE)
        blk["x"][0, :nKF], blk["y"][0, :nKF] = np.asarray(kf["xy"], f32).reshape(-1, 2).T if nKF else (0, 0)
        blk["octave"][0, :nKF] = np.asarray(kf["octave"], i32)
        desc = np.zeros((1, cap, 32), u8)
        desc[0, :nKF] = np.asarray(kf["desc"], u8).reshape(-1, 32)
        ur = np.full((1, cap), -1.0, f32)
        ur[0, :nKF] = np.asarray(kf["uRight"], f32)
        state = np.asarray(kf["state"], u8)
        slot = np.full((1, cap), -1, i32)
        slot[0, :nKF] = np.where(state > 0, nmp + np.arange(nKF), -1)
        if mode == FUSE_SIM3:
            Tcw, Ow = sim3_pose(Scw)
        else:
            Tcw = np.concatenate([np.asarray(kf["Rcw"], f32).reshape(3, 3), np.asarray(kf["tcw"], f32).reshape(3, 1)], 1).reshape(12)
            Ow = np.asarray(kf["Ow"], f32).reshape(3)
        npts = nmp + nKF

        def both(a, b, dt, width=None):
            shape = (npts,) if width is None else (npts, width)
            o = np.zeros(shape, dt)
            o[:nmp] = np.asarray(a, dt).reshape((nmp,) + shape[1:])
            if b is not None:
                o[nmp:] = b
            return o
        null = np.asarray(mps["null"], u8).astype(bool)
        skip = np.asarray(mps["in_kf"], u8) if (mode == FUSE_PLAIN and "in_kf" in mps) else np.zeros(nmp, u8)
        M = dict(wp=both(mps["world_pos"], None, f32, 3), nr=both(mps["normal"], None, f32, 3), mn=both(mps["min_dist"], None, f32),
                 mx=both(mps["max_dist"], None, f32), bad=both(mps["bad"], (state == 2).astype(u8), u8), d=both(mps["mpdesc"], None, u8, 32),
                 nobs=both(mps.get("obs", np.zeros(nmp, i32)), np.asarray(kf.get("obs", np.zeros(nKF, i32)), i32), i32))
        idx = np.where(null, -1, np.arange(nmp)).astype(i32)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d = {k: dev(v) for k, v in M.items()}
        d_kps, d_desc, d_n, d_ur, d_slot = dev(blk.view(u8).reshape(1, cap, -1)), dev(desc), dev(np.array([nKF], i32)), dev(ur), dev(slot)
        d_off, d_cidx, d_nin = (torch.zeros((1, 64 * 48 + 1), dtype=torch.int32, device="cuda"), torch.zeros((1, cap), dtype=torch.int32, device="cuda"),
                                torch.zeros((1,), dtype=torch.int32, device="cuda"))
        minx, maxx, miny, maxy = [float(v) for v in kf["bounds"]]
        st = stream_arg(None, None)
        self._mt.AssignFeaturesToGrid_batch_device(_dp(d_kps), _dp(d_n), cap, 1, minx, miny, float(kf["gw_inv"]), float(kf["gh_inv"]), _dp(d_off),
                                                   _dp(d_cidx), _dp(d_nin), st)
        frames = frames_struct(d_kps, d_desc, d_n, cap, d_off, d_cidx, minx, miny, kf["gw_inv"], kf["gh_inv"], d_uright=d_ur)
        fx, fy, cx, cy, mbf = [float(v) for v in kf["K"][:5]]
        cam = camera(fx, fy, cx, cy, mbf, minx, maxx, miny, maxy)
        tmap = _ffi.TrackMap(_dp(d["wp"]), _dp(d["nr"]), _dp(d["mn"]), _dp(d["mx"]), _dp(d["bad"]), None, _dp(d["d"]), npts)
        L = [dev(np.zeros(1, i32)), dev(Tcw.reshape(1, 12)), dev(Ow.reshape(1, 3)), dev(np.array([0, nmp], np.uint32).view(i32)), dev(idx), dev(skip)]
        lists = fuse_lists_struct(L[0], L[1], L[2], L[3], L[4], nmp, 1, L[5])
        t, out = self.alloc_fuse_out(max(nmp, 1), 1, cap)
        self.Fuse_batch_device(frames, 1, lists, cam, tmap, _dp(d["nobs"]), _dp(d_slot), th, kf["scale_factors"], kf["inv_sigma2"], kf["log_scale"],
                               out, mode, th_low, st)
        torch.cuda.synchronize()
        return (t["match"].cpu().numpy()[:nmp], t["dist"].cpu().numpy()[:nmp], t["action"].cpu().numpy()[:nmp], t["other"].cpu().numpy()[:nmp],
                int(t["nfused"][0].item()))
