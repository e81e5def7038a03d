"""The two ORBmatcher members LoopClosing::ComputeSim3 calls around Sim3Solver::iterate, batched and device-resident
(csrc/orbfe_sim3_search.hip; include/orbfe.h "SearchBySim3 and the loop's SearchByProjection, batched"):
SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) and SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) for a batch of
loop candidates, with the similarity poses computed on the device from the Sim3 solver's results in place, and
compute_sim3_round_device(): SearchByBoW -> Sim3 RANSAC -> SearchBySim3 for all candidates of a round on one stream.

The *_batch_device / *_device methods with device pointers are thin: ints and the structs of _ffi, asynchronous on `stream`.
search_by_sim3_device() / search_by_projection_sim3_device() and their *_pairs_* forms take numpy dicts in the layout of the
test cases, upload, run on torch's current stream and download.  sim3_pair_pose(), sim3_gate_points() and
sim3_search_scratch_bytes() need no GPU."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import check, ptr, stream_arg
from .mapping import sim3_pose
from .sim3 import RESULT_DTYPE
from .tracking import TH_HIGH, TH_LOW, camera, frames_struct

# byte offsets (s, R, t, found) of the two record layouts sim3_pair_poses_device reads
POSE_LAYOUT_RESULT = (RESULT_DTYPE.fields["model"][1] + RESULT_DTYPE["model"].fields["s"][1],
                      RESULT_DTYPE.fields["model"][1] + RESULT_DTYPE["model"].fields["R"][1],
                      RESULT_DTYPE.fields["model"][1] + RESULT_DTYPE["model"].fields["t"][1], RESULT_DTYPE.fields["found"][1])
POSE_LAYOUT_SRT = (0, 4, 40, -1)   # float32 [npairs][13] = s, R row-major, t; stride 52


def _dp(t):
    return None if t is None else t.data_ptr()


def sim3_pair_pose(s12, R12, t12):
    """(T12, T21) float32 [12] each = row-major (sR12 | t12), (sR21 | t21) in the reference's arithmetic (orbfe_sim3_pair_pose)"""
    R = np.ascontiguousarray(np.asarray(R12, np.float32).reshape(9))
    t = np.ascontiguousarray(np.asarray(t12, np.float32).reshape(3))
    T12, T21 = np.zeros(12, np.float32), np.zeros(12, np.float32)
    check(_ffi.lib().orbfe_sim3_pair_pose(float(np.float32(s12)), ptr(R), ptr(t), ptr(T12), ptr(T21)), "orbfe_sim3_pair_pose")
    return T12, T21


def sim3_gate_points(T_own, T_to_other, cam, th, scale_factors, log_scale_factor, world_pos, min_dist, max_dist):
    """the gating of SearchBySim3 for the points of one direction on the host (orbfe_sim3_gate_points, the function the gate kernel
    runs): (q PROJ_QUERY_DTYPE [n], level int32 [n], ok uint8 [n])"""
    To = np.ascontiguousarray(np.asarray(T_own, np.float32).reshape(-1)[:12])
    Tx = np.ascontiguousarray(np.asarray(T_to_other, np.float32).reshape(-1)[:12])
    sf = np.ascontiguousarray(scale_factors, np.float32)
    wp = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3)
    mn, mx = np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32)
    n = len(wp)
    q, level, ok = np.zeros(n, _ffi.PROJ_QUERY_DTYPE), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    check(_ffi.lib().orbfe_sim3_gate_points(ptr(To), ptr(Tx), C.byref(cam), float(th), ptr(sf), float(log_scale_factor), len(sf), n, ptr(wp),
                                            ptr(mn), ptr(mx), ptr(q), ptr(level), ptr(ok)), "orbfe_sim3_gate_points")
    return q, level, ok


def sim3_search_scratch_bytes(npairs, cap, qcap=0, nentries=0, ent_cap=0):
    """bytes of matcher scratch: qcap == 0 SearchBySim3_batch_device, qcap >= 1 SearchByProjectionSim3_batch_device; no GPU needed"""
    n = _ffi.lib().orbfe_sim3_search_scratch_bytes(int(npairs), int(cap), int(qcap), int(nentries), int(ent_cap))
    if n < 0:
        raise ValueError("outside the limits: 1 <= cap <= 15360, npairs * 2 * cap < 2^25, npairs * qcap < 2^25, nentries <= 2^25")
    return int(n)


def _keyframe_block(kfs, cap=None):
    """numpy arrays of an orbfe_track_frames block from keyframe dicts (desc, xy, octave): (kps [B][cap] KP_DTYPE, desc, n, cap)"""
    from . import KP_DTYPE
    B = len(kfs)
    ns = [len(np.asarray(k["octave"])) for k in kfs]
    cap = max(max(ns, default=0), 1) if cap is None else int(cap)
    blk, desc = np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap, 32), np.uint8)
    for r, (k, n) in enumerate(zip(kfs, ns)):
        if n:
            xy = np.asarray(k["xy"], np.float32).reshape(-1, 2)
            blk["x"][r, :n], blk["y"][r, :n] = xy[:, 0], xy[:, 1]
            blk["octave"][r, :n] = np.asarray(k["octave"], np.int32)
            desc[r, :n] = np.asarray(k["desc"], np.uint8).reshape(-1, 32)
    return blk, desc, np.array(ns, np.int32), cap


class LoopCloser:
    """The device-resident LoopClosing calls on a matcher's scratch: LoopCloser(ORBmatcher(...))"""

    sim3_pair_pose = staticmethod(sim3_pair_pose)
    sim3_gate_points = staticmethod(sim3_gate_points)
    sim3_search_scratch_bytes = staticmethod(sim3_search_scratch_bytes)
    sim3_pose = staticmethod(sim3_pose)

    def __init__(self, matcher):
        self._mt = matcher
        self._L = matcher._L

    # ---- raw forms: device pointers (ints) --------------------------------------------------------------------------------
    def sim3_pair_poses_device(self, d_src, stride, npairs, d_T12, d_T21, d_pair_skip=None, layout=POSE_LAYOUT_RESULT, stream=None):
        """orbfe_sim3_pair_poses_device: records of `stride` bytes at d_src with the byte offsets layout = (s, R, t, found or -1);
        POSE_LAYOUT_RESULT reads orbfe_sim3_result records in place, POSE_LAYOUT_SRT a float32 [npairs][13] array (stride 52)"""
        off_s, off_R, off_t, off_found = layout
        check(self._L.orbfe_sim3_pair_poses_device(self._mt._m, d_src, int(stride), int(off_s), int(off_R), int(off_t), int(off_found),
                                                   int(npairs), d_T12, d_T21, d_pair_skip, stream), "orbfe_sim3_pair_poses_device")

    def SearchBySim3_batch_device(self, frames, nkf, d_Tcw, d_slot_mp, tmap, cam, d_kf1, d_kf2, d_T12, d_T21, d_pair_skip, npairs, th,
                                  scale_factors, log_scale_factor, d_match12, d_nfound, d_match1=None, d_match2=None, th_high=TH_HIGH,
                                  stream=None):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(self._L.orbfe_search_by_sim3_batch_device(self._mt._m, C.byref(frames), int(nkf), d_Tcw, d_slot_mp, C.byref(tmap), C.byref(cam),
                                                        d_kf1, d_kf2, d_T12, d_T21, d_pair_skip, int(npairs), float(th), int(th_high), ptr(sf),
                                                        len(sf), float(log_scale_factor), d_match12, d_nfound, d_match1, d_match2, stream),
              "orbfe_search_by_sim3_batch_device")

    def mark_list_members_device(self, d_rows, nrows, cap, d_pair_row, d_list_off, d_list_idx, nentries, npairs, d_list_skip, stream=None):
        check(self._L.orbfe_mark_list_members_device(self._mt._m, d_rows, int(nrows), int(cap), d_pair_row, d_list_off, d_list_idx,
                                                     int(nentries), int(npairs), d_list_skip, stream), "orbfe_mark_list_members_device")

    def SearchByProjectionSim3_batch_device(self, frames, npairs, d_Tcw, d_Ow, cam, tmap, d_list_off, d_list_idx, d_list_skip, nentries, th,
                                            scale_factors, log_scale_factor, qcap, ent_cap, d_matched, d_nmatches, d_status, th_low=TH_LOW,
                                            stream=None):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        check(self._L.orbfe_search_by_projection_sim3_batch_device(self._mt._m, C.byref(frames), int(npairs), d_Tcw, d_Ow, C.byref(cam),
                                                                   C.byref(tmap), d_list_off, d_list_idx, d_list_skip, int(nentries), float(th),
                                                                   ptr(sf), len(sf), float(log_scale_factor), int(th_low), int(qcap),
                                                                   int(ent_cap), d_matched, d_nmatches, d_status, stream),
              "orbfe_search_by_projection_sim3_batch_device")

    def InvertMatches_device(self, d_bow_match, d_kf2, d_n, nkf, cap, npairs, d_match12, stream=None):
        check(self._L.orbfe_sim3_invert_matches_device(self._mt._m, d_bow_match, d_kf2, d_n, int(nkf), int(cap), int(npairs), d_match12, stream),
              "orbfe_sim3_invert_matches_device")

    def Sim3Correspondences_device(self, frames, nkf, d_Tcw, d_slot_mp, tmap, d_kf1, d_kf2, npairs, d_match12, level_sigma2, corr_cap, d_offsets,
                                   d_X1, d_X2, d_sigma2_1, d_sigma2_2, d_idx1, stream=None):
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        check(self._L.orbfe_sim3_correspondences_device(self._mt._m, C.byref(frames), int(nkf), d_Tcw, d_slot_mp, C.byref(tmap), d_kf1, d_kf2,
                                                        int(npairs), d_match12, ptr(s2), len(s2), int(corr_cap), d_offsets, d_X1, d_X2, d_sigma2_1,
                                                        d_sigma2_2, d_idx1, stream), "orbfe_sim3_correspondences_device")

    def KeepInliers_device(self, d_key_mask, cap, npairs, d_match12, stream=None):
        check(self._L.orbfe_sim3_keep_inliers_device(self._mt._m, d_key_mask, int(cap), int(npairs), d_match12, stream),
              "orbfe_sim3_keep_inliers_device")

    def compute_sim3_round_device(self, sim3, frames, nkf, n, Tcw, slot_mp, tmap, cam, bow, kf1, kf2, sets, draws, th, scale_factors, level_sigma2,
                                  log_scale_factor, th_high=TH_HIGH, th_low=TH_LOW):
        """One round of LoopClosing::ComputeSim3 up to SearchBySim3 for P candidates, enqueued on ONE stream -- torch's current
        stream, where the results are allocated and `sets` is uploaded too -- with no host read in between: SearchByBoW(KF, KF) -> vpMatches12 -> Sim3Solver's
        correspondences -> iterate -> the inliers of vpMatches12 -> the similarity poses -> SearchBySim3.  Torch tensors on one
        device: frames / tmap / cam as for SearchBySim3_batch_device with n int32 [nkf], Tcw float32 [nkf][12], slot_mp int32
        [nkf][cap]; bow = dict(kps, desc, valid, fv_node, fv_off, fv_idx, counts) as SearchByBoW_batch_device takes them; kf1 / kf2
        int32 [P]; sets a numpy sim3.SET_DTYPE array [P] (key_offset / n_keys are filled in here: p * cap, cap); draws int32 (the
        solver's draws are an input); sim3 a Sim3 handle with max_pairs >= cap and max_sets >= P.  -> dict of device tensors:
        match12 [P][cap] (vpMatches12 after SearchBySim3), nfound [P], result uint8 [P][...] (orbfe_sim3_result records), pair_skip,
        T12, T21, bow_match, nbow, offsets, idx1, key_mask."""
        import torch
        from .sim3 import SET_DTYPE, STATE_DTYPE
        dev, P, cap = kf1.device, int(kf1.numel()), int(frames.cap)
        st = stream_arg(dev, None)
        i32, u8, f32 = (dict(dtype=t, device=dev) for t in (torch.int32, torch.uint8, torch.float32))
        sets = np.ascontiguousarray(sets, SET_DTYPE).reshape(P).copy()
        sets["key_offset"], sets["n_keys"] = np.arange(P) * cap, cap
        d_sets = torch.from_numpy(sets.view(np.uint8).reshape(P, -1)).to(dev)
        corr_cap = max(P * cap, 1)
        r = dict(bow_match=torch.empty((P, cap), **i32), nbow=torch.empty((P,), **i32), match12=torch.empty((P, cap), **i32),
                 offsets=torch.empty((P + 1,), **i32), X1=torch.zeros((corr_cap, 3), **f32), X2=torch.zeros((corr_cap, 3), **f32),
                 sigma2_1=torch.zeros((corr_cap,), **f32), sigma2_2=torch.zeros((corr_cap,), **f32), idx1=torch.zeros((corr_cap,), **i32),
                 state=torch.zeros((P, STATE_DTYPE.itemsize), **u8), best_mask=torch.zeros((corr_cap,), **u8),
                 key_mask=torch.zeros((corr_cap,), **u8), T12=torch.empty((P, 12), **f32), T21=torch.empty((P, 12), **f32),
                 pair_skip=torch.empty((P,), **u8), nfound=torch.empty((P,), **i32))
        self._mt.SearchByBoW_batch_device(_dp(bow["kps"]), _dp(bow["desc"]), cap, _dp(bow["valid"]), _dp(bow["fv_node"]), _dp(bow["fv_off"]),
                                          _dp(bow["fv_idx"]), _dp(bow["counts"]), _dp(kf1), _dp(kf2), P, _dp(r["bow_match"]), _dp(r["nbow"]),
                                          kf_kf=True, th_low=th_low, stream=st)
        self.InvertMatches_device(_dp(r["bow_match"]), _dp(kf2), _dp(n), nkf, cap, P, _dp(r["match12"]), st)
        self.Sim3Correspondences_device(frames, nkf, _dp(Tcw), _dp(slot_mp), tmap, _dp(kf1), _dp(kf2), P, _dp(r["match12"]), level_sigma2, corr_cap,
                                        _dp(r["offsets"]), _dp(r["X1"]), _dp(r["X2"]), _dp(r["sigma2_1"]), _dp(r["sigma2_2"]), _dp(r["idx1"]), st)
        r["result"], r["mask"] = sim3.iterate_device(r["offsets"], r["X1"], r["X2"], r["sigma2_1"], r["sigma2_2"], d_sets, draws, r["state"],
                                                     r["best_mask"], idx1=r["idx1"], key_mask=r["key_mask"], stream=st.value)
        self.KeepInliers_device(_dp(r["key_mask"]), cap, P, _dp(r["match12"]), st)
        self.sim3_pair_poses_device(_dp(r["result"]), RESULT_DTYPE.itemsize, P, _dp(r["T12"]), _dp(r["T21"]), _dp(r["pair_skip"]),
                                    POSE_LAYOUT_RESULT, st)
        self.SearchBySim3_batch_device(frames, nkf, _dp(Tcw), _dp(slot_mp), tmap, cam, _dp(kf1), _dp(kf2), _dp(r["T12"]), _dp(r["T21"]),
                                       _dp(r["pair_skip"]), P, th, scale_factors, log_scale_factor, _dp(r["match12"]), _dp(r["nfound"]), None, None,
                                       th_high, st)
        r["sets"] = d_sets
        return r

    # ---- numpy forms, for tests and tools ---------------------------------------------------------------------------------
    def _upload_frames(self, kfs, cap, st):
        """keyframe dicts -> (frames struct, cam, tensors kept alive, cap); runs the grid on `st`"""
        import torch
        blk, desc, ns, cap = _keyframe_block(kfs, cap)
        B = len(kfs)
        k0 = kfs[0]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d_kps, d_desc, d_n = dev(blk.view(np.uint8).reshape(B, cap, -1)), dev(desc), dev(ns)
        i32 = dict(dtype=torch.int32, device="cuda")
        d_off, d_cidx, d_nin = torch.zeros((B, 64 * 48 + 1), **i32), torch.zeros((B, cap), **i32), torch.zeros((B,), **i32)
        minx, maxx, miny, maxy = [float(v) for v in k0["bounds"]]
        self._mt.AssignFeaturesToGrid_batch_device(_dp(d_kps), _dp(d_n), cap, B, minx, miny, float(k0["gw_inv"]), float(k0["gh_inv"]), _dp(d_off),
                                                   _dp(d_cidx), _dp(d_nin), st)
        frames = frames_struct(d_kps, d_desc, d_n, cap, d_off, d_cidx, minx, miny, k0["gw_inv"], k0["gh_inv"])
        fx, fy, cx, cy, mbf = [float(v) for v in k0["K"][:5]]
        return frames, camera(fx, fy, cx, cy, mbf, minx, maxx, miny, maxy), (d_kps, d_desc, d_n, d_off, d_cidx, d_nin), cap, ns

    def search_by_sim3_pairs_device(self, kfs, pairs, sims, th, matches_in, pair_skip=None, th_high=TH_HIGH, cap=None, poses_on_device=True,
                                    prepared=False):
        """SearchBySim3 for a batch on numpy data.  kfs: keyframe dicts in the layout of the test cases (desc, xy, octave, state (0
        none, 1 good, 2 bad), world_pos, max_dist, min_dist, mpdesc, Rcw, tcw, K, bounds, gw_inv, gh_inv, scale_factors, log_scale);
        pairs: (row1, row2) per pair (a row outside the block is allowed: that pair does nothing); sims: (s12, R12, t12) per pair;
        matches_in: one int array per pair in index form (-1, j, -2).  The map table is every keyframe's own points, keyframe r's
        feature i at index base[r] + i.  -> list of (matches_out [N1 or cap], nfound, vnMatch1 [cap], vnMatch2 [cap]) per pair.
        prepared=True: nothing runs; -> (reset, launch, fetch) callables for a timing loop (reset restores vpMatches12)."""
        import torch
        f32, i32, u8 = np.float32, np.int32, np.uint8
        st = stream_arg(None, None)
        frames, cam, keep, cap, ns = self._upload_frames(kfs, cap, st)
        B, P = len(kfs), len(pairs)
        base = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        npts = int(base[-1])
        slot = np.full((B, cap), -1, i32)
        Tcw = np.zeros((B, 12), f32)
        M = dict(wp=np.zeros((max(npts, 1), 3), f32), mn=np.zeros(max(npts, 1), f32), mx=np.zeros(max(npts, 1), f32), bad=np.zeros(max(npts, 1), u8),
                 d=np.zeros((max(npts, 1), 32), u8))
        for r, k in enumerate(kfs):
            n, b = int(ns[r]), int(base[r])
            state = np.asarray(k["state"], u8)
            slot[r, :n] = np.where(state > 0, b + np.arange(n), -1)
            Tcw[r] = np.concatenate([np.asarray(k["Rcw"], f32).reshape(3, 3), np.asarray(k["tcw"], f32).reshape(3, 1)], 1).reshape(12)
            if n:
                M["wp"][b:b + n], M["mn"][b:b + n], M["mx"][b:b + n] = np.asarray(k["world_pos"], f32).reshape(-1, 3), k["min_dist"], k["max_dist"]
                M["bad"][b:b + n], M["d"][b:b + n] = state == 2, np.asarray(k["mpdesc"], u8).reshape(-1, 32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d = {k: dev(v) for k, v in M.items()}
        tmap = _ffi.TrackMap(_dp(d["wp"]), None, _dp(d["mn"]), _dp(d["mx"]), _dp(d["bad"]), None, _dp(d["d"]), npts)
        m12 = np.full((max(P, 1), cap), -1, i32)
        for p, mi in enumerate(matches_in):
            mi = np.asarray(mi, i32).reshape(-1)
            m12[p, :len(mi)] = mi
        srt = np.zeros((max(P, 1), 13), f32)
        T12, T21 = np.zeros((max(P, 1), 12), f32), np.zeros((max(P, 1), 12), f32)
        for p, (s, R, t) in enumerate(sims):
            srt[p, 0], srt[p, 1:10], srt[p, 10:13] = f32(s), np.asarray(R, f32).reshape(9), np.asarray(t, f32).reshape(3)
            T12[p], T21[p] = sim3_pair_pose(s, R, t)
        pr = np.asarray(pairs, i32).reshape(-1, 2)
        d_k1, d_k2 = dev(pr[:, 0].copy() if P else np.zeros(1, i32)), dev(pr[:, 1].copy() if P else np.zeros(1, i32))
        d_m12, d_Tcw, d_slot, d_srt = dev(m12), dev(Tcw), dev(slot), dev(srt)
        d_T12, d_T21 = (torch.zeros((max(P, 1), 12), dtype=torch.float32, device="cuda") for _ in range(2)) if poses_on_device else (dev(T12), dev(T21))
        d_skip = None if pair_skip is None else dev(np.asarray(pair_skip, u8))
        if poses_on_device:
            self.sim3_pair_poses_device(_dp(d_srt), 52, P, _dp(d_T12), _dp(d_T21), None, POSE_LAYOUT_SRT, st)
        guard = 64   # a band behind every output that must stay as it was
        d_nf = torch.full((max(P, 1) + guard,), -77, dtype=torch.int32, device="cuda")
        d_v1, d_v2 = (torch.full((max(P, 1) * cap + guard,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
        k0 = kfs[0]
        d_m12_0 = d_m12.clone()

        def launch():
            self.SearchBySim3_batch_device(frames, B, _dp(d_Tcw), _dp(d_slot), tmap, cam, _dp(d_k1), _dp(d_k2), _dp(d_T12), _dp(d_T21), _dp(d_skip), P,
                                           th, k0["scale_factors"], k0["log_scale"], _dp(d_m12), _dp(d_nf), _dp(d_v1), _dp(d_v2), th_high, st)

        def fetch():
            torch.cuda.synchronize()
            nf, v1, v2, mo = d_nf.cpu().numpy(), d_v1.cpu().numpy(), d_v2.cpu().numpy(), d_m12.cpu().numpy()
            if not ((nf[P:] == -77).all() if P else True) or not (v1[max(P, 1) * cap:] == -77).all() or not (v2[max(P, 1) * cap:] == -77).all():
                raise AssertionError("SearchBySim3_batch_device wrote behind an output")
            out = []
            for p in range(P):
                n1 = int(ns[pr[p, 0]]) if 0 <= pr[p, 0] < B else cap
                out.append((mo[p, :n1].copy(), int(nf[p]), v1[p * cap:(p + 1) * cap].copy(), v2[p * cap:(p + 1) * cap].copy()))
            return out
        if prepared:
            return (lambda: d_m12.copy_(d_m12_0)), launch, (lambda: (keep, d, fetch())[2])
        launch()
        return fetch()

    def search_by_sim3_device(self, k1, k2, s12, R12, t12, th, matches_in, th_high=TH_HIGH, cap=None):
        """one SearchBySim3 call on numpy data (the layout of the test cases): -> (matches_out [N1], nfound)"""
        mo, nf, _, _ = self.search_by_sim3_pairs_device([k1, k2], [(0, 1)], [(s12, R12, t12)], th, [matches_in], th_high=th_high, cap=cap)[0]
        return mo, nf

    def search_by_projection_sim3_pairs_device(self, cases, th, th_low=TH_LOW, cap=None, list_skip="device", ent_cap=None, qcap=None,
                                               prepared=False):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) for a batch on numpy data.  cases: (kf, Scw, pts, matched_in) per pair
        in the layout of the test cases (pts: bad, world_pos, normal, max_dist, min_dist, mpdesc; matched_in [nKF]: -1, k >= 0 = point k
        of the pair's list, -2 another point).  The map table is the lists one after the other.  list_skip: "device"
        (mark_list_members_device inside the call), "members" (the helper called on its own and its bytes supplied) or "host" (computed
        with numpy and supplied).  -> (list of (matched_out [nKF], nmatches) per pair, status int32 [2]).  prepared=True: nothing runs;
        -> (reset, launch, fetch) callables for a timing loop (reset restores vpMatched)."""
        import torch
        f32, i32, u8 = np.float32, np.int32, np.uint8
        st = stream_arg(None, None)
        kfs = [c[0] for c in cases]
        frames, cam, keep, cap, ns = self._upload_frames(kfs, cap, st)
        P = len(cases)
        nl = [len(np.asarray(c[2]["bad"])) for c in cases]
        base = np.concatenate([[0], np.cumsum(nl)]).astype(np.int64)
        npts = int(base[-1])
        cat = lambda key, dt, w=None: (np.concatenate([np.asarray(c[2][key], dt).reshape((-1,) if w is None else (-1, w)) for c in cases])   # noqa: E731
                                       if npts else np.zeros((1,) if w is None else (1, w), dt))
        M = dict(wp=cat("world_pos", f32, 3), nr=cat("normal", f32, 3), mn=cat("min_dist", f32), mx=cat("max_dist", f32), bad=cat("bad", u8),
                 d=cat("mpdesc", u8, 32))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d = {k: dev(v) for k, v in M.items()}
        tmap = _ffi.TrackMap(_dp(d["wp"]), _dp(d["nr"]), _dp(d["mn"]), _dp(d["mx"]), _dp(d["bad"]), None, _dp(d["d"]), npts)
        Tcw, Ow = np.zeros((P, 12), f32), np.zeros((P, 3), f32)
        guard = 64
        matched = np.full(P * cap + guard, -77, i32)
        for p, c in enumerate(cases):
            Tcw[p], Ow[p] = sim3_pose(c[1])
            mi = np.asarray(c[3], i32).reshape(-1)
            row = np.full(cap, -1, i32)
            row[:len(mi)] = np.where(mi >= 0, mi + base[p], mi)
            matched[p * cap:(p + 1) * cap] = row
        off = base.astype(np.uint32)
        idx = np.arange(max(npts, 1), dtype=i32)
        d_off, d_idx, d_Tcw, d_Ow, d_matched = dev(off.view(i32)), dev(idx), dev(Tcw), dev(Ow), dev(matched)
        d_skip = None
        if list_skip == "host":
            rows = matched[:P * cap].reshape(P, cap)
            d_skip = dev(np.concatenate([np.isin(np.arange(base[p], base[p + 1]), rows[p][rows[p] >= 0]) for p in range(P)]).astype(u8)
                         if npts else np.zeros(1, u8))
        elif list_skip == "members":
            d_skip = torch.full((max(npts, 1),), 7, dtype=torch.uint8, device="cuda")
            self.mark_list_members_device(_dp(d_matched), P, cap, None, _dp(d_off), _dp(d_idx), npts, P, _dp(d_skip), st)
        qcap = max(max(nl, default=0), 1) if qcap is None else int(qcap)
        ent_cap = max(npts, 1) * 64 if ent_cap is None else int(ent_cap)
        d_nm = torch.full((P + guard,), -77, dtype=torch.int32, device="cuda")
        d_status = torch.full((2 + guard,), -77, dtype=torch.int32, device="cuda")
        k0 = kfs[0]
        d_matched_0 = d_matched.clone()

        def launch():
            self.SearchByProjectionSim3_batch_device(frames, P, _dp(d_Tcw), _dp(d_Ow), cam, tmap, _dp(d_off), _dp(d_idx), _dp(d_skip), npts, th,
                                                     k0["scale_factors"], k0["log_scale"], qcap, ent_cap, _dp(d_matched), _dp(d_nm), _dp(d_status),
                                                     th_low, st)

        def fetch():
            torch.cuda.synchronize()
            mo, nm, status = d_matched.cpu().numpy(), d_nm.cpu().numpy(), d_status.cpu().numpy()
            if not ((mo[P * cap:] == -77).all() and (nm[P:] == -77).all() and (status[2:] == -77).all()):
                raise AssertionError("SearchByProjectionSim3_batch_device wrote behind an output")
            out = []
            for p in range(P):
                row = mo[p * cap:p * cap + int(ns[p])]
                out.append((np.where(row >= 0, row - base[p], row).astype(i32), int(nm[p])))
            return out, status[:2].copy()
        if prepared:
            return (lambda: d_matched.copy_(d_matched_0)), launch, (lambda: (keep, d, fetch())[2])
        launch()
        return fetch()

    def search_by_projection_sim3_device(self, kf, Scw, pts, matched_in, th, th_low=TH_LOW, cap=None, list_skip="device", ent_cap=None):
        """one call on numpy data (the layout of the test cases): -> (matched_out [nKF], nmatches); grows the entry buffer once if needed"""
        out, status = self.search_by_projection_sim3_pairs_device([(kf, Scw, pts, matched_in)], th, th_low, cap, list_skip, ent_cap)
        if status[0] > 0:
            out, status = self.search_by_projection_sim3_pairs_device([(kf, Scw, pts, matched_in)], th, th_low, cap, list_skip, int(status[0]))
        return out[0]
