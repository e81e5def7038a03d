"""What tests/test_gpu_sim3_search.py and tests/test_gpu_sim3_search_edges.py share: the single-pair comparisons of the device calls
with tests/sim3_search_oracle.py and, where oracle/_ref is built, with the compiled reference, and two raw harnesses around
LoopCloser's pointer forms for inputs its numpy forms cannot express (slot tables, counts and list indices out of range, a point
twice in a list, qcap below the live count).  Every output starts as a sentinel with a guard band behind it.  Test support only."""
import numpy as np

import sim3_search_oracle as SO
from oracle import ref_ffi as R

F = np.float32
HAVE_REF = R.available()
GUARD, SENT = 64, -77


def poses(s12, R12, t12):
    from orb_slam2_ssd_semantic_amd import loopclosing
    T12, T21 = loopclosing.sim3_pair_pose(s12, R12, t12)
    return T12.reshape(3, 4), T21.reshape(3, 4)


def oracle_sim3(k1, k2, sim, th, m_in, th_high=100):
    T12, T21 = poses(*sim)
    return SO.search_by_sim3(k1, k2, T12, T21, th, m_in, th_high)


def pad(v, cap):
    out = np.full(cap, -1, np.int32)
    out[:len(v)] = v
    return out


def check_sim3_single(lc, k1, k2, sim, m_in, cap=None, th=7.5, th_high=100, ref=True):
    mo, nf, v1, v2 = lc.search_by_sim3_pairs_device([k1, k2], [(0, 1)], [sim], th, [m_in], th_high=th_high, cap=cap)[0]
    wo, wn, w1, w2 = oracle_sim3(k1, k2, sim, th, m_in, th_high)
    assert np.array_equal(v1, pad(w1, len(v1))) and np.array_equal(v2, pad(w2, len(v2)))
    assert np.array_equal(mo, wo) and nf == wn
    if ref and HAVE_REF and th_high == 100:
        ro, rv = R.search_by_sim3(k1, k2, *sim, th, m_in)
        assert np.array_equal(mo, ro[:len(mo)]) and nf == rv
    return mo, nf, v1, v2


def check_proj(lc, kf, Scw, pts, m_in, cap=None, th=10, th_low=50, list_skip="device"):
    got, nm = lc.search_by_projection_sim3_device(kf, Scw, pts, m_in, th, th_low, cap, list_skip)
    want, wn = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, th, th_low)
    assert np.array_equal(got, want) and nm == wn
    if HAVE_REF and th_low == 50:
        ro, rv = R.search_by_projection_kf_sim3(kf, Scw, pts, m_in, th)
        assert np.array_equal(got, ro) and nm == rv
    return got, nm


def _dp(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sim3_raw(lc, kfs, pairs, sims, rows_in, cap, th=7.5, th_high=100, slot_edit=None, n_device=None, pair_skip=None, T_zero=(), stream=None,
             npoints=None):
    """SearchBySim3_batch_device on keyframe dicts with the tables in the caller's hands.  The map is every keyframe's own points,
    keyframe r's feature i at index base[r] + i.  rows_in: one int array per pair, up to cap long (vpMatches12; -1 behind it);
    slot_edit(slot [B][cap], base) may rewrite the slot table; n_device replaces d_n AFTER the grid was built from the true
    counts; T_zero: pairs whose two poses are all zero; npoints: the map's size as the call is told it.  stream: a torch stream
    (everything is enqueued there, nothing is synchronised) or None (the current one).
    -> fetch(): (match12 [P][cap], nfound [P], vnMatch1 [P][cap], vnMatch2 [P][cap]) after a synchronize."""
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi, loopclosing
    f32, i32, u8 = np.float32, np.int32, np.uint8
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        st = _ffi.stream_arg(None, None)
        frames, cam, keep, cap, ns = lc._upload_frames(kfs, cap, st)
        B, P = len(kfs), len(pairs)
        base = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        npts = int(base[-1])
        slot, Tcw = np.full((B, cap), -1, i32), np.zeros((B, 12), f32)
        M = dict(wp=np.zeros((max(npts, 1), 3), f32), mn=np.zeros(max(npts, 1), f32), mx=np.zeros(max(npts, 1), f32), bad=np.zeros(max(npts, 1), u8),
                 d=np.zeros((max(npts, 1), 32), u8))
        for r, k in enumerate(kfs):
            n, b = int(ns[r]), int(base[r])
            state = np.asarray(k["state"], u8)
            slot[r, :n] = np.where(state > 0, b + np.arange(n), -1)
            Tcw[r] = SO.pose34(k).reshape(12)
            if n:
                M["wp"][b:b + n], M["mn"][b:b + n], M["mx"][b:b + n] = np.asarray(k["world_pos"], f32).reshape(-1, 3), k["min_dist"], k["max_dist"]
                M["bad"][b:b + n], M["d"][b:b + n] = state == 2, np.asarray(k["mpdesc"], u8).reshape(-1, 32)
        if slot_edit is not None:
            slot_edit(slot, base)
        d = {k: _dev(v) for k, v in M.items()}
        tmap = _ffi.TrackMap(_dp(d["wp"]), None, _dp(d["mn"]), _dp(d["mx"]), _dp(d["bad"]), None, _dp(d["d"]), npts if npoints is None else int(npoints))
        m12 = np.full((P, cap), -1, i32)
        T12, T21 = np.zeros((P, 12), f32), np.zeros((P, 12), f32)
        for p in range(P):
            mi = np.asarray(rows_in[p], i32).reshape(-1)
            m12[p, :len(mi)] = mi
            if p not in T_zero:
                T12[p], T21[p] = loopclosing.sim3_pair_pose(*sims[p])
        pr = np.asarray(pairs, i32).reshape(-1, 2)
        d_k1, d_k2, d_m12, d_Tcw, d_slot, d_T12, d_T21 = (_dev(a) for a in (pr[:, 0].copy(), pr[:, 1].copy(), m12, Tcw, slot, T12, T21))
        d_skip = None if pair_skip is None else _dev(np.asarray(pair_skip, u8))
        if n_device is not None:
            keep[2].copy_(_dev(np.asarray(n_device, i32)))
        d_nf = torch.full((P + GUARD,), SENT, dtype=torch.int32, device="cuda")
        d_v1, d_v2 = (torch.full((P * cap + GUARD,), SENT, dtype=torch.int32, device="cuda") for _ in range(2))
        d_m12g = torch.full((P * cap + GUARD,), SENT, dtype=torch.int32, device="cuda")
        d_m12g[:P * cap] = d_m12.reshape(-1)
        k0 = kfs[0]
        lc.SearchBySim3_batch_device(frames, B, _dp(d_Tcw), _dp(d_slot), tmap, cam, _dp(d_k1), _dp(d_k2), _dp(d_T12), _dp(d_T21), _dp(d_skip), P, th,
                                     k0["scale_factors"], k0["log_scale"], _dp(d_m12g), _dp(d_nf), _dp(d_v1), _dp(d_v2), th_high, st)
    alive = (keep, d, frames, d_k1, d_k2, d_Tcw, d_slot, d_T12, d_T21, d_skip)

    def fetch(_alive=alive):
        torch.cuda.synchronize()
        nf, v1, v2, mo = (t.cpu().numpy() for t in (d_nf, d_v1, d_v2, d_m12g))
        assert (nf[P:] == SENT).all() and (v1[P * cap:] == SENT).all() and (v2[P * cap:] == SENT).all() and (mo[P * cap:] == SENT).all(), \
            "SearchBySim3_batch_device wrote behind an output"
        return mo[:P * cap].reshape(P, cap).copy(), nf[:P].copy(), v1[:P * cap].reshape(P, cap).copy(), v2[:P * cap].reshape(P, cap).copy()
    return fetch


def proj_raw(lc, kfs, Scws, pts, lists, rows_in, cap, th=10, th_low=50, qcap=None, ent_cap=None, list_skip=None, stream=None, list_off=None,
             nentries=None):
    """SearchByProjectionSim3_batch_device with the lists in the caller's hands.  pts: ONE map table (the dict of the test cases);
    lists: one int array of map indices per pair (any value, any repetition); rows_in: vpMatched per pair in MAP indices (-1 NULL,
    anything else occupied), up to cap long; list_skip None (marked inside the call) or a uint8 array over the entries; list_off /
    nentries replace the CSR offsets and the entry count the call is told.
    -> fetch(): (matched [P][cap], nmatches [P], status [2]) after a synchronize."""
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi
    from orb_slam2_ssd_semantic_amd.mapping import sim3_pose
    f32, i32, u8 = np.float32, np.int32, np.uint8
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        st = _ffi.stream_arg(None, None)
        frames, cam, keep, cap, ns = lc._upload_frames(kfs, cap, st)
        P = len(kfs)
        npts = len(np.asarray(pts["bad"]))
        M = dict(wp=np.asarray(pts["world_pos"], f32).reshape(-1, 3), nr=np.asarray(pts["normal"], f32).reshape(-1, 3), mn=np.asarray(pts["min_dist"], f32),
                 mx=np.asarray(pts["max_dist"], f32), bad=np.asarray(pts["bad"], u8), d=np.asarray(pts["mpdesc"], u8).reshape(-1, 32))
        if npts == 0:
            M = dict(wp=np.zeros((1, 3), f32), nr=np.zeros((1, 3), f32), mn=np.zeros(1, f32), mx=np.zeros(1, f32), bad=np.zeros(1, u8), d=np.zeros((1, 32), u8))
        d = {k: _dev(v) for k, v in M.items()}
        tmap = _ffi.TrackMap(_dp(d["wp"]), _dp(d["nr"]), _dp(d["mn"]), _dp(d["mx"]), _dp(d["bad"]), None, _dp(d["d"]), npts)
        Tcw, Ow = np.zeros((P, 12), f32), np.zeros((P, 3), f32)
        matched = np.full(P * cap + GUARD, SENT, i32)
        for p in range(P):
            Tcw[p], Ow[p] = sim3_pose(Scws[p])
            row = np.full(cap, -1, i32)
            mi = np.asarray(rows_in[p], i32).reshape(-1)
            row[:len(mi)] = mi
            matched[p * cap:(p + 1) * cap] = row
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32) if list_off is None else np.asarray(list_off, np.uint32)
        idx = np.concatenate([np.asarray(x, i32).reshape(-1) for x in lists] + [np.zeros(1, i32)])
        ne = len(idx) - 1 if nentries is None else int(nentries)
        d_off, d_idx, d_Tcw, d_Ow, d_matched = _dev(off.view(i32)), _dev(idx), _dev(Tcw), _dev(Ow), _dev(matched)
        d_skip = None if list_skip is None else _dev(np.concatenate([np.asarray(list_skip, u8), np.zeros(1, u8)]))
        qcap = max(max((len(x) for x in lists), default=0), 1) if qcap is None else int(qcap)
        ent_cap = max(ne, 1) * 64 if ent_cap is None else int(ent_cap)
        d_nm = torch.full((P + GUARD,), SENT, dtype=torch.int32, device="cuda")
        d_status = torch.full((2 + GUARD,), SENT, dtype=torch.int32, device="cuda")
        k0 = kfs[0]
        lc.SearchByProjectionSim3_batch_device(frames, P, _dp(d_Tcw), _dp(d_Ow), cam, tmap, _dp(d_off), _dp(d_idx), _dp(d_skip), ne, th,
                                               k0["scale_factors"], k0["log_scale"], qcap, ent_cap, _dp(d_matched), _dp(d_nm), _dp(d_status), th_low, st)
    alive = (keep, d, frames, d_off, d_idx, d_Tcw, d_Ow, d_skip)

    def fetch(_alive=alive):
        torch.cuda.synchronize()
        mo, nm, status = d_matched.cpu().numpy(), d_nm.cpu().numpy(), d_status.cpu().numpy()
        assert (mo[P * cap:] == SENT).all() and (nm[P:] == SENT).all() and (status[2:] == SENT).all(), \
            "SearchByProjectionSim3_batch_device wrote behind an output"
        return mo[:P * cap].reshape(P, cap).copy(), nm[:P].copy(), status[:2].copy()
    return fetch


def proj_lists_oracle(kf, Scw, pts, lst, row_in, th=10, th_low=50, qcap=None):
    """the oracle for one pair of proj_raw: entries outside the map make no query, a point twice in a list is one MapPoint, and with
    qcap every live entry (gated in) after the qcap-th is skipped.  -> (row_out in map indices [len(row_in)], nmatches)"""
    lst = np.asarray(lst, np.int64).reshape(-1)
    n = len(np.asarray(pts["bad"]))
    inside = (lst >= 0) & (lst < n)
    safe = np.where(inside, lst, 0)
    sub = {k: np.asarray(pts[k])[safe] for k in ("bad", "world_pos", "normal", "max_dist", "min_dist", "mpdesc")}
    row = np.asarray(row_in, np.int32)
    found = set(int(v) for v in row if v >= 0)
    skip = np.array([not inside[e] or int(lst[e]) in found for e in range(len(lst))], bool)
    if qcap is not None:
        import fuse_oracle as FO
        T, Ow = FO.decompose_sim3(Scw)
        live = 0
        for e in range(len(lst)):
            if skip[e] or sub["bad"][e]:
                continue
            g = FO.gate_point(T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], sub["world_pos"][e], sub["normal"][e], sub["min_dist"][e],
                              sub["max_dist"][e], False)
            if g is None:
                continue
            live += 1
            if live > qcap:
                skip[e] = True
    return SO.search_by_projection_kf_sim3(kf, Scw, sub, row, th, th_low, list_skip=skip, ids=safe)
