"""The device-resident tracker (csrc/orbfe_track.hip) bit for bit against the CPU oracles: the last-frame gating and its
order-preserving compaction, the batched search core on every planted case of tests/proj_edge_cases.py, the two chains end
to end, UnprojectStereo with UpdateLastFrame's selection, and PredictScale on the device.  No tolerances.

One call of the batched core has ONE grid geometry, th, nnratio, ratio rule and sigma table, so the planted calls are grouped
by those (the two image bounds of the window cases, the thresholds of the decision cases ...) and every group runs as one batch
whose frames differ in nF, nq and chain length; th and mono are per call in the chains for the same reason."""
import functools

import numpy as np
import pytest

import proj_cases as PC
import proj_edge_cases as E
import track_oracle as TO
from oracle import oracle_ffi as O

pytestmark = pytest.mark.gpu

F = np.float32
NC = E.COLS * E.ROWS
GUARD = 64          # sentinel elements behind every output buffer
SENT = -7
CORE_TABLES = ["WINDOW_CASES", "DECISION_CASES", "GATE_CASES", "ROUND_CASES", "SLAB_CASES"]


@pytest.fixture(scope="module")
def trk():
    from orb_slam2_ssd_semantic_amd import ORBmatcher, Tracker
    m = ORBmatcher(0.9, True)
    yield Tracker(m)
    m.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _guarded(shape, dtype=None, fill=SENT):
    """a flat device tensor of prod(shape) elements plus GUARD sentinels behind them"""
    import torch
    n = int(np.prod(shape))
    return torch.full((n + GUARD,), fill, dtype=dtype or torch.int32, device="cuda")


def _body(t, shape):
    n = int(np.prod(shape))
    a = t.cpu().numpy()
    assert (a[n:] == SENT).all(), "guard band overwritten"
    return a[:n].reshape(shape)


def _sync():
    import torch
    torch.cuda.synchronize()


class Frames:
    """a batch of current frames on the device: keypoint records, descriptors, counts, uRight, slot state and the grid that
    orbfe_assign_grid_batch_device builds for them"""

    def __init__(self, trk, frames, bounds4, cap=None):
        from orb_slam2_ssd_semantic_amd import KP_DTYPE, tracking
        B = len(frames)
        nmax = max(max(len(f["xy"]) for f in frames), 1)
        self.cap = cap = cap or (nmax + 3 if nmax + 3 <= E.PJ_MAX_NF else nmax)   # three spare rows unless the frame is the largest allowed
        blk = np.zeros((B, cap), KP_DTYPE)
        blk["x"], blk["y"], blk["octave"] = 100.0, 100.0, 3   # rows past a frame's count would land in a cell if they were read
        desc = np.full((B, cap, 32), 0xA5, np.uint8)
        ur = np.full((B, cap), -1.0, F)
        slot = np.zeros((B, cap), np.uint8)
        for f, fr in enumerate(frames):
            n = len(fr["xy"])
            blk["x"][f, :n], blk["y"][f, :n], blk["octave"][f, :n] = fr["xy"][:, 0], fr["xy"][:, 1], fr["octave"]
            if "angle" in fr:
                blk["angle"][f, :n] = fr["angle"]
            desc[f, :n] = fr["desc"]
            if fr.get("uRight") is not None:
                ur[f, :n] = fr["uRight"]
            if fr.get("slot") is not None:
                slot[f, :n] = fr["slot"]
        self.n = np.array([len(f["xy"]) for f in frames], np.int32)
        self.t = dict(kps=_dev(blk.view(np.int32).reshape(B, cap, 7)), desc=_dev(desc), n=_dev(self.n), ur=_dev(ur), slot=_dev(slot))
        import torch
        self.t["off"] = torch.zeros((B, NC + 1), dtype=torch.int32, device="cuda")
        self.t["idx"] = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        self.t["nin"] = torch.zeros((B,), dtype=torch.int32, device="cuda")
        g = [float(v) for v in bounds4]
        trk._mt.AssignFeaturesToGrid_batch_device(self.t["kps"].data_ptr(), self.t["n"].data_ptr(), cap, B, *g, self.t["off"].data_ptr(),
                                                  self.t["idx"].data_ptr(), self.t["nin"].data_ptr(), None)
        self.struct = tracking.frames_struct(self.t["kps"], self.t["desc"], self.t["n"], cap, self.t["off"], self.t["idx"], *g,
                                             d_uright=self.t["ur"], d_slot=self.t["slot"])


def _cur_frame(cur):
    return dict(xy=cur["xy"], octave=cur["octave"], angle=cur["angle"], desc=cur["desc"], uRight=cur["uRight"], slot=cur["state"])


def _grid4(cur):
    minx, _, miny, _ = cur["bounds"]
    return (minx, miny, cur["gw_inv"], cur["gh_inv"])


def _cam(cur):
    from orb_slam2_ssd_semantic_amd import tracking
    fx, fy, cx, cy, bf, _ = cur["K"]
    return tracking.camera(fx, fy, cx, cy, bf, *cur["bounds"])


def _poses(Ts):
    return _dev(np.stack([np.asarray(T, F)[:3, :4].reshape(12) for T in Ts]))


# ------------------------------------------------------------------------------------------------ gating compaction
class Last:
    """a batch of last frames on the device (orbfe_track_last)"""

    def __init__(self, lasts, cap):
        from orb_slam2_ssd_semantic_amd import KP_DTYPE, _ffi
        B = len(lasts)
        self.cap = cap
        blk = np.zeros((B, cap), KP_DTYPE)
        blk["octave"] = 2
        valid, obs = np.ones((B, cap), np.uint8), np.ones((B, cap), np.uint8)   # rows past the count would make queries if read
        wp = np.zeros((B, cap, 3), F)
        wp[:, :, 2] = 2.0
        mpdesc = np.full((B, cap, 32), 0x5A, np.uint8)
        for f, la in enumerate(lasts):
            n = len(la["octave"])
            blk["octave"][f, :n], blk["angle"][f, :n] = la["octave"], la["angle"]
            blk["x"][f, :n], blk["y"][f, :n] = la["xy"][:, 0], la["xy"][:, 1]
            valid[f, :n] = la["has_mp"].astype(bool) & ~la["outlier"].astype(bool)
            obs[f, :n], wp[f, :n], mpdesc[f, :n] = la["obs_gt0"], la["world_pos"], la["mpdesc"]
        self.n = np.array([len(la["octave"]) for la in lasts], np.int32)
        self.t = dict(kps=_dev(blk.view(np.int32).reshape(B, cap, 7)), n=_dev(self.n), valid=_dev(valid), wp=_dev(wp), obs=_dev(obs),
                      mpdesc=_dev(mpdesc), Tcw=_poses([la["Tcw"] for la in lasts]))
        t = self.t
        self.struct = _ffi.TrackLast(t["kps"].data_ptr(), t["n"].data_ptr(), cap, t["valid"].data_ptr(), t["wp"].data_ptr(), t["obs"].data_ptr(),
                                     t["mpdesc"].data_ptr(), t["Tcw"].data_ptr())


GATE_N = (0, 1, 63, 64, 65, 255, 256, 257, 300)
GATE_CAP = 300


@functools.lru_cache(maxsize=None)
def _gate_cases():
    """frames with n in GATE_N x valid rates 0, 1, ~0.5, the motion cycling through small / forward / backward"""
    rng = np.random.default_rng(2024)
    out = []
    for k, n in enumerate(GATE_N):
        for j, rate in enumerate((0.0, 1.0, 0.5)):
            cur, last = PC.last_frame_case(rng, 64, n, ("small", "forward", "backward")[(k + j) % 3])
            last["has_mp"] = (rng.random(n) < rate).astype(np.uint8) if rate == 0.5 else np.full(n, int(rate), np.uint8)
            last["outlier"] = (rng.random(n) < 0.1).astype(np.uint8) if rate == 0.5 else np.zeros(n, np.uint8)
            out.append((cur, last))
    return out


@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_gating_compaction_equals_oracle(trk, mono):
    cases = _gate_cases()
    B, th = len(cases), 7.0 if mono else 15.0
    cur0 = cases[0][0]
    last = Last([la for _, la in cases], GATE_CAP)
    qcap = GATE_CAP
    d_q, d_src, d_nq = _guarded((B, qcap, 8)), _guarded((B, qcap)), _guarded((B,))
    d_T = _poses([c["Tcw"] for c, _ in cases])
    trk.GateLastFrame_batch_device(d_T.data_ptr(), last.struct, _cam(cur0), cur0["K"][5], mono, th,
                                   cur0["scale_factors"], B, d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap)
    _sync()
    q, src, nq = _body(d_q, (B, qcap, 8)), _body(d_src, (B, qcap)), _body(d_nq, (B,))
    windows = set()
    for f, (cur, la) in enumerate(cases):
        wq, wv = O.proj_queries_last_frame(cur["Tcw"], la["Tcw"], cur["K"], cur["bounds"], cur["scale_factors"], la["has_mp"], la["outlier"],
                                           la["world_pos"], la["octave"], la["obs_gt0"], th, mono)
        sel = np.flatnonzero(wv)
        assert nq[f] == len(sel), (f, nq[f], len(sel))
        assert np.array_equal(src[f, :nq[f]], sel), f
        assert q[f, :nq[f]].tobytes() == wq[sel].tobytes(), f
        assert (q[f, nq[f]:] == SENT).all() and (src[f, nq[f]:] == SENT).all(), f
        if len(sel):
            d = int(wq["max_level"][sel[0]]) - int(wq["min_level"][sel[0]])
            windows.add("fwd" if wq["max_level"][sel[0]] == -1 else "bwd" if wq["min_level"][sel[0]] == 0 and d != 2 else "small")
    assert windows == ({"small"} if mono else {"small", "fwd", "bwd"}), windows


# ------------------------------------------------------------------------------------------------ the search core
@functools.lru_cache(maxsize=None)
def _core_groups():
    """every planted call of the core tables plus an nq = 0 and an nF = 0 frame, grouped by what one batched call shares:
    (grid geometry, th, nnratio, rule, sigma table) -> [(name, call, (match, best, second), need)]"""
    groups = {}

    def add(name, c):
        key = (tuple(float(v) for v in c["ci"]["bounds"]), c["th"], float(c["nnratio"]), int(c["rule"]),
               None if c["is2"] is None else tuple(float(v) for v in c["is2"]))
        want = E.run_core(O.search_by_projection, c)
        need = sum(len(E.oracle_area(c, i)) for i in range(len(c["q"])))
        groups.setdefault(key, []).append((name, c, want, need))
    for table in CORE_TABLES:
        for name, build in E.TABLES[table].items():
            for k, c in enumerate(build()["calls"]):
                if not c.get("wd_only"):
                    add("%s[%d]" % (name, k), c)
    base = E.SLAB_CASES["queries_5"]()["calls"][0]
    empty_q = dict(base, q=base["q"][:0], qd=base["qd"][:0])
    cur0 = E.frame(np.zeros((0, 2), F), E.ORIGIN)
    empty_f = E.call(cur0, base["q"][:3], base["qd"][:3], th=base["th"], nnratio=base["nnratio"], rule=base["rule"])
    add("nq=0", empty_q)
    add("nF=0", empty_f)
    return groups


def _run_core_batch(trk, key, members, ent_cap, free_slot=0):
    """one batched call over `members`; returns per member (match, best, second) and the status.  A blocked slot is planted as
    state 2 (a MapPoint with observations), a free one as `free_slot`: 0 (empty) or 1 (a MapPoint without observations)"""
    bounds4, th, nnratio, rule, is2 = key
    frames = []
    for _, c, _, _ in members:
        ci = c["ci"]
        frames.append(dict(xy=ci["xyF"], octave=ci["octF"], desc=ci["descF"], uRight=ci["uRight"],
                           slot=None if ci["blocked"] is None else free_slot + (2 - free_slot) * ci["blocked"]))
    fr = Frames(trk, frames, bounds4)
    B = len(members)
    qcap = max(max(len(c["q"]) for _, c, _, _ in members), 1) + 2
    q = np.zeros((B, qcap), O.PROJ_QUERY_DTYPE)
    q["r"], q["u"], q["v"] = 50.0, 100.0, 100.0    # lanes beyond nq would find candidates if they ran
    pool = np.full((B, qcap, 32), 0x3C, np.uint8)
    src = np.zeros((B, qcap), np.int32)
    for f, (_, c, _, _) in enumerate(members):
        n = len(c["q"])
        perm = np.random.default_rng(f).permutation(n)          # the pool is NOT in query order: descriptors are gathered
        q[f, :n], src[f, :n] = c["q"], perm
        pool[f, perm] = c["qd"]
    d_q, d_src, d_pool = _dev(q.view(np.int32).reshape(B, qcap, 8)), _dev(src), _dev(pool)
    d_nq = _dev(np.array([len(c["q"]) for _, c, _, _ in members], np.int32))
    out = [_guarded((B, qcap)) for _ in range(3)]
    d_status = _guarded((2,))
    trk.SearchByProjection_batch_device(fr.struct, B, d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap, d_pool.data_ptr(), qcap, qcap,
                                        th, nnratio, rule, ent_cap, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                        d_status.data_ptr(), inv_level_sigma2=None if is2 is None else np.array(is2, F))
    _sync()
    return [_body(o, (B, qcap)) for o in out], _body(d_status, (2,))


def _check_core(members, got, tag):
    for f, (name, c, want, _) in enumerate(members):
        n = len(c["q"])
        for key, g, w in zip(("match", "best", "second"), got, want):
            assert np.array_equal(g[f, :n], w), (tag, name, key, np.flatnonzero(g[f, :n] != w)[:8], g[f, :n][g[f, :n] != w][:8], w[g[f, :n] != w][:8])
        assert (got[0][f, n:] == -1).all(), (tag, name)


def _chunks(members, size):
    return [members[i:i + size] for i in range(0, len(members), size)]


@pytest.mark.parametrize("size", [None, 1, 2], ids=["whole-groups", "batches-of-1", "batches-of-2"])
def test_core_batches_equal_oracle(trk, size):
    groups = _core_groups()
    names = [n for ms in groups.values() for n, _, _, _ in ms]
    assert any(n.startswith("candidates_513") for n in names) and any(n.startswith("chain_65") for n in names) and "nq=0" in names and "nF=0" in names
    nfs, rounds = set(), 0
    for key, members in groups.items():
        for part in _chunks(members, size or len(members)):
            need = sum(m[3] for m in part)
            got, status = _run_core_batch(trk, key, part, need)
            assert status[0] == 0, (key, status)
            _check_core(part, got, size)
            rounds = max(rounds, int(status[1]))
            nfs |= {len(m[1]["ci"]["xyF"]) for m in part}
    assert rounds >= 66 and {0, E.PJ_MAX_NF} <= nfs   # chain_65 ran its 66 rounds inside a batch


def test_core_entry_buffer_one_short(trk):
    """ent_cap one below the need: the status holds the exact need, match is -1 everywhere, nothing past any buffer is
    written (the guard bands are checked on every read); the same matcher is right again with the exact need"""
    groups = _core_groups()
    for key, members in groups.items():
        need = sum(m[3] for m in members)
        if need == 0:
            continue
        got, status = _run_core_batch(trk, key, members, need - 1)
        assert status[0] == need and status[1] == 0, (key, status, need)
        assert (got[0] == -1).all(), key
    key, members = max(groups.items(), key=lambda kv: len(kv[1]))
    got, status = _run_core_batch(trk, key, members, sum(m[3] for m in members))
    assert status[0] == 0
    _check_core(members, got, "after-overflow")


def test_core_slot_state_one_does_not_block(trk):
    """slot state 1 is a MapPoint without observations: the search may take it (:108-110 asks for Observations() > 0).  Every
    planted call with a blocked table runs with its free slots planted as 1 instead of 0 and must give the same oracle result;
    a core that blocked from state 1 on would match nothing here, and some expected match does land on such a slot"""
    on_state_one = 0
    for key, members in _core_groups().items():
        part = [m for m in members if m[1]["ci"]["blocked"] is not None]
        if not part:
            continue
        got, status = _run_core_batch(trk, key, part, sum(m[3] for m in part), free_slot=1)
        assert status[0] == 0, (key, status)
        _check_core(part, got, "slot-state-1")
        for _, c, want, _ in part:
            hit = want[0][want[0] >= 0]
            assert (c["ci"]["blocked"][hit] == 0).all()   # the oracle never matches a blocked slot: every hit was planted as 1
            on_state_one += len(hit)
    assert on_state_one > 0


# ------------------------------------------------------------------------------------------------ end to end, last frame
LAST_CASES = [(64, 48, "small", True), (200, 150, "forward", True), (200, 150, "backward", True), (0, 20, "small", True), (20, 0, "small", True)]
MONO_CASES = [(300, 260, "forward", False), (64, 48, "small", False)]


@functools.lru_cache(maxsize=None)
def _last_frame_refs(mono, th):
    rng = np.random.default_rng(99 + int(th) + (7 if mono else 0))
    out = []
    for nC, nL, motion, stereo in (MONO_CASES if mono else LAST_CASES):
        cur, last = PC.last_frame_case(rng, nC, nL, motion, stereo=stereo)
        out.append((cur, last, PC.oracle_last_frame(cur, last, th, mono)))
    return out


@pytest.mark.parametrize("th", [15, 30])
@pytest.mark.parametrize("mono", [False, True], ids=["stereo", "mono"])
def test_track_last_frame_equals_oracle(trk, mono, th):
    refs = _last_frame_refs(mono, th)
    B = len(refs)
    cur0 = refs[0][0]
    fr = Frames(trk, [_cur_frame(c) for c, _, _ in refs], _grid4(cur0))
    last = Last([la for _, la, _ in refs], max(max(len(la["octave"]) for _, la, _ in refs), 1) + 5)
    # a first guess of 16 entries: the wrapper reads the need from the status and calls once more
    d_T = _poses([c["Tcw"] for c, _, _ in refs])
    t = trk.track_last_frame(fr.struct, d_T.data_ptr(), last.struct, _cam(cur0), cur0["K"][5], mono, th,
                             cur0["scale_factors"], B, ent_cap=16)
    _sync()
    assigned, nm, pairs, npairs = (t[k].cpu().numpy() for k in ("assigned", "nmatches", "pairs", "npairs"))
    match, nq, status = t["match"].cpu().numpy(), t["nq"].cpu().numpy(), t["status"].cpu().numpy()
    assert status[0] == 0
    kept, dropped = [], []
    for f, (cur, la, (wa, wnm, wpairs, wq, wvalid, wm)) in enumerate(refs):
        nC = len(cur["xy"])
        assert nq[f] == int(wvalid.sum()) and np.array_equal(match[f, :nq[f]], wm), f
        assert np.array_equal(assigned[f, :nC], wa), (f, np.flatnonzero(assigned[f, :nC] != wa)[:8])
        assert (assigned[f, nC:] == -1).all()
        assert nm[f] == wnm and npairs[f] == len(wpairs), (f, nm[f], wnm)
        assert np.array_equal(pairs[f, :npairs[f]], np.array(wpairs, np.int32).reshape(-1, 2)), f
        kept.append(wnm)
        dropped.append(len(wpairs) - wnm)
    assert max(kept) >= 16 and max(dropped) >= 3   # nothing vacuous: matches survive and the rotation histogram drops some


# ------------------------------------------------------------------------------------------------ end to end, local map
def _world_for(cur, mps, T):
    """map points whose isInFrustum values reproduce the case's: depth from the case's (u - ur) = bf / z, the normal at the
    case's viewing cosine, max_dist half a level above the case's scale level; the case's out-of-view points are `seen`"""
    fx, fy, cx, cy, bf, _ = cur["K"]
    n = len(mps["bad"])
    u, v, ur = mps["proj_xyr"].T.astype(np.float64)
    z = bf / np.maximum(u - ur, 0.5)
    R, t = np.asarray(T, np.float64)[:3, :3], np.asarray(T, np.float64)[:3, 3]
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    P = ((Xc - t) @ R).astype(F)
    Ow = TO.camera_centre(TO.T34(T)).astype(np.float64)
    po = P.astype(np.float64) - Ow
    d = np.linalg.norm(po, axis=1)
    a = po / d[:, None]
    perp = np.cross(a, [0.3, 0.5, 0.8])
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    cos = np.minimum(mps["view_cos"].astype(np.float64), 1.0)
    nrm = (cos[:, None] * a + np.sqrt(np.maximum(1 - cos * cos, 0))[:, None] * perp).astype(F)
    maxd = (d * 1.2 ** (mps["scale_level"] - 0.5)).astype(F)
    po32 = (P - TO.camera_centre(TO.T34(T))).astype(F).astype(np.float64)
    dist32 = np.sqrt(po32[:, 0] * po32[:, 0] + po32[:, 1] * po32[:, 1] + po32[:, 2] * po32[:, 2]).astype(F)
    maxd[mps["scale_level"] == 0] = dist32[mps["scale_level"] == 0]   # level 0 in view is ratio 1 exactly: max_dist = the float distance
    return dict(world_pos=P, normal=nrm, max_dist=maxd, min_dist=(maxd / F(1.2 ** 8)).astype(F), seen=(1 - mps["in_view"]).astype(np.uint8),
                bad=mps["bad"], obs_gt0=mps["obs_gt0"], mpdesc=mps["mpdesc"])


@functools.lru_cache(maxsize=None)
def _local_map_refs(th):
    rng = np.random.default_rng(500 + int(th))
    T = TO._posed()
    out = []
    for nF, nmp in ((64, 80), (200, 300)):
        cur, mps = PC.local_map_case(rng, nF, nmp)
        cur["Tcw"] = T
        w = _world_for(cur, mps, T)
        K5 = cur["K"][:5]
        proj, inv = TO.frustum(T, K5, cur["bounds"], w["world_pos"], w["normal"], w["min_dist"], w["max_dist"], seen=w["seen"], bad=w["bad"])
        # the oracle's own projected values go through the pinned gating, core and replay
        m2 = dict(mps, in_view=inv, proj_xyr=np.stack([proj["u"], proj["v"], proj["ur"]], 1), scale_level=np.maximum(proj["level"], 0),
                  view_cos=proj["view_cos"])
        ok = inv.astype(bool)
        assert ok.sum() > 0.7 * nmp and np.abs(m2["proj_xyr"][ok, :2] - mps["proj_xyr"][ok, :2]).max() < 0.05
        assert np.median(np.abs(m2["proj_xyr"][ok, 2] - mps["proj_xyr"][ok, 2])) < 0.05
        assert (proj["level"][ok] == mps["scale_level"][ok]).mean() > 0.95
        out.append((cur, w, proj, inv, PC.oracle_local_map(cur, m2, th)))
    return out


@pytest.mark.parametrize("th", [1, 3, 5])
def test_track_local_map_equals_oracle(trk, th):
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi
    from orb_slam2_ssd_semantic_amd._ffi import TRACK_PROJ_DTYPE
    refs = _local_map_refs(th)
    B = len(refs)
    cur0 = refs[0][0]
    fr = Frames(trk, [_cur_frame(c) for c, _, _, _, _ in refs], _grid4(cur0))
    cat = {k: np.concatenate([w[k] for _, w, _, _, _ in refs]) for k in refs[0][1]}
    counts = [len(w["bad"]) for _, w, _, _, _ in refs]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    npts = int(off[-1])
    d = {k: _dev(v) for k, v in cat.items()}
    tmap = _ffi.TrackMap(d["world_pos"].data_ptr(), d["normal"].data_ptr(), d["min_dist"].data_ptr(), d["max_dist"].data_ptr(),
                         d["bad"].data_ptr(), d["obs_gt0"].data_ptr(), d["mpdesc"].data_ptr(), npts)
    d_off, d_idx = _dev(off), _dev(np.arange(npts, dtype=np.int32))
    qcap = max(counts) + 4
    t, out = trk.alloc_out(B, fr.cap, qcap)
    d_vis = _guarded((B,))
    d_proj = torch.full((npts * 5 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    d_T = _poses([c["Tcw"] for c, _, _, _, _ in refs])
    need = 0
    for attempt in range(2):
        trk.TrackLocalMap_batch_device(fr.struct, d_T.data_ptr(), _cam(cur0), th,
                                       cur0["scale_factors"], TO.LOG_SF, tmap, d_off.data_ptr(), d_idx.data_ptr(), d["seen"].data_ptr(), npts,
                                       100, 0.8, max(need, 32), B, out, d_visible=d_vis.data_ptr(), d_proj=d_proj.data_ptr())
        _sync()
        need = int(t["status"][0].item())
        if need == 0:
            break
    assert need == 0 and attempt == 1   # 32 entries were too few: the second call had the exact need
    proj = _body(d_proj, (npts * 5,)).view(TRACK_PROJ_DTYPE)
    vis = _body(d_vis, (B,))
    assigned, nm, match, nq, src = (t[k].cpu().numpy() for k in ("assigned", "nmatches", "match", "nq", "qsrc"))
    total = 0
    for f, (cur, w, wproj, winv, (wa, wnm, wq, wvalid, wm)) in enumerate(refs):
        lo, hi = int(off[f]), int(off[f + 1])
        assert proj[lo:hi].tobytes() == wproj.tobytes(), f
        sel = np.flatnonzero(wvalid)
        assert vis[f] == int(winv.sum()) and nq[f] == len(sel) and np.array_equal(src[f, :nq[f]], sel + lo), f
        assert t["q"][f, :nq[f]].cpu().numpy().tobytes() == wq[sel].tobytes(), f
        assert np.array_equal(match[f, :nq[f]], wm), f
        nC = len(cur["xy"])
        want = np.where(wa >= 0, wa + lo, wa)
        assert np.array_equal(assigned[f, :nC], want) and nm[f] == wnm, (f, nm[f], wnm)
        total += wnm
    assert total > 40


# ------------------------------------------------------------------------------------------------ unproject + selection
@pytest.mark.parametrize("th_depth", [0.05, 50.0, 3.0], ids=["below-all", "above-all", "on-a-depth"])
def test_unproject_select_equals_oracle(trk, th_depth):
    import torch
    rng = np.random.default_rng(int(th_depth * 100))
    T = TO._posed()
    cap, frames = 200, []
    for npos in (0, 99, 100, 101, 150):
        n = min(npos + 30, cap)
        xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(F)
        z = np.where(np.arange(n) % 3 == 0, 0.0, -1.0).astype(F)
        where = rng.permutation(n)[:npos]
        z[where] = rng.uniform(0.4, 8.0, npos).astype(F)
        if npos:
            z[where[: npos // 3]] = rng.choice([2.0, 3.0, 4.5], npos // 3)   # ties, among them the threshold itself
        keeps = (rng.random(n) < 0.3).astype(np.uint8)
        frames.append((xy, z, keeps))
    B = len(frames)
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, tracking
    blk = np.zeros((B, cap), KP_DTYPE)
    depth, keeps = np.full((B, cap), 1.0, F), np.zeros((B, cap), np.uint8)   # rows past the count would be unprojected if read
    for f, (xy, z, kp) in enumerate(frames):
        n = len(z)
        blk["x"][f, :n], blk["y"][f, :n], depth[f, :n], keeps[f, :n] = xy[:, 0], xy[:, 1], z, kp
    d_kps, d_depth, d_keeps = _dev(blk.view(np.int32).reshape(B, cap, 7)), _dev(depth), _dev(keeps)
    d_n = _dev(np.array([len(z) for _, z, _ in frames], np.int32))
    d_wp = torch.full((B * cap * 3 + GUARD,), float(SENT), dtype=torch.float32, device="cuda")
    d_cr = torch.full((B * cap + GUARD,), 9, dtype=torch.uint8, device="cuda")
    cam = tracking.camera(*TO.K0, *TO.BOUNDS0)
    d_T = _poses([T] * B)
    trk.UnprojectSelect_batch_device(d_kps.data_ptr(), d_depth.data_ptr(), d_n.data_ptr(), cap, B, d_T.data_ptr(), cam, th_depth,
                                     d_keeps.data_ptr(), d_wp.data_ptr(), d_cr.data_ptr())
    _sync()
    wp, cr = d_wp.cpu().numpy(), d_cr.cpu().numpy()
    assert (wp[B * cap * 3:] == SENT).all() and (cr[B * cap:] == 9).all()
    wp, cr = wp[:B * cap * 3].reshape(B, cap, 3), cr[:B * cap].reshape(B, cap)
    nsel = []
    for f, (xy, z, kp) in enumerate(frames):
        n = len(z)
        wwp, wcr = TO.unproject_select(xy, z, T, TO.K0, th_depth, kp)
        assert wp[f, :n].tobytes() == wwp.tobytes(), f
        assert np.array_equal(cr[f, :n], wcr), (f, np.flatnonzero(cr[f, :n] != wcr)[:8])
        assert not wp[f, n:].any() and not cr[f, n:].any()
        nsel.append(int(TO.select_literal(z, th_depth).sum()))
    assert nsel[0] == 0 and nsel[1] == 99 and nsel[2] == 100 and nsel[3] == 101   # up to 100 + 1 whatever the threshold
    assert nsel[4] == (101 if th_depth < 1 else 150 if th_depth > 10 else nsel[4]) and 101 <= nsel[4] <= 150


# ------------------------------------------------------------------------------------------------ device PredictScale
def test_device_predict_scale_on_the_sweep(trk):
    """the CPU sweep's 100 156 (max_dist, dist) pairs as one frame's list under the identity pose (P = (0, 0, dist), normal
    (0, 0, 1)): the level isInFrustum leaves on the device == the oracle's, which tests/test_track_oracle.py holds against
    the compiled reference.  Ratios below 1 are past max_dist: out of view on both sides."""
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi, tracking
    from orb_slam2_ssd_semantic_amd._ffi import TRACK_PROJ_DTYPE
    mx, ds = TO.predict_sweep()
    n = len(mx)
    P = np.zeros((n, 3), F)
    P[:, 2] = ds
    Pn = np.tile(np.array([0, 0, 1], F), (n, 1))
    d = dict(P=_dev(P), Pn=_dev(Pn), mn=_dev(np.zeros(n, F)), mx=_dev(mx), bad=_dev(np.zeros(n, np.uint8)), obs=_dev(np.ones(n, np.uint8)))
    tmap = _ffi.TrackMap(d["P"].data_ptr(), d["Pn"].data_ptr(), d["mn"].data_ptr(), d["mx"].data_ptr(), d["bad"].data_ptr(), d["obs"].data_ptr(),
                         None, n)
    qcap = 256
    d_q, d_src, d_nq, d_vis = _guarded((qcap, 8)), _guarded((qcap,)), _guarded((1,)), _guarded((1,))
    d_proj = torch.full((n * 5 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    cam = tracking.camera(*TO.K0, *TO.BOUNDS0)
    d_T, d_off, d_idx = _poses([TO.IDENTITY]), _dev(np.array([0, n], np.uint32)), _dev(np.arange(n, dtype=np.int32))
    trk.GateLocalMap_batch_device(d_T.data_ptr(), cam, 1.0, PC.scale_factors(), TO.LOG_SF, tmap, d_off.data_ptr(), d_idx.data_ptr(), None, n, 1,
                                  d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap, d_visible=d_vis.data_ptr(), d_proj=d_proj.data_ptr())
    _sync()
    got = _body(d_proj, (n * 5,)).view(TRACK_PROJ_DTYPE)["level"]
    want = np.array([TO.predict_scale(m, x) if x <= m else -1 for m, x in zip(mx, ds)])
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(float(mx[i]), float(ds[i]), int(got[i]), int(want[i])) for i in bad[:16]]
    assert _body(d_vis, (1,))[0] == int((want >= 0).sum()) and _body(d_nq, (1,))[0] == qcap   # queries past qcap are dropped
    _body(d_q, (qcap, 8)), _body(d_src, (qcap,))   # the guard bands
