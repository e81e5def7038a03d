"""The device-resident tracker (csrc/orbfe_track.hip) at its frustum, pose, chunk and replay edges, bit for bit against the CPU
oracles.  Inputs and expectations come from tests/track_edge_cases.py (tests/test_track_edge_cases.py shows on the CPU that
every table holds what it claims); the kernels run through tracking.Tracker's *_batch_device calls, each stage on its own:

  1. TO.frustum_cases() through GateLocalMap_batch_device, three frames with three poses
  2. the map gate over lists of 0 .. 513 entries at odd offsets, nine poses, indices outside the map, `seen`, NULL outputs,
     a last list_off beyond nentries
  3. queries past qcap in both gates, last-frame octaves outside [0, nlevels)
  4. last->d_n and UnprojectSelect's d_n below 0 and above cap
  5. UnprojectSelect with n = 1023 .. 2049 and cap = n = 15360: the 1024-thread stride loops turn more than once
  6. Replay_batch_device on hand-built matches (the oracle is TO.replay_batch)
  7. SearchByProjection_batch_device with one shared pool and with per-frame pools and sources outside them

No tolerances.  Every output buffer carries a guard band of sentinels, and the part of a buffer a call must leave alone is
compared with the sentinel too."""
import numpy as np
import pytest

import test_gpu_track as G
import track_edge_cases as TE
import track_oracle as TO
from test_gpu_track import Frames, Last, _body, _dev, _guarded, _poses, _sync

pytestmark = pytest.mark.gpu

F = np.float32
SENT = G.SENT


@pytest.fixture(scope="module")
def trk():
    from orb_slam2_ssd_semantic_amd import ORBmatcher, Tracker
    m = ORBmatcher(0.9, True)
    yield Tracker(m)
    m.close()


def _camera():
    from orb_slam2_ssd_semantic_amd import tracking
    return tracking.camera(*TO.K0, *TO.BOUNDS0)


# ------------------------------------------------------------------------------------------------ the map gate
def _run_gate_map(trk, poses, m, list_off, list_idx, seen, th, qcap, nentries=None, visible=True, proj=True):
    from orb_slam2_ssd_semantic_amd import _ffi
    B, npts, total = len(poses), len(m["bad"]), len(list_idx)
    d = {k: _dev(v) for k, v in m.items()}
    tmap = _ffi.TrackMap(d["world_pos"].data_ptr(), d["normal"].data_ptr(), d["min_dist"].data_ptr(), d["max_dist"].data_ptr(),
                         d["bad"].data_ptr(), d["obs_gt0"].data_ptr(), None, npts)
    d_off, d_idx, d_T = _dev(list_off), _dev(list_idx), _poses(poses)
    d_seen = None if seen is None else _dev(seen)
    d_q, d_src, d_nq = _guarded((B, qcap, 8)), _guarded((B, qcap)), _guarded((B,))
    d_vis = _guarded((B,)) if visible else None
    d_proj = _guarded((total, 5)) if proj else None
    trk.GateLocalMap_batch_device(d_T.data_ptr(), _camera(), th, TE.SF, TO.LOG_SF, tmap, d_off.data_ptr(), d_idx.data_ptr(),
                                  None if d_seen is None else d_seen.data_ptr(), total if nentries is None else nentries, B,
                                  d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap,
                                  d_visible=None if d_vis is None else d_vis.data_ptr(), d_proj=None if d_proj is None else d_proj.data_ptr())
    _sync()
    return dict(q=_body(d_q, (B, qcap, 8)), src=_body(d_src, (B, qcap)), nq=_body(d_nq, (B,)),
                vis=_body(d_vis, (B,)) if visible else None, proj=_body(d_proj, (total, 5)) if proj else None)


def _check_gate_map(got, want, qcap, tag):
    touched = np.zeros(len(got["proj"]) if got["proj"] is not None else 0, bool)
    for f, w in enumerate(want):
        cnt = len(w["src"])
        k = min(cnt, qcap)
        assert got["nq"][f] == k, (tag, f, got["nq"][f], cnt)
        assert np.array_equal(got["src"][f, :k], w["qsrc"][:k]), (tag, f)
        assert got["q"][f, :k].tobytes() == w["q"][:k].tobytes(), (tag, f)
        assert (got["q"][f, k:] == SENT).all() and (got["src"][f, k:] == SENT).all(), (tag, f)
        if got["vis"] is not None:
            assert got["vis"][f] == cnt == int(w["in_view"].sum()), (tag, f)
        if got["proj"] is not None:
            mine, exp = got["proj"][w["e0"]:w["e1"]], w["proj"].view(np.int32).reshape(-1, 5)
            assert np.array_equal(mine, exp), (tag, f, np.flatnonzero((mine != exp).any(1))[:8])
            touched[w["e0"]:w["e1"]] = True
    if got["proj"] is not None:
        assert (got["proj"][~touched] == SENT).all(), tag


def test_frustum_table_on_the_device(trk):
    """every isInFrustum gate, the 0.5 / 0.998 cosine edges and the level clamps of TO.frustum_cases() on the device"""
    t = TE.frustum_table()
    got = _run_gate_map(trk, t["poses"], t["map"], t["list_off"], t["list_idx"], t["seen"], t["th"], len(t["entries"]) + 3)
    _check_gate_map(got, t["want"], len(t["entries"]) + 3, "frustum")
    from orb_slam2_ssd_semantic_amd._ffi import TRACK_PROJ_DTYPE
    from oracle import oracle_ffi as O
    made = {}
    for f, w in enumerate(t["want"]):
        srcs = got["src"][f, :got["nq"][f]].tolist()
        for e in range(w["e0"], w["e1"]):
            name, member, _ = t["entries"][t["list_idx"][e]]
            p = int(t["list_idx"][e])
            made[(name, member)] = (got["q"][f, srcs.index(p)].view(O.PROJ_QUERY_DTYPE)[0], got["proj"][e].view(TRACK_PROJ_DTYPE)[0]) if p in srcs else None
    for name, (rej, ok) in TO.frustum_cases().items():
        assert made[(name, 1)] is not None and (made[(name, 0)] is None) == (rej["gate"] is not None), name
        if made[(name, 0)] is None:
            e = int(np.flatnonzero(t["list_idx"] == [i for i, (n, k, _) in enumerate(t["entries"]) if n == name and k == 0][0])[0])
            assert got["proj"][e].tolist() == [0, 0, 0, 0, -1], name
    for member, radius in ((0, 4.0), (1, 2.5)):
        q, p = made[("view_cos_0.998", member)]
        assert q["r"] == F(F(radius) * TE.SF[p["level"]]), (member, q["r"])
    assert [int(made[(k, m)][1]["level"]) for k in ("level_0", "level_7") for m in (0, 1)] == [0, 1, 7, 7]


@pytest.mark.parametrize("variant", ["full", "no-seen", "no-visible-no-proj", "cut"])
def test_map_gate_lists_equal_oracle(trk, variant):
    """nine frames under nine poses, lists back to back with wave and workgroup boundaries inside them"""
    c = TE.map_gate_case()
    want = TE.map_gate_want("full" if variant == "no-visible-no-proj" else variant)
    got = _run_gate_map(trk, c["poses"], c["map"], c["list_off"], c["list_idx"], None if variant == "no-seen" else c["seen"], c["th"], c["qcap"],
                        nentries=c["cut"] if variant == "cut" else None, visible=variant != "no-visible-no-proj", proj=variant != "no-visible-no-proj")
    _check_gate_map(got, want, c["qcap"], variant)


# ------------------------------------------------------------------------------------------------ qcap, octaves, counts
def _run_gate_last(trk, pairs, cap, qcap, n_dev=None, th=TE.LAST_TH, mono=False):
    import torch
    B = len(pairs)
    cur0 = pairs[0][0]
    last = Last([la for _, la in pairs], cap)
    if n_dev is not None:
        last.t["n"].copy_(torch.from_numpy(np.asarray(n_dev, np.int32)))
    d_q, d_src, d_nq = _guarded((B, qcap, 8)), _guarded((B, qcap)), _guarded((B,))
    d_T = _poses([c["Tcw"] for c, _ in pairs])
    trk.GateLastFrame_batch_device(d_T.data_ptr(), last.struct, G._cam(cur0), cur0["K"][5], mono, th, cur0["scale_factors"], B,
                                   d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap)
    _sync()
    return _body(d_q, (B, qcap, 8)), _body(d_src, (B, qcap)), _body(d_nq, (B,))


def _check_gate_last(got, want, qcap, tag):
    q, src, nq = got
    for f, (wq, wsrc) in enumerate(want):
        k = min(len(wsrc), qcap)
        assert nq[f] == k, (tag, f, nq[f], len(wsrc))
        assert np.array_equal(src[f, :k], wsrc[:k]) and q[f, :k].tobytes() == wq[:k].tobytes(), (tag, f)
        assert (q[f, k:] == SENT).all() and (src[f, k:] == SENT).all(), (tag, f)   # the row's own tail; the guard band is checked on read


@pytest.mark.parametrize("qcap", TE.QCAPS)
def test_last_frame_gate_drops_queries_past_qcap(trk, qcap):
    pairs, want = TE.qcap_last_case()
    _check_gate_last(_run_gate_last(trk, pairs, 303, qcap), want, qcap, qcap)


@pytest.mark.parametrize("qcap", TE.QCAPS)
def test_map_gate_drops_queries_past_qcap(trk, qcap):
    c = TE.qcap_map_case()
    got = _run_gate_map(trk, c["poses"], c["map"], c["list_off"], c["list_idx"], None, c["th"], qcap)
    _check_gate_map(got, c["want"], qcap, qcap)   # d_visible holds the full count


def test_last_frame_octave_outside_the_levels_makes_no_query(trk):
    dev, _, planted, want = TE.octave_case()
    got = _run_gate_last(trk, dev, 83, 83)
    _check_gate_last(got, want, 83, "octaves")
    assert not set(planted) & set(got[1][0, :got[2][0]].tolist())


def test_last_frame_count_outside_the_capacity(trk):
    pairs, n_dev, want, _ = TE.count_last_case()
    _check_gate_last(_run_gate_last(trk, pairs, TE.COUNT_CAP_LAST, TE.COUNT_CAP_LAST, n_dev=n_dev), want, TE.COUNT_CAP_LAST, "counts")


# ------------------------------------------------------------------------------------------------ unproject + selection
def _run_unproject(trk, c, cap, n_dev=None, keeps=True):
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    frames = c["frames"]
    B = len(frames)
    blk = np.zeros((B, cap), KP_DTYPE)
    blk["x"], blk["y"] = 100.0, 100.0
    depth, kp = np.full((B, cap), 1.0, F), np.zeros((B, cap), np.uint8)   # rows past the count would be unprojected if read
    for f, (xy, z, k) in enumerate(frames):
        n = len(z)
        blk["x"][f, :n], blk["y"][f, :n], depth[f, :n], kp[f, :n] = xy[:, 0], xy[:, 1], z, k
    d_kps, d_depth, d_keeps = _dev(blk.view(np.int32).reshape(B, cap, 7)), _dev(depth), _dev(kp)
    d_n = _dev(np.array([len(z) for _, z, _ in frames], np.int32) if n_dev is None else n_dev)
    d_wp = torch.full((B * cap * 3 + G.GUARD,), float(SENT), dtype=torch.float32, device="cuda")
    d_cr = torch.full((B * cap + G.GUARD,), 9, dtype=torch.uint8, device="cuda")
    d_T = _poses(c["poses"])
    trk.UnprojectSelect_batch_device(d_kps.data_ptr(), d_depth.data_ptr(), d_n.data_ptr(), cap, B, d_T.data_ptr(), _camera(), c["th_depth"],
                                     d_keeps.data_ptr() if keeps else None, d_wp.data_ptr(), d_cr.data_ptr())
    _sync()
    wp, cr = d_wp.cpu().numpy(), d_cr.cpu().numpy()
    assert (wp[B * cap * 3:] == SENT).all() and (cr[B * cap:] == 9).all(), "guard band overwritten"
    return wp[:B * cap * 3].reshape(B, cap, 3), cr[:B * cap].reshape(B, cap)


def _check_unproject(got, want, tag):
    wp, cr = got
    for f, (wwp, wcr) in enumerate(want):
        n = len(wcr)
        assert wp[f, :n].tobytes() == wwp.tobytes(), (tag, f, np.flatnonzero((wp[f, :n] != wwp).any(1))[:8])
        assert np.array_equal(cr[f, :n], wcr), (tag, f, np.flatnonzero(cr[f, :n] != wcr)[:8])
        assert not wp[f, n:].any() and not cr[f, n:].any(), (tag, f)


def test_unproject_count_outside_the_capacity(trk):
    c = TE.count_unproject_case()
    _check_unproject(_run_unproject(trk, c, TE.COUNT_CAP_UNPROJ, n_dev=c["n_dev"]), c["want"], "counts")


@pytest.mark.parametrize("keeps", [True, False], ids=["keeps", "keeps-null"])
def test_unproject_past_one_stride(trk, keeps):
    """n = 1023, 1024, 1025, 2049 under four poses: the second and third turn of the stride loops, the boundary tie decided by
    the index across them"""
    small, _ = TE.unproject_stride_case()
    _check_unproject(_run_unproject(trk, small, small["cap"], keeps=keeps), small["want"] if keeps else small["want_no_keeps"], keeps)


def test_unproject_at_the_largest_frame(trk):
    """cap = n = 15360: the depth table fills the workgroup's LDS, every thread takes fifteen entries"""
    _, big = TE.unproject_stride_case()
    _check_unproject(_run_unproject(trk, big, big["cap"]), big["want"], "15360")


# ------------------------------------------------------------------------------------------------ the replay
@pytest.mark.parametrize("kind,check_ori,outputs", [("last", 1, True), ("last", 0, True), ("map", 0, True), ("last", 1, False)],
                         ids=["last-ori", "last-plain", "map", "last-ori-null-pairs"])
def test_replay_on_planted_matches(trk, kind, check_ori, outputs):
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    t = list(TE.replay_case().values())
    want = TE.replay_want(kind, bool(check_ori))
    B, qcap, capl = len(t), TE.REPLAY_QCAP, TE.REPLAY_CAP_LAST
    fr = Frames(trk, [dict(xy=x["cur"]["xy"], octave=x["cur"]["octave"], angle=x["cur"]["angle"], desc=x["cur"]["desc"], uRight=None,
                           slot=x["cur"]["state"]) for x in t], (0.0, 0.0, 64.0 / 640.0, 48.0 / 480.0))
    blk = np.zeros((B, capl), KP_DTYPE)
    for f, x in enumerate(t):
        blk["angle"][f] = x["last"]["angle"]
    d_last = _dev(blk.view(np.int32).reshape(B, capl, 7))
    d_match, d_qsrc = _dev(np.stack([x["match"] for x in t])), _dev(np.stack([x["qsrc"] for x in t]))
    d_nq = _dev(np.array([x["nq"] for x in t], np.int32))
    d_as, d_nm, d_pairs, d_np = _guarded((B, fr.cap)), _guarded((B,)), _guarded((B, qcap, 2)), _guarded((B,))
    trk.Replay_batch_device(fr.struct, B, d_match.data_ptr(), d_qsrc.data_ptr(), d_nq.data_ptr(), qcap,
                            d_last.data_ptr() if kind == "last" else None, capl if kind == "last" else 0, check_ori,
                            d_as.data_ptr(), d_nm.data_ptr(), d_pairs.data_ptr() if outputs else None, d_np.data_ptr() if outputs else None)
    _sync()
    assigned, nm, pairs, npairs = _body(d_as, (B, fr.cap)), _body(d_nm, (B,)), _body(d_pairs, (B, qcap, 2)), _body(d_np, (B,))
    for f, (x, (wa, wnm, wpairs)) in enumerate(zip(t, want)):
        nF = x["nF"]
        assert np.array_equal(assigned[f, :nF], wa), (f, np.flatnonzero(assigned[f, :nF] != wa)[:8], assigned[f, :nF][assigned[f, :nF] != wa][:8], wa[assigned[f, :nF] != wa][:8])
        assert (assigned[f, nF:] == -1).all() and nm[f] == wnm, (f, nm[f], wnm)
        if outputs:
            assert npairs[f] == len(wpairs), (f, npairs[f], len(wpairs))
            assert np.array_equal(pairs[f, :npairs[f]], np.array(wpairs, np.int32).reshape(-1, 2)), f
            assert (pairs[f, npairs[f]:] == SENT).all(), f
    if not outputs:
        assert (pairs == SENT).all() and (npairs == SENT).all()


# ------------------------------------------------------------------------------------------------ the core's pools
def _run_pool(trk, calls, srcs, pool, pool_rows, pool_frame_rows, ent_cap):
    from oracle import oracle_ffi as O
    c0 = calls[0]
    frames = [dict(xy=c["ci"]["xyF"], octave=c["ci"]["octF"], desc=c["ci"]["descF"], uRight=c["ci"]["uRight"],
                   slot=None if c["ci"]["blocked"] is None else 2 * c["ci"]["blocked"]) for c in calls]
    fr = Frames(trk, frames, tuple(float(v) for v in c0["ci"]["bounds"]))
    B = len(calls)
    qcap = max(len(c["q"]) for c in calls) + 2
    q = np.zeros((B, qcap), O.PROJ_QUERY_DTYPE)
    q["r"], q["u"], q["v"] = 50.0, 100.0, 100.0    # lanes beyond nq would find candidates if they ran
    src = np.zeros((B, qcap), np.int32)
    for f, c in enumerate(calls):
        q[f, :len(c["q"])], src[f, :len(c["q"])] = c["q"], srcs[f]
    d_q, d_src, d_pool = _dev(q.view(np.int32).reshape(B, qcap, 8)), _dev(src), _dev(pool)
    d_nq = _dev(np.array([len(c["q"]) for c in calls], np.int32))
    out = [_guarded((B, qcap)) for _ in range(3)]
    d_status = _guarded((2,))
    trk.SearchByProjection_batch_device(fr.struct, B, d_q.data_ptr(), d_src.data_ptr(), d_nq.data_ptr(), qcap, d_pool.data_ptr(), pool_rows,
                                        pool_frame_rows, c0["th"], c0["nnratio"], c0["rule"], ent_cap, out[0].data_ptr(), out[1].data_ptr(),
                                        out[2].data_ptr(), d_status.data_ptr())
    _sync()
    return [_body(o, (B, qcap)) for o in out], _body(d_status, (2,))


def _check_pool(calls, got, status, want, tag):
    assert status[0] == 0, (tag, status)
    for f, c in enumerate(calls):
        n = len(c["q"])
        for key, g, w in zip(("match", "best", "second"), got, want[f][0]):
            assert np.array_equal(g[f, :n], w), (tag, f, key, np.flatnonzero(g[f, :n] != w)[:8], g[f, :n][g[f, :n] != w][:8], w[g[f, :n] != w][:8])
        assert (got[0][f, n:] == -1).all() and (got[1][f, n:] == SENT).all() and (got[2][f, n:] == SENT).all(), (tag, f)


def test_core_with_one_shared_pool(trk):
    """pool_frame_rows = 0: every frame reads ONE pool, rows addressed by several frames and by queries of other frames"""
    shared, _ = TE.core_pool_case()
    got, status = _run_pool(trk, shared["calls"], shared["srcs"], shared["pool"], len(shared["pool"]), 0, sum(w[1] for w in shared["want"]))
    _check_pool(shared["calls"], got, status, shared["want"], "shared")


def test_core_with_sources_outside_the_pool(trk):
    """per-frame pools: a source of -1 or pool_rows finds nothing (match -1, best and second 256) and the other queries
    answer as if those queries were not there"""
    _, per = TE.core_pool_case()
    got, status = _run_pool(trk, per["calls"], per["srcs"], per["pools"], TE.POOL_ROWS, TE.POOL_STRIDE, sum(w[1] for w in per["want"]))
    _check_pool(per["calls"], got, status, per["want"], "per-frame")
