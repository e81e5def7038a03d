"""The batched Fuse without a GPU: the host gate orbfe_fuse_gate_points (trk_gate_fuse, the function the search kernel runs) against
tests/fuse_oracle.py and against orbfe_project_points as bit patterns, on fuse_case seeds and on the planted edges; the oracle's
whole Fuse against the compiled reference (ref_fuse / ref_fuse_sim3) where oracle/_ref is built; its action codes against the serial
replay on the mock's Replace / AddObservation; vpFuseCandidates against a loop with a stamp."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as FO
from oracle import ref_ffi as R

F = np.float32
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")
CPU_SEEDS = (0, 1, 2, 5, 6, 9, 10, 11)   # every nKF in {1, 30, 300, 1000}, nmp up to 400 (the serial oracle is a Python loop)


def _gate_both(T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, mode):
    from orb_slam2_ssd_semantic_amd import mapping
    cam = mapping.camera(*K[:5], *bounds)
    got = mapping.fuse_gate_points(T.reshape(-1), Ow, cam, th, sf, log_sf, wp, nr, mn, mx, mode)
    want = FO.gate_points(T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, mode == FO.PLAIN)
    return got, want


def _project_points(T, Ow, K, bounds, wp, nr, mn, mx):
    """orbfe_project_points the way shim/ORBmatcher_orbfe.cc calls it for Fuse: z < 0 out, KeyFrame::IsInImage bounds"""
    from orb_slam2_ssd_semantic_amd import _ffi
    n = len(mn)
    Rm, t = np.ascontiguousarray(T[:, :3]), np.ascontiguousarray(T[:, 3])
    wp, nr = np.ascontiguousarray(wp, F).reshape(-1, 3), np.ascontiguousarray(nr, F).reshape(-1, 3)
    # GetMinDistanceInvariance() / GetMaxDistanceInvariance(), as the shim passes them
    mn, mx, Ow = (F(0.8) * np.asarray(mn, F)).astype(F), (F(1.2) * np.asarray(mx, F)).astype(F), np.ascontiguousarray(Ow, F)
    u, v, iz, d, ur = (np.zeros(n, F) for _ in range(5))
    ok = np.zeros(n, np.uint8)
    p = _ffi.ptr
    _ffi.check(_ffi.lib().orbfe_project_points(p(Rm), p(t), None, None, p(Ow), *[float(x) for x in K[:5]], *[float(b) for b in bounds],
                                               _ffi.ABI.ORBFE_PJ_SKIP_NEG_DEPTH, n, p(wp), p(nr), p(mn), p(mx), p(u), p(v), p(iz), p(d), p(ur),
                                               p(ok)), "orbfe_project_points")
    return u, v, ur, d, ok


def _check_gate(T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, what):
    for mode in (FO.PLAIN, FO.SIM3):
        (q, level, ok), (wq, wlevel, wok) = _gate_both(T, Ow, K, bounds, th, sf, log_sf, wp, nr, mn, mx, mode)
        assert np.array_equal(ok, wok) and np.array_equal(level, wlevel), (what, mode)
        assert np.array_equal(q.view(np.uint32).reshape(-1, 8), wq), (what, mode)
    u, v, ur, d, pok = _project_points(T, Ow, K, bounds, wp, nr, mn, mx)
    assert np.array_equal(pok, ok), what
    sel = ok.astype(bool)
    for name, arr in (("u", u), ("v", v), ("ur", ur)):
        assert np.array_equal(arr[sel].view(np.uint32), q[name][sel].view(np.uint32)), (what, name)
    # r = th * scale_factors[PredictScale(dist3D)] from the distance orbfe_project_points returns
    want_r = np.array([F(F(th) * F(sf[FO.predict_scale(mx[i], d[i], log_sf, len(sf))])) for i in np.flatnonzero(sel)], F)
    assert np.array_equal(q["r"][sel].view(np.uint32), want_r.view(np.uint32)), what
    return ok, level


@pytest.mark.parametrize("seed", CPU_SEEDS + (14, 15))
def test_gate_equals_oracle_and_project_points_on_seeds(seed):
    kf, mps, th = FC.seed_case(seed)
    T, Ow = FC.pose_of(kf)
    ok, _ = _check_gate(T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], mps["world_pos"], mps["normal"], mps["min_dist"],
                        mps["max_dist"], seed)
    assert len(ok) < 40 or 0 < ok.sum() < len(ok)
    Ts, Os = FC.pose_of(kf, FO.SIM3, FC.scw_of(kf, 1.7))
    _check_gate(Ts, Os, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], mps["world_pos"], mps["normal"], mps["min_dist"],
                mps["max_dist"], (seed, "sim3 pose"))


def test_gate_planted_edges():
    cases = FC.planted_gate()
    wp, nr = np.array([c[1] for c in cases], F), np.array([c[2] for c in cases], F)
    mn, mx = np.array([c[3] for c in cases], F), np.array([c[4] for c in cases], F)
    ok, level = _check_gate(FC.IDENTITY, np.zeros(3, F), FC.K0, FC.BOUNDS0, 3.0, FC.SF, FC.LOG_SF, wp, nr, mn, mx, "planted")
    for i, c in enumerate(cases):
        assert ok[i] == c[5], c[0]
        assert c[6] is None or level[i] == c[6], c[0]
        assert ok[i] or level[i] == -1, c[0]


def test_gate_refuses_bad_arguments():
    from orb_slam2_ssd_semantic_amd import _ffi, mapping
    cam = mapping.camera(*FC.K0, *FC.BOUNDS0)
    z = np.zeros((1, 3), F)
    with pytest.raises(_ffi.OrbfeError):
        mapping.fuse_gate_points(FC.IDENTITY, np.zeros(3, F), cam, 3.0, FC.SF, FC.LOG_SF, z, z, np.zeros(1, F), np.ones(1, F), mode=2)
    q, level, ok = mapping.fuse_gate_points(FC.IDENTITY, np.zeros(3, F), cam, 3.0, FC.SF, FC.LOG_SF, np.zeros((0, 3), F), np.zeros((0, 3), F),
                                            np.zeros(0, F), np.zeros(0, F))
    assert len(q) == len(level) == len(ok) == 0
    assert mapping.fuse_scratch_bytes(1000, 20, 1000) > 0
    for bad in ((10, 1, 15361), (10, 1, 0), (10, 1 << 25, 1), (-1, 1, 10)):
        with pytest.raises(ValueError):
            mapping.fuse_scratch_bytes(*bad)


def _oracle_pair(kf, mps, th, mode, Scw=None):
    tmap, idx, skip, slot, nobs = FC.tables(kf, mps, mode)
    T, Ow = FC.pose_of(kf, mode, Scw)
    return FO.fuse_pair(kf, T, Ow, tmap, idx, skip, slot, nobs, th, mode), (tmap, idx, slot, nobs)


@needs_ref
@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_oracle_equals_compiled_reference_plain(seed):
    """the oracle's gate + search drive the serial replay on the mock: everything ref_fuse returns; the action codes equal what the
    serial loop did wherever they are not DEFERRED, and DEFERRED is exactly "an earlier match to this slot had code 1-3" """
    kf, mps, th = FC.seed_case(seed)
    o, (tmap, idx, slot, nobs) = _oracle_pair(kf, mps, th, FO.PLAIN)
    ka, mr, orr, nf, s_action, s_other = FO.mock_replay_plain(kf, mps, o["match"])
    rka, rmr, rorr, rv = R.fuse(kf, mps, th)
    assert nf == rv == o["nfused"] and np.array_equal(ka, rka) and np.array_equal(mr, rmr) and np.array_equal(orr, rorr), seed
    live = {}
    for i, (a, m) in enumerate(zip(o["action"], o["match"])):
        earlier = live.get(int(m), None) if m >= 0 else None
        if a == FO.DEFERRED:
            assert earlier is not None and o["other"][i] == earlier, (seed, i)
        else:
            assert earlier is None and a == s_action[i] and o["other"][i] == s_other[i], (seed, i, a, s_action[i])
            if a in (FO.ADD, FO.REPLACE_SLOT, FO.REPLACE_POINT):
                live[int(m)] = i


@needs_ref
@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_oracle_equals_compiled_reference_sim3(seed):
    kf, mps, th = FC.seed_case(seed)
    Scw = FC.scw_of(kf, [1.0, 0.8, 1.3][seed % 3])
    o, _ = _oracle_pair(kf, mps, th, FO.SIM3, Scw)
    ka, rp, nf = FO.sim3_result(kf, len(mps["bad"]), o["match"], o["action"], o["other"])
    rka, rrp, rv = R.fuse_sim3(kf, Scw, mps, th)
    assert nf == rv == o["nfused"] and np.array_equal(ka, rka) and np.array_equal(rp, rrp), seed
    assert not (o["action"] == FO.DEFERRED).any()


def test_actions_on_a_planted_list():
    """two and three entries on one slot, equal observation counts, a bad slot point hit twice: plain and Sim3 codes by hand"""
    #        slot: 0 empty, 1 good (3 obs), 2 bad, 3 good (2 obs)
    slot = np.array([-1, 10, 11, 12], np.int32)
    bad = np.zeros(13, np.uint8)
    bad[11] = 1
    nobs = np.zeros(13, np.int32)
    nobs[10], nobs[12], nobs[4], nobs[5], nobs[6] = 3, 2, 1, 5, 2
    match = np.array([0, 0, -1, 0, 1, 1, 3, 2, 2], np.int32)
    idx = np.arange(9, dtype=np.int32)
    a, o, nf, first = FO.actions(FO.PLAIN, match, idx, slot, bad, nobs, 4)
    assert a.tolist() == [FO.ADD, FO.DEFERRED, FO.NONE, FO.DEFERRED, FO.REPLACE_POINT, FO.DEFERRED, FO.REPLACE_SLOT, FO.COUNTED, FO.COUNTED]
    assert o.tolist() == [-1, 0, -1, 0, 10, 4, 12, -1, -1] and nf == 8 and first.tolist() == [0, 4, 7, 6]
    a, o, nf, _ = FO.actions(FO.SIM3, match, idx, slot, bad, nobs, 4)
    R6 = FO.REPLACE_CANDIDATE
    assert a.tolist() == [FO.ADD, R6, FO.NONE, R6, R6, R6, R6, FO.COUNTED, FO.COUNTED] and o.tolist() == [-1, 0, -1, 0, 10, 10, 12, -1, -1] and nf == 8


def test_candidates_oracle_on_planted_lists():
    slot = np.array([[3, -1, 5, 3, 9], [5, 7, 2, -1, 1], [-1, -1, -1, -1, -1]], np.int32)
    n = np.array([5, 4, 5], np.int32)
    bad = np.zeros(10, np.uint8)
    bad[7] = 1
    cand, skip = FO.candidates(slot, n, [0, 1, 2, 0], bad, cur_kf=1)
    assert cand.tolist() == [3, 5, 9, 2] and skip.tolist() == [0, 1, 0, 1]
    cand, skip = FO.candidates(slot, n, [1, 0], bad)
    assert cand.tolist() == [5, 2, 3, 9] and not skip.any()
    assert len(FO.candidates(slot, n, [], bad)[0]) == 0


@pytest.mark.parametrize("mode", [FO.PLAIN, FO.SIM3])
def test_pair_lookup_lists_reach_their_edges(mode):
    """empty pairs between full ones, no boundary on a multiple of 4 (the waves of a search workgroup), and a match at position
    1024 of the long list whose slot an entry below 1024 matched first: the collision across the replay's stride"""
    L = FC.pair_lookup(mode)
    lengths = [len(s) for s in L["sels"]]
    assert tuple(lengths) == FC.PAIR_LOOKUP_LENGTHS and L["rows"] == [0, 1] * 4 + [0]
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert 0 in lengths[1:-1] and lengths[0] == lengths[-1] == 0          # empty pairs first, last and between full ones
    assert sum(1 for o in set(off.tolist()) if o % 4) >= 3              # boundaries inside a search workgroup's four entries
    fused = 0
    for row, sel in zip(L["rows"], L["sels"]):
        kf, mps = L["cases"][row]
        tmap, idx, skip, slot, nobs = FC.tables(kf, mps, mode)
        T, Ow = FC.pose_of(kf, mode, L["S"][row])
        r = FO.fuse_pair(kf, T, Ow, tmap, idx[sel], skip[sel], slot, nobs, 3.0, mode)
        fused += r["nfused"] > 0
        if len(sel) == 0:
            assert r["nfused"] == 0 and (r["first"] == -1).all()
        if len(sel) > FC.PAIR_LOOKUP_STRIDE:
            s, m = FC.PAIR_LOOKUP_STRIDE, r["match"]
            assert len(sel) == s + 1 and m[s] >= 0 and 0 <= r["first"][m[s]] < s and sel[r["first"][m[s]]] == sel[s]
            assert r["action"][s] == (FO.DEFERRED if mode == FO.PLAIN else FO.REPLACE_CANDIDATE)
            if mode == FO.PLAIN:
                assert r["other"][s] == r["first"][m[s]]
            assert (m[:s] >= 0).sum() > 100
    assert fused >= 3


@pytest.mark.parametrize("ntargets, cap", [(64, 4096), (64, 4100), (65, 4096)])
def test_candidates_cases_cross_the_scan_chunk(ntargets, cap):
    """1024, 1025 and 1040 blocks of 256 positions: candidates on both sides of block 1024, repeats of earlier points behind it
    (dropped) and points that first occur behind it (kept), a short row, bad points, points of the current keyframe"""
    c = FC.candidates_case(ntargets, cap)
    slot, n, bad = c["slot"], c["n"], c["bad"]
    total, edge = ntargets * cap, FC.CAND_SCAN * FC.CAND_BLOCK
    assert (total + FC.CAND_BLOCK - 1) // FC.CAND_BLOCK == {(64, 4096): 1024, (64, 4100): 1025, (65, 4096): 1040}[(ntargets, cap)]
    assert slot.shape == (ntargets + 1, cap) and len(bad) == FC.CAND_NPOINTS and (n[:ntargets] < cap).sum() == 1
    assert 0.04 < bad.mean() < 0.06
    wc, ws = FO.candidates(slot, n, list(c["targets"]), bad, c["cur"])
    assert len(wc) > 100_000 and len(set(wc.tolist())) == len(wc) and 0 < ws.sum() < len(wc)
    flat = slot[:ntargets].reshape(-1)
    first = {}
    for j in np.flatnonzero(flat >= 0)[::-1]:
        if j % cap < n[j // cap]:
            first[int(flat[j])] = int(j)
    pos = np.array([first[int(p)] for p in wc])
    assert (np.diff(pos) > 0).all()                       # the candidates stand in position order
    if total > edge:
        late = flat[edge:]
        late = late[late >= 0]
        assert (pos >= edge).sum() > 50 and (pos < edge).sum() > 100_000
        assert sum(first[int(p)] < edge for p in late if not bad[p]) > 50   # repeats behind the edge of points in front of it
    else:
        assert pos.max() < edge
