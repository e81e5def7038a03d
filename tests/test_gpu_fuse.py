"""ORBmatcher::Fuse x2 for a batch of (keyframe, list) pairs on the device (csrc/orbfe_fuse.hip): search, replay and vpFuseCandidates
bit for bit against tests/fuse_oracle.py -- which tests/test_fuse_oracle.py holds against the compiled reference -- and, where
oracle/_ref is built, against ref_fuse / ref_fuse_sim3 themselves.  No tolerances.  Outputs start as sentinels with a guard band
behind them, so what must not be written shows."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_oracle as FO
import proj_cases as PC
from oracle import ref_ffi as R

pytestmark = pytest.mark.gpu

F = np.float32
SENT, GUARD = -7, 64
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm(mt):
    from orb_slam2_ssd_semantic_amd import LocalMapper
    return LocalMapper(mt)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Block:
    """keyframes on the device: records, descriptors, counts, uRight and the grid orbfe_assign_grid_batch_device builds"""

    def __init__(self, mt, kfs, cap=None):
        import torch
        from orb_slam2_ssd_semantic_amd import KP_DTYPE, tracking
        self.kfs, B = kfs, len(kfs)
        nmax = max(max(len(k["octave"]) for k in kfs), 1)
        self.cap = cap = cap or (nmax + 3 if nmax + 3 <= 15360 else nmax)
        blk = np.zeros((B, cap), KP_DTYPE)
        blk["x"], blk["y"], blk["octave"] = 100.0, 100.0, 0   # rows past a keyframe's count would be candidates if they were read
        desc, ur = np.zeros((B, cap, 32), np.uint8), np.full((B, cap), -1.0, F)
        n = np.zeros(B, np.int32)
        for b, k in enumerate(kfs):
            m = n[b] = len(k["octave"])
            blk["x"][b, :m], blk["y"][b, :m] = k["xy"][:, 0], k["xy"][:, 1]
            blk["octave"][b, :m] = k["octave"]
            desc[b, :m], ur[b, :m] = k["desc"], k["uRight"]
        k0 = kfs[0]
        self.t = dict(kps=_dev(blk.view(np.uint8).reshape(B, cap, -1)), desc=_dev(desc), n=_dev(n), ur=_dev(ur),
                      off=torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda"), idx=torch.zeros((B, cap), dtype=torch.int32, device="cuda"),
                      nin=torch.zeros((B,), dtype=torch.int32, device="cuda"))
        minx, maxx, miny, maxy = [float(v) for v in k0["bounds"]]
        t = self.t
        mt.AssignFeaturesToGrid_batch_device(t["kps"].data_ptr(), t["n"].data_ptr(), cap, B, minx, miny, float(k0["gw_inv"]), float(k0["gh_inv"]),
                                             t["off"].data_ptr(), t["idx"].data_ptr(), t["nin"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        self.frames = tracking.frames_struct(t["kps"], t["desc"], t["n"], cap, t["off"], t["idx"], minx, miny, k0["gw_inv"], k0["gh_inv"], d_uright=t["ur"])
        self.cam = tracking.camera(*[float(v) for v in k0["K"][:5]], minx, maxx, miny, maxy)
        self.B = B


class World:
    """the flat map of several fuse_case-style (kf, mps): per case the list's points, then the keyframe's own; the slot table"""

    def __init__(self, cases, cap, mode=FO.PLAIN):
        self.tabs, self.base = [], []
        at = 0
        for kf, mps in cases:
            self.tabs.append(FC.tables(kf, mps, mode))
            self.base.append(at)
            at += len(self.tabs[-1][0]["bad"])
        self.npts = at
        self.tmap = {k: np.concatenate([t[0][k] for t in self.tabs]) for k in self.tabs[0][0]} if cases else None
        self.nobs = np.concatenate([t[4] for t in self.tabs])
        self.slot = np.full((len(cases), cap), -1, np.int32)
        for b, t in enumerate(self.tabs):
            self.slot[b, :len(t[3])] = np.where(t[3] >= 0, t[3] + self.base[b], -1)

    def list_of(self, b, sel=None):
        """(list_idx, list_skip) of case b in global indices, optionally a selection / reordering of its entries"""
        idx, skip = self.tabs[b][1], self.tabs[b][2]
        idx = np.where(idx >= 0, idx + self.base[b], -1).astype(np.int32)
        return (idx, skip) if sel is None else (idx[sel], skip[sel])

    def upload(self):
        from orb_slam2_ssd_semantic_amd import _ffi
        m = self.tmap
        self.d = dict(wp=_dev(m["world_pos"]), nr=_dev(m["normal"]), mn=_dev(m["min_dist"]), mx=_dev(m["max_dist"]), bad=_dev(m["bad"]),
                      desc=_dev(m["desc"]), nobs=_dev(self.nobs), slot=_dev(self.slot))
        d = self.d
        self.struct = _ffi.TrackMap(d["wp"].data_ptr(), d["nr"].data_ptr(), d["mn"].data_ptr(), d["mx"].data_ptr(), d["bad"].data_ptr(), None,
                                    d["desc"].data_ptr(), self.npts)
        return self


def _run(lm, blk, world, pairs, th, mode, th_low=50, first=True, use_slots=True):
    """pairs: [(keyframe row, T [3][4], Ow [3], list_idx, list_skip)] -> the outputs as numpy, guard bands checked"""
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi, mapping
    P = len(pairs)
    off = np.concatenate([[0], np.cumsum([len(p[3]) for p in pairs])]).astype(np.uint32)
    ne = int(off[-1])
    idx = np.concatenate([p[3] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    skip = np.concatenate([p[4] for p in pairs] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    T = np.array([np.asarray(p[1], F).reshape(12) for p in pairs], F).reshape(P, 12)
    Ow = np.array([np.asarray(p[2], F).reshape(3) for p in pairs], F).reshape(P, 3)
    d = [_dev(np.array([p[0] for p in pairs], np.int32)), _dev(T), _dev(Ow), _dev(off.view(np.int32)), _dev(idx) if ne else None, _dev(skip) if ne else None]
    lists = mapping.fuse_lists_struct(d[0], d[1], d[2], d[3], d[4], ne, P, d[5])
    i32 = dict(dtype=torch.int32, device="cuda")
    o = dict(match=torch.full((ne + GUARD,), SENT, **i32), dist=torch.full((ne + GUARD,), SENT, **i32),
             action=torch.full((ne + GUARD,), 200, dtype=torch.uint8, device="cuda"), other=torch.full((ne + GUARD,), SENT, **i32),
             nfused=torch.full((P + GUARD,), SENT, **i32), first=torch.full((P * blk.cap + GUARD,), SENT, **i32))
    out = _ffi.FuseOut(o["match"].data_ptr(), o["dist"].data_ptr(), o["action"].data_ptr(), o["other"].data_ptr(), o["nfused"].data_ptr(),
                       o["first"].data_ptr() if first else None)
    k0 = blk.kfs[0]
    lm.Fuse_batch_device(blk.frames, blk.B, lists, blk.cam, world.struct, world.d["nobs"].data_ptr(), world.d["slot"].data_ptr() if use_slots else None,
                         th, k0["scale_factors"], k0["inv_sigma2"], k0["log_scale"], out, mode, th_low, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    sizes = dict(match=ne, dist=ne, action=ne, other=ne, nfused=P, first=P * blk.cap if first else 0)
    for k, n in sizes.items():
        assert (h[k][n:] == (200 if k == "action" else SENT)).all(), (k, "written past its end")
        h[k] = h[k][:n]
    h["off"] = off
    return h


def _want(blk, world, pairs, th, mode, th_low=50, use_slots=True):
    res = [FO.fuse_pair(blk.kfs[p[0]], np.asarray(p[1], F).reshape(3, 4), np.asarray(p[2], F).reshape(3), world.tmap, p[3], p[4],
                        world.slot[p[0]] if use_slots else None, world.nobs, th, mode, th_low, cap=blk.cap) for p in pairs]
    w = {k: np.concatenate([np.atleast_1d(r[k]) for r in res]) for k in ("match", "dist", "action", "other", "nfused", "first")}
    return w, res


def _same(got, want, what):
    for k in ("match", "dist", "action", "other", "nfused", "first"):
        if len(got[k]) or k != "first":
            assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8] if len(got[k]) == len(want[k]) else "length")


def _pair(b, kf, lst, mode=FO.PLAIN, Scw=None):
    T, Ow = FC.pose_of(kf, mode, Scw)
    return (b, T, Ow, lst[0], lst[1])


@pytest.fixture(scope="module")
def two(mt):
    """two fuse_case keyframes (300 and 1000 features) with 400-point lists, uploaded once"""
    cases = [FC.seed_case(10)[:2], FC.seed_case(11)[:2]]
    blk = Block(mt, [c[0] for c in cases])
    return cases, blk, World(cases, blk.cap).upload()


# ------------------------------------------------------------------------------------------------ list lengths, pairs, repeat
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_list_lengths(lm, two, n):
    cases, blk, world = two
    sel = np.arange(n) + 40
    for mode in (FO.PLAIN, FO.SIM3):
        Scw = FC.scw_of(cases[0][0], 1.25)
        pairs = [_pair(0, cases[0][0], world.list_of(0, sel), mode, Scw)]
        got, (want, _) = _run(lm, blk, world, pairs, 3.0, mode), _want(blk, world, pairs, 3.0, mode)
        _same(got, want, (n, mode))
        assert n < 63 or want["nfused"][0] > 0


def test_three_pairs_one_keyframe_in_two_and_a_second_call(lm, two):
    """pair 2 fuses pair 0's list in reverse order into the same keyframe: other first matchers, the same matches; a second call
    writes the same bytes"""
    cases, blk, world = two
    rev = np.arange(400)[::-1].copy()
    for mode in (FO.PLAIN, FO.SIM3):
        S = [FC.scw_of(c[0], 0.9) for c in cases]
        pairs = [_pair(0, cases[0][0], world.list_of(0), mode, S[0]), _pair(1, cases[1][0], world.list_of(1), mode, S[1]),
                 _pair(0, cases[0][0], world.list_of(0, rev), mode, S[0])]
        got, (want, res) = _run(lm, blk, world, pairs, 3.0, mode), _want(blk, world, pairs, 3.0, mode)
        _same(got, want, mode)
        assert np.array_equal(res[2]["match"][::-1], res[0]["match"]) and not np.array_equal(res[2]["action"][::-1], res[0]["action"])
        again = _run(lm, blk, world, pairs, 3.0, mode)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), mode
        # the search alone gives the same matches
        import torch
        from orb_slam2_ssd_semantic_amd import mapping
        ne = len(got["match"])
        m2, d2 = torch.full((ne,), SENT, dtype=torch.int32, device="cuda"), torch.full((ne,), SENT, dtype=torch.int32, device="cuda")
        off = _dev(got["off"].view(np.int32))
        idx, skip = _dev(np.concatenate([p[3] for p in pairs])), _dev(np.concatenate([p[4] for p in pairs]))
        dT, dO = _dev(np.array([p[1].reshape(12) for p in pairs], F)), _dev(np.array([p[2] for p in pairs], F))
        dk = _dev(np.array([p[0] for p in pairs], np.int32))
        k0 = blk.kfs[0]
        lm.FuseSearch_batch_device(blk.frames, blk.B, mapping.fuse_lists_struct(dk, dT, dO, off, idx, ne, 3, skip), blk.cam, world.struct, 3.0,
                                   k0["scale_factors"], k0["inv_sigma2"], k0["log_scale"], m2.data_ptr(), d2.data_ptr(), mode)
        torch.cuda.synchronize()
        assert np.array_equal(m2.cpu().numpy(), got["match"]) and np.array_equal(d2.cpu().numpy(), got["dist"])


# ------------------------------------------------------------------------------------------------ planted windows, gates, replay
def _planted():
    """one keyframe under the identity pose and one list; (kf, mps, names) with names[i] = (what the entry is, feature it must match in
    the plain overload, in the Sim3 overload; None = no assertion beyond the oracle)"""
    feats, pts = [], []

    def feat(x, y, octave=0, nbits=0, ur=-1.0, state=0, obs=0):
        feats.append((x, y, octave, FC.bits(nbits), ur, state, obs))
        return len(feats) - 1

    def pt(name, u, v, plain, sim3, **kw):
        pts.append((name, plain, sim3, FC.point(u, v, **kw)))
    pt("empty window", 40, 40, -1, -1)
    feat(101, 40, 0), feat(99, 41, 5)
    pt("every candidate fails the level filter", 100, 40, -1, -1, level=3)
    feat(201, 40, 1, 0)
    lm1 = feat(199, 40, 2, 5)
    feat(200, 41, 3, 7), feat(200, 39, 4, 0)
    pt("levels level - 2 .. level + 1", 200, 40, lm1, lm1, level=3)
    a = feat(304, 44, 0, 9)                        # PosInGrid rounds: both in cell (30, 4)
    feat(304.5, 44.25, 0, 9)
    pt("tie inside one lane's share (one cell)", 305, 45, a, a)
    feat(406.5, 45, 0, 9)                          # cell (41, 4 or 5)
    e = feat(403.5, 45, 0, 9)                      # cell (40, .): the higher index comes first in the walk (smaller ix)
    pt("tie across lanes", 405, 45, e, e)
    g1 = feat(102.5, 200, 0, 3)                    # e2 = 6.25 > 5.99: out in the plain overload
    g2 = feat(100, 202.25, 0, 10)                  # e2 = 5.0625: in
    pt("chi2, monocular candidates", 100, 200, g2, g1)
    s1 = feat(102, 300, 0, 4, ur=58.25)            # ur = 100 - 40 = 60: e2 = 4 + 3.0625 = 7.0625, between 5.99 and 7.8: in
    s2 = feat(100, 302, 0, 1, ur=62.25)            # e2 = 4 + 5.0625 = 9.0625 > 7.8: out
    pt("chi2, stereo candidates", 100, 300, s1, s2)
    h1 = feat(300, 300, 0, 50)
    pt("bestDist == th_low", 300, 300, h1, h1)
    feat(400, 300, 0, 51)
    pt("bestDist == th_low + 1", 400, 300, -1, -1)
    r1 = feat(100, 400, 0, 2)
    for k in range(3):
        pt("empty slot, entry %d" % k, 100, 400, r1, r1, obs=k)
    r2 = feat(200, 400, 0, 2, state=1, obs=3)
    pt("good slot, equal counts", 200, 400, r2, r2, obs=3)
    pt("good slot, second entry", 200, 400, r2, r2, obs=0)
    r3 = feat(300, 400, 0, 2, state=2, obs=9)
    pt("bad slot, first hit", 300, 400, r3, r3)
    pt("bad slot, second hit", 300, 400, r3, r3, obs=20)
    r4 = feat(400, 400, 0, 2, state=1, obs=5)
    pt("good slot with more observations", 400, 400, r4, r4, obs=1)
    pt("a bad point", 100, 400, -1, -1, bad=1)
    f = np.array([x[:2] for x in feats], F)
    kf = FC.mini_kf(f, [x[2] for x in feats], [x[3] for x in feats], [x[4] for x in feats], [x[5] for x in feats], [x[6] for x in feats])
    return kf, FC.points([p[3] for p in pts]), [(p[0], p[1], p[2]) for p in pts], dict(r1=r1, r2=r2, r3=r3, r4=r4)


def test_planted_windows_gates_and_replay(mt, lm):
    kf, mps, names, r = _planted()
    nmp, nKF = len(names), len(kf["octave"])
    blk = Block(mt, [kf])
    world = World([(kf, mps)], blk.cap).upload()
    idx, skip = world.list_of(0)
    # behind the planted entries: a NULL pointer, indices past the map, a skipped copy of a matching entry
    idx = np.concatenate([idx, [-1, world.npts, 1 << 30, 9]]).astype(np.int32)
    skip = np.concatenate([skip, [0, 0, 0, 1]]).astype(np.uint8)
    by = {n[0]: i for i, n in enumerate(names)}
    for mode in (FO.PLAIN, FO.SIM3):
        pairs = [(0, FC.IDENTITY, np.zeros(3, F), idx, skip)]
        got, (want, _) = _run(lm, blk, world, pairs, 3.0, mode), _want(blk, world, pairs, 3.0, mode)
        _same(got, want, mode)
        for i, (name, plain, sim3) in enumerate(names):
            assert got["match"][i] == (plain if mode == FO.PLAIN else sim3), (mode, name, got["match"][i], got["dist"][i])
        assert (got["match"][nmp:] == -1).all() and (got["dist"][nmp:] == 256).all() and (got["action"][nmp:] == FO.NONE).all()
        assert got["dist"][by["empty window"]] == 256 and got["dist"][by["every candidate fails the level filter"]] == 256
        assert got["dist"][by["bestDist == th_low"]] == 50 and got["dist"][by["bestDist == th_low + 1"]] == 51
        a, o = got["action"], got["other"]
        e0, g0, b0 = by["empty slot, entry 0"], by["good slot, equal counts"], by["bad slot, first hit"]
        if mode == FO.PLAIN:
            assert a[e0:e0 + 3].tolist() == [FO.ADD, FO.DEFERRED, FO.DEFERRED] and o[e0:e0 + 3].tolist() == [-1, e0, e0]
            assert a[g0:g0 + 2].tolist() == [FO.REPLACE_SLOT, FO.DEFERRED] and o[g0:g0 + 2].tolist() == [nmp + r["r2"], g0]
            assert a[by["good slot with more observations"]] == FO.REPLACE_POINT and o[by["good slot with more observations"]] == nmp + r["r4"]
        else:
            assert a[e0:e0 + 3].tolist() == [FO.ADD, FO.REPLACE_CANDIDATE, FO.REPLACE_CANDIDATE] and o[e0:e0 + 3].tolist() == [-1, e0, e0]
            assert a[g0:g0 + 2].tolist() == [FO.REPLACE_CANDIDATE] * 2 and o[g0:g0 + 2].tolist() == [nmp + r["r2"]] * 2
        assert a[b0:b0 + 2].tolist() == [FO.COUNTED, FO.COUNTED] and o[b0:b0 + 2].tolist() == [-1, -1]
        assert got["nfused"][0] == (got["match"] >= 0).sum() and got["first"][r["r1"]] == e0 and got["first"][r["r3"]] == b0
        # th_low moves the acceptance, not the distance; without the slot table every slot is empty
        lo, (wlo, _) = _run(lm, blk, world, pairs, 3.0, mode, th_low=49), _want(blk, world, pairs, 3.0, mode, th_low=49)
        _same(lo, wlo, (mode, "th_low 49"))
        assert lo["match"][by["bestDist == th_low"]] == -1 and lo["dist"][by["bestDist == th_low"]] == 50
        ns, (wns, _) = _run(lm, blk, world, pairs, 3.0, mode, use_slots=False), _want(blk, world, pairs, 3.0, mode, use_slots=False)
        _same(ns, wns, (mode, "no slot table"))
        assert ns["action"][g0] == FO.ADD and ns["action"][b0] == FO.ADD


def test_tie_inside_one_lanes_share_across_cells(mt, lm):
    """th = 40 at level 0: a 10 x 10 cell window, two cells per lane; the tied candidates sit in cells 2 and 3 of the walk (both lane
    1's), the later one with the lower feature index.  Sim3 mode: no reprojection gate at that radius."""
    xy = np.array([(464, 228), (464, 218), (520, 250)], F)
    kf = FC.mini_kf(xy, [0, 0, 0], [FC.bits(9), FC.bits(9), FC.bits(30)])
    mps = FC.points([FC.point(503, 247)])
    blk = Block(mt, [kf])
    world = World([(kf, mps)], blk.cap, FO.SIM3).upload()
    pairs = [(0, FC.IDENTITY, np.zeros(3, F), *world.list_of(0))]
    g = FO.gate_point(FC.IDENTITY, np.zeros(3, F), FC.K0, FC.BOUNDS0, 40.0, FC.SF, FC.LOG_SF, mps["world_pos"][0], mps["normal"][0], 0, mps["max_dist"][0], 0)
    assert FO.features_in_area(kf, g["u"], g["v"], g["r"]) == [1, 0, 2]
    got, (want, _) = _run(lm, blk, world, pairs, 40.0, FO.SIM3), _want(blk, world, pairs, 40.0, FO.SIM3)
    _same(got, want, "tie")
    assert got["match"][0] == 1 and got["dist"][0] == 9


def test_largest_keyframe(mt, lm):
    """n == cap == 15360 (the LDS table of the replay at its limit) and ten entries"""
    rng = np.random.default_rng(5150)
    kf, mps = PC.fuse_case(rng, 15360, 10)
    mps["null"][:] = 0
    mps["bad"][:] = 0
    mps["in_kf"][:] = 0
    blk = Block(mt, [kf])
    assert blk.cap == 15360
    world = World([(kf, mps)], blk.cap).upload()
    for mode in (FO.PLAIN, FO.SIM3):
        pairs = [_pair(0, kf, world.list_of(0), mode, FC.scw_of(kf, 1.0))]
        got, (want, _) = _run(lm, blk, world, pairs, 5.0, mode), _want(blk, world, pairs, 5.0, mode)
        _same(got, want, mode)
        assert want["nfused"][0] >= 1


@pytest.mark.parametrize("seed", [5, 6])
def test_numpy_convenience(lm, seed):
    """LocalMapper.fuse_device uploads one fuse_case and returns what the oracle computes, in both modes"""
    kf, mps, th = FC.seed_case(seed)
    for mode in (FO.PLAIN, FO.SIM3):
        Scw = FC.scw_of(kf, 1.1)
        tmap, idx, skip, slot, nobs = FC.tables(kf, mps, mode)
        T, Ow = FC.pose_of(kf, mode, Scw)
        w = FO.fuse_pair(kf, T, Ow, tmap, idx, skip, slot, nobs, th, mode)
        match, dist, action, other, nfused = lm.fuse_device(kf, mps, th, mode, Scw)
        assert nfused == w["nfused"] and all(np.array_equal(a, w[k]) for a, k in ((match, "match"), (dist, "dist"), (action, "action"), (other, "other")))


def test_limits_refused_and_the_handle_stays_usable(lm, two):
    from orb_slam2_ssd_semantic_amd import OrbfeError, _ffi, mapping, tracking
    cases, blk, world = two
    k0 = blk.kfs[0]
    pairs = [_pair(0, cases[0][0], world.list_of(0))]
    t = blk.t
    lists = mapping.fuse_lists_struct(t["n"], t["ur"], t["ur"], t["off"], t["idx"], 10, 1)
    tens, out = lm.alloc_fuse_out(16, 1, blk.cap)

    def call(frames=blk.frames, lists=lists, sf=k0["scale_factors"], s2=k0["inv_sigma2"], th_low=50, mode=FO.PLAIN):
        lm.Fuse_batch_device(frames, blk.B, lists, blk.cam, world.struct, world.d["nobs"].data_ptr(), world.d["slot"].data_ptr(), 3.0, sf, s2,
                             k0["log_scale"], out, mode, th_low)
    big = tracking.frames_struct(t["kps"], t["desc"], t["n"], 15361, t["off"], t["idx"], 0, 0, 0.1, 0.1)
    many = mapping.fuse_lists_struct(t["n"], t["ur"], t["ur"], t["off"], t["idx"], (1 << 25) + 1, 1)
    neg = mapping.fuse_lists_struct(t["n"], t["ur"], t["ur"], t["off"], t["idx"], -1, 1)
    for kw in (dict(frames=big), dict(lists=many), dict(lists=neg), dict(sf=np.ones(17, F), s2=np.ones(17, F)), dict(th_low=256), dict(th_low=-1),
               dict(mode=2)):
        with pytest.raises(OrbfeError) as ei:
            call(**kw)
        assert ei.value.status == _ffi.ORBFE_ERR_ARG, kw
    with pytest.raises(OrbfeError):
        lm.FuseCandidates_device(world.d["slot"].data_ptr(), t["n"].data_ptr(), 2, 15361, t["n"].data_ptr(), 1, -1, world.d["bad"].data_ptr(), 10,
                                 t["idx"].data_ptr(), None, 10, t["nin"].data_ptr())
    with pytest.raises(OrbfeError):
        lm.FuseCandidates_device(world.d["slot"].data_ptr(), t["n"].data_ptr(), 2, 4096, t["n"].data_ptr(), 1 << 13, -1, world.d["bad"].data_ptr(), 10,
                                 t["idx"].data_ptr(), None, 10, t["nin"].data_ptr())
    got, (want, _) = _run(lm, blk, world, pairs, 3.0, FO.PLAIN), _want(blk, world, pairs, 3.0, FO.PLAIN)
    _same(got, want, "after the refusals")
    assert want["nfused"][0] > 50
    # a keyframe row outside the block cannot be refused without a host read: that pair matches nothing, its neighbour is untouched
    for row in (blk.B, -1, 1 << 30):
        out = _run(lm, blk, world, [(row,) + pairs[0][1:], pairs[0]], 3.0, FO.PLAIN)
        n0 = len(pairs[0][3])
        assert (out["match"][:n0] == -1).all() and (out["dist"][:n0] == 256).all() and (out["action"][:n0] == FO.NONE).all()
        assert (out["other"][:n0] == -1).all() and out["nfused"].tolist() == [0, want["nfused"][0]] and (out["first"][:blk.cap] == -1).all()
        assert np.array_equal(out["match"][n0:], want["match"]) and np.array_equal(out["action"][n0:], want["action"])


# ------------------------------------------------------------------------------------------------ against the compiled reference
NSEEDS, GROUP = 40, 8


@needs_ref
def test_seeds_equal_the_compiled_reference(mt, lm):
    """40 fuse_case seeds, eight per call.  Plain: the serial replay on the mock driven by the DEVICE's d_match == everything ref_fuse
    returns.  Sim3: the device's action codes == everything ref_fuse_sim3 returns.  Both: device == oracle everywhere."""
    fused, counts = 0, np.zeros(7, np.int64)
    for g0 in range(0, NSEEDS, GROUP):
        seeds = range(g0, g0 + GROUP)
        cases = [FC.seed_case(s) for s in seeds]
        blk = Block(mt, [c[0] for c in cases], cap=1000)
        for mode in (FO.PLAIN, FO.SIM3):
            world = World([c[:2] for c in cases], blk.cap, mode).upload()
            S = [FC.scw_of(c[0], [1.0, 0.8, 1.3][s % 3]) for s, c in zip(seeds, cases)]
            pairs = [_pair(b, c[0], world.list_of(b), mode, S[b]) for b, c in enumerate(cases)]
            th = 3.0 if mode == FO.PLAIN else 4.0
            got, (want, _) = _run(lm, blk, world, pairs, th, mode, first=False), _want(blk, world, pairs, th, mode)
            want["first"] = got["first"]
            _same(got, want, (g0, mode))
            counts += np.bincount(got["action"], minlength=7)
            for b, (kf, mps, _) in enumerate(cases):
                e0, e1 = int(got["off"][b]), int(got["off"][b + 1])
                nmp, base = e1 - e0, world.base[b]
                if mode == FO.PLAIN:
                    ka, mr, orr, nf, _, _ = FO.mock_replay_plain(kf, mps, got["match"][e0:e1])
                    rka, rmr, rorr, rv = R.fuse(kf, mps, th)
                    assert nf == rv == got["nfused"][b] and np.array_equal(ka, rka) and np.array_equal(mr, rmr) and np.array_equal(orr, rorr), (g0, b)
                    fused += rv
                else:
                    other = np.where(got["other"][e0:e1] >= 0, got["other"][e0:e1] - base, -1)
                    ka, rp, nf = FO.sim3_result(kf, nmp, got["match"][e0:e1], got["action"][e0:e1], other)
                    rka, rrp, rv = R.fuse_sim3(kf, S[b], mps, th)
                    assert nf == rv == got["nfused"][b] and np.array_equal(ka, rka) and np.array_equal(rp, rrp), (g0, b)
    assert fused > 2000 and (counts >= 20).all(), (fused, counts)


# ------------------------------------------------------------------------------------------------ vpFuseCandidates
def _cands(lm, slot, n, targets, bad, cur=-1, cand_cap=None):
    import torch
    cand, skip, nc = lm.fuse_candidates_device(_dev(slot), _dev(n), _dev(np.asarray(targets, np.int32)) if len(targets) else torch.zeros(0, dtype=torch.int32, device="cuda"),
                                               _dev(bad), cur, cand_cap)
    torch.cuda.synchronize()
    return cand.cpu().numpy(), skip.cpu().numpy(), nc.cpu().numpy()


def _check_cands(lm, slot, n, targets, bad, cur=-1):
    cand, skip, nc = _cands(lm, slot, n, targets, bad, cur)
    wc, ws = FO.candidates(slot, n, list(targets), bad, cur)
    assert nc.tolist() == [len(wc), len(wc)] and np.array_equal(cand[:len(wc)], wc) and np.array_equal(skip[:len(wc)], ws)
    assert (cand[len(wc):] == -1).all()
    return wc


@pytest.mark.parametrize("survivors", [255, 256, 257])
def test_candidates_block_edges(lm, survivors):
    """the count lands on, before and behind a workgroup's 256 positions; bad first occurrences give way to later good ones"""
    rng = np.random.default_rng(survivors)
    cap, npts = 300, 600
    slot = np.full((4, cap), -1, np.int32)
    n = np.array([cap, 290, 0, cap], np.int32)
    good = rng.permutation(npts)[:survivors].astype(np.int32)
    bad = np.zeros(npts, np.uint8)
    bad[np.setdiff1d(np.arange(npts), good)[:40]] = 1
    badp = np.flatnonzero(bad).astype(np.int32)
    slot[0, :200] = np.concatenate([badp[:20], good[:180]])[rng.permutation(200)]
    rest = np.concatenate([good[180:], good[:60], badp[20:]])     # 60 repeats of keyframe 0's points, the other bad points
    slot[1, :len(rest)] = rest[rng.permutation(len(rest))]
    slot[3, :50] = good[100:150]                                   # the current keyframe: 50 of the candidates
    slot[3, 299] = good[0]
    assert len(rest) <= 290
    wc = _check_cands(lm, slot, n, [0, 1, 2], bad, cur=3)
    assert len(wc) == survivors and set(wc.tolist()) == set(good.tolist())
    _check_cands(lm, slot, n, [1, 0, 1], bad)


def test_candidates_planted(lm):
    slot = np.array([[3, -1, 5, 3, 9], [5, 7, 2, -1, 1], [-1, -1, -1, -1, -1], [5, 5, 5, 5, 5]], np.int32)
    n = np.array([5, 4, 5, 5], np.int32)
    bad = np.zeros(10, np.uint8)
    bad[7] = 1
    assert _check_cands(lm, slot, n, [], bad).tolist() == []                       # no targets
    assert _check_cands(lm, slot, n, [2], bad).tolist() == []                      # a target without points
    assert _check_cands(lm, slot, n, [0, 1, 3], bad, cur=1).tolist() == [3, 5, 9, 2]   # 5 sits in all targets; slot 4 of keyframe 1 is past its count
    assert _check_cands(lm, slot, n, [3, 9, -1, 0], bad).tolist() == [5, 3, 9]     # rows outside the block have no points
    bad[5] = 1
    assert _check_cands(lm, slot, n, [3, 0, 1], bad).tolist() == [3, 9, 2]         # bad first occurrences
    cand, skip, nc = _cands(lm, slot, n, [0, 1], bad, cand_cap=2)                   # a short output: the count is still whole
    assert nc.tolist() == [2, 3] and cand.tolist() == [3, 9]


# ------------------------------------------------------------------------------------------------ the device-resident chain
def test_chain_from_images_to_fuse(mt, lm):
    """ORBextractor batch -> orbfe_frame_geometry_batch_device (RGB-D) -> orbfe_assign_grid_batch_device -> Fuse_batch_device on one
    stream, device pointers only: keyframe 0's RGB-D points (unprojected by torch on the device) are fused into keyframe 1, whose
    image is keyframe 0's shifted by four pixels.  Afterwards everything is downloaded and held against the oracle."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera, ORBextractor, _ffi, mapping, tracking
    from orb_slam2_ssd_semantic_amd.synth import synth_frame
    B, w, h, z = 2, 640, 480, 2.0
    fx, fy, cx, cy, bf = 535.4, 539.2, 320.1, 247.6, 40.0
    base = synth_frame(77)
    imgs = np.stack([np.roll(base, 4 * j, axis=1) for j in range(B)])
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    cam_geo = Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), (), bf=bf)
    cam = mapping.camera(fx, fy, cx, cy, bf, 0.0, float(w), 0.0, float(h))
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    d_gray, d_depth = torch.from_numpy(imgs).cuda(), torch.full((B, h, w), z, dtype=torch.float32, device="cuda")
    d_kps, d_desc, d_n = torch.zeros((B, cap, 7), **i32), torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"), torch.zeros(B, **i32)
    d_off, d_idx, d_nin = torch.zeros((B, 64 * 48 + 1), **i32), torch.zeros((B, cap), **i32), torch.zeros(B, **i32)
    gwi, ghi = F(64) / F(w), F(48) / F(h)
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    d_un, d_dep, d_ur = cam_geo.frame_geometry(d_kps, d_n, cap, depth=d_depth, scale=1.0, stream=st)
    mt.AssignFeaturesToGrid_batch_device(d_un.data_ptr(), d_n.data_ptr(), cap, B, 0.0, 0.0, gwi, ghi, d_off.data_ptr(), d_idx.data_ptr(), d_nin.data_ptr(), st)
    # the map: keyframe 0's points, by torch on the same stream
    rec = d_un[0].view(torch.float32)
    zz = d_dep[0]
    P = torch.stack([(rec[:, 0] - F(cx)) / F(fx) * zz, (rec[:, 1] - F(cy)) / F(fy) * zz, zz], 1).contiguous()
    dist = P.norm(dim=1)
    normal = (P / dist.clamp_min(1e-6)[:, None]).contiguous()
    octv = d_un[0][:, 5].to(torch.float32)
    maxd = (dist * torch.pow(torch.tensor(1.2, device="cuda"), octv) * 0.97).contiguous()
    mind = torch.zeros_like(maxd)
    bad = ((torch.arange(cap, device="cuda") >= d_n[0]) | ~(zz > 0)).to(torch.uint8)
    tmap = _ffi.TrackMap(P.data_ptr(), normal.data_ptr(), mind.data_ptr(), maxd.data_ptr(), bad.data_ptr(), None, d_desc[0].data_ptr(), cap)
    T = np.concatenate([np.eye(3, dtype=F), np.array([[4 * z / fx], [0], [0]], F)], 1)
    d_T, d_O = _dev(T.reshape(1, 12)), _dev((-T[:, 3]).reshape(1, 3))
    d_pkf, d_loff, d_lidx = _dev(np.array([1], np.int32)), _dev(np.array([0, cap], np.int32)), torch.arange(cap, **i32)   # held until the sync
    lists = mapping.fuse_lists_struct(d_pkf, d_T, d_O, d_loff, d_lidx, cap, 1)
    frames = tracking.frames_struct(d_un, d_desc, d_n, cap, d_off, d_idx, 0.0, 0.0, gwi, ghi, d_uright=d_ur)
    sf = PC.scale_factors()
    s2 = (F(1) / (sf * sf)).astype(F)
    t, out = lm.alloc_fuse_out(cap, 1, cap, first=True)
    lm.Fuse_batch_device(frames, B, lists, cam, tmap, None, None, 3.0, sf, s2, FC.LOG_SF, out, FO.PLAIN, stream=st)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    un = d_un.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    kf = dict(desc=d_desc[1, :n[1]].cpu().numpy(), xy=np.stack([un["x"][1, :n[1]], un["y"][1, :n[1]]], 1), octave=un["octave"][1, :n[1]],
              uRight=d_ur[1, :n[1]].cpu().numpy(), K=(fx, fy, cx, cy, bf), bounds=(0.0, float(w), 0.0, float(h)), gw_inv=gwi, gh_inv=ghi,
              scale_factors=sf, inv_sigma2=s2, log_scale=FC.LOG_SF)
    hmap = dict(world_pos=P.cpu().numpy(), normal=normal.cpu().numpy(), min_dist=mind.cpu().numpy(), max_dist=maxd.cpu().numpy(),
                bad=bad.cpu().numpy(), desc=d_desc[0].cpu().numpy())
    want = FO.fuse_pair(kf, T, -T[:, 3], hmap, np.arange(cap, dtype=np.int32), None, None, np.zeros(cap, np.int32), 3.0, FO.PLAIN, cap=cap)
    for k in ("match", "dist", "action", "other", "first"):
        assert np.array_equal(t[k].cpu().numpy().reshape(-1), want[k]), k
    assert int(t["nfused"][0].item()) == want["nfused"] > 100
