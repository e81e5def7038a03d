"""The batched, device-resident SearchForTriangulation (csrc/orbfe_tri_search.hip) bit for bit against the CPU oracle's matching core
+ proj_cases.replay_triangulation and, where oracle/_ref is built, the compiled reference body (src/ORBmatcher.cc:827-1019): match12,
nmatches, the ordered pairs.  No tolerances.  Every output has a guard band of sentinels behind it; block rows past a keyframe's
count hold copies of its own features and FeatureVector padding that names real nodes, so reading them would make matches."""
import numpy as np
import pytest

import f12_oracle as FO
import proj_cases as PC
import tri_batch_cases as TC
from oracle import ref_ffi as R

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64
SENT = -7


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    yield m
    m.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["lds-tiles", "thread-per-feature"])
def lm(request, mt):
    """both search kernels: k_tri_search (default) and k_tri_search_flat"""
    from orb_slam2_ssd_semantic_amd import LocalMapper
    m = LocalMapper(mt)
    m.set_triangulation_kernel(request.param)
    yield m
    m.set_triangulation_kernel(0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _guarded(n, fill=SENT):
    import torch
    return torch.full((int(n) + GUARD,), fill, dtype=torch.int32, device="cuda")


def _body(t, shape):
    n = int(np.prod(shape))
    a = t.cpu().numpy()
    assert (a[n:] == SENT).all(), "guard band overwritten"
    return a[:n].reshape(shape)


def _key(c, *rest):
    return (id(c),) + rest


_EXPECTED = {}


def expected(c, th_low=50, only_stereo=False, check_ori=True):
    """oracle core + replay (cached per case object), asserted equal to the compiled reference where that is built"""
    k = _key(c, th_low, only_stereo, check_ori)
    if k not in _EXPECTED:
        m, nm, pairs = TC.expected(c, th_low, only_stereo, check_ori)
        if R.available() and th_low == 50 and not TC.has_dead(c):
            rp, rn = R.search_for_triangulation(*TC.ref_keyframes(c), c["F12"], only_stereo, check_ori)
            assert rn == nm and np.array_equal(rp, pairs)
        _EXPECTED[k] = (c, m, nm, pairs)   # the case object stays alive with its id
    return _EXPECTED[k][1:]


class Block:
    """the keyframes of a batch on the device, as orbfe_bow_transform_batch_device and the extractor lay them out"""

    def __init__(self, frames, cap=None, n=None, nfv=None, off_end=None):
        from orb_slam2_ssd_semantic_amd import KP_DTYPE, mapping
        B, nfv_over = len(frames), nfv
        self.B = B
        cap = self.cap = cap or max(max((len(f["desc"]) for f in frames), default=0), 1) + 3
        kps = np.zeros((max(B, 1), cap), KP_DTYPE)
        desc = np.zeros((max(B, 1), cap, 32), np.uint8)
        ur = np.full((max(B, 1), cap), -1, F)
        mp = np.zeros((max(B, 1), cap), np.uint8)
        node = np.zeros((max(B, 1), cap), np.uint32)
        off = np.full((max(B, 1), cap + 1), cap, np.uint32)
        idx = np.zeros((max(B, 1), cap), np.uint32)
        counts = np.zeros((max(B, 1), 4), np.int32)
        self.n = np.zeros(max(B, 1), np.int32)
        for b, f in enumerate(frames):
            k = len(f["desc"])
            self.n[b] = k
            src = np.arange(cap) % max(k, 1)   # rows past the count: the keyframe's own features again, free and monocular
            if k:
                kps["x"][b], kps["y"][b], kps["octave"][b], kps["angle"][b] = f["xy"][src, 0], f["xy"][src, 1], f["octave"][src], f["angle"][src]
                desc[b] = f["desc"][src]
                ur[b, :k], mp[b, :k] = f["uRight"], f["has_mp"]
            fn, fo, fi = f["fv"]
            nfv, tot = len(fn), len(fi)
            node[b, :nfv], off[b, :nfv + 1], idx[b, :tot] = fn, fo, fi
            node[b, nfv:] = fn[0] if nfv else 0          # padding that names a real node and real features
            off[b, nfv + 1:] = tot
            idx[b, tot:] = np.arange(cap - tot) % max(k, 1)
            counts[b] = (0, nfv, tot, 0)
        for b, v in enumerate(nfv_over or ()):   # what the arrays SAY, where a test overrides it
            if v is not None:
                counts[b, 1] = v
        for b, v in enumerate(off_end or ()):
            if v is not None:
                off[b, len(frames[b]["fv"][0])] = v
        self.t = dict(kps=_dev(kps.view(np.int32).reshape(-1, cap, 7)), desc=_dev(desc), n=_dev(self.n if n is None else np.asarray(n, np.int32)),
                      ur=_dev(ur), mp=_dev(mp), node=_dev(node.view(np.int32)), off=_dev(off.view(np.int32)), idx=_dev(idx.view(np.int32)),
                      counts=_dev(counts))
        t = self.t
        self.kf = mapping.keyframes_struct(t["kps"], t["desc"], t["n"], cap, B, t["node"], t["off"], t["idx"], t["counts"], t["ur"], t["mp"])

    def run(self, lm, pairs, th_low=50, only_stereo=False, check_ori=True, skip=None, want_pairs=True):
        """pairs: [(i1, i2, F12, ex, ey)] -> ([(match12 row [cap], nmatches, pairs [k][2])], raw bytes of all outputs)"""
        import torch
        from orb_slam2_ssd_semantic_amd._ffi import TriOut
        P, cap = len(pairs), self.cap
        kf1, kf2 = _dev(np.array([p[0] for p in pairs], np.int32).reshape(P)), _dev(np.array([p[1] for p in pairs], np.int32).reshape(P))
        F12 = _dev(np.array([p[2] for p in pairs], F).reshape(P, 9))
        epi = _dev(np.array([(p[3], p[4]) for p in pairs], F).reshape(P, 2))
        sk = None if skip is None else _dev(np.asarray(skip, np.uint8))
        m12, nm, pr, npr = _guarded(P * cap), _guarded(P), _guarded(P * cap * 2), _guarded(P)
        out = TriOut(m12.data_ptr(), nm.data_ptr(), pr.data_ptr() if want_pairs else None, npr.data_ptr() if want_pairs else None)
        lm.SearchForTriangulation_batch_device(self.kf, kf1.data_ptr(), kf2.data_ptr(), P, F12.data_ptr(), epi.data_ptr(),
                                               None if sk is None else sk.data_ptr(), TC.SF, TC.S2, out, th_low, only_stereo, check_ori)
        torch.cuda.synchronize()
        M, N, PR, NP = _body(m12, (P, cap)), _body(nm, (P,)), _body(pr, (P, cap, 2)), _body(npr, (P,))
        res = []
        for p in range(P):
            if want_pairs:
                assert 0 <= NP[p] <= cap and (PR[p, NP[p]:] == SENT).all(), "rows past npairs written"
                res.append((M[p], int(N[p]), PR[p, :NP[p]]))
            else:
                assert NP[p] == SENT and (PR[p] == SENT).all()
                res.append((M[p], int(N[p]), None))
        return res, b"".join(a.tobytes() for a in (M, N, PR, NP))


def check(got, c, th_low=50, only_stereo=False, check_ori=True, what=""):
    m, nm, pairs = expected(c, th_low, only_stereo, check_ori)
    gm, gn, gp = got
    n1 = len(m)
    assert (gm[n1:] == -1).all(), (what, "match12 past n1")
    assert np.array_equal(gm[:n1], m), (what, np.nonzero(gm[:n1] != m)[0][:8])
    assert gn == nm, (what, gn, nm)
    if gp is not None:
        assert np.array_equal(gp, pairs), what


def run_cases(lm, cases, names, **kw):
    b = TC.as_batch(cases)
    got, _ = Block(b["frames"]).run(lm, b["pairs"], **kw)
    for g, c, name in zip(got, cases, names):
        check(g, c, what=name, **kw)
    return got


# ------------------------------------------------------------------------------------------------ one candidate decides
@pytest.mark.parametrize("check_ori", [False, True])
def test_planted_edges(lm, check_ori):
    """threshold, ties (the last in list order wins), a closer candidate that fails the line, the epipole gate on levels 0, 2 and 7
    and its bypass for stereo keypoints, dsqr one ulp either side of 3.84 * sigma2, F12 = 0, eligibility, nodes on one side only:
    every planted call of one threshold as a pair of ONE batch, and each gives its planted answer"""
    by_th = {}
    for name, k, c, th in TC.planted():
        by_th.setdefault(th, []).append(("%s[%d]" % (name, k), c))
    assert set(by_th) == {0, 50}
    for th, items in by_th.items():
        got = run_cases(lm, [c for _, c in items], [n for n, _ in items], th_low=th, check_ori=check_ori)
        for (name, c), g in zip(items, got):
            assert g[0][0] == c["want"], name


@pytest.mark.parametrize("only_stereo", [False, True])
def test_featurevector_shapes(lm, only_stereo):
    """no common node (all below / all above), the one common node at the first and at the last position of keyframe 2's list,
    empty FeatureVectors, n1 = 0, n2 = 0, features in no node; has_mp and mono / stereo features on both sides of every scene"""
    S = TC.fv_shapes()
    run_cases(lm, list(S.values()), list(S), only_stereo=only_stereo)
    run_cases(lm, list(S.values()), list(S), only_stereo=only_stereo, check_ori=False)


def test_no_pairs(lm):
    S = TC.fv_shapes()
    b = TC.as_batch([S["interleaved"]])
    got, raw = Block(b["frames"]).run(lm, [])
    assert got == []


def test_list_lengths(lm):
    """node lists of 1, lanes +- 1, tile - 1 / tile / tile + 1 and 3 tiles + 1 keyframe-2 features; 1 and queries-per-pass +- 1
    keyframe-1 features over a list of one tile and of two; 600 x 600 in one node.  The lengths come from the kernel."""
    from orb_slam2_ssd_semantic_amd import mapping
    info = mapping.tri_search_info()
    cases = TC.list_lengths(info)
    assert "n2_%d" % (info["tile"] + 1) in cases and "n1_%d" % (info["queries_per_pass"] + 1) in cases
    run_cases(lm, list(cases.values()), list(cases))
    run_cases(lm, list(cases.values()), list(cases), only_stereo=True, check_ori=False)


def test_rotation_histogram(lm):
    """all matches in one bin, four tied bins (the earlier three stay), second and third under a tenth of the first, differences
    that land in bin 30 -> 0, negative differences"""
    cases = [TC.histogram_case(n) for n in TC.HISTOGRAMS]
    got = run_cases(lm, cases, list(TC.HISTOGRAMS))
    off = run_cases(lm, cases, list(TC.HISTOGRAMS), check_ori=False)
    for name, g, o in zip(TC.HISTOGRAMS, got, off):
        assert (g[1] < o[1]) == (name != "one_bin"), name


# ------------------------------------------------------------------------------------------------ batches
def test_one_keyframe_against_twenty_neighbours(lm):
    """results do not depend on the pair order or on P (1, 2, all); the pair (0, 0); a second run gives identical bytes"""
    b = TC.neighbours()
    blk = Block(b["frames"])
    cases = [TC.pair_of(b, p) for p in range(len(b["pairs"]))]
    got, raw = blk.run(lm, b["pairs"])
    for p, g in enumerate(got):
        check(g, cases[p], what=p)
    assert got[20][1] > 0   # a keyframe against itself matches
    assert blk.run(lm, b["pairs"])[1] == raw
    order = np.random.default_rng(5).permutation(len(cases))
    for g, p in zip(blk.run(lm, [b["pairs"][p] for p in order])[0], order):
        check(g, cases[p], what=("shuffled", p))
    for sub in ([7], [3, 20]):
        for g, p in zip(blk.run(lm, [b["pairs"][p] for p in sub])[0], sub):
            check(g, cases[p], what=("subset", p))
    for g, p in zip(blk.run(lm, b["pairs"][:4], want_pairs=False)[0], range(4)):
        check(g, cases[p], what=("no pairs output", p))


def test_skipped_pairs_and_frame_indices_outside_the_block(lm):
    b = TC.neighbours()
    blk = Block(b["frames"])
    pairs = list(b["pairs"][:6])
    pairs[1] = (-1, 2) + pairs[1][2:]
    pairs[4] = (0, blk.B) + pairs[4][2:]
    got, _ = blk.run(lm, pairs, skip=[0, 0, 1, 0, 0, 1])
    for p, g in enumerate(got):
        if p in (1, 2, 4, 5):
            assert (g[0] == -1).all() and g[1] == 0 and len(g[2]) == 0, p
        else:
            check(g, TC.pair_of(b, p), what=p)


def test_counts_above_cap_are_clamped(lm):
    """d_n larger than cap: the block's cap rows are the keyframe.  Then the node count and the last offset larger than cap, on a
    keyframe that really has cap nodes and cap entries (one feature per node), as keyframe 2 and as keyframe 1 of a pair."""
    c = TC.scene(55, 90, 90, 5)[0]
    b = TC.as_batch([c])
    blk = Block(b["frames"], cap=90, n=[90 + 5, 2 ** 30])
    check(blk.run(lm, b["pairs"])[0][0], c)
    cap = 64
    one = TC.one_node(56, cap, cap)
    m = TC.core_match(one)
    full = TC.with_nodes(one["k2"], np.arange(cap))                                 # cap nodes of one feature each
    part = TC.with_nodes(one["k1"], [m[i] if m[i] >= 0 else -1 for i in range(cap)])   # every feature in its partner's node
    Ft = np.ascontiguousarray(one["F12"].reshape(3, 3).T).reshape(9)   # the pair the other way round: F21 = F12', its epipole far away
    fwd, back = dict(one, k1=part, k2=full), dict(one, k1=full, k2=part, F12=Ft, ex=F(-1e6), ey=F(-1e6), pose=None)
    assert len(full["fv"][0]) == cap == full["fv"][1][-1] and expected(fwd)[1] > 5 and expected(back)[1] > 5
    pairs = [(0, 1, one["F12"], one["ex"], one["ey"]), (1, 0, Ft, back["ex"], back["ey"])]
    for nfv, end in ((cap + 7, cap + 5), (2 ** 30, 2 ** 31 + 9), (-3, None)):
        got = Block([part, full], cap=cap, nfv=[None, nfv], off_end=[None, end]).run(lm, pairs)[0]
        if nfv < 0:   # a negative count is an empty FeatureVector
            assert all((g[0] == -1).all() and g[1] == 0 for g in got)
            continue
        check(got[0], fwd, what=("keyframe 2", nfv))
        check(got[1], back, what=("keyframe 1", nfv))


def test_inputs_the_device_cannot_reject_are_ignored(lm):
    """a keyframe-2 octave outside the levels; FeatureVector entries >= the keyframe's count (the count says 50, the lists name
    all 80 features): neither a candidate nor a query, and no guard band is touched"""
    for name, c in TC.ignored_inputs().items():
        run_cases(lm, [c], [name])
    c = TC.scene(42, 80, 80, 4)[0]
    dead = np.arange(80) >= 50
    short = dict(c, k1=dict(c["k1"], dead=dead), k2=dict(c["k2"], dead=dead))
    b = TC.as_batch([c])
    got = Block(b["frames"], n=[50, 50]).run(lm, b["pairs"])[0][0]
    m, nm, pairs = expected(short)
    assert np.array_equal(got[0][:80], m) and got[1] == nm and np.array_equal(got[2], pairs) and (got[0][50:] == -1).all()
    assert nm > 0 and not np.array_equal(m, expected(c)[0])


def test_largest_block(lm):
    """cap = n1 = n2 = 8192 in 10 nodes: lists of ~800 entries, 13 tiles, 26 passes"""
    c = TC.big()
    b = TC.as_batch([c])
    check(Block(b["frames"], cap=8192).run(lm, b["pairs"])[0][0], c)


def test_equals_the_host_buffer_call(lm, mt):
    """the batch result = the untouched orbfe_search_for_triangulation (one pair, host buffers) + the replay, on the same arrays"""
    b = TC.neighbours()
    got, _ = Block(b["frames"]).run(lm, b["pairs"][:5])
    for p in range(5):
        c = TC.pair_of(b, p)
        m, nm, pairs = TC.expected(c, fn=mt.SearchForTriangulationCore)
        assert np.array_equal(got[p][0][:len(m)], m) and got[p][1] == nm and np.array_equal(got[p][2], pairs)


# ------------------------------------------------------------------------------------------------ pair preparation
K = (535.4, 539.2, 320.1, 247.6)


def _prep(lm, Tcw, Ow, kf1, kf2, mb, mono, median=None):
    import torch
    from orb_slam2_ssd_semantic_amd import mapping
    B, P = len(Tcw), len(kf1)
    cam = mapping.camera(*K, 40.0, 0.0, 640.0, 0.0, 480.0)
    dT, dO = _dev(np.asarray(Tcw, F).reshape(B, 12)), _dev(np.asarray(Ow, F).reshape(B, 3))
    dm = None if median is None else _dev(np.asarray(median, F))
    d1, d2 = _dev(np.asarray(kf1, np.int32)), _dev(np.asarray(kf2, np.int32))
    f12 = torch.full((P * 9 + GUARD,), float(SENT), dtype=torch.float32, device="cuda")
    epi = torch.full((P * 2 + GUARD,), float(SENT), dtype=torch.float32, device="cuda")
    sk = torch.full((P + GUARD,), 77, dtype=torch.uint8, device="cuda")
    lm.TriangulationPairs_batch_device(dT.data_ptr(), dO.data_ptr(), B, cam, mb, mono, None if dm is None else dm.data_ptr(), d1.data_ptr(),
                                       d2.data_ptr(), P, f12.data_ptr(), epi.data_ptr(), sk.data_ptr())
    torch.cuda.synchronize()
    f, e, s = f12.cpu().numpy(), epi.cpu().numpy(), sk.cpu().numpy()
    assert (f[P * 9:] == SENT).all() and (e[P * 2:] == SENT).all() and (s[P:] == 77).all(), "guard band overwritten"
    return f[:P * 9].reshape(P, 9), e[:P * 2].reshape(P, 2), s[:P]


def test_pair_preparation(lm):
    """d_F12 = the host function, d_epi = proj_cases.tri_core_inputs' arithmetic, bit for bit; the stereo baseline gate with
    baseline == mb kept and one ulp below skipped; the monocular gate either side of 0.01; a frame index outside the block"""
    from orb_slam2_ssd_semantic_amd import compute_f12, mapping
    cam = mapping.camera(*K, 40.0, 0.0, 640.0, 0.0, 480.0)
    Tcw, Ow, scenes = [], [], []
    for seed in range(6):
        k1, k2, _ = PC.triangulation_case(np.random.default_rng(seed), 4, 4, 2)
        k1["K"] = k2["K"] = K + (40.0,)
        scenes.append((k1, k2))
        Tcw += [np.zeros((3, 4), F), np.concatenate([k2["Rcw"], k2["tcw"][:, None]], 1)]
        Tcw[-2][:, :3] = np.eye(3)
        Ow += [k1["Ow"], -(k2["Rcw"].astype(np.float64).T @ k2["tcw"].astype(np.float64)).astype(F)]
    kf1, kf2 = list(range(0, 12, 2)) + [0, 12], list(range(1, 12, 2)) + [-1, 1]
    f, e, s = _prep(lm, Tcw, Ow, kf1, kf2, 0.0, 0)
    for p, (k1, k2) in enumerate(scenes):
        want = compute_f12(Tcw[2 * p], Tcw[2 * p + 1], cam).reshape(9)
        assert f[p].view(np.uint32).tolist() == want.view(np.uint32).tolist() == FO.f12_compute(Tcw[2 * p], Tcw[2 * p + 1], *K).view(np.uint32).tolist()
        _, _, ex, ey = PC.tri_core_inputs(k1, k2, False)
        assert e[p].view(np.uint32).tolist() == [F(ex).view(np.uint32), F(ey).view(np.uint32)] and s[p] == 0
    assert s[6] == 1 and s[7] == 1 and not f[6:].any() and not e[6:].any()
    # the baseline as the reference stores it, then mb on it and one ulp either side
    base = [FO.f12_baseline(Ow[2 * p], Ow[2 * p + 1]) for p in range(6)]
    for p in range(6):
        for mb, want in ((base[p], 0), (np.nextafter(base[p], F(np.inf)), 1), (np.nextafter(base[p], F(0)), 0)):
            assert _prep(lm, Tcw, Ow, [2 * p], [2 * p + 1], float(mb), 0)[2][0] == want == int(FO.f12_baseline_skip(Ow[2 * p], Ow[2 * p + 1], 0, mb, 0))
    # mono: baseline / depth against 0.01 -- depths around baseline / 0.01, a few ulps either way
    med = np.ones(12, F)
    seen = set()
    for p in range(6):
        d0 = F(base[p] / F(0.01))
        for step in range(-3, 4):
            d = d0
            for _ in range(abs(step)):
                d = np.nextafter(d, F(np.inf) if step > 0 else F(0))
            med[2 * p + 1] = d
            want = int(FO.f12_baseline_skip(Ow[2 * p], Ow[2 * p + 1], 1, 0.0, d))
            assert _prep(lm, Tcw, Ow, [2 * p], [2 * p + 1], 1e9, 1, med)[2][0] == want
            seen.add(want)
    assert seen == {0, 1}


# ------------------------------------------------------------------------------------------------ the device-resident chain
def test_chain_from_images_to_matched_pairs(mt):
    """ORBextractor batch -> orbfe_frame_geometry_batch_device (RGB-D: uRight) -> orbfe_bow_transform_batch_device (the synthetic
    vocabulary of the BoW tests) -> orbfe_triangulation_pairs_batch_device -> orbfe_search_for_triangulation_batch_device on 4
    synthetic 640 x 480 frames with known poses: every call takes the stream and device pointers only, nothing is read or waited
    for between the stages, and the ONE synchronise sits before the final download.  The oracle is then fed the downloaded
    intermediate arrays."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera, LocalMapper, ORBextractor, ORBVocabulary, compute_f12, mapping
    from orb_slam2_ssd_semantic_amd.synth import synth_frame
    from test_bow import make_voc
    B, w, h, z = 4, 640, 480, 2.0
    fx, fy, cx, cy = K
    rng = np.random.default_rng(404)
    base = synth_frame(77)
    # a fronto-parallel scene at depth z seen by cameras that step sideways (and a little forward): the image shifts by 4 px a step
    frames = np.stack([np.clip(np.rint(np.roll(base, 4 * j, axis=1).astype(np.float64) + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8)
                       for j in range(B)])
    Tcw = np.zeros((B, 3, 4), F)
    Tcw[:, :, :3] = np.eye(3)
    Tcw[:, 0, 3], Tcw[:, 2, 3] = [4 * j * z / fx for j in range(B)], [0.004 * j for j in range(B)]
    Ow = (-Tcw[:, :, 3]).astype(F)
    depth = np.full((B, h, w), z, F)
    depth[:, :, :w // 2] = 0          # the left half has no depth: monocular keypoints there
    lm = LocalMapper(mt)
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    assert cap <= mapping.tri_search_info()["max_cap"]
    cam_geo = Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), (), bf=40.0)
    cam = mapping.camera(fx, fy, cx, cy, 40.0, 0.0, float(w), 0.0, float(h))
    V = ORBVocabulary(mt, **make_voc(15, 10, 3))
    pairs = [(0, 1), (0, 2), (0, 3), (1, 0), (2, 2), (3, 1)]
    P = len(pairs)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    d_gray, d_depth = torch.from_numpy(frames).cuda(), torch.from_numpy(depth).cuda()
    d_kps, d_desc, d_n = torch.zeros((B, cap, 7), **i32), torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"), torch.zeros(B, **i32)
    bl = dict(f_word=torch.zeros((B, cap), **i32), f_node=torch.zeros((B, cap), **i32), f_weight=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
              bow_id=torch.zeros((B, cap), **i32), bow_val=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
              fv_node=torch.zeros((B, cap), **i32), fv_off=torch.zeros((B, cap + 1), **i32), fv_idx=torch.zeros((B, cap), **i32),
              counts=torch.zeros((B, 4), **i32))
    d_kf1, d_kf2 = _dev(np.array([p[0] for p in pairs], np.int32)), _dev(np.array([p[1] for p in pairs], np.int32))
    d_T, d_O = _dev(Tcw.reshape(B, 12)), _dev(Ow)
    d_F12, d_epi = torch.zeros((P, 9), dtype=torch.float32, device="cuda"), torch.zeros((P, 2), dtype=torch.float32, device="cuda")
    d_skip = torch.zeros((P,), dtype=torch.uint8, device="cuda")
    # ---- the chain: enqueue only
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    d_un, _, d_ur = cam_geo.frame_geometry(d_kps, d_n, cap, depth=d_depth, scale=1.0, stream=st)
    V.transform_batch_device(d_desc.data_ptr(), d_n.data_ptr(), B, cap, 2, bl["f_word"].data_ptr(), bl["f_node"].data_ptr(),
                             bl["f_weight"].data_ptr(), bl["bow_id"].data_ptr(), bl["bow_val"].data_ptr(), bl["fv_node"].data_ptr(),
                             bl["fv_off"].data_ptr(), bl["fv_idx"].data_ptr(), bl["counts"].data_ptr(), st)
    lm.TriangulationPairs_batch_device(d_T.data_ptr(), d_O.data_ptr(), B, cam, 0.01, 0, None, d_kf1.data_ptr(), d_kf2.data_ptr(), P,
                                       d_F12.data_ptr(), d_epi.data_ptr(), d_skip.data_ptr(), st)
    kf = mapping.keyframes_struct(d_un, d_desc, d_n, cap, B, bl["fv_node"], bl["fv_off"], bl["fv_idx"], bl["counts"], d_ur, None)
    m12, nm, pr, npr = lm.search_for_triangulation_device(kf, d_kf1, d_kf2, d_F12, d_epi, TC.SF, TC.S2, pair_skip=d_skip, stream=st)
    torch.cuda.synchronize()
    # ---- download and compare
    n = d_n.cpu().numpy()
    kps = d_un.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    desc, ur, counts = d_desc.cpu().numpy(), d_ur.cpu().numpy(), bl["counts"].cpu().numpy()
    host = {k: bl[k].cpu().numpy().view(np.uint32) for k in ("fv_node", "fv_off", "fv_idx")}
    F12, epi, skip = d_F12.cpu().numpy(), d_epi.cpu().numpy(), d_skip.cpu().numpy()
    m12, nm, pr, npr = m12.cpu().numpy(), nm.cpu().numpy(), pr.cpu().numpy(), npr.cpu().numpy()
    assert (n >= 1000).all() and (ur[0, :n[0]] >= 0).any() and (ur[0, :n[0]] < 0).any()
    kfs = []
    for b in range(B):
        nfv, tot = counts[b, 1], counts[b, 2]
        kfs.append(TC.keyframe(desc[b, :n[b]], np.stack([kps["x"][b, :n[b]], kps["y"][b, :n[b]]], 1), kps["octave"][b, :n[b]], kps["angle"][b, :n[b]],
                               ur[b, :n[b]], np.zeros(n[b], np.uint8), (host["fv_node"][b, :nfv], host["fv_off"][b, :nfv + 1], host["fv_idx"][b, :tot])))
    camk = mapping.camera(fx, fy, cx, cy, 40.0, 0.0, float(w), 0.0, float(h))
    total = 0
    for p, (i1, i2) in enumerate(pairs):
        assert F12[p].view(np.uint32).tolist() == compute_f12(Tcw[i1], Tcw[i2], camk).reshape(9).view(np.uint32).tolist()
        ex, ey = FO.f12_epipole(Tcw[i2].reshape(12), Ow[i1], fx, fy, cx, cy)
        assert epi[p].view(np.uint32).tolist() == [F(ex).view(np.uint32), F(ey).view(np.uint32)]
        assert skip[p] == int(FO.f12_baseline_skip(Ow[i1], Ow[i2], 0, 0.01, 0)) == (1 if i1 == i2 else 0)
        if skip[p]:
            assert (m12[p] == -1).all() and nm[p] == 0 and npr[p] == 0
            continue
        m, wn, wp = TC.expected(TC.pair_case(kfs[i1], kfs[i2], F12[p], epi[p, 0], epi[p, 1]))
        assert np.array_equal(m12[p, :n[i1]], m) and (m12[p, n[i1]:] == -1).all() and nm[p] == wn == npr[p]
        assert np.array_equal(pr[p, :npr[p]], wp)
        total += wn
    assert total > 100
