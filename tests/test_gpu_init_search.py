"""The device-resident SearchForInitialization (csrc/orbfe_init_search.hip) bit for bit against tests/init_search_oracle.py and,
where oracle/_ref is built, the compiled reference body (src/ORBmatcher.cc:523-651): matches12, prev as bit patterns, nmatches.
No tolerances.  One call has ONE grid geometry, window and orientation switch, so the cases are grouped by those; every
output buffer has a guard band of sentinels behind it."""
import functools

import numpy as np
import pytest

import init_search_cases as IC
import init_search_oracle as IO
from oracle import ref_ffi as R

pytestmark = pytest.mark.gpu

F = np.float32
NC = 64 * 48
GUARD = 64
SENT = -7
PREV_PAD = F(-3.5)   # prev rows past a pair's count: must come back untouched


@pytest.fixture(scope="module")
def trk():
    from orb_slam2_ssd_semantic_amd import ORBmatcher, Tracker
    m = ORBmatcher(0.9, True)
    yield Tracker(m)
    m.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _guarded(shape, dtype=None, fill=SENT):
    import torch
    return torch.full((int(np.prod(shape)) + GUARD,), fill, dtype=dtype or torch.int32, device="cuda")


def _body(t, shape):
    n = int(np.prod(shape))
    a = t.cpu().numpy()
    assert (a[n:] == SENT).all(), "guard band overwritten"
    return a[:n].reshape(shape)


@functools.lru_cache(maxsize=None)
def expected(key, window, ori, second_call=False):
    """oracle result of a named case (cached: the batches of 1, 2 and all share it), checked against the compiled reference"""
    c = case(key)
    prev = expected(key, window, ori)[1] if second_call else c["prev"]
    o = IO.search_for_initialization(c["f1"], c["f2"], prev, window, check_ori=ori)
    if R.available():
        r = R.search_for_initialization(c["f1"], c["f2"], prev, window, 0.9, ori)
        assert r[2] == o[2] and np.array_equal(r[0], o[0]) and r[1].tobytes() == o[1].tobytes(), key
    return o


@functools.lru_cache(maxsize=None)
def case(key):
    kind, name = key
    if kind == "planted":
        return IC.PLANTED[name]()
    if kind == "contended":
        return IC.contended_case(name)
    if kind == "edge":
        return IC.batch_edges()[name]
    if kind == "random":
        return IC.random_case(name)
    if kind == "big":
        rng = np.random.default_rng(15360)
        f1, f2, prev = IC.PC.initialization_case(rng, 15360, 15360)
        return dict(f1=f1, f2=f2, prev=prev, window=15, check_ori=True)
    raise KeyError(key)


def _block(frames, cap):
    """keypoint records, descriptors and counts of a batch; rows past a frame's count would make queries / candidates if read"""
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    B = len(frames)
    blk = np.zeros((B, cap), KP_DTYPE)
    blk["x"], blk["y"], blk["octave"], blk["angle"] = 100.0, 100.0, 0, 10.0
    desc = np.full((B, cap, 32), 0xA5, np.uint8)
    for f, fr in enumerate(frames):
        n = len(fr["octave"])
        blk["x"][f, :n], blk["y"][f, :n], blk["octave"][f, :n], blk["angle"][f, :n] = fr["xy"][:, 0], fr["xy"][:, 1], fr["octave"], fr["angle"]
        desc[f, :n] = fr["desc"]
    return blk, desc, np.array([len(fr["octave"]) for fr in frames], np.int32)


class Batch:
    """a batch of frame pairs on the device, and one call of the search on it"""

    def __init__(self, trk, cases, cap1=None, cap2=None, n1=None, n2=None):
        import torch
        from orb_slam2_ssd_semantic_amd import tracking
        self.trk, self.B = trk, len(cases)
        B = self.B
        self.cap1 = cap1 = cap1 or min(max(max(len(c["f1"]["octave"]) for c in cases), 1) + 3, 15360)
        self.cap2 = cap2 = cap2 or min(max(max(len(c["f2"]["octave"]) for c in cases), 1) + 3, 15360)
        b1, d1, c1 = _block([c["f1"] for c in cases], cap1)
        b2, d2, c2 = _block([c["f2"] for c in cases], cap2)
        self.n1, self.n2 = c1, c2
        prev = np.full((B, cap1, 2), PREV_PAD, F)
        for p, c in enumerate(cases):
            prev[p, :c1[p]] = c["prev"]
        self.prev_in = prev
        g0 = cases[0]["f2"]
        g = [float(g0["bounds"][0]), float(g0["bounds"][2]), float(g0["gw_inv"]), float(g0["gh_inv"])]
        assert all(c["f2"]["bounds"] == g0["bounds"] for c in cases), "one call has one grid geometry"
        t = self.t = dict(k1=_dev(b1.view(np.int32).reshape(B, cap1, 7)), d1=_dev(d1), n1=_dev(c1 if n1 is None else np.asarray(n1, np.int32)),
                          k2=_dev(b2.view(np.int32).reshape(B, cap2, 7)), d2=_dev(d2), n2=_dev(c2 if n2 is None else np.asarray(n2, np.int32)),
                          off=torch.zeros((B, NC + 1), dtype=torch.int32, device="cuda"), idx=torch.zeros((B, cap2), dtype=torch.int32, device="cuda"),
                          nin=torch.zeros((B,), dtype=torch.int32, device="cuda"))
        trk._mt.AssignFeaturesToGrid_batch_device(t["k2"].data_ptr(), t["n2"].data_ptr(), cap2, B, *g, t["off"].data_ptr(), t["idx"].data_ptr(),
                                                  t["nin"].data_ptr(), None)
        self.second = tracking.frames_struct(t["k2"], t["d2"], t["n2"], cap2, t["off"], t["idx"], *g)

    def run(self, window, ori, prev=None, min_matches=0, ent_cap=None, in_place=False, packed=True):
        """-> dict(m [B, cap1], nm [B], prev [B, cap1, 2], status [2], off1, off2, mcsr, k1, k2)"""
        import torch
        from orb_slam2_ssd_semantic_amd import tracking
        B, cap1, cap2, t = self.B, self.cap1, self.cap2, self.t
        f32 = torch.float32
        d_prev = _guarded((B, cap1, 2), f32)
        d_prev[:B * cap1 * 2] = _dev(self.prev_in if prev is None else prev).reshape(-1)
        o = dict(m=_guarded((B, cap1)), nm=_guarded((B,)), st=_guarded((2,)), prev=d_prev if in_place else _guarded((B, cap1, 2), f32),
                 off1=_guarded((B + 1,)), off2=_guarded((B + 1,)), mcsr=_guarded((B * cap1,)), k1=_guarded((B * cap1, 2), f32),
                 k2=_guarded((B * cap2, 2), f32))
        first, out = tracking.init_search_structs(t["k1"], t["d1"], t["n1"], cap1, o["m"], o["nm"], o["st"], o["prev"],
                                                  *([o["off1"], o["off2"], o["mcsr"], o["k1"], o["k2"]] if packed else []))
        self.trk.SearchForInitialization_batch_device(first, self.second, B, d_prev.data_ptr(), window, out, check_ori=ori,
                                                      min_matches=min_matches, ent_cap=ent_cap)
        torch.cuda.synchronize()
        if not in_place:
            assert np.array_equal(_body(d_prev, (B, cap1, 2)).view(np.uint32), np.asarray(self.prev_in if prev is None else prev, F).view(np.uint32))
        return dict(m=_body(o["m"], (B, cap1)), nm=_body(o["nm"], (B,)), prev=_body(o["prev"], (B, cap1, 2)), status=_body(o["st"], (2,)),
                    off1=_body(o["off1"], (B + 1,)), off2=_body(o["off2"], (B + 1,)), mcsr=_body(o["mcsr"], (B * cap1,)),
                    k1=_body(o["k1"], (B * cap1, 2)), k2=_body(o["k2"], (B * cap2, 2)))


def check_pair(r, p, batch, c, exp, prev_in=None, what=""):
    """pair p of a batch result against (matches12, prev, nmatches) of the oracle"""
    n1, n2 = len(c["f1"]["octave"]), len(c["f2"]["octave"])
    prev_in = batch.prev_in if prev_in is None else prev_in
    assert r["status"][0] == 0, what
    assert r["nm"][p] == exp[2], (what, p, r["nm"][p], exp[2])
    assert np.array_equal(r["m"][p, :n1], exp[0]), (what, p, np.flatnonzero(r["m"][p, :n1] != exp[0])[:8])
    assert (r["m"][p, n1:] == -1).all(), (what, p)
    assert np.array_equal(r["prev"][p, :n1].view(np.uint32), np.asarray(exp[1], F).view(np.uint32)), (what, p)
    assert np.array_equal(r["prev"][p, n1:].view(np.uint32), np.asarray(prev_in[p, n1:], F).view(np.uint32)), (what, p)
    if r["off1"][0] != SENT:   # the packed outputs
        a, b = r["off1"][p], r["off2"][p]
        assert r["off1"][p + 1] - a == n1 and r["off2"][p + 1] - b == n2, (what, p)
        assert np.array_equal(r["mcsr"][a:a + n1], exp[0]) and np.array_equal(r["k1"][a:a + n1], c["f1"]["xy"]), (what, p)
        assert np.array_equal(r["k2"][b:b + n2], c["f2"]["xy"]), (what, p)


def run_group(trk, keys, window, ori, what):
    cases = [case(k) for k in keys]
    bt = Batch(trk, cases)
    r = bt.run(window, ori)
    for p, k in enumerate(keys):
        check_pair(r, p, bt, cases[p], expected(k, window, ori), what=(what, k))
    tot1, tot2 = int(bt.n1.sum()), int(bt.n2.sum())
    assert r["off1"][0] == 0 and r["off1"][-1] == tot1 and r["off2"][-1] == tot2
    assert (r["mcsr"][tot1:] == SENT).all() and (r["k1"][tot1:] == SENT).all() and (r["k2"][tot2:] == SENT).all()
    return r


PLANTED_PLAIN = [("planted", n) for n in IC.PLANTED if not IC.PLANTED[n]().get("check_ori")]
PLANTED_ORI = [("planted", n) for n in IC.PLANTED if IC.PLANTED[n]().get("check_ori")]
CONTENDED_100 = [("contended", i) for i, c in enumerate(IC.CONTENDED) if c[3] == 100]
CONTENDED_30 = [("contended", i) for i, c in enumerate(IC.CONTENDED) if c[3] == 30]
EDGES = [("edge", n) for n in IC.batch_edges()]
GROUPS = {"planted": (PLANTED_PLAIN, IC.WINDOW, False), "planted_ori": (PLANTED_PLAIN + PLANTED_ORI, IC.WINDOW, True),
          "contended_100": (CONTENDED_100, 100, True), "contended_30": (CONTENDED_30 + CONTENDED_100[:1], 30, True),
          "contended_100_no_ori": (CONTENDED_100, 100, False), "edges": (EDGES, 30, True)}


@pytest.mark.parametrize("group", list(GROUPS))
def test_tables_as_whole_batches(trk, group):
    keys, window, ori = GROUPS[group]
    run_group(trk, keys, window, ori, group)


@pytest.mark.parametrize("group", list(GROUPS))
def test_tables_as_batches_of_one_and_two(trk, group):
    keys, window, ori = GROUPS[group]
    for k in keys:
        run_group(trk, [k], window, ori, group + "/1")
    for i in range(0, len(keys), 2):
        run_group(trk, [keys[i], keys[(i + 1) % len(keys)]], window, ori, group + "/2")


def test_planted_outcomes_on_the_device(trk):
    """the planted expectations themselves (not only the oracle): take-overs, the skip, the tie, the lost votes"""
    for name in IC.PLANTED:
        c = IC.PLANTED[name]()
        r = Batch(trk, [c]).run(c["window"], c["check_ori"])
        n1 = len(c["f1"]["octave"])
        assert list(r["m"][0, :n1]) == list(c["expect"]["matches12"]) and r["nm"][0] == c["expect"]["nmatches"], name


def test_random_frames_with_a_second_call_in_place(trk):
    """the 60 seeds of the existing shim test: sizes 1 / 50 / 500 / 2000, windows 30 / 100, orientation check on / off; the
    second call continues from the first one's prev, written in place"""
    groups = {}
    for seed in range(60):
        c = case(("random", seed))
        groups.setdefault((c["window"], c["check_ori"]), []).append(("random", seed))
    assert len(groups) == 4
    total = 0
    for (window, ori), keys in groups.items():
        cases = [case(k) for k in keys]
        bt = Batch(trk, cases)
        r = bt.run(window, ori, in_place=True)
        for p, k in enumerate(keys):
            check_pair(r, p, bt, cases[p], expected(k, window, ori), what=("first", k))
            total += int(r["nm"][p])
        r2 = bt.run(window, ori, prev=r["prev"], in_place=True)
        for p, k in enumerate(keys):
            check_pair(r2, p, bt, cases[p], expected(k, window, ori, True), prev_in=r["prev"], what=("second", k))
    assert total > 1000


@pytest.mark.parametrize("name", ["chain_40", "chain_70", "chain_40_without_query0", "chain_70_without_query0"])
def test_rounds_equal_the_model_on_the_chains(trk, name):
    c = IC.PLANTED[name]()
    r = Batch(trk, [c]).run(c["window"], False)
    rounds = IO.model(c["f1"], c["f2"], c["prev"], c["window"], check_ori=False)[3]
    assert r["status"][1] == rounds == c["expect"]["min_rounds"], (r["status"], rounds)
    check_pair(r, 0, Batch(trk, [c]), c, expected(("planted", name), c["window"], False))


def test_rounds_of_a_batch_are_the_longest_pair(trk):
    keys = [("planted", "chain_40"), ("planted", "chain_70"), ("planted", "tie_is_skipped")]
    r = run_group(trk, keys, IC.WINDOW, False, "rounds")
    assert r["status"][1] == 71


def test_host_form_equals_batch_form(trk):
    keys = [("planted", "skip_20_12_15"), ("planted", "lost_votes_change_the_bins"), ("contended", 1), ("contended", 2), ("random", 7),
            ("edge", "n2_0"), ("edge", "n1_0"), ("edge", "prev_outside")]
    for k in keys:
        c = case(k)
        for ori in (True, False):
            trk._mt.mbCheckOrientation = ori
            m, prev, nm = trk._mt.SearchForInitialization(c["f1"], c["f2"], c["prev"], c["window"])
            e = expected(k, c["window"], ori)
            assert nm == e[2] and np.array_equal(m, e[0]) and prev.tobytes() == np.asarray(e[1], F).tobytes(), (k, ori)
    trk._mt.mbCheckOrientation = True


def test_one_batch_in_two_orders_on_one_handle(trk):
    keys, window, ori = GROUPS["planted_ori"]
    a = run_group(trk, keys, window, ori, "forward")
    b = run_group(trk, keys[::-1], window, ori, "reversed")
    assert np.array_equal(a["nm"], b["nm"][::-1])


def test_entry_buffer_one_short(trk):
    keys, window, ori = GROUPS["contended_100"]
    cases = [case(k) for k in keys]
    bt = Batch(trk, cases)
    need = sum(int(IO.entries(IO.candidate_lists(c["f1"], c["f2"], c["prev"], window)[1])[0][-1]) for c in cases)
    assert need > 1000
    r = bt.run(window, ori, ent_cap=need - 1)
    assert r["status"][0] == need
    assert (r["m"] == -1).all() and (r["nm"] == 0).all() and (r["mcsr"][:int(bt.n1.sum())] == -1).all()
    assert np.array_equal(r["prev"].view(np.uint32), bt.prev_in.view(np.uint32))
    r = bt.run(window, ori, ent_cap=int(r["status"][0]))
    for p, k in enumerate(keys):
        check_pair(r, p, bt, cases[p], expected(k, window, ori), what=("retry", k))
    r = bt.run(window, ori, ent_cap=0)
    assert r["status"][0] == need and (r["m"] == -1).all()


def test_min_matches_in_one_batch(trk):
    """Tracking's 100: the pair below it reaches the Initializer without matches, nmatches and prev keep the reference's values"""
    lo = hi = None
    for seed in range(60):
        k = ("random", seed)
        nm = expected(k, 100, True)[2]
        if lo is None and 8 <= nm < 100:
            lo = k
        if hi is None and nm >= 100:
            hi = k
    assert lo is not None and hi is not None
    keys = [lo, hi, lo]
    cases = [case(k) for k in keys]
    bt = Batch(trk, cases)
    r = bt.run(100, True, min_matches=100)
    for p, k in enumerate(keys):
        e = expected(k, 100, True)
        n1 = len(cases[p]["f1"]["octave"])
        assert r["nm"][p] == e[2] and np.array_equal(r["prev"][p, :n1].view(np.uint32), np.asarray(e[1], F).view(np.uint32))
        a = r["off1"][p]
        if k == hi:
            assert np.array_equal(r["m"][p, :n1], e[0]) and np.array_equal(r["mcsr"][a:a + n1], e[0])
        else:
            assert (r["m"][p] == -1).all() and (r["mcsr"][a:a + n1] == -1).all()
    r0 = bt.run(100, True, min_matches=int(expected(hi, 100, True)[2]))   # nmatches == min_matches stays
    assert np.array_equal(r0["m"][1, :len(cases[1]["f1"]["octave"])], expected(hi, 100, True)[0])


def test_counts_outside_the_capacity_are_clamped(trk):
    """n = cap exactly, and counts of -3 / cap + 10 on the device: read as 0 / cap"""
    c = case(("edge", "plain"))
    n1, n2 = len(c["f1"]["octave"]), len(c["f2"]["octave"])
    e = expected(("edge", "plain"), 30, True)
    bt = Batch(trk, [c, c, c, c], cap1=n1, cap2=n2, n1=[n1, n1 + 10, -3, n1], n2=[n2, n2 + 10, n2, -3])
    r = bt.run(30, True, packed=False)
    for p in (0, 1):
        assert r["nm"][p] == e[2] and np.array_equal(r["m"][p], e[0]) and np.array_equal(r["prev"][p].view(np.uint32), e[1].view(np.uint32)), p
    for p in (2, 3):
        assert r["nm"][p] == 0 and (r["m"][p] == -1).all() and np.array_equal(r["prev"][p].view(np.uint32), bt.prev_in[p].view(np.uint32)), p
    bt = Batch(trk, [c, c, c], cap1=n1, cap2=n2, n1=[n1 + 10, -3, n1], n2=[n2 + 10, n2, -3])
    r = bt.run(30, True)
    assert list(r["off1"]) == [0, n1, n1, 2 * n1] and list(r["off2"]) == [0, n2, 2 * n2, 2 * n2]


def test_one_pair_at_the_largest_capacity(trk):
    k = ("big", 0)
    c = case(k)
    bt = Batch(trk, [c])
    assert bt.cap1 == 15360 and bt.cap2 == 15360
    r = bt.run(15, True)
    assert r["status"][0] > 256 * 1024   # more entries than the first guess for one pair: the retry rule
    r = bt.run(15, True, ent_cap=int(r["status"][0]))
    check_pair(r, 0, bt, c, expected(k, 15, True), what="15360")
    assert r["nm"][0] > 1000


def test_limits_are_refused(trk):
    import torch
    from orb_slam2_ssd_semantic_amd import _ffi, tracking
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    sec = tracking.frames_struct(z, z, z, 8, z, z, 0, 0, 0.1, 0.1)
    for cap1, cap2, th, npairs, err in ((15361, 8, 50, 1, _ffi.ORBFE_ERR_SIZE), (8, 15361, 50, 1, _ffi.ORBFE_ERR_SIZE), (8, 8, 256, 1, _ffi.ORBFE_ERR_ARG),
                                        (1 << 12, 8, 50, 1 << 13, _ffi.ORBFE_ERR_SIZE), (0, 8, 50, 1, _ffi.ORBFE_ERR_ARG)):
        sec.cap = cap2
        first, out = tracking.init_search_structs(z, z, z, cap1, z, z, z)
        with pytest.raises(_ffi.OrbfeError) as ei:
            trk.SearchForInitialization_batch_device(first, sec, npairs, None, 30, out, th_low=th)
        assert ei.value.status == err, (cap1, cap2, th, npairs)
    first, out = tracking.init_search_structs(z, z, z, 8, z, z, z, d_keys1_xy=z)   # packed points without their offsets
    with pytest.raises(_ffi.OrbfeError):
        trk.SearchForInitialization_batch_device(first, sec, 1, None, 30, out)


def test_chain_extractor_search_initializer(trk):
    """two synthetic frames -> extractor (2000 features) -> grid -> SearchForInitialization -> Initialize on one stream, nothing
    read by the host in between; equal to the reference's search on the downloaded frames followed by the Initializer oracle"""
    import torch
    import initializer_cases as INC
    import initializer_oracle as INO
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor, initializer as IN, tracking
    from orb_slam2_ssd_semantic_amd.initializer import InitializerHandle
    from orb_slam2_ssd_semantic_amd.synth import synth_frame
    B, w, h = 2, 640, 480
    rng = np.random.default_rng(11)
    base = synth_frame(77)
    second = np.roll(base, (3, 9), axis=(0, 1)).astype(np.float64) + rng.normal(0, 2.0, base.shape)
    frames = np.stack([base, np.clip(np.rint(second), 0, 255).astype(np.uint8)])
    ext = ORBextractor(2000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    d_gray = torch.from_numpy(frames).cuda()
    d_kps, d_desc, d_n = torch.zeros((B, cap, 7), **i32), torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda"), torch.zeros(B, **i32)
    its = 200
    draws = INC.draws_for(its, 77)
    pair = np.zeros(1, IN.PAIR_DTYPE)
    pair["K"], pair["sigma"], pair["iterations"] = INC.K0, 1.0, its
    d_pair, d_draws = torch.from_numpy(pair.view(np.uint8).reshape(1, -1)).cuda(), torch.from_numpy(draws).cuda()
    g = (0.0, 0.0, float(F(64) / F(w)), float(F(48) / F(h)))
    d_off, d_idx, d_nin = torch.zeros((1, NC + 1), **i32), torch.zeros((1, cap), **i32), torch.zeros((1,), **i32)
    with InitializerHandle(cap, 1) as hnd:
        ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
        trk._mt.AssignFeaturesToGrid_batch_device(d_kps[1:].data_ptr(), d_n[1:].data_ptr(), cap, 1, *g, d_off.data_ptr(), d_idx.data_ptr(),
                                                  d_nin.data_ptr(), st)
        sec = tracking.frames_struct(d_kps[1:], d_desc[1:], d_n[1:], cap, d_off, d_idx, *g)
        t = IN.monocular_initialization_device(trk, hnd, dict(kps=d_kps[:1], desc=d_desc[:1], n=d_n[:1]), sec, d_pair, d_draws, window=100,
                                               min_matches=100)
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
        desc = d_desc.cpu().numpy()

        def frame(i):
            f = dict(xy=np.stack([kps[i]["x"], kps[i]["y"]], 1)[:n[i]].astype(F), octave=kps[i]["octave"][:n[i]].astype(np.int32),
                     angle=kps[i]["angle"][:n[i]].astype(F), desc=desc[i, :n[i]], uRight=np.full(n[i], -1, F), state=np.zeros(n[i], np.uint8),
                     Tcw=np.eye(4, dtype=F), K=(535.4, 539.2, 320.1, 247.6, 40.0, 40.0 / 535.4), scale_factors=IC.PC.scale_factors())
            f.update(IC.geometry(w, h))
            return f
        f1, f2 = frame(0), frame(1)
        search = R.search_for_initialization if R.available() else IO.search_for_initialization
        m, prev, nm = search(f1, f2, f1["xy"], 100, 0.9, True)
        assert int(t["status"][0]) == 0 and int(t["nmatches"][0]) == nm >= 100 and (f1["octave"] == 0).sum() > 300
        assert np.array_equal(t["matches12"].cpu().numpy()[0, :n[0]], m) and list(t["offsets1"].cpu().numpy()) == [0, n[0]]
        assert np.array_equal(t["prev"].cpu().numpy()[0, :n[0]].view(np.uint32), prev.view(np.uint32))
        r = INO.initialize(f1["xy"], f2["xy"], m, INC.K0, 1.0, its, draws)
        rec = t["result"].cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)[0]
        for k in ("ok", "status", "model", "n_matches", "iterH", "iterF", "best", "n_inliers"):
            assert rec[k] == r[k], (k, rec[k], r[k])
        for k in ("SH", "SF", "H21", "F21", "R21", "t21"):
            assert np.asarray(rec[k], F).tobytes() == np.asarray(r[k], F).tobytes(), k
        assert np.asarray(t["P3D"].cpu().numpy()[:n[0]], F).tobytes() == np.asarray(r["P3D"], F).tobytes()
        assert np.array_equal(t["triangulated"].cpu().numpy()[:n[0]].astype(bool), np.asarray(r["triangulated"]).astype(bool))
        assert r["SH"] > 0 and r["SF"] > 0
