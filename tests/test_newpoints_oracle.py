"""CreateNewMapPoints' per-match body on the host (orbfe_triangulate_match = csrc/orbfe_newpoints.h, the function the kernel runs)
bit for bit against tests/newpoints_oracle.py, the round planner, and the oracle's own serial / round loops against each other.
The oracle is an UNPINNED numpy restatement: LocalMapping.cc is not among the compiled reference sources.  No GPU."""
import numpy as np
import pytest

import newpoints_cases as NC
import newpoints_oracle as NO

f32 = np.float32


def _cam(c):
    from orb_slam2_ssd_semantic_amd.tracking import camera
    return camera(c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], 0, 0, 0, 0)


def _key(k):
    from orb_slam2_ssd_semantic_amd import mapping
    return mapping.newpt_key(k["ux"], k["uy"], k["octave"], k["depth"], k["uright"], k["rx"], k["ry"])


def host(args):
    from orb_slam2_ssd_semantic_amd import mapping
    T1, O1, T2, O2, cam, mb, k1, k2, sf, s2, scale_factor = args
    return mapping.triangulate_match(T1, O1, T2, O2, _cam(cam), mb, _key(k1), _key(k2), sf, s2, scale_factor)


def same(got, want, what):
    assert got[0] == want[0], (what, NO.VERDICTS[got[0]], NO.VERDICTS[want[0]])
    if want[0] != NO.W_ZERO:
        assert np.array_equal(np.asarray(got[1], f32).view(np.uint32), np.asarray(want[1], f32).view(np.uint32)), (what, got[1], want[1])


@pytest.mark.parametrize("seed", NC.SEEDS)
def test_scene_matches_bit_exact(seed):
    frames, pairs, can, _, _, _ = NC.scene_matches(seed)
    for j, (a, b) in enumerate(pairs):
        same(host(NC.match_args(frames, 0, 1, a, b)), can[j], (seed, j))


def test_scenes_clear_of_thresholds_and_cover_the_gates():
    """no comparison within a relative 1e-4 of its threshold in either trig mode (no seed is rejected: 12 of 12 candidate seeds
    passed when these four were chosen); together the scenes leave the loop at every gate and meet both sides of every comparison"""
    verdicts, sides = set(), set()
    for seed in NC.SEEDS:
        _, _, can, _, near, s = NC.scene_matches(seed)
        assert near == [], (seed, near)
        verdicts |= {v for v, _ in can}
        sides |= s
    assert verdicts >= {NO.LOW_PARALLAX, NO.DEPTH1, NO.DEPTH2, NO.ERR1, NO.ERR2, NO.SCALE, NO.OK}
    for name in ("rays<stereo", "rays<0.9998", "z1>0", "z2>0", "err1", "err2", "scale_lo", "scale_hi"):
        assert (name, True) in sides and (name, False) in sides, name
    assert ("stereo1<stereo2", True) in sides and ("stereo2<stereo1", True) in sides   # both unprojections (the equal case is planted)


def test_trig_modes_agree():
    """canonical trig and the host libm's cosf(2 * atan2f(..)) give the same verdict on every case.  The cosine only picks a
    branch, so equal verdicts reached through equal branches give equal points: 0 ulp measured on all cases, asserted as such
    (DESIGN.md 8o)."""
    worst = 0
    for seed in NC.SEEDS:
        _, _, can, hst, _, _ = NC.scene_matches(seed)
        for j, (a, b) in enumerate(zip(can, hst)):
            assert a[0] == b[0], (seed, j)
            worst = max(worst, int(np.abs(a[1].view(np.int32).astype(np.int64) - b[1].view(np.int32).astype(np.int64)).max()))
    for c in NC.planted():
        a, b = NO.triangulate_match(*c["args"]), NO.triangulate_match(*c["args"], trig="host")
        assert a[0] == b[0], c["name"]
        worst = max(worst, int(np.abs(a[1].view(np.int32).astype(np.int64) - b[1].view(np.int32).astype(np.int64)).max()))
    print("largest x3D difference between the trig modes: %d ulp" % worst)
    assert worst == 0


@pytest.mark.parametrize("case", NC.planted(), ids=lambda c: c["name"])
def test_planted(case):
    want = NO.triangulate_match(*case["args"])
    if case["want"] is not None:
        assert want[0] == case["want"], (NO.VERDICTS[want[0]], NO.VERDICTS[case["want"]])
    if case["never"] is not None:
        assert want[0] != case["never"]
    same(host(case["args"]), want, case["name"])


def test_planted_reach_their_edges():
    """the planted quantities sit ON the edge: equal sides where the name says so, adjacent floats around the 0.9998 cut"""
    by = {c["name"]: c for c in NC.planted()}

    def trace(name):
        tr = []
        NO.triangulate_match(*by[name]["args"], trace=tr)
        return {n: (a, b) for n, a, b in tr}
    for name, cmp_ in (("z1_zero", "z1>0"), ("z2_zero", "z2>0"), ("err_equal", "err1"), ("scale_equal", "scale_lo"), ("cos_rays_zero", "rays>0"),
                       ("stereo_equal", "rays>0")):
        a, b = trace(name)[cmp_]
        assert float(a) == float(b), (name, a, b)
    t = trace("stereo_equal")
    assert t["rays<stereo"] == (f32(0), f32(1))       # min(cosStereo1 = 1, cosStereo2 = 0 + 1)
    lo, hi = trace("cut_below")["rays<0.9998"][0], trace("cut_above")["rays<0.9998"][0]
    assert lo < 0.9998 <= hi and np.nextafter(f32(lo), f32(2)) == f32(hi)
    a, b = trace("err_above")["err1"]
    assert a > b == 0.0 and a < 1e-15


def test_argument_errors():
    from orb_slam2_ssd_semantic_amd import mapping
    args = list(NC.planted()[0]["args"])
    args[6] = dict(args[6], octave=8)
    with pytest.raises(ValueError):
        host(args)
    args[6] = dict(args[6], octave=-1)
    with pytest.raises(ValueError):
        host(args)
    assert mapping.NEWPT == {n: i for i, n in enumerate(NO.VERDICTS)}


# ------------------------------------------------------------------------------------------------ the planner
def plan(kf1, kf2):
    from orb_slam2_ssd_semantic_amd import mapping
    got = mapping.plan_rounds(kf1, kf2)
    want = NO.plan_rounds(kf1, kf2)
    for g, w in zip(got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w)
    return got


def test_plan_rounds():
    N = 7
    r, order, off = plan([0] * N, list(range(1, N + 1)))
    assert list(r) == list(range(N)) and list(order) == list(range(N)) and list(off) == list(range(N + 1))
    # 3 keyframes with disjoint neighbourhoods of 4, 2 and 3: max-degree rounds
    kf1 = [0] * 4 + [10] * 2 + [20] * 3
    kf2 = [1, 2, 3, 4, 11, 12, 21, 22, 23]
    r, order, off = plan(kf1, kf2)
    assert list(r) == [0, 1, 2, 3, 0, 1, 0, 1, 2] and list(off) == [0, 3, 6, 8, 9]
    assert list(order) == [0, 4, 6, 1, 5, 7, 2, 8, 3]          # stable: ascending pair index inside a round
    r, _, off = plan([1, 2, 3], [2, 3, 4])                      # a chain
    assert list(r) == [0, 1, 2] and len(off) == 4
    r, order, off = plan([1, 3, 1], [2, 4, 3])                  # (a, b), (c, d), (a, c)
    assert list(r) == [0, 0, 1] and list(order) == [0, 1, 2] and list(off) == [0, 2, 3]
    r, order, off = plan([], [])
    assert len(r) == 0 and len(order) == 0 and list(off) == [0]
    r, _, _ = plan([5, 5], [5, 6])                              # a pair (i, i)
    assert list(r) == [0, 1]
    rng = np.random.default_rng(5)
    for _ in range(50):
        P = int(rng.integers(0, 40))
        kf1, kf2 = rng.integers(0, 9, P), rng.integers(0, 9, P)
        r, order, off = plan(kf1, kf2)
        assert sorted(order) == list(range(P)) and off[-1] == P
        for j in range(len(off) - 1):
            seg = order[off[j]:off[j + 1]]
            assert (np.diff(seg) > 0).all() and (r[seg] == j).all()
            fr = [f for p in seg for f in {int(kf1[p]), int(kf2[p])}]
            assert len(fr) == len(set(fr)), "a keyframe twice in one round"


def test_newpoints_scratch_bytes():
    from orb_slam2_ssd_semantic_amd import mapping
    assert mapping.newpoints_scratch_bytes(0, 1, 0) > 0
    a, b = mapping.newpoints_scratch_bytes(10, 256, 11), mapping.newpoints_scratch_bytes(20, 256, 11)
    assert b > a >= 10 * 256 * 12 and a % 256 == 0
    assert mapping.newpoints_scratch_bytes(4095, 8192, 1) > 0
    for bad in ((1, 0, 1), (1, 8193, 1), (-1, 8, 1), (4096, 8192, 1), (1, 8, -1)):
        with pytest.raises(ValueError):
            mapping.newpoints_scratch_bytes(*bad)


# ------------------------------------------------------------------------------------------------ the loops
def _small_scene(seed, nkf):
    return NC.scene(seed, nkf, 40, nnodes=3, p_stereo=0.6)


def _loop_outputs_equal(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in ("pairs", "verdict", "new_idx", "new_xyz")) and \
        all(x["skip"] == y["skip"] for x, y in zip(a, b))


@pytest.mark.parametrize("seed", range(4))
def test_serial_loop_equals_planned_round_loop(seed):
    """the oracle's serial loop in the given order = its round loop in the planned order, on random pair lists (both monocular
    and stereo gates)"""
    rng = np.random.default_rng(100 + seed)
    nkf, cap = 5, 48
    frames = _small_scene(200 + seed, nkf)
    P = int(rng.integers(4, 9))
    pairs = [tuple(int(v) for v in rng.choice(nkf, 2, replace=False)) for _ in range(P)]
    _, order, off = NO.plan_rounds([p[0] for p in pairs], [p[1] for p in pairs])
    pos = np.argsort(order)
    for f in frames:
        f["has_mp"] = (np.arange(len(f["desc"])) % 5 == 0).astype(np.uint8)   # a few points to take the median of
    kw = NC.loop_kw(mono=bool(seed % 2))
    s1, s2 = NO.new_state(frames, cap), NO.new_state(frames, cap)
    serial = NO.serial_loop(frames, pairs, s1, cap, pos=pos, **kw)
    rounds = NO.round_loop(frames, [pairs[i] for i in order], off, s2, cap, **kw)
    assert _loop_outputs_equal([serial[i] for i in order], rounds)
    for a, b in zip(s1, s2):
        assert np.array_equal(a, b)
    assert sum(len(o["new_idx"]) for o in serial) > 0


def test_state_matters():
    """one keyframe against three neighbours that see the same landmarks: carrying the slots from neighbour to neighbour gives
    another result than matching all three against the initial state (what the GPU test then asserts of the device)"""
    frames, cap = _small_scene(300, 4), 48
    pairs = [(0, 1), (0, 2), (0, 3)]
    kw = NC.loop_kw()
    serial = NO.serial_loop(frames, pairs, NO.new_state(frames, cap), cap, **kw)
    static = NO.round_loop(frames, pairs, [0, 3], NO.new_state(frames, cap), cap, **kw)
    assert not _loop_outputs_equal(serial, static)
    assert len(serial[1]["pairs"]) < len(static[1]["pairs"])


def test_wide_loop_fills_more_than_one_claim_block():
    """the wide case: more than 256 new points in a pair, feature indices in the last quarter of the block, more FeatureVector
    nodes than two laps of the search's workgroups in every frame, a cap that is no multiple of 256, and -- in the one-round form --
    keyframe-0 slots that both pairs claim, from different 256-blocks of their new points"""
    from orb_slam2_ssd_semantic_amd import mapping
    W = mapping.tri_search_info()["node_workgroups"]
    w = NC.wide_loop()
    serial, static, cap = w["serial"], w["static"], w["cap"]
    assert cap % 256 != 0 and cap > 768 and w["pairs"] == [(0, 1), (0, 2)]
    assert list(NO.plan_rounds([0, 0], [1, 2])[2]) == [0, 1, 2]        # the planned rounds are the serial loop
    assert len(serial[0]["new_idx"]) > 256 and len(static[0]["new_idx"]) > 256 and len(static[1]["new_idx"]) > 256
    assert max(int(o["new_idx"].max()) for o in serial) >= 768
    assert all(len(f["fv"][0]) > 2 * W for f in w["frames"])
    assert not _loop_outputs_equal(serial, static)
    k0, k1 = ({int(i): k for k, i in enumerate(o["new_idx"][:, 0])} for o in static)
    shared = set(k0) & set(k1)
    assert shared and {(k0[s] // 256, k1[s] // 256) for s in shared} >= {(1, 0), (0, 0)}
    ids = w["s_static"][2]
    assert all(ids[0, s] == cap + k1[s] for s in shared)               # the later pair's point stays
    assert not shared & {int(i) for i in serial[1]["new_idx"][:, 0]}   # carried state: the second pair never sees a filled slot


def test_id_base_shifts_every_id():
    frames, cap = _small_scene(300, 4), 48
    pairs = [(0, 1), (0, 2), (0, 3)]
    s0, s1, s2 = (NO.new_state(frames, cap) for _ in range(3))
    a = NO.serial_loop(frames, pairs, s0, cap, **NC.loop_kw())
    b = NO.serial_loop(frames, pairs, s1, cap, id_base=1000, **NC.loop_kw())
    c = NO.round_loop(frames, pairs, [0, 3], s2, cap, id_base=1000, **NC.loop_kw())
    assert _loop_outputs_equal(a, b) and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    assert np.array_equal(np.where(s0[2] >= 0, s0[2] + 1000, -1), s1[2]) and (s0[2] >= 0).sum() > 10
    assert (s2[2][s2[2] >= 0] >= 1000).all()
    # two calls on carried state = one call: the second call's ids go on where the first one's end
    t = NO.new_state(frames, cap)
    NO.serial_loop(frames, pairs[:1], t, cap, **NC.loop_kw())
    NO.serial_loop(frames, pairs[1:], t, cap, id_base=cap, **NC.loop_kw())
    assert all(np.array_equal(x, y) for x, y in zip(t, s0))


def test_median_edge_frames():
    T, has, xyz, n, names = NC.median_edge_frames()
    assert has.sum(1).tolist() == [255, 256, 257, 100] and names[3] == "all_equal"
    for b in range(4):
        z = sorted(float(NO.np_cam_coord(T[b], 2, xyz[b, i])) for i in range(n[b]) if has[b, i])
        assert (len(set(z)) == 1) == (b == 3)
        assert NO.scene_median_depth(T[b], has[b], xyz[b], n[b], 1) == np.float32(z[-1])
        assert NO.scene_median_depth(T[b], has[b], xyz[b], n[b], 1000) == np.float32(z[0])
        assert NO.scene_median_depth(T[b], has[b], xyz[b], n[b], 2) == np.float32(z[(len(z) - 1) // 2])
        assert b == 3 or z[0] < z[(len(z) - 1) // 2] < z[-1]
