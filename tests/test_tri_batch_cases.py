"""Every case of tests/tri_batch_cases.py reaches the edge it is planted on, under the CPU oracle's matching core
(oracle_ffi.search_for_triangulation) + proj_cases.replay_triangulation, and -- where oracle/_ref is built -- under the compiled
reference body (ref_ffi.search_for_triangulation, src/ORBmatcher.cc:827-1019).  No GPU."""
import numpy as np

import tri_batch_cases as TC
from oracle import oracle_ffi as O
from oracle import ref_ffi as R

INFO = dict(lanes=8, tile=64, queries_per_pass=32)   # any sizes do for the shape of the table; the GPU test takes the kernel's


def _ref_agrees(c, only_stereo=False, check_ori=True):
    if not R.available() or TC.has_dead(c):
        return
    m, nm, pairs = TC.expected(c, 50, only_stereo, check_ori)
    rp, rn = R.search_for_triangulation(*TC.ref_keyframes(c), c["F12"], only_stereo, check_ori)
    assert rn == nm and np.array_equal(rp, pairs)


def test_planted_calls_give_their_planted_answers(oracle):
    seen = set()
    for name, k, c, th in TC.planted():
        m = TC.core_match(c, th)
        assert m.tolist() == [c["want"]], (name, k, m)
        if th == 50:
            _ref_agrees(c, check_ori=False)
            _ref_agrees(c, check_ori=True)
        seen.add(name)
    assert seen == set(TC.PLANTED_NAMES)
    for name in TC.PLANTED_NAMES:   # the members that must differ do
        case = TC.PLANTED_TABLES[name]()
        got = [TC.E.run_tri(O.search_for_triangulation, c) for c in case["calls"]]
        for a, b in case["differ"]:
            assert got[a].tolist() != got[b].tolist(), (name, a, b)


def test_tie_and_gate_cases_hold_what_they_claim(oracle):
    """the tie case really has two (three) PASSING candidates at one distance; the closer candidate of gate_fail_closer really is
    closer and really fails on the line alone"""
    for name, n in (("tie", 2), ("three_tied", 3)):
        call = TC.PLANTED_TABLES[name]()["calls"][0]
        d = TC.H.distances(call["k1"]["desc"], call["k2"]["desc"])[0]
        assert len(d) == n and len(set(d.tolist())) == 1 and d[0] <= 50
        for j in range(n):   # each one alone is accepted
            solo = dict(call, k2=dict(call["k2"], elig=np.eye(n, dtype=np.uint8)[j]))
            assert TC.E.run_tri(O.search_for_triangulation, solo).tolist() == [j]
    for k, closer in ((0, 0), (1, 1)):
        call = TC.PLANTED_TABLES["gate_fail_closer"]()["calls"][k]
        d = TC.H.distances(call["k1"]["desc"], call["k2"]["desc"])[0]
        assert d[closer] < d[1 - closer] <= 50
        solo = dict(call, k2=dict(call["k2"], elig=np.eye(2, dtype=np.uint8)[closer]))
        assert TC.E.run_tri(O.search_for_triangulation, solo).tolist() == [-1]
        on_line = dict(call, k2=dict(call["k2"], xy=np.array([[300, 100], [340, 100]], np.float32)))
        assert TC.E.run_tri(O.search_for_triangulation, on_line).tolist() == [closer]


def test_epipole_cases_straddle_the_gate(oracle):
    calls = TC.PLANTED_TABLES["epipole_levels"]()["calls"]
    for base, o in ((0, 0), (4, 7)):
        lim = np.float32(np.float32(100) * TC.SF[o])
        d2 = [np.float32((TC.E.TRI_EX - calls[base + j]["k2"]["xy"][0, 0]) ** 2) for j in (0, 1)]
        assert d2[0] >= lim > d2[1] and calls[base]["k2"]["octave"][0] == o
        assert np.nextafter(calls[base]["k2"]["xy"][0, 0], np.float32(1e9)) == calls[base + 1]["k2"]["xy"][0, 0]


def test_fv_shapes(oracle):
    S = TC.fv_shapes()
    for name in ("all_below", "all_above", "empty_fv1", "empty_fv2", "n1_zero", "n2_zero"):
        m, nm, pairs = TC.expected(S[name])
        assert nm == 0 and len(pairs) == 0 and (m == -1).all(), name
    a, b = S["all_below"], S["all_above"]
    assert a["k1"]["fv"][0].max() < a["k2"]["fv"][0].min() and b["k1"]["fv"][0].min() > b["k2"]["fv"][0].max()
    for name, pos in (("common_first", 0), ("common_last", -1)):
        c = S[name]
        common = set(c["k1"]["fv"][0].tolist()) & set(c["k2"]["fv"][0].tolist())
        assert len(common) == 1 and c["k2"]["fv"][0][pos] in common, name
        m, nm, _ = TC.expected(c)
        assert nm > 0, name
        assert set(TC.nodes_of(c["k2"])[m[m >= 0]].tolist()) == common
    assert TC.expected(S["interleaved"])[1] > 0
    for name, c in S.items():
        for only in (False, True):
            _ref_agrees(c, only)
    # a feature present in no node exists on both sides of the plain scene
    c = TC.scene(31, 60, 60, 3)[0]
    assert (TC.nodes_of(c["k1"]) < 0).any() and (TC.nodes_of(c["k2"]) < 0).any()


def test_list_lengths_table(oracle):
    cases = TC.list_lengths(INFO)
    assert {"n2_1", "n2_7", "n2_8", "n2_9", "n2_63", "n2_64", "n2_65", "n2_193", "n1_31", "n1_32", "n1_33", "both_600"} <= set(cases)
    for name, c in cases.items():
        n1, n2 = len(c["k1"]["desc"]), len(c["k2"]["desc"])
        assert len(c["k1"]["fv"][0]) == (1 if n1 else 0) and c["k2"]["fv"][1][-1] == n2, name
        if name.startswith("n2_"):
            assert n2 == int(name.split("_")[1])
    m, nm, _ = TC.expected(cases["both_600"])
    assert nm > 60
    assert (m >= 64).any() and (m[m >= 0] < 64).any()   # winners in the first tile and in later ones
    _ref_agrees(cases["both_600"])
    _ref_agrees(cases["n2_65"], only_stereo=True)


def _tri_info():
    from orb_slam2_ssd_semantic_amd import mapping
    return mapping.tri_search_info()   # host only: the kernel's own constants


def test_many_nodes_gives_every_workgroup_a_second_node(oracle):
    """more keyframe-1 nodes than two laps of the search's workgroups; heavy nodes (several tiles, several passes) in the first lap
    and behind it; workgroups that go from a multi-tile node to a single-tile one and back; a node absent from keyframe 2 and a
    node without queries between two nodes that match; standing matches in every lap"""
    info = _tri_info()
    W, T, Q = info["node_workgroups"], info["tile"], info["queries_per_pass"]
    c, plant = TC.many_nodes(info)
    assert len(c["k1"]["desc"]) == len(c["k2"]["desc"]) == 1500
    w = TC.node_walk(c)
    nfv1 = len(w["n1"])
    assert nfv1 > 2 * W and nfv1 == len(c["k1"]["fv"][0])
    live = (w["n2"] > 0) & (w["n1"] > 0)
    heavy = np.nonzero((w["n2"] > 2 * T) & (w["n1"] > Q) & (w["elig"] > Q))[0]
    assert (heavy < W).any() and (heavy >= W).any(), heavy
    assert (w["matches"][heavy] > 0).all()
    one_tile_two_passes = np.nonzero(live & (w["n2"] <= T) & (w["elig"] > Q))[0]
    assert len(one_tile_two_passes) >= 1 and (one_tile_two_passes + W < nfv1).any()   # ... and the same workgroup goes on
    seqs = TC.workgroup_sequences(nfv1, W)
    assert len(seqs) == W and min(len(s) for s in seqs) >= 2 and sorted(a for s in seqs for a in s) == list(range(nfv1))
    multi = live & (w["n2"] > T)
    single = live & (w["n2"] <= T)
    steps = [(a, b) for s in seqs for a, b in zip(s, s[1:])]
    assert any(multi[a] and single[b] and w["matches"][b] > 0 for a, b in steps)
    assert any(single[a] and multi[b] and w["matches"][a] > 0 and w["matches"][b] > 0 for a, b in steps)
    for name, gap in (("absent", lambda a: w["n2"][a] == 0 and w["n1"][a] > 0), ("taken", lambda a: live[a] and w["elig"][a] == 0)):
        s = seqs[plant[name]]
        assert len(s) == 3 and w["matches"][s[0]] > 0 and gap(s[1]) and w["matches"][s[2]] > 0, (name, s)
    for lap in range(3):
        assert w["matches"][lap * W:(lap + 1) * W].sum() >= 30, lap
    # every mode the GPU test runs still reaches every lap
    for only, ori in ((False, False), (True, True), (True, False)):
        ww = TC.node_walk(c, only, ori)
        assert all(ww["matches"][lap * W:(lap + 1) * W].sum() > 0 for lap in range(3)), (only, ori)
        _ref_agrees(c, only, ori)
    _ref_agrees(c)


def test_nodes_at_the_workgroup_count(oracle):
    """W, W + 1, 2 W and 2 W + 1 nodes of one feature: the way round where keyframe 1 has them has exactly that many nodes, its
    LAST node keeps a match (at W + 1 and 2 W + 1 the only node of its lap), and so does every lap before it"""
    W = _tri_info()["node_workgroups"]
    for n in (W, W + 1, 2 * W, 2 * W + 1):
        fwd, back = TC.nodes_at(n)
        assert len(back["k1"]["fv"][0]) == n == back["k1"]["fv"][1][-1] == len(fwd["k2"]["fv"][0])
        assert (np.diff(back["k1"]["fv"][1].astype(np.int64)) == 1).all()
        w = TC.node_walk(back)
        assert w["matches"][n - 1] > 0, n
        assert all(w["matches"][lap * W:(lap + 1) * W].sum() > 0 for lap in range((n + W - 1) // W)), n
        assert TC.expected(fwd)[1] > 5 and TC.expected(back, only_stereo=True, check_ori=False)[1] > 0, n
        _ref_agrees(fwd)
        _ref_agrees(back)


def test_histogram_cases_have_their_shape(oracle):
    for name, (plan, keep) in TC.HISTOGRAMS.items():
        c = TC.histogram_case(name)
        m = TC.core_match(c)
        idx = np.nonzero(m >= 0)[0]
        assert len(idx) == sum(n for _, n in plan), name
        hist = [0] * 30
        for i in idx:
            hist[O.rot_bin(float(c["k1"]["angle"][i]), float(c["k2"]["angle"][m[i]]))] += 1
        got = tuple(b for b in O.three_maxima(hist) if b >= 0)
        assert got == keep, (name, hist, got)
        kept = TC.expected(c)[1]
        assert kept == sum(hist[b] for b in keep) and (kept < len(idx)) == (name != "one_bin"), name
        _ref_agrees(c)
    hist_of = {name: TC.histogram_case(name) for name in ("bin_30_wraps_to_0", "negative_difference")}
    assert (hist_of["bin_30_wraps_to_0"]["k1"]["angle"] == 910).sum() == 3
    assert np.isin(hist_of["negative_difference"]["k1"]["angle"], [5.0, 1.0]).sum() == 7


def test_batches(oracle):
    b = TC.neighbours()
    assert len(b["frames"]) == 21 and len(b["pairs"]) == 21 and b["pairs"][-1][:2] == (0, 0)
    counts = [TC.expected(TC.pair_of(b, p))[1] for p in range(21)]
    assert min(counts[:20]) > 10
    # the neighbours hold the same features in other orders: as many matches, other indices
    sets = [frozenset(map(tuple, TC.expected(TC.pair_of(b, p), check_ori=False)[2].tolist())) for p in range(3)]
    assert len(set(sets)) == 3
    _ref_agrees(TC.pair_of(b, 3))
    _ref_agrees(TC.pair_of(b, 20), only_stereo=True)
    for name, c in TC.ignored_inputs().items():
        assert TC.has_dead(c)
        plain = dict(c, k1=dict(c["k1"], dead=np.zeros_like(c["k1"]["dead"])), k2=dict(c["k2"], dead=np.zeros_like(c["k2"]["dead"])))
        assert not np.array_equal(TC.expected(c)[0], TC.expected(plain)[0]), name   # the ignored features would have matched
