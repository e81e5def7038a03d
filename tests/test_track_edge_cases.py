"""tests/track_edge_cases.py holds what it claims, on the oracles alone (CPU; tests/test_gpu_track_edges.py runs the same tables
through csrc/orbfe_track.hip).  Each test fails if a planted condition is absent:

 1. frustum table: every gate of TO.GATES rejects at least one entry of the three lists under that list's pose; the rejected
    member of every pair makes no query and its neighbour makes one; the planted radius (2.5 / 4.0 either side of 0.998) and
    levels (0 / 1, 7 / 7) hold in the expected queries; the lists are posed | empty | identity under three different poses.
 2. map-gate lists: nine frames of 0, 1, 63, 64, 65, 255, 256, 257, 513 entries back to back, no two poses equal, the expected
    projection of a shared point differs between frames; most lists start off a multiple of 64, none is ascending, points
    repeat across frames; indices -1 and npoints and `seen` entries are planted and change the answer; in-view rates about
    0, 1 and 0.5; every frame with a nonzero rate has an accepted and a rejected entry in the 64 entries below and in the
    (up to) 64 entries from every multiple of 64 that it crosses (a side of ONE entry -- lengths 65 and 257 -- holds an
    accepted entry: it cannot hold both); the cut call's nentries falls inside one list and before the next.
 3. qcap: the frames' oracle counts lie above and below every qcap of (1, 64, 255, 256); the map list's count exceeds 256;
    the features given octave -1 / nlevels make queries under their own octave, and both values are planted.
 4. counts: the rows below 0 / behind the count / up to cap are live -- read, they would change the answer.
 5. unproject: n = 1023, 1024, 1025, 2049 and 15360 under different poses; select_literal == select_closed on every frame;
    the entries ranked nsel - 1 and nsel share a depth and differ in index (700 and n - 1: either side of index 1024 where
    n allows); equal depths sit mirrored about index 1024.
 6. replay: nq covers {0, 1, 255, 256, 257, 600}; the bin counts by O.rot_bin are the planted 10:1:1, 11:1:1, 20:5:1,
    40:40:30:30, one bin, none, and O.three_maxima keeps what the issue says; the twice-matched slots end -1 (kept + dropped,
    counted twice before the drop) and with the later source (kept + kept); slot states 0 / 1 / 2 give -1 / -2 / -2; entries
    >= n and entries behind nq look live; matches lie on both sides of position 256.
 7. pools: in the shared pool rows are addressed by two frames and by queries they were not made for; in the per-frame pools
    both -1 and pool_rows are planted on queries that match when their row is readable, removing them changes another
    query's answer (the claims chain), and the row behind pool_rows holds a descriptor that would change the answers."""
import numpy as np

import proj_cases as PC
import proj_edge_cases as E
import track_edge_cases as TE
import track_oracle as TO
from oracle import oracle_ffi as O

F = np.float32


# ------------------------------------------------------------------------------------------------ 1
def test_frustum_table_runs_every_gate(oracle):
    t = TE.frustum_table()
    want, entries = t["want"], t["entries"]
    assert [int(v) for v in t["list_off"]] == [0, want[0]["e1"], want[0]["e1"], len(entries)] and want[1]["e0"] == want[1]["e1"]
    assert sorted(t["list_idx"].tolist()) == list(range(len(entries))) == list(range(2 * len(TO.frustum_cases())))
    P = [TO.T34(T).tobytes() for T in t["poses"]]
    assert len(set(P)) == 3 and P[2] == TO.T34(TO.IDENTITY).tobytes()
    gates, made = set(), {}
    for f, w in enumerate(want):
        T = TO.T34(t["poses"][f])
        for k, e in enumerate(range(w["e0"], w["e1"])):
            name, member, c = entries[t["list_idx"][e]]
            assert np.array_equal(c["T"], t["poses"][f]), (name, "runs under its own pose")
            r, gate = TO.frustum_point(T, TO.camera_centre(T), TO.K0, TO.BOUNDS0, c["P"], c["Pn"], c["min_dist"], c["max_dist"], seen=c["seen"], bad=c["bad"])
            assert gate == c["gate"] and (r is not None) == bool(w["in_view"][k]), (name, member, gate)
            if gate is not None:
                gates.add(gate)
            hit = np.flatnonzero(w["src"] == k)
            made[(name, member)] = (w["q"][hit[0]], w["proj"][k]) if len(hit) else None
    assert gates == set(TO.GATES)
    for name, (rej, ok) in TO.frustum_cases().items():
        assert made[(name, 1)] is not None, name
        assert (made[(name, 0)] is None) == (rej["gate"] is not None), name
    sf = PC.scale_factors()
    for member, radius in ((0, 4.0), (1, 2.5)):
        q, p = made[("view_cos_0.998", member)]
        assert q["r"] == F(F(radius) * sf[p["level"]]) and TO.frustum_cases()["view_cos_0.998"][member]["want"]["radius"] == F(radius)
    assert [int(made[(k, m)][1]["level"]) for k in ("level_0", "level_7") for m in (0, 1)] == [0, 1, 7, 7]
    assert [int(made[("level_0", m)][0]["min_level"]) for m in (0, 1)] == [-1, 0]


# ------------------------------------------------------------------------------------------------ 2
def test_map_gate_lists_sit_on_the_chunk_and_index_edges(oracle):
    c = TE.map_gate_case()
    off, idx, seen, m = c["list_off"].astype(np.int64), c["list_idx"], c["seen"], c["map"]
    full, no_seen, cut = (TE.map_gate_want(v) for v in ("full", "no-seen", "cut"))
    assert tuple(np.diff(off)) == TE.GATE_LENGTHS and sorted(TE.GATE_LENGTHS) == [0, 1, 63, 64, 65, 255, 256, 257, 513] and len(m["bad"]) == TE.MAP_N == 600
    poses = [TO.T34(T).tobytes() for T in c["poses"]]
    assert len(poses) == 9 and len(set(poses)) == 9
    assert sum(int(o) % 64 != 0 for o, n in zip(off[:-1], TE.GATE_LENGTHS) if n) >= 7
    sets = []
    for f, n in enumerate(TE.GATE_LENGTHS):
        mine = idx[off[f]:off[f + 1]]
        sets.append(set(mine.tolist()))
        if n > 1:
            assert not np.all(np.diff(mine) > 0), f
    assert all(len(sets[a] & sets[b]) > 10 for a in (4, 7) for b in (8,))   # points shared between frames ...
    shared = sorted(set(full[7]["qsrc"].tolist()) & set(full[8]["qsrc"].tolist()))
    assert len(shared) > 20
    for p in shared[:20]:   # ... whose expected queries differ with the pose
        a, b = full[7]["q"][np.flatnonzero(full[7]["qsrc"] == p)[0]], full[8]["q"][np.flatnonzero(full[8]["qsrc"] == p)[0]]
        assert a["u"] != b["u"] and a["v"] != b["v"]
    kinds = {what for _, _, what in c["planted"]}
    assert kinds == set(TE.REJECT_KINDS) and {"index -1", "index npoints", "seen"} <= kinds
    assert (idx == -1).sum() >= 3 and (idx == TE.MAP_N).sum() >= 3
    for f, e, what in c["planted"]:
        assert full[f]["in_view"][e] == 0 and full[f]["proj"]["level"][e] == -1, (f, e, what)
        if what == "seen":
            assert seen[off[f] + e] == 1 and no_seen[f]["in_view"][e] == 1, (f, e)
    assert sum(int(w["in_view"].sum()) for w in no_seen) > sum(int(w["in_view"].sum()) for w in full)
    for f, (n, rate) in enumerate(zip(TE.GATE_LENGTHS, TE.GATE_RATES)):
        inv = full[f]["in_view"]
        assert len(inv) == n
        if n:
            got = inv.mean()
            assert (got == 0 if rate == 0 else got > 0.9 if rate == 1 else 0.35 < got < 0.6), (f, got)
        if rate == 0:
            continue
        for b in TE.gate_boundaries(n):
            for side in (inv[b - 64:b], inv[b:b + 64]):
                assert side.any() and (len(side) == 1 or not side.all()), (f, b)
    assert sum(b % TE.CHUNK == 0 for n, r in zip(TE.GATE_LENGTHS, TE.GATE_RATES) if r for b in TE.gate_boundaries(n)) == 3   # 257: 256; 513: 256, 512
    assert TE.gate_boundaries(65) == [64] and TE.gate_boundaries(64) == [] and TE.gate_boundaries(513)[-1] == 512
    # the cut: inside frame 7's list, frame 8's offsets both beyond it
    assert off[7] < c["cut"] < off[8] < off[9] and cut[7]["e1"] == c["cut"] and cut[8]["e0"] == cut[8]["e1"] == c["cut"]
    assert 0 < len(cut[7]["src"]) < len(full[7]["src"]) and all(len(cut[f]["src"]) == len(full[f]["src"]) for f in range(7))
    assert max(len(w["src"]) for w in no_seen) < c["qcap"]


# ------------------------------------------------------------------------------------------------ 3
def test_qcap_cases_overflow_and_underflow(oracle):
    pairs, want = TE.qcap_last_case()
    counts = [len(s) for _, s in want]
    assert counts[0] > 256 and counts[3] > 256 and 1 < counts[1] < 64 and counts[2] == 0 and TE.QCAPS == (1, 64, 255, 256)
    assert len({TO.T34(c["Tcw"]).tobytes() for c, _ in pairs}) == len(pairs)
    w = TE.qcap_map_case()["want"][0]
    assert int(w["in_view"].sum()) == len(w["src"]) > 256 and len(w["in_view"]) <= 600
    dev, ora, planted, owant = TE.octave_case()
    own = TE.gate_last_expect([(dev[0][0], ora[0][1])], octave_key="octave")   # invalid marks in place: the planted ones are gone
    assert set(planted.values()) == {-1, TO.NLEVELS} and len(planted) == len(TE.OCT_RANKS)
    alive = TE.gate_last_expect([(dev[0][0], dict(ora[0][1], has_mp=dev[0][1]["has_mp"]))])[0][1]
    for i, o in planted.items():
        assert dev[0][1]["octave"][i] == o and dev[0][1]["has_mp"][i] == 1 and not dev[0][1]["outlier"][i]
        assert i in alive and i not in owant[0][1] and i not in own[0][1]
    assert len(owant[0][1]) == len(alive) - len(planted) and min(planted) == alive[0] and max(planted) == alive[-1]
    assert np.array_equal(dev[1][1]["octave"], ora[1][1]["octave"])


# ------------------------------------------------------------------------------------------------ 4
def test_count_cases_have_live_rows_outside_the_count(oracle):
    pairs, n_dev, want, full = TE.count_last_case()
    cap = TE.COUNT_CAP_LAST
    assert n_dev.tolist() == [-3, cap + 7, cap - 30] and all(len(la["octave"]) == cap for _, la in pairs)
    assert len(want[0][1]) == 0 and len(full[0][1]) > 50                      # read with |n| or cap rows, frame 0 makes queries
    assert len(want[1][1]) == len(full[1][1]) > 50 and want[1][1][-1] >= cap - 3   # the over-count frame: up to the last rows
    assert len(full[2][1]) > len(want[2][1]) > 20 and full[2][1][-1] >= cap - 30 > want[2][1][-1]
    c = TE.count_unproject_case()
    cap = TE.COUNT_CAP_UNPROJ
    assert c["n_dev"].tolist() == [-3, cap + 7, cap - 30]
    (wp0, cr0), (wp1, cr1), (wp2, cr2) = c["want"]
    assert not wp0.any() and not cr0.any() and (c["frames"][0][1] > 0).sum() > 50
    assert wp1[cap - 20:].any() and cr1.sum() > 50 and (c["frames"][1][1][cap - 5:] > 0).any()
    assert not wp2[cap - 30:].any() and (c["frames"][2][1][cap - 30:] > 0).sum() > 10 and wp2[:cap - 30].any()
    assert len({TO.T34(T).tobytes() for T in c["poses"]}) == 3


# ------------------------------------------------------------------------------------------------ 5
def test_unproject_stride_cases_hold_their_ties(oracle):
    small, big = TE.unproject_stride_case()
    frames = small["frames"] + big["frames"]
    assert [len(z) for _, z, _ in frames] == [1023, 1024, 1025, 2049, E.PJ_MAX_NF] and big["cap"] == E.PJ_MAX_NF == 15360
    assert small["cap"] < 2100 and len({TO.T34(T).tobytes() for T in small["poses"] + big["poses"]}) == 5
    for (xy, z, kp), (wp, cr) in zip(frames, small["want"] + big["want"]):
        n, th = len(z), small["th_depth"]
        lit, closed = TO.select_literal(z, th), TO.select_closed(z, th)
        assert np.array_equal(lit, closed)
        nsel, a, b = TE.boundary_tie(z, th)
        assert nsel == int(lit.sum()) > 101 and a == (float(TE.TIE_Z), TE.TIE_LO) and b == (float(TE.TIE_Z), n - 1), (n, a, b)
        assert lit[TE.TIE_LO] and not lit[n - 1] and cr[TE.TIE_LO] == 1 and cr[n - 1] == 0 and wp[n - 1].any()
        assert (n - 1 >= TE.STRIDE) == (n > TE.STRIDE) and TE.TIE_LO < TE.STRIDE
        if n > TE.STRIDE + 8:
            assert all(z[TE.STRIDE + k] == z[TE.STRIDE - 1 - k] > 0 for k in range(1, 7))
        assert (kp == 1).sum() > n // 5 and (n <= TE.STRIDE + 8 or (z[TE.STRIDE:] > 0).sum() > (n - TE.STRIDE) // 2)
    for (wp, cr), (wp2, cr2), (_, z, kp) in zip(small["want"], small["want_no_keeps"], small["frames"]):
        assert wp.tobytes() == wp2.tobytes() and cr2.sum() > cr.sum() and np.array_equal(cr2.astype(bool) & ~kp.astype(bool), cr.astype(bool))


# ------------------------------------------------------------------------------------------------ 6
def test_replay_cases_hold_the_planted_histograms(oracle):
    t = TE.replay_case()
    names = list(t)
    assert {fr["nq"] for fr in t.values()} == set(TE.REPLAY_NQ) == {0, 1, 255, 256, 257, 600}
    ori, plain, mp = TE.replay_want("last", True), TE.replay_want("last", False), TE.replay_want("map", False)

    def bins(name):
        return {b: c for b, c in enumerate(TE.replay_bins(t[name])) if c}
    planted = {"none": ({}, (-1, -1, -1)), "one": ({4: 1}, (4, -1, -1)), "10:1:1": ({2: 10, 5: 1, 9: 1}, (2, 5, 9)),
               "11:1:1": ({2: 11, 5: 1, 9: 1}, (2, -1, -1)), "20:5:1": ({1: 20, 6: 5, 10: 1}, (1, 6, -1)),
               "40:40:30:30": ({1: 40, 3: 40, 5: 30, 7: 30}, (1, 3, 5)), "one-bin": ({7: 30}, (7, -1, -1))}
    for name, (counts, keep) in planted.items():
        assert bins(name) == counts, (name, bins(name))
        assert O.three_maxima(TE.replay_bins(t[name])) == keep, name
        f = names.index(name)
        kept = sum(c for b, c in counts.items() if b in keep)
        assert ori[f][1] == kept and plain[f][1] == mp[f][1] == sum(counts.values()) == len(ori[f][2]), name
    assert len(bins("dense")) > 8 and 0 < ori[names.index("dense")][1] < plain[names.index("dense")][1]
    # the slot matched twice, once in a dropped bin (earlier) and once in a kept one (later): NULL, both counted before the drop
    fr, f = t["20:5:1"], names.index("20:5:1")
    two = [(p, b) for p, s, b in fr["plan"] if s == 1]
    assert [b for _, b in two] == [10, 1] and two[0][0] < two[1][0] and fr["cur"]["state"][1] == 1
    assert ori[f][0][1] == -1 and plain[f][0][1] == fr["qsrc"][two[1][0]] and ori[f][1] == 26 - 1
    # ... and the mirror, both bins kept: the later query's source
    fr, f = t["40:40:30:30"], names.index("40:40:30:30")
    two = [(p, b) for p, s, b in fr["plan"] if s == 150]
    assert [b for _, b in two] == [1, 3] and two[0][0] < two[1][0] and ori[f][0][150] == fr["qsrc"][two[1][0]] != fr["qsrc"][two[0][0]]
    assert sorted(fr["match"][:600][fr["match"][:600] >= 200].tolist()) == [200, 202] and (fr["clean"] < 200).all()
    seven = [s for p, s, b in fr["plan"] if b == 7]
    assert len(seven) == 30 and all(ori[f][0][s] == -1 for s in seven) and all(plain[f][0][s] >= 0 for s in seven)
    # slot states without a match, and a matched state-1 slot
    a = ori[names.index("none")][0]
    assert a.tolist() == [-1, -2, -2] * 4 and t["none"]["cur"]["state"].tolist() == [0, 1, 2] * 4
    assert ori[names.index("one")][0].tolist() == [-1, -2, -2, -1, int(t["one"]["qsrc"][0]), -2, -1, -2, -2]
    for name, fr in t.items():
        nq = fr["nq"]
        assert len(fr["match"]) == len(fr["qsrc"]) == TE.REPLAY_QCAP and (fr["match"][nq:] >= 0).all() and (fr["match"][nq:] < fr["nF"]).all()
        assert np.all(np.diff(fr["qsrc"][:nq]) > 0) and fr["qsrc"].max() < TE.REPLAY_CAP_LAST
        if nq > 256:
            pos = np.flatnonzero(fr["clean"] >= 0)
            assert {255, 256} <= set(pos.tolist()) and (pos < 256).sum() > 5 and (pos > 256).sum() >= 0, name
    assert any((fr["match"][:fr["nq"]] >= fr["nF"]).any() for fr in t.values())
    assert (np.flatnonzero(t["40:40:30:30"]["clean"] >= 0) > 512).sum() > 5


# ------------------------------------------------------------------------------------------------ 7
def test_pool_cases_share_rows_and_leave_the_pool(oracle):
    shared, per = TE.core_pool_case()
    assert [len(c["q"]) for c in shared["calls"]] == [65, 64, 5] and len(shared["pool"]) == 134
    rows = [set(s.tolist()) for s in shared["srcs"]]
    assert all(len(rows[f] & rows[f + 1]) >= 2 for f in range(2))   # two frames address one row
    for f, (c, src, foreign) in enumerate(zip(shared["calls"], shared["srcs"], shared["foreign"])):
        own = np.array([np.array_equal(shared["pool"][src[i]], c["qd"][i]) for i in range(len(src))])
        assert not own[foreign].any() and own[np.setdiff1d(np.arange(len(src)), foreign)].all(), f
        (m, b, s), need = shared["want"][f]
        assert need > 0 and (m >= 0).sum() >= max(len(src) // 8, 1)   # four queries contend for every slot
    assert TE.POOL_ROWS < TE.POOL_STRIDE and max(len(c["q"]) for c in per["calls"]) <= TE.POOL_ROWS
    planted, chained, leaked = set(), 0, 0
    for f, (c, src, out) in enumerate(zip(per["calls"], per["srcs"], per["off_pool"])):
        (m, b, s), need = per["want"][f]
        (fm, fb, fs), fneed = per["full"][f]
        planted |= set(src[out].tolist())
        assert set(src[out].tolist()) <= {-1, TE.POOL_ROWS} and need < fneed
        assert (m[out] == -1).all() and (b[out] == 256).all() and (s[out] == 256).all()
        assert (fm[out] >= 0).any() or len(out) == 1, f          # readable, the planted queries match
        assert np.array_equal(per["pools"][f][TE.POOL_ROWS], c["qd"][out[0]])
        rest = np.setdiff1d(np.arange(len(src)), out)
        assert np.array_equal(per["pools"][f][src[rest]], c["qd"][rest])
        chained += int((m[rest] != fm[rest]).sum() + (b[rest] != fb[rest]).sum())
        readable = src >= 0   # were row pool_rows addressable, the answers would change
        (rm, rb, _), _ = TE._core_want(c, per["pools"][f][np.where(readable, src, 0)], readable)
        leaked += int((rm != m).sum() + (rb != b).sum())
    assert planted == {-1, TE.POOL_ROWS} and chained > 0 and leaked > 0
