"""tests/proj_edge_cases.py reaches the edges it names: for every table the CPU oracle alone gives the planted answers, the
members of every pair differ, and the oracle agrees with a plain numpy restatement of the box test, the cell rectangle and the
decision rule (every operation rounded to binary32).  No case is dropped silently: every test counts the cases it checked
against the table's length.  CPU only; tests/test_gpu_projection_edges.py runs the same tables through the HIP kernels."""
import ctypes as C

import numpy as np
import pytest

import hamming_cases as H
import proj_edge_cases as E
from oracle import oracle_ffi as O

F = np.float32


# ------------------------------------------------------------------------------------------------ plain restatements
def cells_np(g, xy):
    """PosInGrid for every keypoint: cell or -1"""
    minx, miny, gwi, ghi = g
    with np.errstate(all="ignore"):
        p = [((xy[:, k] - mn).astype(F) * inv).astype(F).astype(np.float64) for k, mn, inv in ((0, minx, gwi), (1, miny, ghi))]
        px, py = (np.copysign(np.floor(np.abs(v) + 0.5), v) for v in p)
        ok = np.isfinite(px) & np.isfinite(py) & (px >= 0) & (px < E.COLS) & (py >= 0) & (py < E.ROWS)
        return np.where(ok, np.where(ok, px, 0) * E.ROWS + np.where(ok, py, 0), -1).astype(np.int64)


def area_np(ci, cells, Q):
    """GetFeaturesInArea: the keypoints of the rectangle's cells, column-major, ascending index inside a cell, that pass the
    level filter and the strict box test"""
    g = tuple(F(v) for v in ci["bounds"])
    u, v, r = F(Q["u"]), F(Q["v"]), F(Q["r"])
    rect = E.rect_of(g, u, v, r)
    if rect is None:
        return np.zeros(0, np.int64)
    x0, y0, nx, ny = rect
    xy, octv = ci["xyF"], ci["octF"]
    px, py = cells // E.ROWS, cells % E.ROWS
    ok = (cells >= 0) & (px >= x0) & (px < x0 + nx) & (py >= y0) & (py < y0 + ny)
    if Q["min_level"] > 0 or Q["max_level"] >= 0:
        ok &= octv >= Q["min_level"]
        if Q["max_level"] >= 0:
            ok &= octv <= Q["max_level"]
    with np.errstate(all="ignore"):
        ok &= (np.abs((xy[:, 0] - u).astype(F)) < r) & (np.abs((xy[:, 1] - v).astype(F)) < r)
    idx = np.flatnonzero(ok)
    return idx[np.argsort(cells[idx], kind="stable")]


def core_np(c, areas):
    """the sequential loop of SearchByProjection over the calls' queries (src/ORBmatcher.cc:63-157 / :1578-1724 and Fuse's gate)"""
    ci, q = c["ci"], c["q"]
    xy, octv, uR = ci["xyF"], ci["octF"], ci["uRight"]
    taken = np.zeros(len(xy), bool) if ci["blocked"] is None else np.asarray(ci["blocked"]) != 0
    taken = taken.copy()
    is2 = c["is2"]
    out = []
    for i, Q in enumerate(q):
        b1 = b2 = 256
        l1 = l2 = bi = -1
        cand = areas[i]
        d = H.distances(c["qd"][i], ci["descF"][cand])[0] if len(cand) else []
        for k, dist in zip(cand, d):
            if taken[k]:
                continue
            if (Q["flags"] & 2) and uR is not None and uR[k] > 0 and np.abs(F(Q["ur"] - uR[k])) > Q["r"]:
                continue
            if (Q["flags"] & 4) and is2 is not None:
                ex, ey = F(Q["u"] - xy[k, 0]), F(Q["v"] - xy[k, 1])
                e2 = F(F(ex * ex) + F(ey * ey))
                lv = min(max(int(octv[k]), 0), len(is2) - 1)
                stereo = uR is not None and uR[k] >= 0
                if stereo:
                    er = F(Q["ur"] - uR[k])
                    e2 = F(e2 + F(er * er))
                if float(F(e2 * F(is2[lv]))) > (7.8 if stereo else 5.99):
                    continue
            if dist < b1:
                b2, l2, b1, l1, bi = b1, l1, int(dist), int(octv[k]), int(k)
            elif dist < b2:
                b2, l2 = int(dist), int(octv[k])
        m = -1
        if b1 <= c["th"] and not (c["rule"] and l1 == l2 and F(b1) > F(F(c["nnratio"]) * F(b2))):
            m = bi
            taken[bi] = bool(Q["flags"] & 1)
        out.append((m, b1, b2))
    return out


# ------------------------------------------------------------------------------------------------ the projection tables
def check_projection_case(name, case):
    answers = []
    for ci_, c in enumerate(case["calls"]):
        ci, q, want = c["ci"], c["q"], c["want"]
        g = tuple(F(v) for v in ci["bounds"])
        cells = cells_np(g, ci["xyF"])
        areas = [E.oracle_area(c, i) for i in range(len(q))]
        mine = [area_np(ci, cells, q[i]) for i in range(len(q))]
        for i in range(len(q)):
            assert np.array_equal(areas[i], mine[i]), (name, ci_, i, "GetFeaturesInArea against the restatement")
        rects = [E.rect_of(g, q["u"][i], q["v"][i], q["r"][i]) for i in range(len(q))]
        m, b, s = E.run_core(O.search_by_projection, c)
        assert [(int(x), int(y), int(z)) for x, y, z in zip(m, b, s)] == core_np(c, areas), (name, ci_, "core against the restatement")
        for i in range(len(q)):
            if want.get("ncand") is not None and want["ncand"][i] is not None:
                assert len(areas[i]) == want["ncand"][i], (name, ci_, i, len(areas[i]))
            if "cands" in want:
                assert areas[i].tolist() == list(want["cands"][i]), (name, ci_, i, areas[i])
            if "rect" in want:
                assert rects[i] == want["rect"][i], (name, ci_, i)
            for key, got in (("match", m), ("best", b), ("second", s)):
                if key in want:
                    assert int(got[i]) == want[key][i], (name, ci_, i, key, int(got[i]))
        answers.append([(tuple(areas[i].tolist()), rects[i], int(m[i]), int(b[i]), int(s[i])) for i in range(len(q))])
        if "chain" in c:
            check_chain(name, c, m)
    for a, bb in case["differ"]:
        a, bb = (a, 0) if isinstance(a, int) else a, (bb, 0) if isinstance(bb, int) else bb
        assert answers[a[0]][a[1]] != answers[bb[0]][bb[1]], (name, a, bb, "planted members do not differ")
    return answers


def check_chain(name, c, m):
    """link i needs i sequential steps: alone (the earlier queries removed) the first `chain` links after the head are
    rejected, in the full loop each one is accepted: its predecessor has claimed its second-best slot by then"""
    L = c["chain"]
    assert int(m[0]) == 0
    for i in range(1, L + 1):
        sub = dict(c, q=c["q"][i:], qd=c["qd"][i:])
        ms = E.run_core(O.search_by_projection, sub)[0]
        assert int(ms[0]) == -1 and int(m[i]) == i, (name, i)


@pytest.mark.parametrize("table", ["WINDOW_CASES", "SLAB_CASES", "DECISION_CASES", "GATE_CASES", "ROUND_CASES"])
def test_projection_tables_reach_their_edges(oracle, table):
    checked = 0
    for name, build in E.TABLES[table].items():
        check_projection_case(name, build())
        checked += 1
    assert checked == len(E.TABLES[table]) and checked > 0


def test_window_cases_hold_the_planted_counts(oracle):
    """the counts the issue names: only the centre at r = 10 and one step below, all five in order [2, 4, 0, 3, 1] one step above;
    rectangles of 1, 64, 65 and 3072 cells; every level window; every case at both image bounds"""
    assert len(E.WINDOW_CASES) == 2 * len(E._WINDOW_BUILDERS)
    for bn in E.BOUNDS:
        box = E.WINDOW_CASES["box_radius-" + bn]()["calls"][0]
        assert [E.oracle_area(box, i).tolist() for i in range(3)] == [[0], [0], [2, 4, 0, 3, 1]]
        cc = E.WINDOW_CASES["cell_counts-" + bn]()["calls"][0]
        assert [r[2] * r[3] for r in cc["want"]["rect"]] == [1, 64, 65, 65, 3072]
        assert len(E.oracle_area(cc, 4)) == int((cells_np(E.grid_params(E.BOUNDS[bn]), cc["ci"]["xyF"]) >= 0).sum())
        lv = E.WINDOW_CASES["levels-" + bn]()["calls"][0]
        assert [(int(a), int(b)) for a, b in zip(lv["q"]["min_level"], lv["q"]["max_level"])] == E.LEVEL_WINDOWS
    minx, _, miny, _ = E.DISTORTED
    assert minx < 0 and miny < 0 and minx != round(minx) and miny != round(miny)


def test_slab_cases_sit_on_the_switches(oracle):
    for n in (511, 512, 513):
        c = E.SLAB_CASES["candidates_%d" % n]()["calls"][0]
        cnt = [len(E.oracle_area(c, i)) for i in range(len(c["q"]))]
        assert cnt[12] == n - 1 and cnt[-1] == n and max(cnt[:12] + cnt[13:-1]) < 100
    for t in (16384, 16385):
        c = E.SLAB_CASES["lds_words_%d" % t]()["calls"][0]
        assert max(len(c["ci"]["xyF"]), 1) + 8 * len(c["q"]) == t
    assert [len(E.SLAB_CASES["queries_%d" % n]()["calls"][0]["q"]) for n in (1, 4, 5, 64, 65, 1024, 1025)] == [1, 4, 5, 64, 65, 1024, 1025]
    assert len(E.SLAB_CASES["features_15360"]()["calls"][0]["ci"]["xyF"]) == E.PJ_MAX_NF
    c = E.SLAB_CASES["window_distances_65535"]()["calls"][0]
    assert len(c["ci"]["xyF"]) == E.WD_MAX_NF and (E.WD_MAX_NF - 1) in E.oracle_area(c, 0).tolist()
    c = E.SLAB_CASES["queries_1025"]()["calls"][0]   # contended: more than 64 queries lose their round-0 choice to an earlier claim
    free = E.run_core(O.search_by_projection, dict(c, q=np.array([(u, v, r, a, b, ur, fl & ~1, p) for u, v, r, a, b, ur, fl, p in c["q"]], c["q"].dtype)))[0]
    assert int((free != E.run_core(O.search_by_projection, c)[0]).sum()) > 64


def test_gate_cases_cover_every_flag_and_the_four_bounds(oracle):
    flags, no_right, no_sigma = set(), False, False
    for name, build in E.GATE_CASES.items():
        for c in build()["calls"]:
            flags |= set(int(f) for f in c["q"]["flags"])
            no_right |= c["ci"]["uRight"] is None and bool((c["q"]["flags"] & 2).any())
            no_sigma |= c["is2"] is None and bool((c["q"]["flags"] & 4).any())
    assert {0, 1, 2, 4, 7} <= flags and no_right and no_sigma
    # the chi-square products are the four floats themselves: e2 = 1 exactly
    c = E.GATE_CASES["chi2_gate"]()["calls"][0]
    ci, q = c["ci"], c["q"]
    prod = set()
    for i in np.flatnonzero(q["flags"] & 4):
        k = int(E.oracle_area(c, i)[0])
        ex, ey = F(q["u"][i] - ci["xyF"][k, 0]), F(q["v"][i] - ci["xyF"][k, 1])
        e2 = F(F(ex * ex) + F(ey * ey))
        if ci["uRight"][k] >= 0:
            er = F(q["ur"][i] - ci["uRight"][k])
            e2 = F(e2 + F(er * er))
        assert e2 == F(1)
        prod.add(F(e2 * c["is2"][min(max(int(ci["octF"][k]), 0), len(c["is2"]) - 1)]).tobytes())
    B = E.CHI2_BOUNDS
    assert {B[k].tobytes() for k in B} <= prod
    assert float(B["stereo_over"]) > 7.8 > float(B["stereo_under"]) and float(B["mono_over"]) > 5.99 > float(B["mono_under"])
    assert B["stereo_over"] == F(7.8) and B["mono_under"] == F(5.99)
    assert not B["stereo_over"] > F(7.8)   # a compare in float keeps what the double compare skips
    # the right gate: equality and one step above
    r = E.GATE_CASES["right_gate"]()["calls"][0]
    d = np.abs((r["q"]["ur"] - F(100)).astype(F))
    assert d[0] == r["q"]["r"][0] and d[1] > r["q"]["r"][1] and r["q"]["ur"][1] == E.up(r["q"]["ur"][0]) and d[3] == r["q"]["r"][3] and d[4] > r["q"]["r"][4]


# ------------------------------------------------------------------------------------------------ the grid table
def cells_from_grid(off, idx, n):
    cell = np.full(n, -1, np.int64)
    for c in np.flatnonzero(np.diff(off.astype(np.int64))):
        members = idx[off[c]:off[c + 1]]
        assert np.all(np.diff(members.astype(np.int64)) > 0), "a cell's list is in keypoint order"
        cell[members] = c
    return cell


def test_grid_cases_reach_their_edges_and_the_host_form_equals_the_oracle(oracle):
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    checked = 0
    for name, build in E.GRID_CASES.items():
        case = build()
        xy, g = case["xy"], E.grid_params(case["bounds"])
        off, idx = O.assign_grid(xy, *[float(v) for v in g])
        cell = cells_from_grid(off, idx, len(xy))
        assert cell.tolist() == case["cell"], (name, np.flatnonzero(cell != np.array(case["cell"]))[:8])
        assert np.array_equal(cell, cells_np(g, xy)), name
        hoff, hidx, nin = np.zeros(E.COLS * E.ROWS + 1, np.uint32), np.zeros(max(len(xy), 1), np.uint32), C.c_int32()
        assert L.orbfe_assign_grid_host(_ffi.ptr(np.ascontiguousarray(xy, F)), len(xy), *[float(v) for v in g], _ffi.ptr(hoff), _ffi.ptr(hidx),
                                        C.byref(nin)) == 0
        assert nin.value == len(idx) and np.array_equal(hoff, off) and np.array_equal(hidx[:nin.value], idx), name
        checked += 1
    assert checked == len(E.GRID_CASES) == 2 * len(E._GRID_BUILDERS)
    # the planted directions: inside one step below the last column's tie and outside at it (634.9999 / 635.0 at 640 wide)
    t = E.GRID_CASES["round_ties-origin"]()
    i = 4 * 4   # k = 63: the keypoints (dn(lo), lo, hi, up(hi))
    assert t["cell"][i + 1] // E.ROWS == 63 and t["cell"][i + 2] == -1 and t["xy"][i + 2, 0] == F(635.0) and t["xy"][i + 1, 0] == E.dn(635.0)
    n = E.GRID_CASES["nonfinite-origin"]()
    bad = ~np.isfinite(n["xy"]).all(1) | (np.abs(n["xy"]) > 1e20).any(1)
    assert bad.sum() == 10 and all(n["cell"][k] == -1 for k in np.flatnonzero(bad))
    for k, cnt in (("one_cell_2000", 2000), ("one_cell_300", 300)):
        assert len(set(E.GRID_CASES[k + "-distorted"]()["cell"])) == 1 and len(E.GRID_CASES[k + "-origin"]()["cell"]) == cnt


# ------------------------------------------------------------------------------------------------ the triangulation table
def test_triangulation_cases_reach_their_edges(oracle):
    checked = 0
    for name, build in E.TRI_CASES.items():
        case = build()
        got = [E.run_tri(O.search_for_triangulation, c) for c in case["calls"]]
        for k, c in enumerate(case["calls"]):
            if c["want"] is not None:
                assert got[k].tolist() == c["want"], (name, k, got[k])
        for a, b in case["differ"]:
            assert got[a].tolist() != got[b].tolist(), (name, a, b)
        if name.startswith("sizes_"):
            n1 = int(name.split("_")[1])
            assert len(got[0]) == n1 and int((got[0] >= 0).sum()) > n1 // 10 and got[0][-1] >= -1
        checked += 1
    assert checked == len(E.TRI_CASES)
    for o in (0, 3, 7):   # dsqr one float either side of 3.84 * sigma2 as a double
        y_in, y_out, d_in, d_out, bound = E.tri_dsqr_steps(o)
        assert y_out == E.up(y_in) and d_in < bound <= d_out
