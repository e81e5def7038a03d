"""tests/flow_edge_cases.py reaches the edges it names: with the CPU oracle alone, every size has the level plan its tag claims,
every frame pair puts both values into the pre-morphology mask, every flow is finite, the library's host-side plan equals the
oracle's over a sweep of sizes across the level steps, and the extended keypoint rule gives the planted keep lists."""
import ctypes as C

import numpy as np
import pytest

import flow_edge_cases as E
import flow_oracle as FO
from flow_checks import oracle_pair


def _of(c, th=40.0):
    return oracle_pair((c["w"], c["h"]), lambda: E.pair(c), th)


def test_level_plans_are_the_ones_the_tags_claim():
    counts, ties, one_axis, w2s = set(), set(), [], set()
    for c in E.SIZES:
        w2, h2 = c["w"] // 2, c["h"] // 2
        plan = FO.level_plan(w2, h2)[::-1]
        assert [(p[0], p[1]) for p in plan] == c["levels"], c
        counts.add(len(plan))
        w2s.add(w2)
        for lv, (lw, lh) in enumerate(c["levels"]):
            for full, got in ((w2, lw), (h2, lh)):
                v = full * 0.5 ** lv
                if v - np.floor(v) == 0.5:
                    ties.add("down" if got < v else "up")
                    assert got % 2 == 0, (c, lv)   # half to even
        if len(plan) > 1:
            lw, lh = c["levels"][1]
            if (w2 == 2 * lw) != (h2 == 2 * lh):
                one_axis.append((c["w"], c["h"]))
    assert counts == {1, 2, 3, 4}
    assert ties == {"down", "up"}
    assert (260, 258) in one_axis and (258, 256) in one_axis and (256, 262) in one_axis   # x only, y only
    assert {256, 257} <= w2s
    assert len({(c["w"], c["h"]) for c in E.SIZES}) == len(E.SIZES) == 29
    for wh in E.ONE_HANDLE:
        E.case_of(*wh)
    assert {len(E.case_of(*wh)["levels"]) for wh in E.ONE_HANDLE} == {1, 2, 3, 4}


def test_every_size_has_both_mask_values_before_the_morphology():
    """Zero share of the pre-morphology mask at threshold 40 in [0.02, 0.98], so the threshold and all three morphology passes
    have work at every size.  E.FLOW_ONLY names the sizes allowed to miss it, so that no other size can lose this coverage
    silently.  It is empty: (19, 23), (40, 22), (64, 20), (512, 16) and (514, 16) were expected to need it, but the bowl and
    the 96 px wave move their flow past the clamped threshold, so they are held to the same condition as the rest."""
    assert E.FLOW_ONLY == []
    checked, lacking = 0, []
    for c in E.SIZES:
        pre = _of(c).taps["mask_pre"]
        assert pre.shape == (c["h"], c["w"]) and set(np.unique(pre)) <= {0, 1}
        z = float((pre == 0).mean())
        if not 0.02 <= z <= 0.98:
            lacking.append((c["w"], c["h"]))
        checked += 1
    assert checked == len(E.SIZES)
    assert lacking == E.FLOW_ONLY, lacking


def test_every_flow_tap_is_finite():
    n = 0
    for c in E.SIZES:
        for f in _of(c).taps["flow_levels"] + [_of(c).taps["flow2"]]:
            assert np.isfinite(f).all(), c
        n += 1
    for (w, h) in E.DEGENERATE_SIZES:
        for name in E.DEGENERATE:
            of = oracle_pair((name, w, h), lambda: E.degenerate(name, w, h), 40.0)
            for f in of.taps["flow_levels"] + [of.taps["flow2"]]:
                assert np.isfinite(f).all(), (name, w, h)
            n += 1
    assert n == len(E.SIZES) + len(E.DEGENERATE) * len(E.DEGENERATE_SIZES)


def test_threshold_list_sits_on_both_sides_of_the_clamp():
    f = np.float32
    assert all(f(t) < f(40) for t in E.TH_AS_40) and f(E.TH_AS_40[0]) == np.nextafter(f(40), f(0))
    assert f(E.TH_OTHER[0]) == np.nextafter(f(40), f(np.inf)) and np.isinf(f(E.TH_OTHER[2])) and np.isnan(f(E.TH_OTHER[3]))
    c = E.case_of(*E.THRESHOLD_SIZE)
    a, b = E.pair(c)
    base = _of(c)
    assert c["w"] % 2 == 1 and c["h"] % 2 == 1      # the strip outside the pyrUp'ed flow exists on both axes
    for th in E.TH_AS_40:
        of = FO.Flow()
        of.compute_mask(a, th)
        assert np.array_equal(of.compute_mask(b, th), base.taps["mask"])
    of = FO.Flow()
    of.compute_mask(a, float("inf"))
    assert of.compute_mask(b, float("inf")).all()
    of.reset()
    of.compute_mask(a, float("nan"))
    of.compute_mask(b, float("nan"))
    pre = of.taps["mask_pre"]
    assert not pre[:-1, :-1].any() and pre[-1, :].all() and pre[:, -1].all()   # NaN: only the odd strip stays 1
    assert not of.taps["mask"].any()                                          # and is eroded away


# ---- the library's host-side plan ---------------------------------------------------------------------------------------
SWEEP_H = [16, 17] + list(range(126, 134)) + list(range(254, 264)) + list(range(510, 528)) + [1100]


def test_library_plan_equals_the_oracle_over_the_level_steps():
    """orbfe_flow_plan (host only) against FO.level_plan for every w in 16..1100 against the heights around each level step,
    and the transpose: level count, sizes, ksize, and the blur taps bit for bit"""
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    n = C.c_int32()
    lw, lh, ks = (np.zeros(4, np.int32) for _ in range(3))
    taps = np.zeros((4, 19), np.float32)
    args = (C.byref(n), _ffi.ptr(lw), _ffi.ptr(lh), _ffi.ptr(ks), _ffi.ptr(taps))
    want_taps = {}
    ora = {}
    bad = []
    for w in range(16, 1101):
        for h in SWEEP_H:
            for (a, b) in ((w, h), (h, w)):
                assert L.orbfe_flow_plan(a, b, *args) == _ffi.ORBFE_OK
                key = (a // 2, b // 2)
                if key not in ora:
                    ora[key] = FO.level_plan(*key)[::-1]
                o = ora[key]
                ok = n.value == len(o)
                for l, (ow, oh, sigma, oks) in enumerate(o):
                    if not ok:
                        break
                    if (oks, sigma) not in want_taps:
                        t = np.zeros(19, np.float32)
                        t[:oks] = FO.gaussian_kernel(oks, sigma)
                        want_taps[(oks, sigma)] = t.tobytes()
                    ok = (lw[l], lh[l], ks[l]) == (ow, oh, oks) and taps[l].tobytes() == want_taps[(oks, sigma)]
                if not ok:
                    bad.append((a, b))
    assert not bad, bad[:20]
    assert sorted(want_taps) == [(3, 0.0), (3, 0.5), (9, 1.5), (19, 3.5)]


# ---- the keypoint rule ----------------------------------------------------------------------------------------------------
def _rule(case):
    kk, dd = FO.mask_rule(case["mask"], case["kps"], case["desc"])
    keep = case["keep"]
    assert np.array_equal(kk.view(np.uint8), case["kps"][keep].view(np.uint8)), "keypoints"
    assert np.array_equal(dd, case["desc"][keep]), "descriptors"


@pytest.mark.parametrize("pattern", E.KEEP_PATTERNS)
def test_mask_rule_gives_the_planted_keep_lists(pattern):
    for n in E.RULE_COUNTS:
        c = E.rule_case(n, pattern)
        assert len(c["kps"]) == n and c["mask"].sum() > c["mask"].size * 0.65
        if n >= 256 and pattern in ("first_of_256", "last_of_256"):
            assert 1 <= c["keep"].sum() <= 3
        _rule(c)


def test_mask_rule_share_values_coordinates_and_batch():
    assert 20 * 20 * 0.65 == 260.0 and 7 * 9 * 0.65 != int(7 * 9 * 0.65)   # the bound is an integer at 20x20 only
    for (w, h) in ((20, 20), (7, 9)):
        for extra in (0, 1):
            c = E.share_case(w, h, extra)
            assert int(c["mask"].sum()) == int(h * w * 0.65) + extra
            assert bool(c["keep"][1]) == (extra == 0)
            _rule(c)
    c = E.value_case()
    assert {2, 255} <= set(np.unique(c["mask"]))
    _rule(c)
    c = E.coordinate_case()
    x, y = c["kps"]["x"], c["kps"]["y"]
    assert np.isnan(x).any() and np.isnan(y).any() and np.isinf(x).any() and (x == -1).any() and (x == c["mask"].shape[1]).any()
    _rule(c)
    # inside the plane the extended rule is the old one: mask[int(y)][int(x)] == 1
    ins = (x > -1) & (x < c["mask"].shape[1]) & (y > -1) & (y < c["mask"].shape[0])
    old = c["mask"][y[ins].astype(np.int32), x[ins].astype(np.int32)] == 1
    assert np.array_equal(old, c["keep"][ins]) and not c["keep"][~ins].any()
    fr = E.batch_case()
    sums = [float(f["mask"].sum()) / f["mask"].size for f in fr]
    assert sums[0] > 0.65 and sums[1] <= 0.65 and sums[2] > 0.65
    assert 0 < fr[0]["keep"].sum() < len(fr[0]["keep"]) and fr[1]["keep"].all() and not fr[2]["keep"].any()
    assert not (fr[1]["mask"][fr[1]["kps"]["y"].astype(int), fr[1]["kps"]["x"].astype(int)] == 1).all()
    for f in fr:
        _rule(f)
