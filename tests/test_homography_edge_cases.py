"""tests/homography_edge_cases.py checked on the CPU, so that tests/test_gpu_homography_edges.py cannot go blind when someone
edits a case: (a) a census of the oracle's trace, branch by named branch, with the case that reaches it; (b) seven LM rules
broken in the oracle one at a time, each of which must change the H bits of a named case; (c) the branches no input reaches,
with the argument for each (also DESIGN.md section 8c).

(c) Unreachable, and why no case is listed for them:
  * run_kernel4 returning false inside RANSAC (`sFit[h] == 0`, the oracle's fit_failed).  It needs a spread
    sum |x_i - c| below DBL_EPSILON in one coordinate of one point set.  Then every difference x_j - x_i of that coordinate
    is below DBL_EPSILON in magnitude, so each cross product haveCollinearPoints forms is at most DBL_EPSILON * (|dy1| + |dy2|),
    nine orders below its bound FLT_EPSILON * (|dx1| + |dy1| + |dx2| + |dy2|): getSubset rejects the sample before it is
    fitted.  test_zero_spread_subsets_are_rejected_as_collinear checks this on random subsets.
  * a failed refit after a successful RANSAC (`state == ST_RANSAC && !fit`).  The four points of the accepted sample fit their
    own model to rounding, so they are inliers at any threshold a caller would pass, and the inliers' spreads are at least the
    sample's, which passed the test above.  The refit tap's zero branch and tap_info[3] = 0 are therefore reached only by
    method 0, n = 4 and failed calls.
  * `lim = min(HO_K, sNiters - base)` being 0 or negative: the chunk loop ends (sDone) as soon as the loop counter reaches
    niters, so a new chunk starts only with base < sNiters.  lim = 1 (max_iters 33, 65) and lim = 32 are in the table.
Reachable, against first expectation: a subset draw that fails at it > 0 (`sIdx[h][0] < 0` with it > 0): the case
subset_fails_at_1 does it."""
import numpy as np
import pytest

import homography_edge_cases as EC
import homography_oracle as HO

_CASES = EC.table()


def _run(name):
    s, d, kw = _CASES[name]
    H, mask, t = HO.find_homography(s, d, taps=True, **kw)
    return H, mask, t


@pytest.fixture(scope="module")
def runs():
    """name -> (H, mask, taps) of the unbroken oracle, computed once"""
    return {name: _run(name) for name in _CASES}


def _lm(runs, name):
    return runs[name][2]["trace"]["lm"]


def test_cases_are_small(runs):
    for name, (s, d, kw) in _CASES.items():
        assert len(s) <= EC.MAX_PAIRS and s.dtype == np.float32 and d.dtype == np.float32 and s.shape == d.shape, name
        assert runs[name][2]["iters"] <= EC.MAX_RANSAC_ITERS, name
        assert runs[name][0] is not None, name   # every edge case has a model: its H is what the GPU test compares


def test_trace_does_not_change_results():
    s, d, kw = _CASES["lm_ten_iterations"]
    H, mask = HO.find_homography(s, d, **kw)
    H2, mask2, t = HO.find_homography(s, d, taps=True, **kw)
    assert H.tobytes() == H2.tobytes() and np.array_equal(mask, mask2)
    tr = {}
    out = HO.refine(s, d, np.ones(len(s), bool), HO.run_kernel(s, d), trace=tr)
    assert out.tobytes() == H.tobytes() and tr["lm_iters"] == len(tr["lm"]) == 10
    s, d, kw = _CASES["n_256"]
    tr = {}
    a, b = HO.ransac(s, d), HO.ransac(s, d, trace=tr)
    assert a["H"].tobytes() == b["H"].tobytes() and (a["iters"], a["niters"]) == (b["iters"], b["niters"]) == (42, 38)
    assert tr["accepts"][-1] == (41, 38)


# ---- (a) the census: branch -> the case that reaches it --------------------------------------------------------------
def _any(steps, **want):
    return any(all(st[k] == v for k, v in want.items()) for st in steps)


LM_CENSUS = [
    ("R > 0.75", "lm_ten_iterations", lambda lm: _any(lm, band="high")),
    ("0.25 <= R <= 0.75", "lm_mid_band", lambda lm: _any(lm, band="mid")),
    ("0.25 <= R <= 0.75 (second case)", "lm_mid_band_last", lambda lm: _any(lm, band="mid")),
    ("R < 0.25", "lm_ten_iterations", lambda lm: _any(lm, band="low")),
    ("lambda halved to below lc: zeroed", "lm_ten_iterations", lambda lm: _any(lm, lam="zeroed")),
    ("lambda halved and kept (lambda >= lc)", "lm_ten_iterations", lambda lm: _any(lm, lam="kept")),
    ("inversion, then an iteration that compares lambda with the new lc", "lm_ten_iterations",
     lambda lm: any(a["inverted"] and b["band"] == "high" for a, b in zip(lm, lm[1:]))),
    ("inversion, lc read, then a second inversion", "lm_nu_between",
     lambda lm: sum(st["inverted"] for st in lm) >= 2 and _any(lm[2:], lam="kept")),
    ("nu clamped at 10", "lm_ten_iterations", lambda lm: _any(lm, nu="clamp10")),
    ("2 < nu < 10", "lm_nu_between", lambda lm: _any(lm, nu="between")),
    ("nu clamped at 2", "lm_mid_band", lambda lm: _any(lm, nu="clamp2")),
    ("nu clamped at 2 in the iteration after a rejected step, lambda != 0", "lm_clamp2_after_reject",
     lambda lm: any(not a["accepted"] and b["nu"] == "clamp2" and not b["inverted"] for a, b in zip(lm, lm[1:]))),
    ("step accepted", "lm_ten_iterations", lambda lm: _any(lm, accepted=True)),
    ("step rejected", "lm_ten_iterations", lambda lm: _any(lm, accepted=False)),
    ("rejected step with nu strictly between the clamps", "n_255", lambda lm: _any(lm, nu="between", accepted=False)),
]


@pytest.mark.parametrize("branch,name,reached", LM_CENSUS, ids=[c[0] for c in LM_CENSUS])
def test_census_lm_branches(runs, branch, name, reached):
    assert reached(_lm(runs, name)), (branch, name, _lm(runs, name))


LM_EXITS = [("iters", "lm_ten_iterations", 10), ("iters", "lm_tenth_step_a", 10), ("iters", "lm_tenth_step_b", 10),
            ("d", "lm_clamp2_after_reject", 7), ("d", "identity_pixels", 1), ("r", "lm_residual_exit", 1),
            ("r", "lm_residual_exit_ransac", 1)]


@pytest.mark.parametrize("why,name,iters", LM_EXITS, ids=[f"{c[0]}:{c[1]}" for c in LM_EXITS])
def test_census_lm_exits(runs, why, name, iters):
    tr = runs[name][2]["trace"]
    assert (tr["lm_exit"], tr["lm_iters"]) == (why, iters), name


def test_census_ransac_exit_counters(runs):
    want = {1: 1, 31: 31, 32: 32, 33: 33, 64: 64, 65: 65, 0: 1, -3: 1}
    assert set(want) == set(EC.CHUNK_EDGE_ITERS)
    for mi, it in want.items():
        t = runs[f"max_iters_{mi}"][2]
        assert (t["iters"], t["niters"]) == (it, it), mi
    # max_iters <= 0 is max_iters = 1, bit for bit
    for mi in (0, -3):
        assert runs[f"max_iters_{mi}"][0].tobytes() == runs["max_iters_1"][0].tobytes()
        assert np.array_equal(runs[f"max_iters_{mi}"][1], runs["max_iters_1"][1])
    # the 64 and 65 runs accept a model in the second chunk (iteration 63), the last lane of it
    assert runs["max_iters_64"][2]["trace"]["accepts"][-1][0] == 63
    assert runs["max_iters_65"][2]["trace"]["accepts"][-1][0] == 63


def test_census_threshold_defaults(runs):
    for name in ("threshold_0.0", "threshold_-1.0"):
        assert runs[name][0].tobytes() == runs["threshold_3.0"][0].tobytes(), name
        assert np.array_equal(runs[name][1], runs["threshold_3.0"][1]), name
    assert 0 < runs["threshold_3.0"][1].sum() < len(runs["threshold_3.0"][1])


def test_census_ransac_branches(runs):
    # the workgroup stride: one below, at and one above HO_T = 256
    assert [(runs[f"n_{n}"][2]["iters"], runs[f"n_{n}"][2]["niters"]) for n in (255, 256, 257)] == [(51, 51), (42, 38), (38, 38)]
    # niters below the loop counter at the moment of an update
    assert any(niters < it for it, niters in runs["n_256"][2]["trace"]["accepts"])
    # a collinear rejection inside a draw that then succeeds
    assert runs["duplicated_block"][2]["trace"]["collinear"] > 0 and runs["duplicated_block"][2]["ransac_ok"]
    # RANSACUpdateNumIters returning 0
    assert runs["identity_pixels"][2]["trace"]["accepts"] == [(0, 0)] and runs["identity_pixels"][2]["iters"] == 1
    # a draw that fails after iteration 0: the loop leaves with the model it has, counter below niters
    t = runs["subset_fails_at_1"][2]
    assert t["ransac_ok"] and (t["iters"], t["niters"]) == (1, 2) and t["trace"]["collinear"] > 10000
    # no case has a failed 4-point fit or a failed refit: see (c) in the module docstring
    for name in _CASES:
        t = runs[name][2]
        assert t["trace"].get("fit_failed", 0) == 0, name
        assert t["refit_ok"] == t["ransac_ok"], name


# ---- (b) sensitivity: each broken rule changes the H bits of a named case -----------------------------------------------
SENSITIVE = {
    "lc_stale": ("lm_ten_iterations", "lm_nu_between"),
    "nu_unclamped_10": ("lm_ten_iterations", "lm_clamp2_after_reject"),
    "nu_not_halved": ("lm_ten_iterations", "lm_nu_between"),
    "lambda_always_zero": ("lm_ten_iterations", "lm_nu_between"),
    "iters_9": ("lm_tenth_step_a", "lm_tenth_step_b"),
    "mid_as_low": ("lm_mid_band",),
    "no_r_exit": ("lm_residual_exit", "lm_residual_exit_ransac"),
}


def test_every_rule_has_a_sensitive_case():
    assert set(SENSITIVE) == set(HO.LM_RULES) and HO.LM_BREAK == frozenset()
    assert all(name in _CASES for names in SENSITIVE.values() for name in names)


@pytest.mark.parametrize("rule", HO.LM_RULES)
def test_broken_rule_changes_h(runs, monkeypatch, rule):
    monkeypatch.setattr(HO, "LM_BREAK", frozenset([rule]))
    for name in SENSITIVE[rule]:
        H, mask, _ = _run(name)
        assert H is not None and H.tobytes() != runs[name][0].tobytes(), (rule, name)
        assert np.array_equal(mask, runs[name][1]), (rule, name)   # LM never touches the mask


def test_reached_but_not_proven(runs, monkeypatch):
    """what the census reaches without the H depending on it, so nobody mistakes these cases for proofs"""
    monkeypatch.setattr(HO, "LM_BREAK", frozenset(["mid_as_low"]))
    assert _run("lm_mid_band_last")[0].tobytes() == runs["lm_mid_band_last"][0].tobytes()
    monkeypatch.setattr(HO, "LM_BREAK", frozenset(["no_r_exit"]))
    assert _run("identity_pixels")[0].tobytes() == runs["identity_pixels"][0].tobytes()


# ---- (c) run_kernel cannot fail on a subset that get_subset lets through -----------------------------------------------
def test_zero_spread_subsets_are_rejected_as_collinear():
    rng = np.random.default_rng(17)
    refused = 0
    for trial in range(400):
        pts = [(rng.random((4, 2)) * [640, 480]).astype(np.float32) for _ in range(2)]
        which, axis, kind = rng.integers(0, 2), rng.integers(0, 2), trial % 4
        if kind == 0:     # one coordinate of one set constant
            pts[which][:, axis] = pts[which][0, axis]
        elif kind == 1:   # ... differing by less than DBL_EPSILON in sum
            pts[which][:, axis] = (rng.random(4) * 5e-17).astype(np.float32)
        elif kind == 2:   # a whole set shrunk below DBL_EPSILON
            pts[which] = (pts[which] * np.float32(1e-20)).astype(np.float32)
        else:             # control: an ordinary subset
            pass
        src, dst = pts
        fit = HO.run_kernel(src, dst)
        rejected = (HO.have_collinear_points([tuple(map(float, p)) for p in src], 4) or
                    HO.have_collinear_points([tuple(map(float, p)) for p in dst], 4))
        if fit is None:
            refused += 1
            assert rejected, (trial, src, dst)
        if kind == 3:
            assert fit is not None and not rejected, trial
    assert refused >= 250
