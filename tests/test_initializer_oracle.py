"""tests/initializer_oracle.py, the numpy restatement of the monocular Initializer, checked on its own (CPU): hand-worked pieces,
the restated float SVD against LAPACK, noiseless scenes against their ground truth, and every steered case of
tests/initializer_cases.py shown to take the branch it is named for.

Measured figures (this file prints them; the assertions sit at four times the measured value, as test_pnp_oracle.py does):
  float SVD on the KAT matrices (16x9, 8x9, 3x3, 4x4), against float64 LAPACK on the same float32 matrix:
    |U diag(w) Vt - A| / max|A|   3.93e-7      |U^T U - I|   5.02e-7      |Vt Vt^T - I|   5.90e-7      |w - w_lapack| / w_max   3.49e-7
    8 x 9: |A vt[8]| / max|A|     6.85e-8      | ||vt[8]|| - 1 |   5.63e-8
  noiseless general scenes, against ground truth:   |R21 - R|  2.78e-6   |t21 - t/|t||  1.80e-5   |X |t| - X_true| / max|X_true|  3.99e-5
"""
import numpy as np
import pytest

import initializer_cases as IC
import initializer_oracle as IO

SVD_RESIDUAL, SVD_ORTHO_U, SVD_ORTHO_VT, SVD_VALUES = 3.93e-7, 5.02e-7, 5.90e-7, 3.49e-7
NULL_RESIDUAL, NULL_NORM = 6.85e-8, 5.63e-8
SCENE_R, SCENE_T, SCENE_X = 2.78e-6, 1.80e-5, 3.99e-5
GENERAL = ("general_63", "general_64", "general_65", "general_257", "general_100_it65", "general_120_it200")
PLANAR = ("planar_64", "planar_257")


def test_normalize_hand_worked():
    pts, T = IO.normalize(np.array([[0, 0], [2, 0], [0, 4], [2, 4]], np.float32))
    assert np.array_equal(pts, np.array([[-1, -1], [1, -1], [-1, 1], [1, 1]], np.float32))
    assert np.array_equal(T, np.array([[1, 0, -1], [0, 0.5, -1], [0, 0, 1]], np.float32))
    # the mean and the absolute moment run over ALL keys, matched or not
    pts, T = IO.normalize(np.array([[1, 1], [3, 5], [8, 0]], np.float32))
    assert T[0, 0] == np.float32(1.0 / float(np.float32(8.0) / np.float32(3))) and T[0, 2] == np.float32(-4) * T[0, 0]


def _draw_for(p, size):
    """a raw rand() value that RandomInt(0, size - 1) turns into p"""
    r = int(np.ceil(p * 2147483648.0 / size)) + 1
    assert IO.index_from_draw(r, size) == p
    return r


def test_set_replay_hand_worked():
    # always position 0: the first pick is 0, then whatever the back element was when it moved in: 9, 8, ...
    d = [_draw_for(0, 10 - k) for k in range(8)]
    assert IO.sets_from_draws(d, 1, 10)[0].tolist() == [0, 9, 8, 7, 6, 5, 4, 3]
    assert IO.set_without_list(d, 10) == [0, 9, 8, 7, 6, 5, 4, 3]
    # always the back element: nothing moves
    d = [_draw_for(9 - k, 10 - k) for k in range(8)]
    assert IO.sets_from_draws(d, 1, 10)[0].tolist() == [9, 8, 7, 6, 5, 4, 3, 2]
    # 3, then 3 again (now holding 9), then 8 (the back, which is 8), then 3 (now holding 7, moved in when 9 left)
    d = [_draw_for(3, 10), _draw_for(3, 9), _draw_for(7, 8), _draw_for(3, 7)] + [_draw_for(0, 6 - k) for k in range(4)]
    want = [3, 9, 7, 8, 0, 5, 4, 6]
    assert IO.sets_from_draws(d, 1, 10)[0].tolist() == want
    assert IO.set_without_list(d, 10) == want


@pytest.mark.parametrize("N", [8, 9, 10, 64, 1000])
def test_set_replay_without_the_list(N):
    rng = np.random.default_rng(N)
    d = rng.integers(0, 2 ** 31, 8 * 200)
    if N <= 10:   # small ranges with many repeated positions
        d[:800] = [_draw_for(int(p) % (N - k % 8), N - k % 8) for k, p in enumerate(rng.integers(0, 3, 800))]
    sets = IO.sets_from_draws(d, 200, N)
    for it in range(200):
        assert IO.set_without_list(d[8 * it:8 * it + 8], N) == sets[it].tolist()
        assert len(set(sets[it].tolist())) == 8 and sets[it].min() >= 0 and sets[it].max() < N


@pytest.mark.parametrize("what", ["16x9", "8x9", "3x3", "4x4"])
def test_float_svd_against_lapack(what):
    A = IC.kat_matrices(what)
    w, u, vt = IO.svd_f(A)
    A64, u64, w64, vt64 = A.astype(np.float64), u.astype(np.float64), w.astype(np.float64), vt.astype(np.float64)
    k = w.shape[1]
    assert u.shape[1:] == (A.shape[1], A.shape[1]) and vt.shape[1:] == (A.shape[2], A.shape[2])   # FULL_UV
    res = np.abs(np.einsum("bik,bk,bkj->bij", u64[:, :, :k], w64, vt64[:, :k, :]) - A64).max() / np.abs(A64).max()
    ou = np.abs(np.einsum("bki,bkj->bij", u64, u64) - np.eye(u.shape[2])).max()
    ov = np.abs(np.einsum("bik,bjk->bij", vt64, vt64) - np.eye(vt.shape[1])).max()
    sv = np.linalg.svd(A64, compute_uv=False)
    dv = (np.abs(sv - w64) / sv[:, :1]).max()
    print(f"{what}: residual {res:.3g} orthoU {ou:.3g} orthoVt {ov:.3g} values {dv:.3g}")
    assert res <= 4 * SVD_RESIDUAL and ou <= 4 * SVD_ORTHO_U and ov <= 4 * SVD_ORTHO_VT and dv <= 4 * SVD_VALUES
    assert (np.diff(w, axis=1) <= 0).all()
    if what == "8x9":   # the refill row is the null vector
        nr = np.abs(np.einsum("bij,bj->bi", A64, vt64[:, 8, :])).max() / np.abs(A64).max()
        nn = np.abs(np.linalg.norm(vt64[:, 8, :], axis=1) - 1).max()
        print(f"8x9: |A vt[8]| {nr:.3g}  | |vt[8]| - 1 | {nn:.3g}")
        assert nr <= 4 * NULL_RESIDUAL and nn <= 4 * NULL_NORM
    if what in ("3x3", "4x4"):   # the rank-deficient first matrix: a null singular value, its left vector refilled to unit length
        assert w[0, -1] <= 4 * SVD_VALUES * w[0, 0]


def test_svd_without_the_extra_rows_gives_the_same_vt():
    A = IC.kat_matrices("16x9")
    w, u, vt = IO.svd_f(A)
    w2, u2, vt2 = IO.svd_f(A, full=False)
    assert np.array_equal(vt.view(np.uint32), vt2.view(np.uint32)) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))
    assert np.array_equal(u[:, :, :9].view(np.uint32), u2.view(np.uint32))


def test_inv3_and_products():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(20, 3, 3)).astype(np.float32)
    I = IO.mm(A, IO.inv3(A)).astype(np.float64)
    assert np.abs(I - np.eye(3)).max() < 1e-4
    assert np.array_equal(IO.inv3(np.zeros((3, 3), np.float32)), np.zeros((3, 3), np.float32))   # det == 0: zeros
    B = rng.normal(size=(20, 3, 3)).astype(np.float32)
    assert np.abs(IO.mm(A, B) - A.astype(np.float64) @ B.astype(np.float64)).max() < 1e-5
    assert np.abs(IO.mm_t(A, B, ta=True) - np.swapaxes(A, 1, 2).astype(np.float64) @ B.astype(np.float64)).max() < 1e-5
    assert np.abs(IO.mm_t(A, B, alpha=-1.0, tb=True) + A.astype(np.float64) @ np.swapaxes(B, 1, 2).astype(np.float64)).max() < 1e-5
    assert np.abs(IO.det3(A) - np.linalg.det(A.astype(np.float64))).max() < 1e-12


@pytest.mark.parametrize("name", GENERAL)
def test_general_scene(name):
    r, c = IC.answer(name), IC.case(name)
    m = c["matched"]
    assert r["status"] == IO.STATUS_OK and r["model"] == IO.MODEL_F and r["ok"] == 1
    assert r["n_matches"] == len(m) and r["n_inliers"] == len(m)   # every true match is an inlier
    assert r["n_hyp"] == 4 and r["nGood"][r["best"]] == len(m) and r["second"] == 1
    tn = np.linalg.norm(c["t"])
    eR = np.abs(r["R21"] - c["R"]).max()
    et = np.abs(r["t21"] - c["t"] / tn).max()
    eX = (np.abs(r["P3D"][m] * tn - c["X"][m]).max(axis=1) / np.abs(c["X"][m]).max(axis=1)).max()
    print(f"{name}: R {eR:.3g} t {et:.3g} X {eX:.3g}")
    assert eR <= 4 * SCENE_R and et <= 4 * SCENE_T and eX <= 4 * SCENE_X
    assert abs(np.linalg.norm(r["t21"].astype(np.float64)) - 1) < 1e-6
    assert r["triangulated"][m].all() and r["triangulated"].sum() == len(m)
    unmatched = np.setdiff1d(np.arange(len(c["keys1"])), m)
    assert not r["P3D"][unmatched].any()


@pytest.mark.parametrize("name", PLANAR)
def test_planar_scene(name):
    r, c = IC.answer(name), IC.case(name)
    m = c["matched"]
    with np.errstate(all="ignore"):
        RH = r["SH"] / (r["SH"] + r["SF"])
    assert RH > 0.40 and r["model"] == IO.MODEL_H and r["n_hyp"] == 8 and r["ok"] == 1
    good = r["nGood"]
    assert good[r["best"]] == len(m) and r["second"] < 0.75 * good[r["best"]]   # exactly one of the eight wins
    assert (good > 0.75 * good[r["best"]]).sum() == 1
    tn = np.linalg.norm(c["t"])
    assert np.abs(r["R21"] - c["R"]).max() <= 4 * SCENE_R and np.abs(r["t21"] - c["t"] / tn).max() <= 4 * SCENE_T
    assert (np.abs(r["P3D"][m] * tn - c["X"][m]).max(axis=1) / np.abs(c["X"][m]).max(axis=1)).max() <= 4 * SCENE_X


def test_case_tie():
    r = IC.answer("tie")
    t = r["tap"]
    assert (t["sets"] == t["sets"][0]).all()                       # a duplicate set ...
    assert t["scoreF"][0] == t["scoreF"][1] == t["scoreF"][2] > 0   # ... the same score ...
    assert t["scoreH"][0] == t["scoreH"][1] == t["scoreH"][2]
    assert r["iterF"] == 0 and r["iterH"] in (0, -1)               # ... and the first of them stays


def test_natural_ties_keep_the_first():
    r = IC.answer("general_120_it200")
    s = r["tap"]["scoreF"]
    assert (s == s.max()).sum() > 1 and r["iterF"] == int(np.argmax(s)) and r["SF"] == s.max()


def test_case_pure_rotation():
    r = IC.answer("pure_rotation")
    assert r["model"] == IO.MODEL_H and r["n_hyp"] == 0 and r["ok"] == 0 and r["best"] == -1 and r["n_inliers"] == r["n_matches"]
    K = IC.case("pure_rotation")["K"]
    w = IO.svd_f(IO.mm(IO.mm(IO.inv3(K), r["H21"]), K)[None])[0][0]
    assert w[0] / w[1] < 1.00001 or w[1] / w[2] < 1.00001


def test_case_two_sided():
    r = IC.answer("two_sided")
    assert r["model"] == IO.MODEL_F and r["second"] > 1 and r["ok"] == 0                 # nsimilar > 1
    assert sorted(r["nGood"][:4].tolist())[-2:] == [60, 60]


def test_case_too_few():
    r = IC.answer("too_few")
    good = r["nGood"][r["best"]]
    assert r["model"] == IO.MODEL_F and r["second"] == 1 and r["parallax_ok"] == 1 and r["ok"] == 0
    assert good == r["n_inliers"] == 30 and good < max(int(0.9 * r["n_inliers"]), 50)   # maxGood < nMinGood is what stops it


def test_case_low_parallax():
    r = IC.answer("low_parallax")
    good = r["nGood"][r["best"]]
    assert r["model"] == IO.MODEL_F and r["second"] == 1 and good >= max(int(0.9 * r["n_inliers"]), 50)   # the ladder gets there
    assert r["parallax_ok"] == 0 and r["ok"] == 0 and not r["P3D"].any()
    assert IO.PARALLAX_CUT < r["parallax_cos"] < np.float32(0.99998)


def test_case_ambiguous_plane():
    r = IC.answer("ambiguous_plane")
    best = r["nGood"][r["best"]]
    assert r["model"] == IO.MODEL_H and r["n_hyp"] == 8 and r["second"] >= 0.75 * best and r["ok"] == 0
    assert r["parallax_ok"] == 1 and best > 50 and best > 0.9 * r["n_inliers"]   # nothing else stands in the way
    r = IC.answer("ambiguous_tie")
    assert r["nGood"][0] == r["nGood"][1] == r["nGood"].max() and r["best"] == 0 and r["second"] == r["nGood"][0]


def test_case_far_point():
    c = IC.case("far_point")
    r = IC.answer("far_point")
    best = r["best"]
    r = IC.answer("far_point", 0, best)
    rt = r["tap"]["rt"]
    assert r["ok"] == 1 and rt[0, 4] == IO.RT_FAR and rt[0, 3] >= np.float32(0.99998)
    assert (rt[1:, 4] == IO.RT_GOOD).all()
    assert r["n_cos"][best] == 90 and r["nGood"][best] == 89   # in vCosParallax, not in nGood
    assert r["P3D"][0].any() and r["triangulated"][0] == 0 and r["triangulated"][1:].all()
    assert np.isfinite(r["P3D"]).all() and c["matches12"][0] == 0


def test_case_sizes_of_vcosparallax():
    r = IC.answer("one_behind")
    assert 1 in r["n_cos"][:4].tolist()
    h = r["n_cos"][:4].tolist().index(1)
    assert h != r["best"] and r["nGood"][h] == 1
    rt = IC.answer("one_behind", 0, h)["tap"]["rt"]
    assert rt[0, 4] == IO.RT_GOOD and r["sel_cos"][h] == rt[0, 3]            # size 1: idx = 0, its only entry
    for n in (50, 51, 52):
        r = IC.answer(f"sized_{n}")
        b = r["best"]
        assert r["n_cos"][b] == n and r["nGood"][b] == n
        rt = IC.answer(f"sized_{n}", 0, b)["tap"]["rt"]
        srt = np.sort(rt[:, 3])
        assert r["sel_cos"][b] == srt[min(50, n - 1)] and r["parallax_cos"] == r["sel_cos"][b]
        if n == 52:
            assert srt[50] != srt[51]   # so that an idx of size - 1 would have shown


def test_undefined_inputs_are_refused():
    c = IC.case("general_8")
    m = c["matches12"].copy()
    m[np.nonzero(m >= 0)[0][0]] = -1
    with pytest.raises(ValueError):
        IO.initialize(c["keys1"], c["keys2"], m, c["K"], 1.0, 4, c["draws"])
    # no iteration with a positive score: all matches far off any model
    rng = np.random.default_rng(3)
    k1 = rng.uniform(0, 640, (12, 2)).astype(np.float32)
    k2 = rng.uniform(0, 640, (12, 2)).astype(np.float32)
    r = IO.initialize(k1, k2, np.arange(12, dtype=np.int32), c["K"], 1e-3, 1, IC.draws_for(1, 0))
    assert r["status"] == IO.STATUS_NO_MODEL and r["ok"] == 0 and r["iterH"] == r["iterF"] == -1 and r["SH"] == r["SF"] == 0


def test_parallax_cut_on_every_float():
    """the cut equals acosf(c) * 180 / pi > 1 (and >= 1) on every float in [0.999, 1], with the host's acosf"""
    gt, ge = IO.derive_parallax_cut()
    assert gt.view(np.uint32) == ge.view(np.uint32) == IO.PARALLAX_CUT_BITS
    acosf = IO.host_acosf()
    c = IO.floats_between(0.999, 1.0)
    assert len(c) > 16000
    P = np.array([IO.parallax_of(x, acosf) for x in c], np.float32)
    cut = np.array([IO.parallax_cut(x) for x in c])
    assert np.array_equal(cut, P > np.float32(1)) and np.array_equal(cut, P >= np.float32(1))
    # outside: NaN and values past +-1 fail both tests as acosf's NaN does; anything from -1 up to 0.999 passes
    for x, want in ((np.nan, False), (1.0000001, False), (-1.0000001, False), (-1.0, True), (0.0, True), (0.998, True)):
        assert IO.parallax_cut(np.float32(x)) == want
        p = IO.parallax_of(np.float32(x), acosf)
        assert bool(p > np.float32(1)) == want and bool(p >= np.float32(1)) == want
