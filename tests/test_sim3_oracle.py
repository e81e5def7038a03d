"""tests/sim3_oracle.py, the restatement of the reference's Sim3Solver: known answers, the quirks it keeps (size_t thresholds,
the NaN rotation of a pure translation, the later tie, the `>= best` return of a re-iterated solver), and its canonical
mode (fixed fp64 atan2 / sin / cos) against its libm mode on every case of tests/sim3_cases.py."""
import math

import numpy as np
import pytest

import sim3_cases as SC
import sim3_oracle as SO

F = np.float32
# the largest float-ulp difference of a T12 entry between the canonical and the libm oracle over every iteration of every case,
# as measured when the cases were written: the float store of R absorbs the last-bit differences
T12_ULP_MEASURED = 0


def ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def test_exact_recovery():
    c = SC.full_table()["exact"]
    (r,), s = SC.reference("exact")
    s_true, R_true, t_true = c["truth"]
    assert r["found"] and r["n_inliers"] == len(c["X1"]) and r["mask"].all()
    # R comes out of float trig (a few float ulps), nom / den are double sums of 9 float products: 16 float ulps of s
    assert abs(float(s.best["s"]) - s_true) <= 16 * float(np.finfo(F).eps) * s_true
    assert np.allclose(s.best["R"], R_true, atol=1e-6) and np.allclose(s.best["t"], t_true, atol=1e-4)
    assert np.allclose(r["T12"][:3, :3], s_true * R_true, atol=1e-5) and np.array_equal(r["T12"][3], [0, 0, 0, 1])


def test_size_t_threshold():
    thr = SO.max_errors(np.array([1.2, 1.44], F))
    assert thr.dtype == F and thr.tolist() == [11.0, 13.0]   # 9.210 * 1.2 = 11.05, 9.210 * 1.44 = 13.26, truncated
    err = F(11.5)
    assert not err < thr[0] and err < thr[1]
    assert SO.max_errors([1.0])[0] == 9.0


def test_pure_translation_gives_nan_rotation_and_the_loop_goes_on():
    outs, s = SC.reference("nan_translation")
    for r in outs:
        assert not r["found"] and not r["no_more"] and r["iterations_run"] == 5
        for it in r["log"]:
            assert np.isnan(it["R"]).all() and it["count"] == 0
            assert np.isnan(it["err1"]).all() and np.isnan(it["err2"]).all()
    assert s.iterations == 10 and s.best_inliers == 0
    # 0 >= 0: every iteration replaces the best, so the best is the last (NaN) model
    assert np.isnan(s.best["R"]).all() and np.array_equal(s.best["T12"].view(np.uint32), outs[-1]["log"][-1]["T12"].view(np.uint32))
    N = SO.n_matrix(s.X1[[0, 1, 2]].T, s.X2[[0, 1, 2]].T)[0]
    assert (N[0, 1:] == 0).all()
    _, V = SO.jacobi_f32(N)
    assert V[0].tolist() == [1.0, 0.0, 0.0, 0.0]


def test_later_tie_wins():
    X1, X2, s1, s2, inl = SC.scene(100, 30, 4242)
    draws = SC.steered_draws(inl, 4, (1, 3), np.random.default_rng(1))
    s = SO.Solver(X1, X2, s1, s2, SC.K_A, SC.K_B, True)
    s.min_inliers, s.max_its = 100, 300   # N == min_inliers: no count is > 100, so no return
    r = s.iterate(4, draws)
    log = r["log"]
    assert not r["found"] and log[1]["count"] == log[3]["count"] == s.best_inliers > log[0]["count"]
    assert not np.array_equal(log[1]["T12"], log[3]["T12"])
    assert np.array_equal(s.best["T12"], log[3]["T12"])


def test_second_call_returns_only_at_the_best():
    c = SC.full_table()["second_call"]
    (a, b), s = SC.reference("second_call")
    assert a["found"] and a["iterations_run"] == 2
    best = a["n_inliers"]
    assert b["found"] and b["iterations_run"] == 7 and b["n_inliers"] >= best
    passed = b["log"][2]["count"]
    assert c["min_inliers"] < passed < best   # enough for a first return, not for one after a better model
    assert all(it["count"] < best for it in b["log"][:-1])
    assert s.iterations == 9


def test_small_sets():
    tab = SC.full_table()
    (r,), s = SC.reference("n_19")
    assert not r["found"] and r["no_more"] and r["iterations_run"] == 0 and s.best is None and not r["mask"].any()
    assert tab["n_20"]["max_its"] == 1
    (r,), s = SC.reference("n_20")
    assert not r["found"] and r["no_more"] and r["iterations_run"] == 1 and s.iterations == 1
    assert SO.ransac_iterations(0.99, 20, 300, 19) == 1
    # N == 3: the index list shrinks to empty, the triple is a permutation of all three
    X1, X2, s1, s2, _ = SC.scene(3, 0, 9)
    s = SO.Solver(X1, X2, s1, s2, SC.K_A, SC.K_B, True)
    s.set_ransac_parameters(0.99, 3, 300)
    assert s.max_its == 1
    r = s.iterate(5, [2 ** 31 - 1, 0, 12345])
    assert r["log"][0]["triple"] == [2, 0, 1] and r["iterations_run"] == 1 and r["no_more"] and not r["found"]
    assert r["log"][0]["count"] == 3   # 3 > 3 is false: no return
    assert SO.triple_from_draws([0, 0, 0], 5) == [0, 4, 3] and SO.triple_from_draws([2 ** 31 - 1] * 3, 5) == [4, 3, 2]


def test_no_more_exactly_at_the_clamp():
    c = dict(SC.full_table()["all_outliers"])
    d = c["calls"][0][1]
    c["max_its"] = 7
    c["calls"] = [(5, d[:15]), (5, d[15:30]), (5, d[30:45])]
    (a, b, e), s = SC.run(c, "canonical")
    assert (a["iterations_run"], a["no_more"]) == (5, False)
    assert (b["iterations_run"], b["no_more"]) == (2, True) and s.iterations == 7
    assert (e["iterations_run"], e["no_more"]) == (0, True)
    assert SO.ransac_iterations(0.99, 20, 300, 64) == 149 and SO.ransac_iterations(0.99, 20, 300, 100) == 300
    assert SO.ransac_iterations(0.99, 6, 300, 6) == 1 and SO.ransac_iterations(0.99, 20, 5, 100) == 5


@pytest.mark.parametrize("name", sorted(SC.full_table()))
def test_canonical_equals_libm_where_it_decides(name):
    c = SC.full_table()[name]
    oc, sc = SC.reference(name, "canonical")
    ol, sl = SC.reference(name, "libm")
    m = SC.margin(c, ol)
    print(f"{name}: margin {m:.3g}")
    assert m > SC.MARGIN
    worst = 0
    for a, b in zip(oc, ol):
        assert (a["found"], a["no_more"], a["n_inliers"], a["iterations_run"]) == (b["found"], b["no_more"], b["n_inliers"], b["iterations_run"])
        assert np.array_equal(a["mask"], b["mask"])
        assert np.array_equal(a["state"]["best_mask"], b["state"]["best_mask"])
        for x, y in zip(a["log"], b["log"]):
            assert x["triple"] == y["triple"] and x["count"] == y["count"]
            assert np.array_equal(np.isnan(x["T12"]), np.isnan(y["T12"]))
            ok = ~np.isnan(x["T12"])
            if ok.any():
                worst = max(worst, int(np.abs(ordered(x["T12"]) - ordered(y["T12"]))[ok].max()))
    print(f"{name}: largest T12 difference {worst} float ulp")
    assert worst <= 4 * T12_ULP_MEASURED
    assert sc.iterations == sl.iterations and sc.best_inliers == sl.best_inliers


def test_canonical_trig_against_libm():
    """the share of 50 000 random arguments where a canonical function and the host's libm differ, and by how much: fdlibm's
    functions are within 1 ulp of the true value, so a difference is one last bit (recorded in DESIGN.md section 8e)"""
    rng = np.random.default_rng(0)
    th = rng.uniform(0, 2 * math.pi, 50000)
    ys, xs = rng.uniform(0, 1, 50000), rng.uniform(-1, 1, 50000)

    def ulps(a, b):
        return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))
    for nm, pairs in (("sin", [(SO.c_sin(v), math.sin(v)) for v in th]), ("cos", [(SO.c_cos(v), math.cos(v)) for v in th]),
                      ("atan2", [(SO.c_atan2(y, x), math.atan2(y, x)) for y, x in zip(ys, xs)])):
        d = [ulps(a, b) for a, b in pairs]
        print(f"{nm}: {np.count_nonzero(d) / len(d):.4%} of {len(d)} differ, at most {max(d)} ulp")
        assert max(d) <= 1
    # exact points
    assert SO.c_sin(0.0) == 0.0 and SO.c_cos(0.0) == 1.0 and SO.c_atan2(0.0, 1.0) == 0.0 and SO.c_atan2(0.0, -1.0) == math.pi
    assert SO.c_atan2(1.0, 0.0) == math.pi / 2 and SO.c_atan2(1.0, 1.0) == math.pi / 4
    assert math.isnan(SO.c_atan2(math.nan, 1.0)) and math.isnan(SO.c_sin(math.inf)) and math.isnan(SO.c_cos(1e7))


def test_ransac_iterations_helper():
    """orbfe_sim3_ransac_iterations is host code: the clamp and the double -> int conversion against the oracle's"""
    from orb_slam2_ssd_semantic_amd import sim3 as S3
    for p_, mi, mx, n in ((0.99, 20, 300, 64), (0.99, 20, 300, 100), (0.99, 6, 300, 6), (0.99, 20, 5, 100), (0.99, 20, 300, 19), (0.99, 20, 300, 21),
                          (0.99, 20, 300, 257), (0.5, 3, 300, 1000000), (0.99, 6, 300, 0)):
        assert S3.ransac_iterations(p_, mi, mx, n) == SO.ransac_iterations(p_, mi, mx, n), (p_, mi, mx, n)
