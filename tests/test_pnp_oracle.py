"""tests/pnp_oracle.py checked without a GPU: hand-worked answers for the parts that can be worked by hand (the draw replay,
SetRansacParameters, the `||` loop count), the restated one-sided Jacobi SVD against numpy's LAPACK SVD on the known-answer
matrices, the condition that `find` returns exactly the ground-truth inliers of noiseless scenes, the steered cases really
exercising the rule they are named for, and the host-only parts of the C-ABI against the oracle."""
import numpy as np
import pytest

import pnp_cases as PC
import pnp_oracle as PO

# The largest figures measured over pnp_cases.kat_matrices() against numpy's LAPACK SVD (printed by test_svd_against_lapack; DESIGN.md
# section 8h).  Each is asserted at four times itself: the margin for the unknown ratio of a one-sided Jacobi's and LAPACK's
# backward error constants.  The singular values are compared relative to the value itself wherever it exceeds ||A|| * n *
# DBL_EPSILON; the largest figure, 2.3e-13, is on a value of 2.5e-5 * ||A||, i.e. 5.7e-18 * ||A||: LAPACK's error is bounded
# relative to ||A||, so it, not the Jacobi, sets that figure.  Relative to ||A|| the values agree within the residual's bound.
SVD_MEASURED = dict(residual=1.32e-15, orthogonality=4.54e-15, values=2.27e-13)


# ---- hand-worked ---------------------------------------------------------------------------------------------------------------
def test_draw_to_index_replay():
    # index = (int)((r / 2^31) * size): r = 0 -> 0; r = 2^31 - 1 -> size - 1; r = 2^30 (one half) -> size // 2
    assert PO.index_from_draw(0, 10) == 0
    assert PO.index_from_draw(2 ** 31 - 1, 10) == 9
    assert PO.index_from_draw(2 ** 30, 10) == 5
    assert PO.index_from_draw(2 ** 30, 7) == 3
    # four draws of 0 on 0..9: take position 0 each time; the back element moves in: 0, then 9, then 8, then 7
    assert PO.quad_from_draws([0, 0, 0, 0], 10) == [0, 9, 8, 7]
    # always the last position: 9, 8, 7, 6
    top = 2 ** 31 - 1
    assert PO.quad_from_draws([top, top, top, top], 10) == [9, 8, 7, 6]
    # position 2 (r / 2^31 = 0.25 of 10 -> 2), then position 2 again of 9 (0.25 * 9 = 2.25 -> 2): it now holds 9; then 0; then the last of 7, which is 6
    q = 2 ** 29
    assert PO.quad_from_draws([q, q, 0, top], 10) == [2, 9, 0, 6]
    # draws_picking inverts it
    for quad in ([3, 1, 4, 5], [9, 8, 0, 2], [0, 9, 1, 8]):
        d = PC.draws_picking([quad], 10)
        assert PO.quad_from_draws(d, 10) == quad


def test_set_ransac_parameters_by_hand():
    # Relocalization's call: (0.99, 10, 300, 4, 0.5, 5.991)
    # N = 8: nMinInliers = max(4, 10) = 10 > N; epsilon = 10 / 8 = 1.25; log(1 - 1.25^3) is a NaN -> INT_MIN -> max(1, .) = 1
    assert PO.ransac_params(0.99, 10, 300, 4, 0.5, 8) == (10, np.float32(1.25), 1)
    # N = 20: 20 * 0.5 = 10; epsilon stays 0.5; ceil(log(0.01) / log(1 - 0.125)) = ceil(34.49) = 35
    assert PO.ransac_params(0.99, 10, 300, 4, 0.5, 20) == (10, np.float32(0.5), 35)
    # N = 100: 50 inliers; N = 1000: 500; the iteration count depends on epsilon only
    assert PO.ransac_params(0.99, 10, 300, 4, 0.5, 100) == (50, np.float32(0.5), 35)
    assert PO.ransac_params(0.99, 10, 300, 4, 0.5, 1000) == (500, np.float32(0.5), 35)
    # the clamp from above, the truncation of N * epsilon (0.4f * 24 = 9.6 -> 9 < 10), min_inliers == N -> one iteration
    assert PO.ransac_params(0.99, 10, 20, 4, 0.5, 20)[2] == 20
    assert PO.ransac_params(0.99, 10, 300, 4, 0.4, 24)[0] == 10
    assert PO.ransac_params(0.99, 10, 300, 4, 0.5, 10) == (10, np.float32(1.0), 1)
    # pow(epsilon, 3) although the set is 4: epsilon 0.3 -> ceil(log(0.01) / log(1 - 0.027)) = ceil(168.2...) = 169
    assert PO.ransac_params(0.99, 4, 300, 4, 0.3, 1000)[2] == 169


def test_loop_runs_while_either_condition_holds():
    # iterate(5) on a fresh solver whose clamp is 9 and which never returns: 9 iterations, then bNoMore; again: 5 more
    _, prm, runs = PC.rules_replay("past5")
    assert prm[2] == 9
    assert runs[0]["n_iterations"] == 5 and runs[0]["out"]["iterations_run"] == 9 and runs[0]["out"]["no_more"]
    _, _, runs = PC.rules_replay("again")
    assert [r["out"]["iterations_run"] for r in runs] == [9, 3, 2] and all(r["out"]["no_more"] for r in runs)
    assert [r["iterations"] for r in runs] == [9, 12, 14]


# ---- the restated SVD against LAPACK ---------------------------------------------------------------------------------------------
def test_svd_against_lapack():
    worst = dict(residual=0.0, orthogonality=0.0, values=0.0, values_to_norm=0.0)
    for (m, n), A in PC.kat_matrices().items():
        w, Ut, Vt = PO.svd(A)
        for k in range(len(A)):
            na = np.linalg.norm(A[k])
            ref = np.linalg.svd(A[k], compute_uv=False)
            assert np.all(np.diff(w[k]) <= 0), "descending"
            if na == 0:
                assert np.all(w[k] == 0)
                continue
            worst["residual"] = max(worst["residual"], np.linalg.norm(Ut[k].T @ np.diag(w[k]) @ Vt[k] - A[k]) / na)
            worst["orthogonality"] = max(worst["orthogonality"], np.linalg.norm(Vt[k] @ Vt[k].T - np.eye(n)))
            # the left vectors of singular values above the refill's floor are orthonormal
            live = w[k] > na * n * PO.DBL_EPSILON
            U = Ut[k][live]
            worst["orthogonality"] = max(worst["orthogonality"], np.linalg.norm(U @ U.T - np.eye(len(U))))
            big = ref > na * n * PO.DBL_EPSILON
            worst["values"] = max(worst["values"], float(np.max(np.abs(w[k][big] - ref[big]) / ref[big], initial=0.0)))
            worst["values_to_norm"] = max(worst["values_to_norm"], float(np.max(np.abs(w[k] - ref)) / na))
    print("SVD against LAPACK, largest over the table:", worst)
    for name, measured in SVD_MEASURED.items():
        assert worst[name] <= 4 * measured, (name, worst)
    assert worst["values_to_norm"] <= 4 * SVD_MEASURED["residual"], worst


def test_solve_and_invert_against_lapack():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((10, 6, 4))
    b = rng.standard_normal((10, 6))
    x = PO.sv_solve(A, b)
    for k in range(10):
        assert np.allclose(x[k], np.linalg.lstsq(A[k], b[k], rcond=None)[0], rtol=1e-10, atol=1e-12)
    B = rng.standard_normal((10, 3, 3))
    assert np.allclose(PO.sv_invert(B), np.linalg.inv(B), rtol=1e-9, atol=1e-12)
    # a singular value under SVBkSb's threshold is left out: the pseudo-inverse
    B[0, :, 2] = B[0, :, 1]
    assert np.allclose(PO.sv_invert(B[:1])[0], np.linalg.pinv(B[0]), rtol=1e-8, atol=1e-10)
    # qr_solve: least squares; a zero column leaves x untouched (P6)
    xq = PO.qr_solve(A, b, np.zeros((10, 4)))
    for k in range(10):
        assert np.allclose(xq[k], np.linalg.lstsq(A[k], b[k], rcond=None)[0], rtol=1e-10, atol=1e-12)
    A[0, :, 2] = 0
    keep = np.full((10, 4), 7.0)
    assert np.array_equal(PO.qr_solve(A, b, keep)[0], keep[0])


def test_compute_pose_recovers_the_pose():
    sc = PC.scene(9, 50, inlier_ratio=1.0)
    R, t, err, _ = PO.compute_pose(sc["P3Dw"][None].astype(np.float64), sc["P2D"][None].astype(np.float64), PC.K)
    assert err[0] < 1e-3 and np.allclose(R[0], sc["R"], atol=1e-5) and np.allclose(t[0], sc["t"], atol=1e-5)


# ---- a condition, not a tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", PC.FIND_SEEDS)
def test_find_returns_the_ground_truth(seed):
    sc, s, _, out = PC.find_replay(seed)
    assert out["Tcw"] is not None
    assert np.array_equal(out["mask"], sc["truth"]) and out["n_inliers"] == int(sc["truth"].sum())


# ---- the steered cases show their rule -------------------------------------------------------------------------------------------
def test_rule_cases_show_their_rule():
    _, prm, runs = PC.rules_replay("tie")
    taps = runs[0]["taps"]
    assert taps[0]["n_inliers"] == taps[2]["n_inliers"] == prm[0] and not np.array_equal(taps[0]["R"], taps[2]["R"])
    assert np.array_equal(runs[0]["best_Tcw"], PO.tcw_from(taps[0]["R"], taps[0]["t"]))   # strict >: the earlier stays
    # Refine lands exactly on min_inliers and fails; at the clamp the best goes out (rule 4, rule 5)
    assert taps[0]["refined"] and taps[0]["refine_inliers"] == prm[0]
    out = runs[0]["out"]
    assert out["no_more"] and out["n_inliers"] == prm[0] and np.array_equal(out["Tcw"], runs[0]["best_Tcw"])
    _, prm, runs, info = PC.older_replay()
    taps = runs[0]["taps"]
    assert prm[0] <= taps[2]["n_inliers"] < taps[0]["n_inliers"] and not np.array_equal(info["mask0"], info["mask2"])
    assert taps[2]["refined"] and taps[2]["refine_inliers"] == info["refine_best"] != info["refine_current"]
    assert np.array_equal(runs[0]["best_mask"], info["mask0"])


# ---- the host-only C-ABI (needs no device) -----------------------------------------------------------------------------------------
def test_cabi_ransac_params_equals_oracle():
    from orb_slam2_ssd_semantic_amd import _ffi, pnp
    L = _ffi.lib()
    for name in ("orbfe_pnp_create", "orbfe_pnp_destroy", "orbfe_pnp_get_stream", "orbfe_pnp_ransac_params", "orbfe_pnp_iterations",
                 "orbfe_pnp_iterate", "orbfe_pnp_iterate_device", "orbfe_pnp_set_tap_iteration", "orbfe_pnp_tap", "orbfe_pnp_kat"):
        assert getattr(L, name) is not None
    for n in (0, 3, 8, 9, 10, 11, 20, 24, 100, 1000, 5000):
        for args in ((0.99, 10, 300, 4, 0.5), (0.99, 8, 300, 4, 0.4), (0.99, 30, 64, 4, 0.1), (0.5, 4, 300, 4, 0.3), (1.0, 6, 300, 4, 0.2)):
            p = pnp.ransac_params(*args, n=n)
            r = PO.ransac_params(*args, n=n)
            got = (int(p["min_inliers"][0]), p["epsilon"][0].tobytes(), int(p["max_its"][0]))
            assert got == (r[0], r[1].tobytes(), r[2]), (n, args, p, r)
            assert p["th2"][0] == np.float32(5.991)
    st = np.zeros(1, pnp.STATE_DTYPE)
    prm = pnp.ransac_params(0.99, 10, 300, 4, 0.5, n=100)
    assert pnp.iterations(st, prm, 5) == 35   # the `||`
    st["iterations"] = 33
    assert pnp.iterations(st, prm, 5) == 5
    st["iterations"] = 40
    assert pnp.iterations(st, prm, 5) == 5
