"""PnPsolver's EPnP RANSAC on the GPU (csrc/orbfe_pnp.hip) against tests/pnp_oracle.py, bit for bit: the device primitives (the
one-sided Jacobi SVD at every size EPnP uses, SVBkSb solve and invert, qr_solve, one whole compute_pose), the host call over the
case table with the taps of every iteration run, the rules of the acceptance scan one steered case each, the memoised Refine,
the batched device form against host calls with the scatter into the frame mask, the argument errors and the Python class.
NaNs compare by position (the payload and sign of a generated NaN belong to the processor); every other value compares as
bits."""
import ctypes as C

import numpy as np
import pytest

import pnp_cases as PC
import pnp_oracle as PO
from orb_slam2_ssd_semantic_amd import PnP, PnPSolver, _ffi
from orb_slam2_ssd_semantic_amd import pnp as PN
from pnp_checks import run_against_replay, same_bits

MAX_POINTS = 2048


@pytest.fixture(scope="module")
def pn():
    h = PnP(MAX_POINTS, 32)
    h.set_tap_iteration(0)
    yield h
    h.close()


# ---- KATs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what,shape", [(PN.KAT_SVD3, (3, 3)), (PN.KAT_SVD6X3, (6, 3)), (PN.KAT_SVD6X4, (6, 4)), (PN.KAT_SVD6X5, (6, 5)),
                                        (PN.KAT_SVD12, (12, 12))])
def test_kat_svd(what, shape):
    A = PC.kat_matrices()[shape].copy()
    if shape[0] == shape[1]:
        A[23, 0, 0] = np.nan   # a NaN never compares: every sweep runs, the result is NaNs by position
    w, Ut, Vt = PN.kat(what, A)
    ow, oUt, oVt = PO.svd(A)
    for k in range(len(A)):
        assert same_bits(w[k], ow[k]) and same_bits(Ut[k], oUt[k]) and same_bits(Vt[k], oVt[k]), k


@pytest.mark.gpu
def test_kat_solve_invert_qr():
    rng = np.random.default_rng(11)
    for what, k in ((PN.KAT_SOLVE6X3, 3), (PN.KAT_SOLVE6X4, 4), (PN.KAT_SOLVE6X5, 5)):
        A = rng.standard_normal((16, 6, k))
        b = rng.standard_normal((16, 6))
        A[1, :, 1] = A[1, :, 0]   # a singular value under SVBkSb's threshold: skipped
        A[2, :, k - 1] = 0        # an exact zero: the refilled row, skipped too
        A[3] = 0
        assert np.any(np.abs(PO.svd(A[1:2])[0][0]) <= PO._threshold(PO.svd(A[1:2])[0])[0])
        assert same_bits(PN.kat(what, A, b), PO.sv_solve(A, b)), k
    B = rng.standard_normal((16, 3, 3))
    B[1, :, 2] = B[1, :, 1]
    B[2] = 0
    B[3] *= 1e-200
    assert same_bits(PN.kat(PN.KAT_INVERT3, B), PO.sv_invert(B))
    A = rng.standard_normal((16, 6, 4))
    b = rng.standard_normal((16, 6))
    A[1, :, 2] = 0     # a zero column: x stays at the zeros it started with
    A[2, :5, 0] = 0    # the pivot scan never reads the last row (P7): found singular although A[5][0] is not zero
    A[3, 0, 0] = np.nan
    x = PN.kat(PN.KAT_QR_SOLVE, A, b)
    assert same_bits(x, PO.qr_solve(A, b, np.zeros((16, 4))))
    assert np.all(x[1] == 0) and np.all(x[2] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_kat_compute_pose(n):
    for seed, kw in ((1, {}), (2, dict(coplanar=True)), (3, dict(duplicates=2))):
        sc = PC.scene(seed, n, inlier_ratio=1.0, **kw)
        P3, P2 = sc["P3Dw"].astype(np.float64), sc["P2D"].astype(np.float64)
        K = tuple(float(np.float32(v)) for v in PC.K)
        R, t, err, N, errs = PN.kat(PN.KAT_COMPUTE_POSE, (K, P3, P2))
        oR, ot, oerr, oN, oerrs = PO.compute_pose(P3[None], P2[None], K, detail=True)
        assert same_bits(R, oR[0]) and same_bits(t, ot[0]) and same_bits(np.array([err]), oerr[:1]) and N == oN[0], (n, seed)
        assert same_bits(errs, oerrs[0])


# ---- iterate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PC.ITERATE_CASES))
def test_iterate_case(pn, name):
    sc, prm, runs = PC.replay(name)
    run_against_replay(pn, sc, prm, runs)


@pytest.mark.gpu
def test_below_min_inliers_runs_nothing(pn):
    for name in ("n3", "n9"):
        sc, prm, runs = PC.replay(name)
        (res, _), _ = run_against_replay(pn, sc, prm, runs)
        assert res["no_more"] and not res["found"] and res["iterations_run"] == 0 and res["refine_runs"] == 0


@pytest.mark.gpu
def test_rule_loop_runs_past_n_iterations(pn):
    sc, prm, runs = PC.rules_replay("past5")
    (res, taps), = run_against_replay(pn, sc, prm, runs)
    assert runs[0]["n_iterations"] == 5 and res["iterations_run"] == 9 == len(taps) and res["no_more"]


@pytest.mark.gpu
def test_rule_tie_keeps_the_earlier_best_and_refine_on_min_fails(pn):
    sc, prm, runs = PC.rules_replay("tie")
    (res, taps), = run_against_replay(pn, sc, prm, runs)
    assert taps[0]["n_inliers"] == taps[2]["n_inliers"] == prm[0] and not same_bits(taps[0]["R"], taps[2]["R"])
    # Refine landed exactly on min_inliers: no return; at the clamp the best model of iteration 0 goes out, unrefined
    assert taps[0]["refine_ran"] and taps[0]["refine_inliers"] == prm[0]
    assert res["found"] and res["no_more"] and not res["refined"] and res["n_inliers"] == prm[0]
    assert same_bits(res["Tcw"], PO.tcw_from(taps[0]["R"], taps[0]["t"]))


@pytest.mark.gpu
def test_rule_refine_runs_on_the_older_best_mask(pn):
    sc, prm, runs, info = PC.older_replay()
    (res, taps), = run_against_replay(pn, sc, prm, runs)
    assert taps[2]["n_inliers"] == info["count2"] >= prm[0] and taps[2]["refine_inliers"] == info["refine_best"] != info["refine_current"]
    assert same_bits(res["Tcw"], PO.tcw_from(taps[0]["R"], taps[0]["t"]))


@pytest.mark.gpu
def test_rule_called_again_after_no_more_and_after_a_return(pn):
    sc, prm, runs = PC.rules_replay("again")
    out = run_against_replay(pn, sc, prm, runs)
    assert [int(r["iterations_run"]) for r, _ in out] == [9, 3, 2] and all(r["no_more"] for r, _ in out)
    sc, prm, runs = PC.replay("n64")   # every call returns through Refine and the next one goes on
    out = run_against_replay(pn, sc, prm, runs)
    assert all(r["found"] and r["refined"] for r, _ in out) and len(out) == 3


@pytest.mark.gpu
def test_refine_is_memoised_per_best(pn):
    """the oracle refines at every iteration at or above min_inliers; the kernel once per best mask and call, with the same
    results (run_against_replay compares refine_inliers at every iteration)"""
    for replay in (PC.rules_replay("tie"), PC.rules_replay("again"), PC.older_replay()[:3], PC.replay("n10"), PC.replay("n11_one_outlier")):
        sc, prm, runs = replay
        out = run_against_replay(pn, sc, prm, runs)
        best = 0
        for (res, taps), r in zip(out, runs):
            memo, want = False, []
            for t in r["taps"]:
                ran = 0
                if t["n_inliers"] >= prm[0]:
                    if t["n_inliers"] > best:
                        best, memo = t["n_inliers"], False
                    if not memo:
                        ran, memo = 1, True
                want.append(ran)
            assert list(taps["refine_ran"]) == want and int(res["refine_runs"]) == sum(want) <= sum(t["refined"] for t in r["taps"])
    sc, prm, runs = PC.rules_replay("tie")
    (res, taps), = run_against_replay(pn, sc, prm, runs)
    assert sum(t["refined"] for t in runs[0]["taps"]) == 2 and int(res["refine_runs"]) == 1 and list(taps["refine_ran"][:3]) == [1, 0, 0]


# ---- the batched device form -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nsets", [1, 3, 17])
def test_iterate_device_against_host_calls(pn, nsets):
    import torch
    names = ["n64", "n0", "n11", "n65", "coplanar", "clamp_63", "n10", "duplicates", "behind", "n9", "one_octave", "n63", "ratio_1.0",
             "n11_one_outlier", "clamp_65", "n3", "n255"][:nsets]
    if nsets == 1:
        names = ["n65"]
    P3, P2, SG, KI, off, sets, draws, n_keys_total = [], [], [], [], [0], np.zeros(nsets, PN.SET_DTYPE), [], 0
    expect = []
    rng = np.random.default_rng(5)
    for si, name in enumerate(names):
        if name == "n0":   # an empty set
            sc = dict(P3Dw=np.zeros((0, 3), np.float32), P2D=np.zeros((0, 2), np.float32), sigma2=np.zeros(0, np.float32))
            prm, run = (10, np.float32(0.5), 1), None
        else:
            sc, prm, runs = PC.replay(name)
            run = runs[0]
        n = len(sc["P3Dw"])
        n_keys = n + 7
        kp = np.sort(rng.choice(n_keys, n, replace=False)).astype(np.int32)
        sets[si]["K"] = PC.K
        sets[si]["params"]["min_inliers"], sets[si]["params"]["epsilon"], sets[si]["params"]["max_its"] = prm[0], prm[1], prm[2]
        sets[si]["params"]["th2"] = np.float32(5.991)
        sets[si]["n_iterations"] = run["n_iterations"] if run else 5
        sets[si]["draws_offset"] = sum(len(d) for d in draws)
        sets[si]["key_offset"], sets[si]["n_keys"] = n_keys_total, n_keys
        n_keys_total += n_keys
        draws.append(run["draws"] if run else np.zeros(0, np.int32))
        P3.append(sc["P3Dw"]), P2.append(sc["P2D"]), SG.append(sc["sigma2"]), KI.append(kp)
        off.append(off[-1] + n)
        expect.append((run, kp, n_keys))
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev).view(dt)   # noqa: E731
    d_draws = np.concatenate(draws + [np.zeros(1, np.int32)])
    d_state = torch.zeros(nsets * PN.STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(max(off[-1], 1), dtype=torch.uint8, device=dev)
    d_key = torch.full((n_keys_total,), 9, dtype=torch.uint8, device=dev)
    res, mask = pn.iterate_device(t(np.array(off, np.int32), torch.int32), t(np.concatenate(P3), torch.float32).view(-1, 3),
                                  t(np.concatenate(P2), torch.float32).view(-1, 2), t(np.concatenate(SG), torch.float32),
                                  t(sets, torch.uint8), t(d_draws, torch.int32), d_state, d_best,
                                  keypoint_index=t(np.concatenate(KI), torch.int32), key_mask=d_key)
    torch.cuda.synchronize()
    res = res.cpu().numpy().reshape(-1).view(PN.RESULT_DTYPE)
    state = d_state.cpu().numpy().view(PN.STATE_DTYPE)
    mask, best, key = mask.cpu().numpy(), d_best.cpu().numpy(), d_key.cpu().numpy()
    for si, (run, kp, n_keys) in enumerate(expect):
        lo, hi = off[si], off[si + 1]
        km = key[sets[si]["key_offset"]:sets[si]["key_offset"] + n_keys]
        if run is None:
            assert res[si]["no_more"] and not res[si]["found"] and res[si]["iterations_run"] == 0 and not km.any()
            continue
        o = run["out"]
        assert int(res[si]["iterations_run"]) == o["iterations_run"] and bool(res[si]["found"]) == (o["Tcw"] is not None), si
        assert bool(res[si]["no_more"]) == o["no_more"] and int(res[si]["n_inliers"]) == o["n_inliers"], si
        assert same_bits(res[si]["Tcw"], o["Tcw"] if o["Tcw"] is not None else np.zeros((4, 4), np.float32)), si
        assert np.array_equal(mask[lo:hi].astype(bool), o["mask"]) and np.array_equal(best[lo:hi].astype(bool), run["best_mask"]), si
        assert int(state[si]["iterations"]) == run["iterations"] and same_bits(state[si]["best_Tcw"], run["best_Tcw"]), si
        want = np.zeros(n_keys, np.uint8)
        want[kp[o["mask"]]] = 1
        assert np.array_equal(km, want), si


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys", [1, 257, 700])
def test_prepare_device_against_the_constructor(pn, n_keys):
    import torch
    rng = np.random.default_rng(n_keys)
    keys = np.zeros(n_keys, _ffi.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 640, n_keys).astype(np.float32), rng.uniform(0, 480, n_keys).astype(np.float32)
    keys["octave"] = rng.integers(0, 8, n_keys)
    n_mp = 300
    pos = rng.standard_normal((n_mp, 3)).astype(np.float32)
    idx = rng.integers(0, n_mp, n_keys).astype(np.int32)
    idx[rng.random(n_keys) < 0.3] = -1
    for edge in (0, 62, 63, 64, 65, 255, 256, n_keys - 1):   # none or bad at the first, the last and the wave / chunk boundaries
        if edge < n_keys:
            idx[edge] = -1
    for edge in (1, 127, 128, 511, 512, n_keys - 2):         # ... and present right next to them
        if 0 <= edge < n_keys:
            idx[edge] = edge % n_mp
    if n_keys == 257:
        idx[:] = np.where(np.arange(n_keys) % 2 == 0, idx, np.abs(idx))   # most present
        idx[256] = 5                                                       # the last one present, alone in its chunk
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev).view(dt)   # noqa: E731
    P2D, sg, P3, kp, cnt = PN.pnp_prepare_device(pn, t(keys, torch.uint8), t(PC.SCALE2, torch.float32), t(idx, torch.int32),
                                                 t(pos, torch.float32).view(-1, 3))
    torch.cuda.synchronize()
    oP2D, osg, oP3, okp = PO.construct(np.stack([keys["x"], keys["y"]], 1), keys["octave"], PC.SCALE2, idx, pos)
    c = int(cnt.cpu()[0])
    assert c == len(okp)
    assert same_bits(P2D.cpu().numpy()[:c], oP2D) and same_bits(sg.cpu().numpy()[:c], osg) and same_bits(P3.cpu().numpy()[:c], oP3)
    assert np.array_equal(kp.cpu().numpy()[:c], okp)
    assert not P2D.cpu().numpy()[c:].any() and not kp.cpu().numpy()[c:].any()   # nothing past the count


# ---- the Python class, argument errors ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", PC.FIND_SEEDS[:2])
def test_solver_class_find(pn, seed):
    sc, s, d, out = PC.find_replay(seed)
    n = len(sc["truth"])
    kp = (np.arange(n) * 2 + 1).astype(np.int64)
    solver = PnPSolver(sc["P3Dw"], sc["P2D"], sc["sigma2"], PC.K, keypoint_index=kp, n_keys=2 * n + 3, handle=pn)
    solver.set_ransac_parameters(**{("max_iterations" if k == "max_its" else k): v for k, v in PC.FIND_PARAMS.items()})
    Tcw, inl, cnt = solver.find(d)
    assert same_bits(Tcw, out["Tcw"]) and cnt == out["n_inliers"] == int(sc["truth"].sum())
    want = np.zeros(2 * n + 3, bool)
    want[kp[sc["truth"]]] = True
    assert np.array_equal(inl, want)


@pytest.mark.gpu
def test_argument_errors(pn):
    L = _ffi.lib()
    sc = PC.scene(1, 20, inlier_ratio=1.0)
    params = PN.ransac_params(0.99, 10, 300, 4, 0.5, n=20)
    state = np.zeros(1, PN.STATE_DTYPE)
    bm = np.zeros(20, np.uint8)
    res = np.zeros(1, PN.RESULT_DTYPE)
    d = PC.draws_for(1, 40)
    k = np.array(PC.K, np.float32)
    args = [pn.h, _ffi.ptr(sc["P3Dw"]), _ffi.ptr(sc["P2D"]), _ffi.ptr(sc["sigma2"]), 20, _ffi.ptr(k), _ffi.ptr(params), 5, _ffi.ptr(d),
            _ffi.ptr(state), _ffi.ptr(bm), _ffi.ptr(res), None]
    for i in (0, 1, 2, 3, 5, 6, 8, 9, 10, 11):
        bad = list(args)
        bad[i] = None
        assert L.orbfe_pnp_iterate(*bad) == _ffi.ORBFE_ERR_ARG, i
    bad = list(args)
    bad[4] = MAX_POINTS + 1
    assert L.orbfe_pnp_iterate(*bad) == _ffi.ORBFE_ERR_ARG
    bad[4] = -1
    assert L.orbfe_pnp_iterate(*bad) == _ffi.ORBFE_ERR_ARG
    bad = list(args)
    bad[7] = (1 << 20) + 1
    assert L.orbfe_pnp_iterate(*bad) == _ffi.ORBFE_ERR_ARG
    state["iterations"] = -1
    assert L.orbfe_pnp_iterate(*args) == _ffi.ORBFE_ERR_ARG
    state["iterations"] = 0
    assert L.orbfe_pnp_iterate(*args) == _ffi.ORBFE_OK
    assert L.orbfe_pnp_kat(99, 1, _ffi.ptr(np.zeros(9)), _ffi.ptr(np.zeros(21))) == _ffi.ORBFE_ERR_ARG
    h2 = PnP(16, 1)   # a handle that never asked for taps has none
    cnt = np.zeros(1, np.int32)
    assert L.orbfe_pnp_tap(h2.h, 0, 0, _ffi.ptr(np.zeros(128, np.uint8)), 128, _ffi.ptr(cnt)) == _ffi.ORBFE_ERR_STATE
    h2.close()
    # the batched form: (h, offsets, P3Dw, P2D, sigma2, sets, draws, nsets, state, best_mask, result, mask, keypoint_index, key_mask, stream)
    one = C.c_void_p(8)
    assert L.orbfe_pnp_iterate_device(pn.h, one, one, one, one, one, one, 33, one, one, one, one, None, None, None) == _ffi.ORBFE_ERR_ARG
    assert "max_sets" in _ffi.last_error()
    assert L.orbfe_pnp_iterate_device(pn.h, one, one, one, one, one, one, 1, one, one, one, one, one, None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_pnp_iterate_device(pn.h, one, one, None, one, one, one, 1, one, one, one, one, None, None, None) == _ffi.ORBFE_ERR_ARG
    for past in (1, 31):   # the last call that ran had one set
        assert L.orbfe_pnp_tap(pn.h, past, 0, _ffi.ptr(np.zeros(128, np.uint8)), 128, _ffi.ptr(cnt)) == _ffi.ORBFE_ERR_STATE, past


@pytest.mark.gpu
def test_tap_capacity_and_an_iteration_that_did_not_run():
    """orbfe_pnp_tap: one byte short of the iteration records is ORBFE_ERR_CAP, exactly enough is ORBFE_OK with every record;
    the errors of an iteration at or past iterations_run were not recorded: ORBFE_ERR_STATE"""
    L = _ffi.lib()
    sc = PC.scene(1, 20, inlier_ratio=1.0)
    params = PN.ransac_params(0.99, 10, 300, 4, 0.5, n=20)
    args = (sc["P3Dw"], sc["P2D"], sc["sigma2"], PC.K, params, 5)
    with PnP(64, 1) as h:
        state = np.zeros(1, PN.STATE_DTYPE)
        d = PC.draws_for(1, PN.iterations(state, params, 5))
        h.set_tap_iteration(0)
        res, _ = h.iterate(*args, d, state, np.zeros(20, np.uint8))
        run = int(res["iterations_run"])
        assert run >= 1
        need = run * PN.ITER_DTYPE.itemsize
        buf = np.zeros(need, np.uint8)
        cnt = C.c_int32(-1)
        assert L.orbfe_pnp_tap(h.h, 0, PN.TAP_ITERATIONS, _ffi.ptr(buf), need - 1, C.byref(cnt)) == _ffi.ORBFE_ERR_CAP
        assert L.orbfe_pnp_tap(h.h, 0, PN.TAP_ITERATIONS, _ffi.ptr(buf), need, C.byref(cnt)) == _ffi.ORBFE_OK and cnt.value == run
        err = np.zeros(64, np.float32)
        assert L.orbfe_pnp_tap(h.h, 0, PN.TAP_ERRORS, _ffi.ptr(err), err.nbytes, C.byref(cnt)) == _ffi.ORBFE_OK and cnt.value == 20
        for k in (run, run + 1):   # the same call again, recording an iteration it does not reach
            h.set_tap_iteration(k)
            res, _ = h.iterate(*args, d, np.zeros(1, PN.STATE_DTYPE), np.zeros(20, np.uint8))
            assert int(res["iterations_run"]) == run
            assert L.orbfe_pnp_tap(h.h, 0, PN.TAP_ERRORS, _ffi.ptr(err), err.nbytes, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE, k
