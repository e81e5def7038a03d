"""Sim3Solver's RANSAC on the GPU (csrc/orbfe_sim3.hip) against the canonical mode of tests/sim3_oracle.py, bit for bit: the
device primitives (float 4x4 Jacobi, canonical atan2 / sin / cos, N matrix -> rotation), the host call over the case table with
the taps of every iteration run, the batched device form against host calls, the device constructor, the argument errors
and the Python class.  NaNs compare by position (the payload and sign of a generated NaN belong to the processor); every
other value compares as bits."""
import ctypes as C
import math

import numpy as np
import pytest

import sim3_cases as SC
import sim3_oracle as SO
from orb_slam2_ssd_semantic_amd import Sim3, Sim3Solver, _ffi
from orb_slam2_ssd_semantic_amd import sim3 as S3
from sim3_checks import check_case, model_equal, same_bits

MAX_PAIRS = 512
F = np.float32


@pytest.fixture(scope="module")
def sm():
    h = Sim3(MAX_PAIRS, 32)
    yield h
    h.close()


# ---- KATs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kat_jacobi4():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(300, 4, 4)).astype(F)
    A = (A + A.transpose(0, 2, 1)) * F(0.5)
    A[0] = np.diag(np.array([4, 3, 2, 1], F))          # already sorted
    A[1] = np.diag(np.array([1, 4, 2, 3], F))          # diagonal, unsorted
    A[2] = np.eye(4, dtype=F) * F(2.5)                 # one eigenvalue four times
    A[3] = np.diag(np.array([1, 7, 7, 1], F))          # repeated pairs
    A[4] = 0
    A[5] = np.ones((4, 4), F)                          # rank one
    A[6] *= F(1e-30)
    A[7] *= F(1e30)
    for k in range(8, 40):                              # real N matrices
        tri = rng.choice(60, 3, replace=False)
        X1, X2 = SC.scene(60, 10, k)[:2]
        A[k] = SO.n_matrix(X1[tri].T, X2[tri].T)[0]
    W, V = S3.kat(S3.KAT_JACOBI4, A)
    for k in range(len(A)):
        ow, ov = SO.jacobi_f32(A[k])
        assert same_bits(W[k], ow) and same_bits(V[k], ov), k


def _trig_grid():
    rng = np.random.default_rng(2)
    v = [0.0, -0.0, 5e-324, 1e-310, 2.0 ** -1022, 2.0 ** -27, 2.0 ** -28, 0.3, 0.29999999999999, 0.78125, 0.7812500000001]
    pio4_hi = np.array([0x3fe921fb << 32], np.uint64).view(np.float64)[0]
    for base in (pio4_hi, math.pi / 4, math.pi / 2, math.pi, 3 * math.pi / 2, 2 * math.pi, 3 * math.pi / 4, 5 * math.pi / 4, 7 * math.pi / 4):
        for k in range(-3, 4):
            x = base
            for _ in range(abs(k)):
                x = np.nextafter(x, math.inf if k > 0 else -math.inf)
            v.append(float(x))
    v += [float(np.float64(np.array([(0x3fe921fb << 32) | 0xffffffff], np.uint64).view(np.float64)[0])), 6.283185482025146, 6.2831854820251465,
          100.0, 823549.0, 823549.5, math.inf, math.nan, 1e300]
    v += rng.uniform(0, 2 * math.pi, 2000).tolist()
    v += (rng.uniform(0, 2 * math.pi, 200) * 10.0 ** rng.uniform(-12, 0, 200)).tolist()
    v = np.array(v, np.float64)
    return np.r_[v, -v]


@pytest.mark.gpu
def test_kat_canonical_trig():
    x = _trig_grid()
    with np.errstate(all="ignore"):
        assert same_bits(S3.kat(S3.KAT_SIN, x), np.array([SO.c_sin(t) for t in x]))
        assert same_bits(S3.kat(S3.KAT_COS, x), np.array([SO.c_cos(t) for t in x]))
    rng = np.random.default_rng(3)
    sp = [0.0, -0.0, 1.0, -1.0, 5e-324, 1e-310, 1e-300, 1e300, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 66, 2.0 ** -29, 2.0 ** 61, 2.0 ** -61,
          math.inf, math.nan]
    yx = [(a, b) for a in sp for b in sp]
    yx += [(a * 1.0, 1.0) for a in (0.4375, 0.6875, 1.1875, 2.4375)] + [(np.nextafter(a, 0), 1.0) for a in (0.4375, 0.6875, 1.1875, 2.4375)]
    yx += list(zip(rng.uniform(0, 1, 2000), rng.uniform(-1, 1, 2000)))
    yx += list(zip(rng.normal(size=500) * 10.0 ** rng.uniform(-20, 20, 500), rng.normal(size=500) * 10.0 ** rng.uniform(-20, 20, 500)))
    yx = np.array(yx, np.float64)
    assert same_bits(S3.kat(S3.KAT_ATAN2, yx), np.array([SO.c_atan2(y, x) for y, x in yx]))


@pytest.mark.gpu
def test_kat_rotation():
    rng = np.random.default_rng(4)
    Ns = []
    for k in range(60):
        tri = rng.choice(60, 3, replace=False)
        X1, X2 = SC.scene(60, 10, 100 + k, angle=rng.uniform(0, math.pi))[:2]
        Ns.append(SO.n_matrix(X1[tri].T, X2[tri].T)[0])
    t = SC.full_table()["nan_translation"]
    Ns.append(SO.n_matrix(t["X1"][:3].T, t["X2"][:3].T)[0])      # zero imaginary part: all NaN
    half = SC.scene(30, 0, 7, angle=math.pi)                       # a half turn: theta near 2 * pi... or 0
    Ns.append(SO.n_matrix(half[0][:3].T, half[1][:3].T)[0])
    Ns = np.array(Ns, F)
    got = S3.kat(S3.KAT_ROTATION, Ns)
    for k in range(len(Ns)):
        assert same_bits(got[k], SO.rotation_from_n(Ns[k], "canonical")), k
    assert np.isnan(got[60]).all()


# ---- the host call ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SC.full_table()))
def test_host_call_case(sm, name):
    c = SC.full_table()[name]
    outs, _ = SC.reference(name)
    small = sum(o["iterations_run"] for o in outs) <= 12
    check_case(sm, c, outs, errors_at=list(range(5)) if small else None)


@pytest.mark.gpu
def test_three_calls_equal_one_run_of_15(sm):
    c = SC.full_table()["three_calls"]
    state, best_mask = check_case(sm, c, SC.reference("three_calls")[0])
    one = dict(c, calls=[(15, np.concatenate([d[:15] for _, d in c["calls"]]))])
    (o,), s = SC.run(one, "canonical")
    assert o["found"] and o["iterations_run"] == 13 == int(state["iterations"][0])
    assert model_equal(state["best"][0], s.best) and np.array_equal(best_mask, s.best_mask)


@pytest.mark.gpu
def test_return_lanes_cover_a_chunk():
    """the steered cases return on the first lane, a middle lane and the last lane of a chunk of 32, and in the second chunk"""
    got = {k: SC.reference(k)[0][0]["iterations_run"] - 1 for k in SC.full_table() if k.startswith("its_") and k != "its_300_none"}
    assert got == {"its_1_first": 0, "its_5_middle": 2, "its_33_last_lane": 31, "its_33_second_chunk": 32, "its_300_second_chunk": 45}
    assert any(np.isnan(l["err2"]).any() or np.isinf(l["err2"]).any() for l in SC.reference("behind")[0][0]["log"])


# ---- the batched device form ---------------------------------------------------------------------------------------------------
def _batch(names, empty):
    """CSR arrays of the first call of the named cases; empty: with an empty set after the first one"""
    tab = SC.full_table()
    cs = [tab[k] for k in names]
    if empty:
        cs.insert(1, dict(tab["n_3"], X1=np.zeros((0, 3), F), X2=np.zeros((0, 3), F), sigma2_1=np.zeros(0, F), sigma2_2=np.zeros(0, F), name="empty"))
    rng = np.random.default_rng(len(cs))
    off = np.zeros(len(cs) + 1, np.int32)
    sets = np.zeros(len(cs), S3.SET_DTYPE)
    draws, idx1, koff = [], [], 0
    for i, c in enumerate(cs):
        n = len(c["X1"])
        off[i + 1] = off[i] + n
        nit, d = c["calls"][0]
        n1 = n + 7
        sets[i] = (c["K1"], c["K2"], c["fix_scale"], c["min_inliers"], c["max_its"], nit, sum(len(x) for x in draws), koff, n1, 0)
        draws.append(d)
        idx1.append(np.sort(rng.permutation(n1)[:n]).astype(np.int32))
        koff += n1
    cat = lambda k, w: np.concatenate([np.asarray(c[k], F).reshape(-1, w) for c in cs]).reshape(-1, w)   # noqa: E731
    return dict(cases=cs, off=off, sets=sets, draws=np.concatenate(draws).astype(np.int32), idx1=np.concatenate(idx1), nkeys=koff,
                X1=cat("X1", 3), X2=cat("X2", 3), s1=cat("sigma2_1", 1).ravel(), s2=cat("sigma2_2", 1).ravel())


def _run_batch(h, b, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    N = len(b["X1"])
    state = torch.zeros((len(b["sets"]), 144), dtype=torch.uint8, device=dev)
    best_mask = torch.full((max(N, 1),), 0, dtype=torch.uint8, device=dev)
    result = torch.full((len(b["sets"]), 144), 0xAB, dtype=torch.uint8, device=dev)
    mask = torch.full((max(N, 1),), 0xCD, dtype=torch.uint8, device=dev)
    key_mask = torch.full((b["nkeys"],), 0xEF, dtype=torch.uint8, device=dev)
    ins = [t(b[k]) for k in ("off", "X1", "X2", "s1", "s2")] + [t(b["sets"].view(np.uint8).reshape(-1, 64)), t(b["draws"])]
    idx1 = t(b["idx1"])
    ins.append(idx1)
    torch.cuda.synchronize()   # the fills above ran on the default stream
    ctx = torch.cuda.stream(stream) if stream is not None else None
    if ctx:
        ctx.__enter__()
    h.iterate_device(*ins[:7], state, best_mask, result=result, mask=mask, idx1=idx1, key_mask=key_mask)
    if ctx:
        ctx.__exit__(None, None, None)
    return state, best_mask, result, mask, key_mask, ins   # the inputs stay alive until the caller has synchronised


def _check_batch(b, outs, host, max_pairs):
    state, best_mask, result, mask, key_mask = (x.cpu().numpy() for x in outs[:5])
    state = state.view(S3.STATE_DTYPE).ravel()
    result_raw = result
    result = result.view(S3.RESULT_DTYPE).ravel()
    koff = 0
    for i, c in enumerate(b["cases"]):
        lo, hi = b["off"][i], b["off"][i + 1]
        n, n1 = hi - lo, hi - lo + 7
        km = key_mask[koff:koff + n1]
        koff += n1
        if n > max_pairs:
            assert result_raw[i, :16].view(np.int32).tolist() == [0, 1, 0, 0]
            assert (result_raw[i, 16:] == 0xAB).all() and (mask[lo:hi] == 0xCD).all() and (km == 0xEF).all()
            assert not state[i:i + 1].view(np.uint8).any() and not best_mask[lo:hi].any()
            continue
        st = np.zeros(1, S3.STATE_DTYPE)
        bm = np.zeros(n, np.uint8)
        nit, d = c["calls"][0]
        res, m = host.iterate(c["X1"], c["X2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], c["fix_scale"], c["min_inliers"],
                              c["max_its"], nit, d, st, bm)
        assert same_bits(result[i]["model"]["T12"], res["model"]["T12"]), c["name"]
        for f in ("found", "no_more", "n_inliers", "iterations_run"):
            assert result[i][f] == res[f], (c["name"], f)
        assert np.array_equal(mask[lo:hi], m) and np.array_equal(best_mask[lo:hi], bm)
        assert state[i]["iterations"] == st[0]["iterations"] and state[i]["best_inliers"] == st[0]["best_inliers"]
        for f in ("T12", "R", "t"):
            assert same_bits(state[i]["best"][f], st[0]["best"][f])
        want = np.zeros(n1, np.uint8)
        want[b["idx1"][lo:hi][m.astype(bool)]] = 1
        assert np.array_equal(km, want), c["name"]


_BATCHES = {1: ["its_5_middle"], 2: ["n_65"],
            17: ["n_3", "n_19", "n_20", "n_21", "n_63", "n_64", "n_65", "n_257", "its_1_first", "its_5_middle", "its_33_last_lane",
                 "behind", "nan_translation", "exact", "scale_free_on_fixed_data", "all_outliers"]}


@pytest.mark.gpu
@pytest.mark.parametrize("nsets", [1, 2, 17])
def test_batched_device_form(sm, nsets):
    import torch
    b = _batch(_BATCHES[nsets], nsets > 1)
    assert len(b["cases"]) == nsets
    with Sim3(128, 32) as h:          # n_257 is past this handle's max_pairs
        h.set_tap_iteration(0)
        outs = _run_batch(h, b)
        torch.cuda.synchronize()
        _check_batch(b, outs, sm, 128)
        if nsets > 1:
            assert len(h.tap(1, S3.TAP_ITERATIONS)) == 0   # the empty set


@pytest.mark.gpu
def test_two_handles_two_streams(sm):
    import torch
    b = _batch(_BATCHES[17], True)
    with Sim3(MAX_PAIRS, 32) as h1, Sim3(MAX_PAIRS, 32) as h2:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1 = _run_batch(h1, b, s1)
        o2 = _run_batch(h2, b, s2)
        s1.synchronize()
        s2.synchronize()
        _check_batch(b, o1, sm, MAX_PAIRS)
        for x, y in zip(o1[:5], o2[:5]):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_prepare_device(sm):
    import torch
    rng = np.random.default_rng(5)
    n = 1001
    W1, W2 = rng.normal(size=(n, 3)).astype(F) * 5, rng.normal(size=(n, 3)).astype(F) * 5
    R1, R2 = SC.rodrigues([1, 2, 3], 0.7).astype(F), SC.rodrigues([-1, 0.5, 2], 2.1).astype(F)
    t1, t2 = np.array([0.1, -2, 3], F), np.array([5, 0.25, -1], F)
    X1, X2 = sm.prepare_device(torch.from_numpy(W1).cuda(), torch.from_numpy(W2).cuda(), R1, t1, R2, t2)
    torch.cuda.synchronize()
    assert same_bits(X1.cpu().numpy(), SO.camera_points(W1, R1, t1)) and same_bits(X2.cpu().numpy(), SO.camera_points(W2, R2, t2))


# ---- errors, Python class --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(sm):
    L = _ffi.lib()
    c = SC.full_table()["n_64"]
    n = 64
    st = np.zeros(1, S3.STATE_DTYPE)
    bm = np.zeros(n, np.uint8)
    res = np.full(1, 0, S3.RESULT_DTYPE)
    res["found"] = -7
    k = np.array(c["K1"], F)
    d = c["calls"][0][1]
    p = _ffi.ptr

    def call(h=sm.h, X1=c["X1"], nn=n, nit=5, draws=d, state=st, mi=20):
        return L.orbfe_sim3_iterate(h, p(X1), p(c["X2"]), p(c["sigma2_1"]), p(c["sigma2_2"]), nn, p(k), p(k), 1, mi, 300, nit, p(draws), p(state),
                                    p(bm), p(res), None)
    for bad in (dict(nn=MAX_PAIRS + 1), dict(nit=-1), dict(nit=(1 << 20) + 1), dict(draws=None), dict(X1=None), dict(state=None), dict(nn=-1),
                dict(mi=-1), dict(h=None)):
        assert call(**bad) == _ffi.ORBFE_ERR_ARG, bad
        assert _ffi.last_error(), bad
    assert res["found"][0] == -7 and not st.view(np.uint8).any()   # nothing ran
    h = C.c_void_p()
    assert L.orbfe_sim3_create(0, 0, 1, C.byref(h)) == _ffi.ORBFE_ERR_ARG and L.orbfe_sim3_create(0, 1, 0, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    one = C.c_void_p(8)
    assert L.orbfe_sim3_iterate_device(sm.h, one, one, one, one, one, one, one, 33, one, one, one, one, None, None, None) == _ffi.ORBFE_ERR_ARG
    assert "max_sets" in _ffi.last_error()
    assert L.orbfe_sim3_iterate_device(sm.h, one, one, one, one, one, one, one, 1, one, one, one, one, one, None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_sim3_iterate_device(sm.h, one, one, None, one, one, one, one, 1, one, one, one, one, None, None, None) == _ffi.ORBFE_ERR_ARG
    cnt = C.c_int32()
    assert L.orbfe_sim3_tap(sm.h, 31, 0, p(bm), 64, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE
    with Sim3(64, 1) as fresh:   # no taps until they are asked for
        assert L.orbfe_sim3_tap(fresh.h, 0, 0, p(bm), 64, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE
    assert L.orbfe_sim3_kat(9, 1, p(bm), p(bm)) == _ffi.ORBFE_ERR_ARG
    assert call() == _ffi.ORBFE_OK and res["iterations_run"][0] >= 1


@pytest.mark.gpu
def test_tap_capacity_and_an_iteration_that_did_not_run():
    """orbfe_sim3_tap: one byte short of the iteration records is ORBFE_ERR_CAP, exactly enough is ORBFE_OK with every record;
    the errors of an iteration at or past iterations_run were not recorded: ORBFE_ERR_STATE"""
    L = _ffi.lib()
    c = SC.full_table()["n_64"]
    args = (c["X1"], c["X2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], 1, 20, 300, 5, c["calls"][0][1])
    with Sim3(64, 1) as h:
        h.set_tap_iteration(0)
        res, _ = h.iterate(*args, np.zeros(1, S3.STATE_DTYPE), np.zeros(64, np.uint8))
        run = int(res["iterations_run"])
        assert 1 <= run <= 5
        need = run * S3.ITER_DTYPE.itemsize
        buf = np.zeros(need, np.uint8)
        cnt = C.c_int32(-1)
        assert L.orbfe_sim3_tap(h.h, 0, S3.TAP_ITERATIONS, _ffi.ptr(buf), need - 1, C.byref(cnt)) == _ffi.ORBFE_ERR_CAP
        assert L.orbfe_sim3_tap(h.h, 0, S3.TAP_ITERATIONS, _ffi.ptr(buf), need, C.byref(cnt)) == _ffi.ORBFE_OK and cnt.value == run
        err = np.zeros((64, 2), F)
        assert L.orbfe_sim3_tap(h.h, 0, S3.TAP_ERRORS, _ffi.ptr(err), err.nbytes, C.byref(cnt)) == _ffi.ORBFE_OK and cnt.value == 64
        for k in (run, run + 1):   # the same call again, recording an iteration it does not reach
            h.set_tap_iteration(k)
            res, _ = h.iterate(*args, np.zeros(1, S3.STATE_DTYPE), np.zeros(64, np.uint8))
            assert int(res["iterations_run"]) == run
            assert L.orbfe_sim3_tap(h.h, 0, S3.TAP_ERRORS, _ffi.ptr(err), err.nbytes, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE, k


@pytest.mark.gpu
def test_python_class(sm):
    c = SC.full_table()["second_call"]
    outs, osolver = SC.reference("second_call")
    n = len(c["X1"])
    rng = np.random.default_rng(8)
    n1 = n + 11
    idx1 = np.sort(rng.permutation(n1)[:n])
    s = Sim3Solver(c["X1"], c["X2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], c["fix_scale"], idx1=idx1, n1=n1, handle=sm)
    s.set_ransac_parameters(0.99, c["min_inliers"], 300)
    assert s.max_its == c["max_its"]
    st = np.zeros(1, S3.STATE_DTYPE)
    bm = np.zeros(n, np.uint8)
    for (nit, d), o in zip(c["calls"], outs):
        T12, no_more, inl, ninl = s.iterate(nit, d)
        res, m = sm.iterate(c["X1"], c["X2"], c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"], c["fix_scale"], c["min_inliers"], c["max_its"], nit,
                            d, st, bm)
        assert same_bits(T12, res["model"]["T12"]) and same_bits(T12, o["T12"]) and ninl == o["n_inliers"] and no_more == o["no_more"]
        want = np.zeros(n1, bool)
        want[idx1[m.astype(bool)]] = True
        assert np.array_equal(inl, want) and s.iterations_run == o["iterations_run"]
    assert same_bits(s.get_estimated_rotation(), osolver.best["R"]) and same_bits(s.get_estimated_translation(), osolver.best["t"])
    assert s.get_estimated_scale() == float(osolver.best["s"])
    # draws of its own: find() on a fresh solver runs and gives a model on this easy set
    f = Sim3Solver.from_world(c["X1"], np.eye(3), np.zeros(3), c["X2"], np.eye(3), np.zeros(3), c["sigma2_1"], c["sigma2_2"], c["K1"], c["K2"],
                              handle=sm, seed=3)
    f.set_ransac_parameters(0.99, 20, 300)
    T12, inl, ninl = f.find()
    assert T12 is not None and ninl > 20 and inl.sum() == ninl
