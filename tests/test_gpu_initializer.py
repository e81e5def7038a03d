"""csrc/orbfe_initializer.hip against tests/initializer_oracle.py on the GPU, bit for bit: the known-answer primitives, the host call
over the case table of tests/initializer_cases.py (every result field, the points, the flags, the taps of a middle and of the last
iteration), the batched device form against the host calls one by one, two handles on two streams, the argument errors and the
Python class."""
import ctypes as C

import numpy as np
import pytest

import initializer_cases as IC
import initializer_oracle as IO
from orb_slam2_ssd_semantic_amd import Initializer, InitializerHandle, OrbfeError, _ffi
from orb_slam2_ssd_semantic_amd import initializer as IN

pytestmark = pytest.mark.gpu

# the fields of the result that are part of parity: everything but the parallax in degrees (the device's acosf) and the padding
FIELDS = [n for n in IN.RESULT_DTYPE.names if n not in ("parallax", "reserved")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def expected_record(r):
    e = np.zeros(1, IN.RESULT_DTYPE)
    for n in FIELDS:
        e[n] = r[n]
    return e[0]


def assert_result(res, r, what):
    e = expected_record(r)
    for n in FIELDS:
        assert same(np.asarray(res[n]), np.asarray(e[n])), f"{what}: {n}: device {res[n]} oracle {e[n]}"


@pytest.fixture(scope="module")
def handle():
    with InitializerHandle(4096, 32) as h:
        yield h


def run_case(h, name):
    c = IC.case(name)
    return h.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], c["sigma"], c["iterations"], c["draws"])


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kat", [("16x9", IN.KAT_SVD16X9), ("8x9", IN.KAT_SVD8X9), ("3x3", IN.KAT_SVD3), ("4x4", IN.KAT_SVD4)])
def test_kat_svd(what, kat):
    A = IC.kat_matrices(what)
    w, u, vt = IO.svd_f(A)
    out = IN.kat(kat, A)
    k, ur, vr = w.shape[1], u.shape[1], vt.shape[1]
    assert same(out[:, :k], w), "singular values"
    assert same(out[:, k:k + ur * ur].reshape(-1, ur, ur), u), "u"
    assert same(out[:, k + ur * ur:].reshape(-1, vr, vr), vt), "vt"


def test_kat_inv3():
    rng = np.random.default_rng(7)
    A = rng.normal(size=(50, 3, 3)).astype(np.float32)
    A[0] = 0
    A[1, 2] = A[1, 0]
    assert same(IN.kat(IN.KAT_INV3, A).reshape(-1, 3, 3), IO.inv3(A))


def test_kat_compute_h21_f21():
    p1, p2 = IC.kat_points(12)
    x = np.concatenate([p1.reshape(12, 16), p2.reshape(12, 16)], 1)
    assert same(IN.kat(IN.KAT_H21, x).reshape(-1, 3, 3), IO.compute_h21(p1, p2))
    assert same(IN.kat(IN.KAT_F21, x).reshape(-1, 3, 3), IO.compute_f21(p1, p2))


def test_kat_triangulate():
    c = IC.case("general_65")
    first = np.nonzero(c["matches12"] >= 0)[0]
    xy = np.concatenate([c["keys1"][first], c["keys2"][c["matches12"][first]]], 1)
    P1 = np.zeros((3, 4), np.float32)
    P1[:, :3] = c["K"]
    Rt = np.concatenate([c["R"], (c["t"] / np.linalg.norm(c["t"]))[:, None]], 1).astype(np.float32)
    P2 = IO.mm(c["K"], Rt)
    x3, _ = IO.triangulate(xy, P1, P2)
    inp = np.concatenate([xy, np.tile(P1.reshape(1, 12), (len(xy), 1)), np.tile(P2.reshape(1, 12), (len(xy), 1))], 1)
    assert same(IN.kat(IN.KAT_TRIANGULATE, inp), x3)


def test_kat_parallax_cut_on_every_float():
    c = IO.floats_between(0.999, 1.0)
    extra = np.array([np.nan, 1.0000001, -1.0000001, -1.0, 0.0, 0.998, -0.5], np.float32)
    x = np.concatenate([c, extra])
    want = np.array([IO.parallax_cut(v) for v in x], np.float32)
    assert want[:len(c)].sum() > 14000 and not want[len(c) - 1]
    assert np.array_equal(IN.kat(IN.KAT_PARALLAX, x)[:, 0], want)


# ---- the host call over the case table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IC.TABLE))
def test_host_call_equals_oracle(handle, name):
    c = IC.case(name)
    r0 = IC.answer(name)
    its = c["iterations"]
    hyp = max(r0["best"], 0)
    for tap_it in sorted({its // 2, its - 1}):   # a middle and the last iteration
        r = IC.answer(name, tap_it, hyp)
        handle.set_tap_iteration(tap_it, hyp)
        res, P3D, tri = run_case(handle, name)
        assert_result(res, r, name)
        assert same(P3D, r["P3D"]) and same(tri, r["triangulated"])
        it = handle.tap(0, IN.TAP_ITERATIONS)
        t = r["tap"]
        assert len(it) == its
        assert same(it["set"], t["sets"]), "mvSets"
        for f, o in (("Hn", "Hn"), ("Fn", "Fn"), ("H21i", "H21i"), ("F21i", "F21i"), ("scoreH", "scoreH"), ("scoreF", "scoreF")):
            assert same(it[f], t[o]), f"{name}: tap {f}"
        m = handle.tap(0, IN.TAP_MATCHES)
        assert m.shape == (r["n_matches"], 9)
        assert same(m[:, :4], t["chi"]), "chiSquare of both models"
        rt = t["rt"] if t["rt"] is not None else np.zeros((r["n_matches"], 5), np.float32)
        assert same(m[:, 4:], rt), "CheckRT records"


def test_every_tapped_iteration_of_a_long_run(handle):
    name = "general_120_it200"
    r = IC.answer(name)
    handle.set_tap_iteration(0, 0)
    run_case(handle, name)
    it = handle.tap(0, IN.TAP_ITERATIONS)
    assert len(it) == 200 and same(it["scoreF"], r["tap"]["scoreF"]) and same(it["scoreH"], r["tap"]["scoreH"])
    assert (it["scoreF"] == it["scoreF"].max()).sum() > 1 and r["iterF"] == int(np.argmax(it["scoreF"]))


# ---- the batched device form ------------------------------------------------------------------------------------------------------------
def device_batch(names):
    import torch
    cs = [IC.case(n) for n in names]
    off1 = np.cumsum([0] + [len(c["keys1"]) for c in cs]).astype(np.int32)
    off2 = np.cumsum([0] + [len(c["keys2"]) for c in cs]).astype(np.int32)
    pairs = np.zeros(len(cs), IN.PAIR_DTYPE)
    doff = 0
    for p, c in zip(pairs, cs):
        p["K"], p["sigma"], p["iterations"], p["draws_offset"] = c["K"], c["sigma"], c["iterations"], doff
        doff += 8 * c["iterations"]
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return dict(offsets1=t(off1), offsets2=t(off2), keys1=t(np.concatenate([c["keys1"] for c in cs])),
                keys2=t(np.concatenate([c["keys2"] for c in cs])), matches12=t(np.concatenate([c["matches12"] for c in cs])),
                pairs=t(pairs.view(np.uint8).reshape(len(cs), -1)), draws=t(np.concatenate([c["draws"] for c in cs]))), off1


def check_batch(names, res, P3D, tri, off1):
    res = res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)
    P3D, tri = P3D.cpu().numpy(), tri.cpu().numpy()
    for i, n in enumerate(names):
        r = IC.answer(n)
        assert_result(res[i], r, f"pair {i} ({n})")
        assert same(P3D[off1[i]:off1[i + 1]], r["P3D"]) and same(tri[off1[i]:off1[i + 1]], r["triangulated"])


BATCH17 = ["general_8", "planar_64", "general_257", "tie", "pure_rotation", "two_sided", "general_9", "too_few", "low_parallax", "far_point",
           "general_63", "one_behind", "sized_51", "ambiguous_plane", "general_64", "planar_257", "general_65"]


@pytest.mark.parametrize("npairs", [1, 2, 17])
def test_batched_form_equals_the_host_calls(npairs):
    import torch
    names = BATCH17[:npairs] if npairs > 1 else ["general_257"]
    args, off1 = device_batch(names)
    with InitializerHandle(int(off1[-1]), npairs) as h:
        res, P3D, tri = h.initialize_device(**args)
        torch.cuda.synchronize()
        check_batch(names, res, P3D, tri, off1)
        for i, n in enumerate(names):   # ... which are the host calls one by one
            hres, hP, ht = run_case(h, n)
            dres = res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)[i]
            for f in FIELDS:
                assert same(np.asarray(hres[f]), np.asarray(dres[f])), (n, f)
            assert same(hP, P3D.cpu().numpy()[off1[i]:off1[i + 1]])


def test_two_handles_on_two_streams():
    import torch
    a, b = ["general_257", "planar_64", "two_sided"], ["low_parallax", "general_65"]
    args_a, off_a = device_batch(a)
    args_b, off_b = device_batch(b)
    with InitializerHandle(int(off_a[-1]), 3) as ha, InitializerHandle(int(off_b[-1]), 2) as hb:
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        out_a = ha.initialize_device(**args_a, stream=sa.cuda_stream)
        out_b = hb.initialize_device(**args_b, stream=sb.cuda_stream)
        out_a2 = ha.initialize_device(**args_a, stream=sa.cuda_stream)
        sa.synchronize()
        sb.synchronize()
        check_batch(a, *out_a, off_a)
        check_batch(b, *out_b, off_b)
        check_batch(a, *out_a2, off_a)


def test_argument_errors(handle):
    import torch
    c = IC.case("general_9")
    args = (c["keys1"], c["keys2"], c["matches12"], c["K"], 1.0, c["iterations"], c["draws"])

    def refused(*a):
        with pytest.raises(OrbfeError) as e:
            handle.initialize(*a)
        assert e.value.status == _ffi.ORBFE_ERR_ARG

    m = c["matches12"].copy()
    m[:2] = -1
    refused(c["keys1"], c["keys2"], m, *args[3:])                                   # 7 matches
    m = c["matches12"].copy()
    m[3] = len(c["keys2"])
    refused(c["keys1"], c["keys2"], m, *args[3:])                                   # a match index out of range
    refused(*args[:5], 0, c["draws"])                                               # iterations
    refused(*args[:5], IN.MAX_ITERATIONS + 1, np.zeros(8 * (IN.MAX_ITERATIONS + 1), np.int32))
    with InitializerHandle(8, 1) as small:                                          # a capacity exceeded
        with pytest.raises(OrbfeError) as e:
            small.initialize(*args)
        assert e.value.status == _ffi.ORBFE_ERR_ARG
        big, _ = device_batch(["general_8", "general_9"])
        with pytest.raises(OrbfeError) as e:
            small.initialize_device(**big)                                          # two pairs on a handle for one
        assert e.value.status == _ffi.ORBFE_ERR_ARG
    # the device form reports per pair what the host form refuses: pair 0 has 7 matches, pair 1 an index past n2, pair 2 does not
    # fit the handle; pair 3 is fine and is not disturbed
    names = ["general_9", "general_9", "general_257", "general_63"]
    b, off1 = device_batch(names)
    mm = b["matches12"].cpu().numpy().copy()
    mm[:2] = -1
    mm[off1[1] + 3] = 1000
    b["matches12"] = torch.from_numpy(mm).to(b["matches12"].device)
    with InitializerHandle(int(off1[-1]), 4) as h:
        res, P3D, tri = h.initialize_device(**b)
        torch.cuda.synchronize()
        rec = res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)
        assert rec["status"].tolist()[:2] == [IN.STATUS_FEW_MATCHES, IN.STATUS_BAD_INDEX] and not rec["ok"][:2].any()
        assert_result(rec[3], IC.answer("general_63"), "pair 3")
        assert_result(rec[2], IC.answer("general_257"), "pair 2")
    with InitializerHandle(int(off1[2]) + 10, 4) as h:   # pair 2 ends past max_matches, pair 3 lies wholly past it
        res, P3D, tri = h.initialize_device(**device_batch(names)[0])
        torch.cuda.synchronize()
        rec = res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)
        assert rec["status"].tolist() == [0, 0, IN.STATUS_BAD_SIZES, IN.STATUS_BAD_SIZES]
        assert_result(rec[0], IC.answer("general_9"), "pair 0")
    # taps: a pair that did not run, an iteration that did not run
    handle.set_tap_iteration(5, 0)
    run_case(handle, "general_8")   # 4 iterations
    cnt = C.c_int32()
    buf = np.zeros((4096, 9), np.float32)
    L = _ffi.lib()
    assert L.orbfe_initializer_tap(handle.h, 0, IN.TAP_MATCHES, _ffi.ptr(buf), buf.nbytes, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE
    assert L.orbfe_initializer_tap(handle.h, 1, IN.TAP_ITERATIONS, _ffi.ptr(buf), buf.nbytes, C.byref(cnt)) == _ffi.ORBFE_ERR_STATE
    assert L.orbfe_initializer_tap(handle.h, 0, IN.TAP_ITERATIONS, _ffi.ptr(buf), 16, C.byref(cnt)) == _ffi.ORBFE_ERR_CAP
    assert L.orbfe_initializer_set_tap_iteration(handle.h, 0, 8) == _ffi.ORBFE_ERR_ARG
    handle.set_tap_iteration(0, 0)


def test_no_model(handle):
    """no iteration with a positive score: ok = 0, status NO_MODEL (undefined in the reference)"""
    rng = np.random.default_rng(3)
    k1 = rng.uniform(0, 640, (12, 2)).astype(np.float32)
    k2 = rng.uniform(0, 640, (12, 2)).astype(np.float32)
    m = np.arange(12, dtype=np.int32)
    K = IC.case("general_8")["K"]
    d = IC.draws_for(1, 0)
    r = IO.initialize(k1, k2, m, K, 1e-3, 1, d)
    res, P3D, tri = handle.initialize(k1, k2, m, K, 1e-3, 1, d)
    assert res["status"] == IN.STATUS_NO_MODEL and not P3D.any() and not tri.any()
    assert_result(res, r, "no model")


def test_python_class_with_the_default_rand():
    c = IC.case("general_100_it65")
    ini = Initializer(c["keys1"], c["K"], sigma=1.0, iterations=40)
    ok, R21, t21, P3D, tri = ini.initialize(c["keys2"], c["matches12"])
    rng = np.random.default_rng(0)
    d = np.concatenate([rng.integers(0, 2 ** 31, 8 * 40), rng.integers(0, 2 ** 31, 8 * 40)]).astype(np.int32)
    r = IO.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], 1.0, 40, d[:320])
    assert ok and r["ok"] == 1 and same(R21, r["R21"]) and same(t21, r["t21"]) and same(P3D, r["P3D"])
    assert np.array_equal(tri, r["triangulated"].astype(bool)) and tri.dtype == bool
    assert_result(ini.result, r, "class")
    # the second call consumes the next iterations * 8 draws
    ini.initialize(c["keys2"], c["matches12"])
    r2 = IO.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], 1.0, 40, d[320:])
    assert_result(ini.result, r2, "class, second call")
    assert not same(r["tap"]["sets"], r2["tap"]["sets"])


def test_chain_extractor_matcher_initializer():
    """extractor blocks of two synthetic frames -> the device matcher's output block -> initialize_device on one stream, nothing
    read by the host in between; equal to the oracle fed the same keys and matches"""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor, ORBmatcher
    from orb_slam2_ssd_semantic_amd.synth import synth_frame
    B, w, h = 2, 640, 480
    rng = np.random.default_rng(11)
    base = synth_frame(77)
    second = np.roll(base, (3, 9), axis=(0, 1)).astype(np.float64) + rng.normal(0, 2.0, base.shape)
    frames = np.stack([base, np.clip(np.rint(second), 0, 255).astype(np.uint8)])
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    st = torch.cuda.current_stream().cuda_stream
    d_gray = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    mt = ORBmatcher(0.9, True)
    d_q = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_t = torch.ones(1, dtype=torch.int32, device="cuda")
    d_match = torch.full((1, cap), -1, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.check(_ffi.lib().orbfe_match_bf_frames_device(mt.handle, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, d_q.data_ptr(),
                                                       d_t.data_ptr(), 1, 0.9, 50, 1, d_match.data_ptr(), d_nm.data_ptr(), C.c_void_p(st)),
               "orbfe_match_bf_frames_device")
    # the keys' coordinates out of the extractor's 28-byte records and the CSR offsets out of its counts, on the device
    xy = d_kps.view(torch.float32)[:, :, :2].contiguous()
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    off1, off2 = torch.cat([zero, d_n[0:1]]), torch.cat([zero, d_n[1:2]])
    K = IC.K0
    its = 200
    draws = IC.draws_for(its, 77)
    pair = np.zeros(1, IN.PAIR_DTYPE)
    pair["K"], pair["sigma"], pair["iterations"] = K, 1.0, its
    with InitializerHandle(cap, 1) as hnd:
        res, P3D, tri = hnd.initialize_device(off1, off2, xy[0], xy[1], d_match[0], torch.from_numpy(pair.view(np.uint8).reshape(1, -1)).cuda(),
                                              torch.from_numpy(draws).cuda())
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
        k1 = np.stack([kps[0]["x"], kps[0]["y"]], 1)[:n[0]]
        k2 = np.stack([kps[1]["x"], kps[1]["y"]], 1)[:n[1]]
        m = d_match.cpu().numpy()[0, :n[0]]
        assert (m >= 0).sum() >= 100 and int(d_nm.cpu()[0]) == (m >= 0).sum()
        r = IO.initialize(k1, k2, m, K, 1.0, its, draws)
        rec = res.cpu().numpy().view(IN.RESULT_DTYPE).reshape(-1)[0]
        assert_result(rec, r, "chain")
        assert same(P3D.cpu().numpy()[:n[0]], r["P3D"]) and same(tri.cpu().numpy()[:n[0]], r["triangulated"])
        assert r["SH"] > 0 and r["SF"] > 0
