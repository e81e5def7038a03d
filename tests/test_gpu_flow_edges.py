"""The optical-flow mask (csrc/orbfe_flow.hip) at the sizes, level plans, pitches, thresholds and contents of
tests/flow_edge_cases.py, bit for bit against tests/flow_oracle.py (and tests/warp_oracle.py for the homography forms); and the
masked-Frame keypoint rule alone (k_mask_keypoints) on planted records against FO.mask_rule: the seams of its 256-wide scan,
n > cap, the 65 % comparison at equality, mask values other than 0 / 1, a pitched mask, and coordinates at and past the plane
(the range is decided in float, so a NaN is outside)."""
import ctypes as C

import numpy as np
import pytest

import flow_edge_cases as E
import flow_oracle as FO
import warp_cases as WC
import warp_oracle as WO
from flow_checks import check_stages, oracle_pair
from orb_slam2_ssd_semantic_amd import KP_DTYPE, Flow, _ffi
from orb_slam2_ssd_semantic_amd import flow as FL

PAD = 0xA5


def _pair_on(fl, c, th, label):
    a, b = E.pair(c)
    of = oracle_pair((c["w"], c["h"]), lambda: (a, b), th)
    m0 = fl.compute_mask(a, th)
    assert m0.all(), label + ": first frame"
    m1 = fl.compute_mask(b, th)
    check_stages(fl, of, a.shape, label)
    assert np.array_equal(m1, of.taps["mask"]), label + ": returned mask"
    return of


# ---- the size table -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", E.SIZES, ids=lambda c: f"{c['w']}x{c['h']}")
def test_size_table_every_tap_bit_exact(c):
    w, h = c["w"], c["h"]
    fl = Flow(max_width=w, max_height=h)
    assert [(p[0], p[1]) for p in FL.plan(w, h)] == c["levels"]
    of = _pair_on(fl, c, 40.0, f"{w}x{h} th=40")
    pre = of.taps["mask_pre"]
    if pre.any() and not pre.all():
        fl.reset()
        _pair_on(fl, c, E.SECOND_THRESHOLD, f"{w}x{h} th={E.SECOND_THRESHOLD}")
    else:
        assert (w, h) in E.FLOW_ONLY
    fl.close()


@pytest.mark.gpu
def test_one_handle_runs_sizes_with_different_level_counts():
    """the scratch sized for the largest plan (524 x 512: four levels) against smaller plans, one after another"""
    fl = Flow(524, 512)
    for (w, h) in E.ONE_HANDLE:
        fl.reset()
        _pair_on(fl, E.case_of(w, h), 40.0, f"one handle {w}x{h}")
    fl.close()


# ---- degenerate contents --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", E.DEGENERATE_SIZES)
@pytest.mark.parametrize("name", E.DEGENERATE)
def test_degenerate_contents(name, w, h):
    a, b = E.degenerate(name, w, h)
    of = oracle_pair((name, w, h), lambda: (a, b), 40.0)
    for f in of.taps["flow_levels"] + [of.taps["flow2"]]:
        assert np.isfinite(f).all()
    fl = Flow(w, h)
    fl.compute_mask(a, 40.0)
    m = fl.compute_mask(b, 40.0)
    check_stages(fl, of, a.shape, f"{name} {w}x{h}")
    assert np.array_equal(m, of.taps["mask"])
    fl.close()


# ---- thresholds -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_thresholds_below_at_and_past_the_clamp():
    c = E.case_of(*E.THRESHOLD_SIZE)
    w, h = c["w"], c["h"]
    a, b = E.pair(c)
    base = oracle_pair((w, h), lambda: (a, b), 40.0)
    fl = Flow(w, h)
    for th in E.TH_AS_40:
        fl.reset()
        fl.compute_mask(a, th)
        m = fl.compute_mask(b, th)
        assert np.array_equal(fl.tap(0, FL.TAP_PRE), base.taps["mask_pre"]), th
        assert np.array_equal(m, base.taps["mask"]), th
    for th in E.TH_OTHER:
        of = FO.Flow()
        of.compute_mask(a, th)
        om = of.compute_mask(b, th)
        fl.reset()
        fl.compute_mask(a, th)
        m = fl.compute_mask(b, th)
        assert np.array_equal(fl.tap(0, FL.TAP_PRE), of.taps["mask_pre"]), th
        assert np.array_equal(fl.tap(0, FL.TAP_MASK), om) and np.array_equal(m, om), th
        if np.isinf(th):
            assert m.all()
        if np.isnan(th):
            assert of.taps["mask_pre"][-1, :].all() and not of.taps["mask_pre"][:-1, :-1].any() and not m.any()
    fl.close()


# ---- pitched planes -------------------------------------------------------------------------------------------------------
def _three_frames(w, h):
    """three frames whose two pairs give masks with both values: the bowl, the bowl translated, the bowl turned by 180 degrees"""
    a, b = E.gen_bowl(w, h)
    return [a, b, a[::-1, ::-1].copy()]


def _pitched(w, h):
    stride = w + 13
    mstride = w + 7
    return stride, stride * h + 29, mstride, mstride * h + 11


def _pack_gray(frames, w, h, stride, fs, seed):
    buf = np.random.default_rng(seed).integers(0, 256, len(frames) * fs, dtype=np.uint8)   # random padding
    for i, f in enumerate(frames):
        buf[i * fs:i * fs + stride * h].reshape(h, stride)[:, :w] = f
    return buf


def _unpack_masks(buf, n, w, h, mstride, mfs):
    """(masks [n, h, w], True when every byte outside them still holds PAD)"""
    masks = np.stack([buf[i * mfs:i * mfs + mstride * h].reshape(h, mstride)[:, :w] for i in range(n)])
    pad = np.ones(buf.size, bool)
    for i in range(n):
        pad[i * mfs:i * mfs + mstride * h].reshape(h, mstride)[:, :w] = False
    return masks, bool((buf[pad] == PAD).all())


def _oracle_sequence(frames, th, Hs=None, use=None):
    of = FO.Flow()
    return [WO.compute_mask_homo(of, f, Hs[i], th) if (Hs is not None and use[i]) else of.compute_mask(f, th)
            for i, f in enumerate(frames)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(259, 131), (131, 97)])
@pytest.mark.parametrize("homo", [False, True], ids=["plain", "homo"])
def test_pitched_device_planes(w, h, homo):
    """stride > w, frame_stride > stride * h, mask_stride > w, mask_frame_stride > mask_stride * h, random gray padding, the mask
    buffer prefilled: frame 0 takes the fill-ones path, frames 1 and 2 the morphology's; with and without d_mask_ones"""
    import torch
    frames = _three_frames(w, h)
    n = len(frames)
    stride, fs, mstride, mfs = _pitched(w, h)
    use = np.array([1, 0, 1], np.int32)
    Hs = np.stack([WC.motion(w, h, k=0.2 * (i + 1)) for i in range(n)]).astype(np.float64)
    want = np.stack(_oracle_sequence(frames, 40.0, Hs if homo else None, use))
    assert want[0].all() and all(0 < (m == 0).mean() < 1 for m in want[1:])
    d_gray = torch.from_numpy(_pack_gray(frames, w, h, stride, fs, w)).cuda()
    d_H, d_use = torch.from_numpy(Hs).cuda(), torch.from_numpy(use).cuda()
    L = _ffi.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_ones in (True, False):
        fl = Flow(w, h, max_batch=n)
        d_mask = torch.full((n * mfs,), PAD, dtype=torch.uint8, device="cuda")
        d_ones = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ones_arg = C.c_void_p(d_ones.data_ptr()) if with_ones else None
        if homo:
            s = L.orbfe_flow_compute_masks_homo_device(fl.h, C.c_void_p(d_gray.data_ptr()), n, w, h, stride, fs, C.c_void_p(d_H.data_ptr()),
                                                       C.c_void_p(d_use.data_ptr()), 40.0, C.c_void_p(d_mask.data_ptr()), mstride, mfs,
                                                       ones_arg, st)
        else:
            s = L.orbfe_flow_compute_masks_device(fl.h, C.c_void_p(d_gray.data_ptr()), n, w, h, stride, fs, 40.0,
                                                  C.c_void_p(d_mask.data_ptr()), mstride, mfs, ones_arg, st)
        assert s == _ffi.ORBFE_OK
        torch.cuda.synchronize()
        got, pad_ok = _unpack_masks(d_mask.cpu().numpy(), n, w, h, mstride, mfs)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), (with_ones, i)
        assert pad_ok, "a byte outside the mask planes was written"
        ones = d_ones.cpu().numpy()
        if with_ones:
            assert list(ones) == [int(m.sum()) for m in want]
        else:
            assert (ones == -7).all()
        assert np.array_equal(fl.tap(2, FL.TAP_MASK), want[2]) and np.array_equal(fl.tap(0, FL.TAP_MASK), want[0])
        if homo:
            assert np.array_equal(fl.tap(2, FL.TAP_WARP), WO.warp(frames[2], Hs[2]))
        fl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(259, 131), (131, 97)])
def test_pitched_host_planes(w, h):
    """the two host forms with stride > w and mask_stride > w (their hipMemcpy2DAsync calls)"""
    frames = _three_frames(w, h)
    stride, _, mstride, _ = _pitched(w, h)
    Hs = [WC.motion(w, h, k=0.2 * (i + 1)).astype(np.float64) for i in range(3)]
    use = [1, 0, 1]
    L = _ffi.lib()
    for homo in (False, True):
        want = _oracle_sequence(frames, 40.0, Hs if homo else None, use)
        fl = Flow(w, h)
        for i, f in enumerate(frames):
            g = _pack_gray([f], w, h, stride, stride * h, 10 + i)
            m = np.full(mstride * h, PAD, np.uint8)
            if homo and use[i]:
                Hm = np.ascontiguousarray(Hs[i])
                s = L.orbfe_flow_compute_mask_homo(fl.h, _ffi.ptr(g), w, h, stride, _ffi.ptr(Hm), 40.0, _ffi.ptr(m), mstride)
            else:
                s = L.orbfe_flow_compute_mask(fl.h, _ffi.ptr(g), w, h, stride, 40.0, _ffi.ptr(m), mstride)
            assert s == _ffi.ORBFE_OK
            got, pad_ok = _unpack_masks(m, 1, w, h, mstride, mstride * h)
            assert np.array_equal(got[0], want[i]), (homo, i)
            assert pad_ok, (homo, i)
        fl.close()


# ---- the full size changes, the half size does not --------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_size_changes_while_the_half_size_stays():
    big = E.gen_bowl(140, 80)
    frames = [big[0][:70, :130], big[1][:71, :131], big[0][2:73, 3:133], big[1][4:74, 1:132]]   # 130x70, 131x71, 130x71, 131x70
    fl, of = Flow(132, 71), FO.Flow()
    for i, f in enumerate(frames[:3]):
        f = np.ascontiguousarray(f)
        m = fl.compute_mask(f, 40.0)
        om = of.compute_mask(f, 40.0)
        assert np.array_equal(m, om), i
        if i:
            check_stages(fl, of, f.shape, f"frame {i} {f.shape[1]}x{f.shape[0]}")
            assert 0 < (om == 0).mean() < 1
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_mask(np.zeros((70, 132), np.uint8), 40.0)    # half size 66x35, not 65x35
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    f = np.ascontiguousarray(frames[3])
    assert np.array_equal(fl.compute_mask(f, 40.0), of.compute_mask(f, 40.0))
    check_stages(fl, of, f.shape, "after the refused call")
    fl.close()


# ---- the keypoint rule alone ------------------------------------------------------------------------------------------------
SENT = 0xCD


def _run_rule(cases, cap, mstride=None, gap=0, n_dev=None, ones=None):
    """cases: frames of one batch (same mask shape).  Uploads their records into blocks of `cap` slots (sentinel bytes in the
    slots >= n and in 8 slots past the last block), runs orbfe_mask_keypoints_device on a mask buffer of pitch mstride with
    `gap` bytes between the planes, and checks every frame against FO.mask_rule and against the planted keep flags."""
    import torch
    B = len(cases)
    h, w = cases[0]["mask"].shape
    mstride = mstride or w
    mfs = mstride * h + gap
    mbuf = np.full(B * mfs, 0, np.uint8)
    if mstride > w or gap:
        mbuf[:] = np.random.default_rng(B).integers(0, 2, mbuf.size, dtype=np.uint8)   # padding that would change answers
    kb = np.full(((B * cap + 8) * 28,), SENT, np.uint8)
    db = np.full(((B * cap + 8) * 32,), SENT, np.uint8)
    ns = []
    for i, c in enumerate(cases):
        mbuf[i * mfs:i * mfs + mstride * h].reshape(h, mstride)[:, :w] = c["mask"]
        n = min(len(c["kps"]), cap)
        kb[i * cap * 28:(i * cap + n) * 28] = c["kps"][:n].view(np.uint8)
        db[i * cap * 32:(i * cap + n) * 32] = c["desc"][:n].reshape(-1)
        ns.append(n)
    dev_n = np.array(ns if n_dev is None else n_dev, np.int32)
    sums = np.array([int(c["mask"].astype(np.int64).sum()) for c in cases] if ones is None else ones, np.int32)
    d_mask, d_k, d_d = torch.from_numpy(mbuf).cuda(), torch.from_numpy(kb).cuda(), torch.from_numpy(db).cuda()
    d_n, d_ones = torch.from_numpy(dev_n).cuda(), torch.from_numpy(sums).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s = _ffi.lib().orbfe_mask_keypoints_device(C.c_void_p(d_mask.data_ptr()), w, h, mstride, mfs, C.c_void_p(d_ones.data_ptr()), B,
                                               C.c_void_p(d_k.data_ptr()), C.c_void_p(d_d.data_ptr()), C.c_void_p(d_n.data_ptr()), cap, st)
    assert s == _ffi.ORBFE_OK
    torch.cuda.synchronize()
    gk, gd, gn = d_k.cpu().numpy(), d_d.cpu().numpy(), d_n.cpu().numpy()
    assert np.array_equal(d_mask.cpu().numpy(), mbuf)
    for i, c in enumerate(cases):
        n = ns[i]
        wk, wd = FO.mask_rule(c["mask"], c["kps"][:n], c["desc"][:n])
        filtered = float(sums[i]) > h * w * 0.65
        m = len(wk)
        if filtered:
            assert gn[i] == m, (i, int(gn[i]), m)
        else:
            assert gn[i] == dev_n[i] and m == n, i     # untouched
        if "keep" in c:
            assert np.array_equal(wk.view(np.uint8), c["kps"][:n][c["keep"][:n]].view(np.uint8)), (i, "planted keep list")
        k = gk[i * cap * 28:(i + 1) * cap * 28].reshape(cap, 28)
        d = gd[i * cap * 32:(i + 1) * cap * 32].reshape(cap, 32)
        assert np.array_equal(k[:m].reshape(-1), wk.view(np.uint8).reshape(-1)), (i, "keypoints")
        assert np.array_equal(d[:m], wd), (i, "descriptors follow their keypoints")
        assert not k[m:n].any() and not d[m:n].any(), (i, "freed slots are zero")
        assert (k[n:] == SENT).all() and (d[n:] == SENT).all(), (i, "slots >= n untouched")
    assert (gk[B * cap * 28:] == SENT).all() and (gd[B * cap * 32:] == SENT).all(), "slots past the last block untouched"


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", E.KEEP_PATTERNS)
def test_rule_counts_across_the_scan_seams(pattern):
    for n in E.RULE_COUNTS:
        _run_rule([E.rule_case(n, pattern)], cap=max(n, 1) + 3)


@pytest.mark.gpu
def test_rule_clamps_a_count_past_the_capacity():
    c = E.rule_case(257, "alternating")
    _run_rule([c], cap=257, n_dev=[257 + 5])
    c = E.rule_case(256, "last_of_256")
    _run_rule([c], cap=256, n_dev=[256 + 5])


@pytest.mark.gpu
def test_rule_share_comparison_at_equality():
    """sum(mask) > rows * cols * 0.65 in double: 260 ones of 20 x 20 (the bound is exactly 260.0) do not filter, 261 do; the same
    at 7 x 9, where the bound 40.95 is no integer"""
    assert 20 * 20 * 0.65 == 260.0
    for (w, h) in ((20, 20), (7, 9)):
        for extra in (0, 1):
            _run_rule([E.share_case(w, h, extra)], cap=4)


@pytest.mark.gpu
def test_rule_mask_values_and_coordinates():
    _run_rule([E.value_case()], cap=6)           # 2 and 255 under a keypoint: dropped; ones = the sum of the values
    c = E.coordinate_case()
    _run_rule([c], cap=len(c["kps"]) + 2)
    _run_rule([c], cap=len(c["kps"]) + 2, mstride=c["mask"].shape[1] + 5)


@pytest.mark.gpu
def test_rule_batch_with_a_pitched_mask():
    fr = E.batch_case()
    w = fr[0]["mask"].shape[1]
    _run_rule(fr, cap=304, mstride=w + 9, gap=17)
    # through the wrapper: a pitched view of a wider tensor
    import torch
    B, (h, w) = len(fr), fr[0]["mask"].shape
    cap = 304
    wide = torch.zeros((B, h, w + 9), dtype=torch.uint8, device="cuda")
    wide[:, :, :w] = torch.from_numpy(np.stack([f["mask"] for f in fr])).cuda()
    kb = np.zeros((B, cap), KP_DTYPE)
    db = np.zeros((B, cap, 32), np.uint8)
    for i, f in enumerate(fr):
        kb[i, :len(f["kps"])] = f["kps"]
        db[i, :len(f["kps"])] = f["desc"]
    d_k, d_d = torch.from_numpy(kb.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(db.reshape(-1)).cuda()
    d_n = torch.tensor([len(f["kps"]) for f in fr], dtype=torch.int32, device="cuda")
    d_ones = torch.tensor([int(f["mask"].sum()) for f in fr], dtype=torch.int32, device="cuda")
    FL.mask_keypoints(wide[:, :, :w], d_ones, d_k, d_d, d_n, cap)
    torch.cuda.synchronize()
    gk = d_k.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    for i, f in enumerate(fr):
        wk, _ = FO.mask_rule(f["mask"], f["kps"], f["desc"])
        assert int(d_n[i]) == len(wk) and np.array_equal(gk[i, :len(wk)].view(np.uint8), wk.view(np.uint8)), i
