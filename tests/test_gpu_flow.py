"""FlowSLAM::Flow::ComputeMask on the GPU (csrc/orbfe_flow.hip) against tests/flow_oracle.py, stage by stage and bit for bit;
the device sequence form against the host call; the chain extract -> flow masks -> masked keypoints against the compiled
reference's masked Frame constructor (perfect/src/Frame.cc:328-420)."""
import ctypes as C

import numpy as np
import pytest
import scipy.ndimage as ndi

import flow_oracle as FO
from flow_checks import check_stages
from orb_slam2_ssd_semantic_amd import KP_DTYPE, Flow, _ffi
from orb_slam2_ssd_semantic_amd import flow as FL
from orb_slam2_ssd_semantic_amd.synth import synth_frame


def _u8(a):
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


def moving_patch(seed, h, w, pdx, pdy, bdx=0.0, bdy=0.0):
    """(a, b): a textured background (translated by (bdx, bdy) in b) with a textured 1/4-size patch that moves by (pdx, pdy)"""
    bg = synth_frame(seed, h=h + 64, w=w + 64).astype(np.float64)
    patch = synth_frame(seed + 1, h=h // 4, w=w // 4).astype(np.float64)
    a = bg[32:32 + h, 32:32 + w].copy()
    b = ndi.shift(bg, (bdy, bdx), order=3, mode="nearest")[32:32 + h, 32:32 + w]
    y0, x0 = h // 3, w // 3
    a[y0:y0 + h // 4, x0:x0 + w // 4] = patch
    yi, xi = int(round(y0 + pdy)), int(round(x0 + pdx))
    b[yi:yi + h // 4, xi:xi + w // 4] = patch
    return _u8(a), _u8(b)


def shifted_photo(dx, dy, A=None):
    from orb_slam2_ssd_semantic_amd import photos
    img = photos.vga_gray_frames(both_flags=False, jpeg=False)[1][1].astype(np.float64)
    if A is None:
        b = ndi.shift(img, (dy, dx), order=3, mode="nearest")
    else:
        h, w = img.shape
        c = np.array([h / 2.0, w / 2.0])
        Ainv = np.linalg.inv(np.asarray(A, np.float64))
        b = ndi.affine_transform(img, Ainv, offset=c - Ainv @ (c + np.array([dy, dx])), order=3, mode="nearest")
    return _u8(img), _u8(b)


def resized(img, h, w):
    return _u8(ndi.zoom(img.astype(np.float64), (h / img.shape[0], w / img.shape[1]), order=1))


def near_threshold(th):
    """a background translated by d = sqrt(2 th) full-size px on both axes: the half-size flow is about d/2 per axis, so the
    squared magnitude of the upsampled flow is about th, and the estimator's spread puts pixels on both sides of it"""
    d = np.sqrt(2 * th)
    return moving_patch(31, 480, 640, 0, 0, bdx=d, bdy=d)


CASES = {
    "patch_static_bg": lambda: moving_patch(1, 480, 640, 12, -7),
    "patch_moving_bg": lambda: moving_patch(2, 480, 640, -10, 6, bdx=2.5, bdy=-1.25),
    "photo_shift": lambda: shifted_photo(3.4, -1.7),
    "photo_affine": lambda: shifted_photo(1.0, 0.5, [[1.03, 0.02], [-0.02, 0.98]]),
    "odd_641x481": lambda: tuple(resized(x, 481, 641) for x in moving_patch(3, 480, 640, 9, 9, bdx=1.0)),
    "hd_1280x720": lambda: moving_patch(4, 720, 1280, 20, -14, bdx=-3.0, bdy=1.5),
    "small_128x96": lambda: moving_patch(5, 96, 128, 6, 3, bdx=0.7),
}
THS = {"patch_static_bg": [0.0, 64.0], "patch_moving_bg": [40.0, 400.0], "photo_shift": [64.0], "photo_affine": [0.0],
       "odd_641x481": [40.0], "hd_1280x720": [64.0, 400.0], "small_128x96": [0.0]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_compute_mask_bit_exact_stage_by_stage(case):
    a, b = CASES[case]()
    h, w = a.shape
    fl = Flow(max_width=w, max_height=h)
    of = FO.Flow()
    for th in THS[case]:
        fl.reset()
        of.reset()
        m0 = fl.compute_mask(a, th)
        assert np.array_equal(m0, of.compute_mask(a, th)) and m0.all()
        m1 = fl.compute_mask(b, th)
        om = of.compute_mask(b, th)
        check_stages(fl, of, a.shape, f"{case} th={th}")
        assert np.array_equal(m1, om)
    fl.close()


@pytest.mark.gpu
@pytest.mark.parametrize("th", [40.0, 64.0])
def test_flow_near_the_threshold(th):
    """a translation whose upsampled squared flow magnitude crosses th inside the frame: both sides of the >= edge"""
    a, b = near_threshold(th)
    fl, of = Flow(), FO.Flow()
    fl.compute_mask(a, th)
    of.compute_mask(a, th)
    m = fl.compute_mask(b, th)
    assert np.array_equal(m, of.compute_mask(b, th))
    check_stages(fl, of, a.shape, f"near th={th}")
    t = (of.taps["flow2"] ** 2).sum(-1)
    assert (t < th).any() and (t >= th).any()
    assert np.abs(t - th).min() < 0.05 * th   # pixels right at the edge exist


@pytest.mark.gpu
def test_device_sequence_equals_host_calls_across_calls_and_reset():
    import torch
    h, w = 240, 320
    seq = [synth_frame(40, h=h, w=w)]
    for i in range(1, 7):
        seq.append(_u8(ndi.shift(seq[0].astype(np.float64), (0.8 * i, -1.3 * i), order=3, mode="nearest")))
    seq[4] = moving_patch(41, h, w, 8, 5)[1]   # an abrupt change in the middle
    host = Flow(w, h)
    want = [host.compute_mask(f, 40.0) for f in seq]
    fl = Flow(w, h, max_batch=4)
    d = torch.from_numpy(np.stack(seq)).cuda()
    m1, o1 = fl.compute_masks(d[:3], 40.0)
    m2, o2 = fl.compute_masks(d[3:], 40.0)   # mask 3 comes from frame 2 (the previous call's last) and frame 3
    torch.cuda.synchronize()
    got = list(m1.cpu().numpy()) + list(m2.cpu().numpy())
    ones = list(o1.cpu().numpy()) + list(o2.cpu().numpy())
    for i, (g, e) in enumerate(zip(got, want)):
        assert np.array_equal(g, e), i
        assert ones[i] == int(e.sum()), i
    assert not got[4].all()
    fl.reset()
    m3, o3 = fl.compute_masks(d[4:6], 40.0)
    torch.cuda.synchronize()
    assert m3[0].cpu().numpy().all() and int(o3[0]) == w * h   # after reset: no previous frame
    host.reset()
    host.compute_mask(seq[4], 40.0)
    assert np.array_equal(m3[1].cpu().numpy(), host.compute_mask(seq[5], 40.0))
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_masks(d[:5], 40.0)   # more than max_batch
    assert e.value.status == _ffi.ORBFE_ERR_SIZE


@pytest.mark.gpu
def test_errors_and_state_after_a_size_mismatch():
    a, b = moving_patch(7, 240, 320, 6, 4)
    fl = Flow(640, 480)
    fl.compute_mask(a, 40.0)
    small = synth_frame(8, h=200, w=300)
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_mask(small, 40.0)
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_mask(synth_frame(9, h=480, w=642), 40.0)   # larger than max_width
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_mask(np.zeros((8, 8), np.uint8), 40.0)
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    of = FO.Flow()
    of.compute_mask(a, 40.0)
    assert np.array_equal(fl.compute_mask(b, 40.0), of.compute_mask(b, 40.0))   # the state survived the refused calls
    L = _ffi.lib()
    h = C.c_void_p()
    assert L.orbfe_flow_create(0, 640, 480, 0, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    buf = np.zeros(16, np.uint8)
    assert L.orbfe_flow_tap(fl.h, 0, FL.TAP_FLOW, 7, _ffi.ptr(buf), 16, None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_tap(fl.h, 0, FL.TAP_MASK, 0, _ffi.ptr(buf), 16, None, None) == _ffi.ORBFE_ERR_CAP
    fl.reset()
    fl.compute_mask(a, 40.0)
    assert L.orbfe_flow_tap(fl.h, 0, FL.TAP_FLOW, 0, _ffi.ptr(buf), 16, None, None) == _ffi.ORBFE_ERR_STATE
    fl.close()


@pytest.mark.gpu
def test_chain_extract_flow_mask_keypoints_equals_reference_masked_frame():
    """orbfe_extract_batch_device -> orbfe_flow_compute_masks_device -> orbfe_mask_keypoints_device, against the compiled
    reference's masked Frame constructor given the same frame and the oracle's mask: both sides of the 65 % rule, and a mask
    that removes every keypoint."""
    import torch
    from oracle import ref_ffi as R
    from orb_slam2_ssd_semantic_amd import ORBextractor
    R.configure(bump=True, canonical_trig=True, blur_mode=0)
    h, w = 480, 640
    a, b = moving_patch(50, h, w, 14, -9)                  # a moving patch: most of the mask is 1 -> filtered
    c = _u8(ndi.shift(b.astype(np.float64), (9, 13), order=3, mode="nearest"))   # the whole frame moves: mask mostly 0 -> kept
    frames = np.stack([a, b, c])
    B = len(frames)
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    st = torch.cuda.current_stream().cuda_stream
    d_gray = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    fl = Flow(w, h, max_batch=B)
    masks, ones = fl.compute_masks(d_gray, 40.0)
    FL.mask_keypoints(masks, ones, d_kps, d_desc, d_n, cap)
    torch.cuda.synchronize()
    of = FO.Flow()
    omasks = [of.compute_mask(f, 40.0) for f in frames]
    assert np.array_equal(masks.cpu().numpy(), np.stack(omasks))
    fracs = [m.mean() for m in omasks]
    assert fracs[0] == 1.0 and fracs[1] > 0.65 and fracs[1] < 1.0 and fracs[2] <= 0.65, fracs
    kk = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    dd = d_desc.cpu().numpy()
    nn = d_n.cpu().numpy()
    ref_ext = R.RefExtractor(1000, 1.2, 8, 20, 7)
    depth = np.ones((h, w), np.float32)
    for i in range(B):
        got = R.frame_ctor(R.FRAME_MASKED, frames[i], depth, omasks[i], extractor=ref_ext)
        n = int(nn[i])
        assert got["N"] == n, (i, got["N"], n)
        assert np.array_equal(kk[i, :n].view(np.uint8), got["keys"][:n].view(np.uint8))
        assert np.array_equal(dd[i, :n], got["desc"][:n])
        assert not kk[i, n:].view(np.uint8).any() and not dd[i, n:].any()   # freed slots zeroed again
    # a mask with a zero under every keypoint (and > 65 % ones): every keypoint goes
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    torch.cuda.synchronize()
    kk = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    n0 = d_n.cpu().numpy().copy()
    holes = np.ones((B, h, w), np.uint8)
    for i in range(B):
        k = kk[i, :n0[i]]
        holes[i, k["y"].astype(np.int32), k["x"].astype(np.int32)] = 0
    holes[2, :, :w // 2] = 0   # frame 2: 50 % ones -> nothing removed
    d_holes = torch.from_numpy(holes).cuda()
    d_ones = torch.from_numpy(holes.reshape(B, -1).sum(1).astype(np.int32)).cuda()
    FL.mask_keypoints(d_holes, d_ones, d_kps, d_desc, d_n, cap)
    torch.cuda.synchronize()
    n1 = d_n.cpu().numpy()
    assert n1[0] == 0 and n1[1] == 0 and n1[2] == n0[2], (n0, n1)
    assert not d_kps[:2].any() and not d_desc[:2].any()
