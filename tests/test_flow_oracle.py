"""CPU checks of tests/flow_oracle.py (the restated OpenCV path of FlowSLAM::Flow::ComputeMask) and of the library's host-side
constants.  The oracle is unpinned against real OpenCV; these tests are what keeps it honest: the integer stages equal
scipy.ndimage bit for bit, and the restated Farneback recovers known motion."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import flow_oracle as FO
from orb_slam2_ssd_semantic_amd.synth import synth_frame, synth_tum_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def photo(i=0):
    from orb_slam2_ssd_semantic_amd import photos
    return photos.vga_gray_frames(both_flags=False, jpeg=False)[i][1]


def moved(img, dx=0.0, dy=0.0, A=None):
    """img resampled so that content moves by (dx, dy) (plus the linear map A about the centre), cubic spline, rounded to u8"""
    a = img.astype(np.float64)
    if A is None:
        b = ndi.shift(a, (dy, dx), order=3, mode="nearest")
    else:
        h, w = a.shape
        c = np.array([h / 2.0, w / 2.0])
        Ainv = np.linalg.inv(np.asarray(A, np.float64))   # (row, col) order
        off = c - Ainv @ (c + np.array([dy, dx]))
        b = ndi.affine_transform(a, Ainv, offset=off, order=3, mode="nearest")
    return np.clip(np.round(b), 0, 255).astype(np.uint8)


# ---- scipy cross-checks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(480, 640), (96, 128), (240, 320), (60, 82)])
def test_pyr_down_equals_scipy_correlate(shape):
    rng = np.random.default_rng(shape[0])
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    full = ndi.correlate(img.astype(np.int64), np.outer(k, k), mode="mirror")
    ref = ((full[0::2, 0::2] + 128) >> 8).astype(np.uint8)
    assert np.array_equal(FO.pyr_down_u8(img), ref)
    assert np.array_equal(FO.pyr_down_u8(synth_frame(3)), (((ndi.correlate(synth_frame(3).astype(np.int64), np.outer(k, k), mode="mirror")
                                                            [0::2, 0::2]) + 128) >> 8).astype(np.uint8))


def _blobs(shape, seed, frac):
    rng = np.random.default_rng(seed)
    m = np.ones(shape, np.uint8)
    m[rng.random(shape) < frac] = 0
    m = ndi.binary_dilation(m == 0, iterations=2)
    return (~m).astype(np.uint8)


@pytest.mark.parametrize("seed,frac,shape", [(0, 0.002, (480, 640)), (1, 0.01, (481, 641)), (2, 0.0005, (96, 128)), (3, 0.05, (40, 37))])
def test_morphology_equals_scipy(seed, frac, shape):
    el = FO.ellipse21().astype(bool)
    m = _blobs(shape, seed, frac)
    m[:3, :] = 0   # zeros touching the border
    e = FO.erode(m)
    assert np.array_equal(e, ndi.grey_erosion(m, footprint=el, mode="constant", cval=255))
    d = FO.dilate(m)
    assert np.array_equal(d, ndi.grey_dilation(m, footprint=el, mode="constant", cval=0))
    full = FO.dilate(FO.erode(FO.erode(m)))
    ref = ndi.grey_dilation(ndi.grey_erosion(ndi.grey_erosion(m, footprint=el, mode="constant", cval=255), footprint=el, mode="constant",
                                             cval=255), footprint=el, mode="constant", cval=0)
    assert np.array_equal(full, ref)


# ---- KATs ---------------------------------------------------------------------------------------------------------------
def test_ellipse_element():
    el = FO.ellipse21()
    half = [(int(r.sum()) - 1) // 2 for r in el]
    assert tuple(half) == FO.ELLIPSE_HALF == (0, 4, 6, 7, 8, 9, 9, 10, 10, 10, 10, 10, 10, 10, 9, 9, 8, 7, 6, 4, 0)
    assert np.array_equal(el, el[::-1]) and np.array_equal(el, el[:, ::-1])
    for r in el:   # one centred run per row
        nz = np.nonzero(r)[0]
        assert nz[0] + nz[-1] == 20 and len(nz) == nz[-1] - nz[0] + 1


@pytest.mark.parametrize("w,h,sizes", [
    (640, 480, [(320, 240), (160, 120), (80, 60)]),
    (641, 481, [(320, 240), (160, 120), (80, 60)]),
    (1280, 720, [(640, 360), (320, 180), (160, 90), (80, 45)]),
    (128, 96, [(64, 48)]),
])
def test_level_plan(w, h, sizes):
    plan = FO.level_plan(w // 2, h // 2)[::-1]   # level 0 first
    assert [(p[0], p[1]) for p in plan] == sizes
    assert [p[3] for p in plan] == [3, 3, 9, 19][:len(sizes)]   # cvRound(2.5) = 2 -> 3; cvRound(7.5) = 8 -> 9; cvRound(17.5) = 18 -> 19
    assert np.array_equal(FO.gaussian_kernel(3, 0.0), np.array([0.25, 0.5, 0.25], np.float32))


def test_first_call_all_ones_threshold_clamp_and_odd_edges():
    f = FO.Flow()
    a = synth_tum_like(5, 97, 131)
    assert np.array_equal(f.compute_mask(a, 0.0), np.ones((97, 131), np.uint8))   # no previous frame
    assert f.last.shape == (48, 65)
    b = moved(a, 2.0, 0.0)
    f.compute_mask(b, 0.0)
    pre = f.taps["mask_pre"]
    t = (f.taps["flow2"] ** 2).sum(-1)
    assert f.taps["flow2"].shape == (96, 130, 2)
    assert pre[:, 130].all() and pre[96, :].all()   # outside pyrUp(flow): stays 1
    assert np.array_equal(pre[:96, :130] == 0, ~(t < np.float32(40.0)))   # th 0 clamps to 40
    g = FO.Flow()
    g.compute_mask(a, 40.0)
    g.compute_mask(b, 39.0)
    assert np.array_equal(g.taps["mask_pre"], pre)
    g.compute_mask(a, 40.0)
    h = FO.Flow()
    h.compute_mask(b, 1000.0)
    h.compute_mask(a, 41.0)
    assert not np.array_equal(g.taps["mask_pre"], h.taps["mask_pre"]) or (g.taps["flow2"] ** 2).sum(-1).max() < 40


def test_mask_rule():
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    k = np.zeros(4, KP_DTYPE)
    k["x"] = [1.9, 5.2, 7.99, 2.0]
    k["y"] = [0.5, 3.9, 9.0, 2.0]
    d = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    m = np.ones((10, 10), np.uint8)
    m[3, 5] = 0
    kk, dd = FO.mask_rule(m, k, d)
    assert list(kk["x"]) == list(k["x"][[0, 2, 3]]) and np.array_equal(dd, d[[0, 2, 3]])
    m[:4, :] = 0   # 60 % ones: not more than 65 %, everything kept
    kk, dd = FO.mask_rule(m, k, d)
    assert len(kk) == 4


# ---- motion recovery ----------------------------------------------------------------------------------------------------
# Interior (20 px away from the border of the 320 x 240 half-size frame) flow error against the true motion.  synth_frame is
# textured everywhere, so Farneback's local polynomial fit is well posed at every pixel: the median error must stay under
# 0.05 px and the 95th percentile under 0.1 px (measured: at most 0.027 / 0.061, the affine case).  The photograph has flat
# sky / wall regions where the fit is ill posed and the flow is whatever the coarser levels leave there, so only its median
# (< 0.1 px, measured at most 0.094) and 75th percentile (< 0.3 px, measured at most 0.24) are bounded.  A wrong sign, a
# swapped channel, a missing x2 between levels or a broken border table moves the median by more than 0.3 px.
CASES = [
    ("synth", 0.6, -0.4, None), ("synth", 2.0, 1.0, None), ("synth", -3.0, 0.0, None),
    ("synth", 0.0, 0.0, [[1.02, 0.01], [-0.01, 0.99]]),
    ("photo", 1.3, -0.6, None), ("photo", 2.0, 2.0, None), ("photo", 0.5, 0.0, [[1.0, 0.02], [-0.02, 1.0]]),
]


def _truth(shape, dx, dy, A):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if A is None:
        return np.full((h, w), dx), np.full((h, w), dy)
    A = np.asarray(A, np.float64)
    c = np.array([h / 2.0, w / 2.0])
    r, q = yy - c[0], xx - c[1]
    ny = A[0, 0] * r + A[0, 1] * q + c[0] + dy
    nx = A[1, 0] * r + A[1, 1] * q + c[1] + dx
    return nx - xx, ny - yy


@pytest.mark.parametrize("src,dx,dy,A", CASES)
def test_farneback_recovers_known_motion(src, dx, dy, A):
    img = synth_frame(11) if src == "synth" else photo(0)
    a = img
    b = moved(img, 2 * dx, 2 * dy, A)   # full-size motion; the half-size flow is half of it
    fl = FO.farneback(FO.pyr_down_u8(a), FO.pyr_down_u8(b))
    tx, ty = _truth(img.shape, 2 * dx, 2 * dy, A)
    tx, ty = tx[0::2, 0::2][:fl.shape[0], :fl.shape[1]] / 2, ty[0::2, 0::2][:fl.shape[0], :fl.shape[1]] / 2
    err = np.hypot(fl[..., 0] - tx, fl[..., 1] - ty)[20:-20, 20:-20]
    if src == "synth":
        assert np.median(err) < 0.05 and np.percentile(err, 95) < 0.1, (np.median(err), np.percentile(err, 95))
    else:
        assert np.median(err) < 0.1 and np.percentile(err, 75) < 0.3, (np.median(err), np.percentile(err, 75))


# ---- the library's host constants ---------------------------------------------------------------------------------------
def test_library_host_constants_equal_the_oracle_bit_for_bit():
    from orb_slam2_ssd_semantic_amd import flow
    g, xg, xxg, ig = flow.poly_constants()
    og, oxg, oxxg, oig = FO.prepare_gaussian()
    for a, b in ((g, og), (xg, oxg), (xxg, oxxg)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(np.array(ig).view(np.uint64), np.array(oig).view(np.uint64))
    for (w, h) in ((640, 480), (641, 481), (1280, 720), (128, 96), (300, 201), (1920, 1080)):
        lib = flow.plan(w, h)
        ora = FO.level_plan(w // 2, h // 2)[::-1]
        assert len(lib) == len(ora)
        for (lw, lh, ks, taps), (ow, oh, sigma, oks) in zip(lib, ora):
            assert (lw, lh, ks) == (ow, oh, oks)
            assert np.array_equal(taps.view(np.uint32), FO.gaussian_kernel(oks, sigma).view(np.uint32))


def test_flow_entry_points_reject_bad_arguments_without_a_device():
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    h = C.c_void_p()
    assert L.orbfe_flow_create(0, 8, 480, 1, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_create(0, 640, 480, 0, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_compute_mask(None, None, 640, 480, 640, 40.0, None, 640) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_plan(8, 8, None, None, None, None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_mask_keypoints_device(None, 640, 480, 640, 0, None, 1, None, None, None, 100, None) == _ffi.ORBFE_ERR_ARG


def test_flow_without_a_device_is_nodevice(have_gpu):
    from orb_slam2_ssd_semantic_amd import Flow, OrbfeError, _ffi
    if have_gpu:
        Flow().close()
        return
    with pytest.raises(OrbfeError) as e:
        Flow()
    assert e.value.status == _ffi.ORBFE_ERR_NODEVICE


def test_flow_shim_compiles_and_links(tmp_path):
    from orb_slam2_ssd_semantic_amd import _build
    lib = _build.build()
    shim = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd", "shim")
    main = tmp_path / "main.cpp"
    main.write_text('#include "Flow.h"\n'
                    'int main() {\n'
                    '    FlowSLAM::Flow f;\n'
                    '    cv::Mat g, m;\n'
                    '    f.ComputeMask(g, m, 40.f);   // empty frame: nothing happens, no device touched\n'
                    '    try { f.ComputeMask(g, g, m, 40.f); return 1; } catch (const std::exception &) {}\n'
                    '    return m.empty() ? 0 : 2;\n'
                    '}\n')
    exe = tmp_path / "flow_shim"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", shim, str(main),
                           os.path.join(shim, "Flow_orbfe.cc"), "-L", os.path.dirname(lib), "-lorbfe",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    hdr = open(os.path.join(shim, "Flow.h")).read()
    for s in ("namespace FlowSLAM", "class Flow", "void ComputeMask(const cv::Mat &GrayImg, cv::Mat &mask, float BInaryThreshold);",
              "void ComputeMask(const cv::Mat &GrayImg, const cv::Mat &Homo, cv::Mat &mask, float BInaryThreshold);"):
        assert s in hdr, s
