"""CPU checks of tests/warp_oracle.py (OpenCV 3.2's warpPerspective, restated for FlowSLAM::Flow::ComputeMask(GrayImg, Homo, ...))
and of the new homography entry points without a device.  The oracle is unpinned against real OpenCV; what keeps it honest here:
exact results where the answer is known (identity, integer shifts), the restated table against its closed form, the inverse
against numpy, a ±1 agreement with an independent float64 bilinear warp on smooth content, a planar scene realigned by its
homography, and masks that behave as the fork intends.  The last test shows that the GPU table reaches the warp's edges."""
import os
import subprocess

import numpy as np
import pytest

import flow_oracle as FO
import warp_cases as WC
import warp_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- exact answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(640, 480), (100, 17), (16, 16), (129, 96)])
def test_identity_is_an_exact_copy(w, h):
    g = WC.frame(w + h, w, h)
    assert np.array_equal(WO.warp(g, np.eye(3)), g)
    assert np.array_equal(WO.warp(g, np.eye(3, dtype=np.float32)), g)


@pytest.mark.parametrize("dx,dy", [(5, -3), (-7, 2), (0, 11), (63, 1), (-1, -1)])
def test_integer_translation_is_the_exact_shift_with_a_zero_border(dx, dy):
    h, w = 96, 129
    g = WC.frame(3, w, h)
    H = np.array([[1.0, 0, dx], [0, 1, dy], [0, 0, 1]])
    want = np.zeros_like(g)
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs - dx, ys - dy
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    want[ok] = g[sy[ok], sx[ok]]
    assert np.array_equal(WO.warp(g, H), want)


def test_table_equals_the_closed_form_and_sums_to_32768():
    """every entry but (0, 0) equals the closed form; (0, 0) is (32767, 0, 0, 1) (the short saturation plus the sum fix) and
    gives the closed form's output for every pair of pixel values, so the two tables are interchangeable for u8"""
    t = WO.inter_tab_linear().astype(np.int64)
    c = WO.closed_form_tab()
    assert t.shape == (1024, 4) and (t.sum(1) == 32768).all() and (c.sum(1) == 32768).all()
    assert np.array_equal(t[1:], c[1:])
    assert t[0].tolist() == [32767, 0, 0, 1] and c[0].tolist() == [32768, 0, 0, 0]
    v = np.arange(256, dtype=np.int64)
    v0, v3 = v[:, None], v[None, :]
    for v1 in (0, 255):
        for v2 in (0, 255):
            got = (v0 * t[0, 0] + v1 * t[0, 1] + v2 * t[0, 2] + v3 * t[0, 3] + 16384) >> 15
            want = (v0 * c[0, 0] + v1 * c[0, 1] + v2 * c[0, 2] + v3 * c[0, 3] + 16384) >> 15
            assert np.array_equal(got, want)


@pytest.mark.parametrize("name", [n for n in WC.H_NAMES if n != "singular"])
def test_inverse_matches_numpy(name):
    H = WC.homography(name, 640, 480)
    got = np.array(WO.invert3(WO.as_matrix(H))).reshape(3, 3)
    want = np.linalg.inv(np.asarray(H, np.float64))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_singular_matrix_inverts_to_zeros_and_fills_with_the_corner():
    H = WC.homography("singular", 64, 48)
    assert WO.invert3(WO.as_matrix(H)) == [0.0] * 9
    g = WC.frame(4, 64, 48)
    assert (WO.warp(g, H) == g[0, 0]).all()


def test_bad_matrices_and_frames_are_refused():
    g = WC.frame(5, 32, 32)
    for bad in (np.eye(3, dtype=np.uint8), np.eye(2), np.zeros((2, 3))):
        with pytest.raises(AssertionError):
            WO.warp(g, bad)
    with pytest.raises(AssertionError):
        WO.warp(np.zeros((0, 0), np.uint8), np.eye(3))


# ---- independent checks -----------------------------------------------------------------------------------------------------
def _float_bilinear_warp(src, H):
    """an independent warp: numpy's inverse, exact float64 source coordinates, float64 bilinear weights, rounded; NaN where a
    neighbour is outside the frame"""
    h, w = src.shape
    Mi = np.linalg.inv(np.asarray(H, np.float64))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    q = np.tensordot(Mi, np.stack([xs, ys, np.ones_like(xs)]), 1)
    X, Y = q[0] / q[2], q[1] / q[2]
    x0, y0 = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    fx, fy = X - x0, Y - y0
    ok = (x0 >= 0) & (x0 < w - 1) & (y0 >= 0) & (y0 < h - 1)
    xc, yc = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    s = src.astype(np.float64)
    v = (s[yc, xc] * (1 - fx) * (1 - fy) + s[yc, xc + 1] * fx * (1 - fy) + s[yc + 1, xc] * (1 - fx) * fy +
         s[yc + 1, xc + 1] * fx * fy)
    return np.where(ok, np.round(v), np.nan)


@pytest.mark.parametrize("name", ["subpixel_translation", "rotation_scale", "camera_plane", "float32_entries", "near_ties"])
def test_smooth_content_within_one_of_a_float_bilinear_warp(name):
    """on content whose gradient is at most 16 levels per pixel: the 1/32-pixel coordinates and 15-bit weights stay within ±1"""
    h, w = 240, 320
    canvas = WC.smooth_canvas(11, w, h, cell=16)
    g = np.clip(np.round(128 + 0.6 * (canvas[64:64 + h, 64:64 + w] - 128)), 0, 255).astype(np.uint8)
    gi = g.astype(np.int64)
    assert max(np.abs(np.diff(gi, axis=0)).max(), np.abs(np.diff(gi, axis=1)).max()) <= 16
    H = WC.homography(name, w, h)
    got = WO.warp(g, H).astype(np.float64)
    ref = _float_bilinear_warp(g, H)
    ok = ~np.isnan(ref)
    assert ok.mean() > 0.8
    assert np.abs(got[ok] - ref[ok]).max() <= 1


def test_planar_scene_is_realigned_by_its_homography():
    """frame 1 is the planar scene of frame 0 after a camera motion G; warping frame 1 with H = G^-1 (what findHomography of
    current -> last points estimates) gives frame 0 back, away from the borders"""
    h, w = 240, 320
    canvas = WC.smooth_canvas(12, w, h)
    G = WC.motion(w, h)
    f0, f1 = WC.view(canvas, np.eye(3), w, h), WC.view(canvas, G, w, h)
    back = WO.warp(f1, np.linalg.inv(G))
    inner = (slice(30, h - 30), slice(30, w - 30))
    d = np.abs(back[inner].astype(np.int64) - f0[inner])
    assert d.max() <= 4 and d.mean() < 0.5, (d.max(), d.mean())   # cubic-spline views, bilinear warp
    assert np.abs(f1[inner].astype(np.int64) - f0[inner]).mean() > 10   # the motion itself is large


# ---- the masks ----------------------------------------------------------------------------------------------------------------
def _inner(a, m=40):
    return a[m:-m, m:-m]


def test_first_warped_pair_after_an_unwarped_frame_masks_only_the_moving_patch():
    h, w = 480, 640
    canvas = WC.smooth_canvas(21, w, h)
    patch = np.round(WC.smooth_canvas(22, 128, 128)[:128, :128]).astype(np.uint8)
    G = WC.motion(w, h)
    x0, y0 = 240, 160
    a = WC.with_patch(WC.view(canvas, np.eye(3), w, h), patch, x0, y0)
    b = WC.with_patch(WC.view(canvas, G, w, h), patch, x0 + 14, y0 + 10)   # the camera moves by G, the patch by its own motion
    fw, fp = FO.Flow(), FO.Flow()
    assert fw.compute_mask(a, 40.0).all() and fp.compute_mask(a, 40.0).all()
    mw = WO.compute_mask_homo(fw, b, np.linalg.inv(G), 40.0)
    mp = fp.compute_mask(b, 40.0)
    assert np.array_equal(fw.last, FO.pyr_down_u8(WO.warp(b, np.linalg.inv(G))))   # the state: the warped frame's half
    near = np.zeros((h, w), bool)
    near[y0 - 40:y0 + 128 + 60, x0 - 40:x0 + 128 + 40] = True     # the patch in both frames, the morphology's reach around it
    zw = _inner(mw == 0)
    assert zw[_inner(near)].mean() > 0.3                            # the patch is masked
    assert zw[~_inner(near)].mean() < 0.01                          # and essentially nothing else
    assert _inner(mp == 0).mean() > 0.9                             # unwarped, the camera motion masks most of the frame


def test_steady_motion_is_compensated_only_on_the_first_warped_pair():
    """Flow.cc:79 -> :51: the state becomes the warped frame's half-size image, so under steady camera motion the second warped
    pair compares warp(F1) ~ F0 with warp(F2) ~ F1: the motion is back (the reference's behaviour, reproduced)"""
    h, w = 240, 320
    frames, Hs = WC.planar_sequence(31, 3, w, h, k=1.0)
    of, op = FO.Flow(), FO.Flow()
    of.compute_mask(frames[0], 40.0)
    m1 = WO.compute_mask_homo(of, frames[1], Hs[1], 40.0)
    m2 = WO.compute_mask_homo(of, frames[2], Hs[2], 40.0)
    op.compute_mask(frames[0], 40.0)
    p1 = op.compute_mask(frames[1], 40.0)
    assert _inner(m1 == 0).mean() < 0.01
    assert _inner(m2 == 0).mean() > 0.6 and _inner(p1 == 0).mean() > 0.6


# ---- the GPU table's reach ----------------------------------------------------------------------------------------------------
def test_gpu_table_reaches_the_warp_edges():
    """what tests/test_gpu_flow_homo.py's table reaches, from the oracle: the block split changes output pixels (so a kernel that
    computes M0*x in one step fails), W < 0, the INT clamp, short saturation, all three border cases, tx and ty at 0 and 31,
    and both the one-block (w < 64) and multi-block frames"""
    seen = set()
    for w, h in WC.SIZES:
        for name in WC.H_NAMES:
            H = WC.homography(name, w, h)
            g = WC.frame(1, w, h)
            sx, sy, alpha, X, Y, Wr = WO.coordinates(WO.invert3(WO.as_matrix(H)), w, h)
            if (WO.warp(g, H) != WO.warp(g, H, split=False)).any():
                seen.add(("split", w > 64))
            if (Wr < 0).any():
                seen.add("w<0")
            if (np.abs(X) == 2 ** 31 - 1).any() or (X == -2 ** 31).any() or (np.abs(Y) == 2 ** 31 - 1).any() or (Y == -2 ** 31).any():
                seen.add("int clamp")
            if ((X >> 5) != sx).any() and ((Y >> 5) != sy).any():
                seen.add("short")
            for c in np.unique(WO.border_case(sx, sy, w, h)):
                seen.add(("border", int(c)))
            for t, nm in ((alpha & 31, "tx"), (alpha >> 5, "ty")):
                for v in (0, 31):
                    if (t == v).any():
                        seen.add((nm, v))
            seen.add(("blocks", -(-w // WO.block_size(w, h)[0])))
    want = {("split", True), "w<0", "int clamp", "short", ("border", 0), ("border", 1), ("border", 2), ("tx", 0), ("tx", 31),
            ("ty", 0), ("ty", 31), ("blocks", 1)}
    assert want <= seen, want - seen
    assert max(n for k, n in (s for s in seen if isinstance(s, tuple) and s[0] == "blocks")) >= 10


# ---- the entry points and the shim without a device ---------------------------------------------------------------------------
def test_homo_entry_points_reject_bad_arguments_without_a_device():
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    H = np.eye(3)
    g = np.zeros((480, 640), np.uint8)
    assert L.orbfe_flow_compute_mask_homo(None, _ffi.ptr(g), 640, 480, 640, _ffi.ptr(H), 40.0, _ffi.ptr(g), 640) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_compute_mask_homo(None, _ffi.ptr(g), 640, 480, 640, None, 40.0, _ffi.ptr(g), 640) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_flow_compute_masks_homo_device(None, None, 1, 640, 480, 640, 0, None, None, 40.0, None, 640, 0, None,
                                                  None) == _ffi.ORBFE_ERR_ARG


def test_python_tap_names():
    from orb_slam2_ssd_semantic_amd import flow as FL
    assert FL.TAP_WARP == 6 and FL.TAP_POLY == 5


def test_flow_shim_homography_overload_reaches_the_library(tmp_path, have_gpu):
    """the homography overload built against the stub: warpPerspective's assertions throw before any device is touched, and a
    3x3 CV_64F / CV_32F matrix reaches orbfe_flow_* (without a device: the handle's NODEVICE error, not a missing-OpenCV one)"""
    from orb_slam2_ssd_semantic_amd import _build
    lib = _build.build()
    shim = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd", "shim")
    main = tmp_path / "main.cpp"
    main.write_text('#include <cstdio>\n#include <string>\n#include "Flow.h"\n'
                    'static std::string run(FlowSLAM::Flow &f, const cv::Mat &g, const cv::Mat &H, cv::Mat &m) {\n'
                    '    try { f.ComputeMask(g, H, m, 40.f); return "ok"; } catch (const std::exception &e) { return e.what(); }\n'
                    '}\n'
                    'int main() {\n'
                    '    FlowSLAM::Flow f;\n'
                    '    cv::Mat g(48, 64, CV_8U), empty, m, h8(3, 3, CV_8U), h23(2, 3, CV_64F), h64(3, 3, CV_64F), h32(3, 3, CV_32F);\n'
                    '    for (int r = 0; r < 48; r++) for (int c = 0; c < 64; c++) g.ptr(r)[c] = (uint8_t)(r * 5 + c * 3);\n'
                    '    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) {\n'
                    '        h64.at<double>(r, c) = r == c; h32.at<float>(r, c) = r == c; h8.ptr(r)[c] = r == c; }\n'
                    '    printf("empty|%s\\n", run(f, empty, h64, m).c_str());\n'
                    '    printf("u8|%s\\n", run(f, g, h8, m).c_str());\n'
                    '    printf("2x3|%s\\n", run(f, g, h23, m).c_str());\n'
                    '    printf("untouched|%d\\n", (int)m.empty());\n'
                    '    printf("f64|%s\\n", run(f, g, h64, m).c_str());\n'
                    '    printf("f32|%s\\n", run(f, g, h32, m).c_str());\n'
                    '    printf("mask|%d %d %d\\n", m.rows, m.cols, m.empty() ? -1 : (int)m.ptr(47)[63]);\n'
                    '    return 0;\n'
                    '}\n')
    exe = tmp_path / "flow_shim_homo"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", shim, str(main),
                           os.path.join(shim, "Flow_orbfe.cc"), "-L", os.path.dirname(lib), "-lorbfe",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    r = subprocess.run([str(exe)], timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = dict(line.split("|", 1) for line in r.stdout.splitlines())
    assert "empty frame" in out["empty"]
    assert "3x3 CV_32F or CV_64F" in out["u8"] and "3x3 CV_32F or CV_64F" in out["2x3"]
    assert out["untouched"] == "1"
    for k in ("f64", "f32"):
        assert "warpPerspective" not in out[k] and "OPENCV" not in out[k]
        if have_gpu:
            assert out[k] == "ok", out[k]
        else:
            assert "orbfe_flow_create" in out[k], out[k]
    if have_gpu:
        assert out["mask"] == "48 64 1"   # the first frame's mask: all ones
