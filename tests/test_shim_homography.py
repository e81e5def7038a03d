"""shim/findHomography_orbfe.cc: Tracking::TrackHomo's `homo = findHomography(points_current, points_last, RANSAC, 3);` compiles
and links against the OpenCV-free stub (CPU), and on the GPU its H and mask equal tests/homography_oracle.py's."""
import os
import subprocess

import numpy as np
import pytest

import homography_cases as HC
import homography_oracle as HO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd", "shim")


def build(out):
    from orb_slam2_ssd_semantic_amd import _build
    lib = _build.build()
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", SHIM,
           os.path.join(ROOT, "tests", "cpp", "test_find_homography.cpp"), os.path.join(SHIM, "findHomography_orbfe.cc"),
           "-L", os.path.dirname(lib), "-lorbfe", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)]
    subprocess.check_call(cmd)
    return out


def test_track_homo_line_compiles_and_links(tmp_path):
    exe = build(tmp_path / "test_find_homography")
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "test_find_homography.cpp")).read()
    assert "homo = findHomography(points_current, points_last, RANSAC, 3);" in src
    # with real OpenCV the shim source is empty, so cv::findHomography cannot collide
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-DORBFE_WITH_OPENCV", "-I", os.path.join(ROOT, "include"), "-I",
                           SHIM, os.path.join(SHIM, "findHomography_orbfe.cc")])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ratio_0.5", "n_500", "collinear", "n_3"])
def test_track_homo_line_equals_oracle(tmp_path, case):
    exe = build(tmp_path / "test_find_homography")
    s, d, _ = HC.table(2048)[case]
    inp = tmp_path / "in.bin"
    out = tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([len(s)], np.int32).tofile(f)
        np.ascontiguousarray(s, np.float32).tofile(f)
        np.ascontiguousarray(d, np.float32).tofile(f)
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = open(out, "rb").read()
    empty = np.frombuffer(blob[:4], np.int32)[0]
    H = np.frombuffer(blob[4:76], np.float64)
    mask = np.frombuffer(blob[76:], np.uint8)
    oH, om = HO.find_homography(s, d, HO.RANSAC, 3)
    assert bool(empty) == (oH is None)
    if oH is not None:
        assert np.array_equal(H.view(np.uint64), oH.ravel().view(np.uint64))
    assert np.array_equal(mask, om)
