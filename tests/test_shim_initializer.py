"""shim/Initializer_orbfe.cc: Tracking::MonocularInitialization's call sequence -- Initializer(frame 1, 1.0, 200), Initialize on
frames 2 and 3 -- on mock frames compiles and links without OpenCV (CPU), and on the GPU its results equal the ones the Python
oracle recorded in tests/golden/initializer_shim.npz (draws from rand() after srand(0), 1600 per call)."""
import os
import subprocess

import numpy as np
import pytest

import initializer_shim_case as IS
from oracle import ref_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd", "shim")
REFBUILD = os.path.join(ROOT, "oracle", "refbuild")
# the mock Frame of the matcher shim tests, force-included in place of the reference's Frame.h
MOCKS = ["-std=gnu++14", "-DORBFE_WITH_OPENCV", "-I", os.path.join(REFBUILD, "shimhdr_ext"), "-I", os.path.join(REFBUILD, "cvstub"),
         "-include", os.path.join(REFBUILD, "ref_mocks.h"), "-DMAPPOINT_H", "-DKEYFRAME_H", "-DFRAME_H", "-I", os.path.join(ROOT, "include")]
STANDIN = ["-I", os.path.join(ROOT, "tests", "cpp", "initializer_mock")]


def build(out):
    from orb_slam2_ssd_semantic_amd import _build
    lib = _build.build()
    obj = str(out) + "_shim.o"
    subprocess.check_call(["g++", "-O1", "-Wall", "-Wno-reorder", "-DREF_MOCKS_STRICT", *MOCKS, *STANDIN, "-c",
                           os.path.join(SHIM, "Initializer_orbfe.cc"), "-o", obj])
    subprocess.check_call(["g++", "-O1", "-Wall", *MOCKS, *STANDIN, os.path.join(ROOT, "tests", "cpp", "test_initializer.cpp"), obj,
                           "-L", os.path.dirname(lib), "-lorbfe", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-pthread",
                           "-o", str(out)])
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype.itemsize == 4 else a, b.view(np.uint32) if b.dtype.itemsize == 4 else b)


def test_shim_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path / "test_initializer"))
    src = open(os.path.join(ROOT, "tests", "cpp", "test_initializer.cpp")).read()
    assert "new Initializer(*frames[0], 1.0, 200)" in src and "->Initialize(*frames[f], matches[f], Rcw, tcw, mvIniP3D, vbTriangulated)" in src
    ref_include = os.path.join(ref_ffi.REFERENCE, "include")
    if os.path.exists(os.path.join(ref_include, "Initializer.h")):   # under the reference's own header, where it is at hand
        subprocess.check_call(["g++", "-fsyntax-only", "-Wall", "-Wno-reorder", "-DREF_MOCKS_STRICT", *MOCKS, "-I", ref_include,
                               os.path.join(SHIM, "Initializer_orbfe.cc")])


def test_fixture_is_the_oracles_replay():
    g = np.load(IS.GOLDEN)
    want = IS.pack(IS.replay())
    assert sorted(g.files) == ["head", "model", "points", "triangulated"]
    assert np.array_equal(g["head"], want["head"]) and same(g["model"], want["model"]) and same(g["points"], want["points"])
    assert np.array_equal(g["triangulated"], want["triangulated"])
    assert g["head"].tolist() == [[0, 1, 0], [1, 0, 150]]   # too little parallax on frame 2, a map from frame 3
    assert g["triangulated"].sum() == 120
    # the second call's sets come from the next 1600 draws, not from the first
    s = IS.rand_stream(0, 3200)
    assert not np.array_equal(s[:1600], s[1600:])


@pytest.mark.gpu
def test_shim_sequence_equals_fixture(tmp_path):
    exe = build(tmp_path / "test_initializer")
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    IS.write_input(inp)
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = IS.pack(IS.parse_output(open(out, "rb").read()))
    g = np.load(IS.GOLDEN)
    assert np.array_equal(got["head"], g["head"]), (got["head"].tolist(), g["head"].tolist())
    assert same(got["model"], g["model"]) and same(got["points"], g["points"]) and np.array_equal(got["triangulated"], g["triangulated"])
