"""The C-ABI library loads and exports every symbol include/orbfe.h declares (no compute without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(orbfe_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported():
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    names = header_symbols()
    assert len(names) >= 25
    assert set(names) == set(_ffi.SYMBOLS), set(names) ^ set(_ffi.SYMBOLS)
    for n in names:
        assert getattr(L, n) is not None
    assert L.orbfe_version() == 100
    assert L.orbfe_strerror(0) == b"ok"
    assert b"no usable HIP device" in L.orbfe_strerror(-6)


def test_struct_layouts():
    from orb_slam2_ssd_semantic_amd import _ffi
    assert _ffi.KP_DTYPE.itemsize == 28  # cv::KeyPoint
    assert C.sizeof(_ffi.OrbfeParams) == 40
    assert [n for n in _ffi.KP_DTYPE.names] == ["x", "y", "size", "angle", "response", "octave", "class_id"]


def test_layouts_are_the_compilers(tmp_path):
    """Every struct of include/orbfe.h, as the binding derives it (ctypes.Structure class and numpy dtype), has the size and the
    member offsets the host C compiler gives it; the package's public mirrors are those records."""
    from orb_slam2_ssd_semantic_amd import _ffi, cloud, initializer, pnp, sim3
    structs = _ffi.ABI.structs
    header = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    assert sorted(structs) == sorted(re.findall(r"typedef struct (\w+) \{", header)) and len(structs) >= 30
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbfe.h"', 'int main(void) {']
    for name, cls in structs.items():
        src.append(f'printf("{name} %zu", sizeof({name}));')
        src += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in cls._fields_]
        src.append('printf("\\n");')
    (tmp_path / "layout.c").write_text("\n".join(src + ["return 0; }", ""]))
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe])
    seen = set()
    for line in subprocess.check_output([exe], text=True).splitlines():
        name, *want = line.split()
        want = [int(v) for v in want]
        cls, d = structs[name], _ffi.dtype(name)
        assert [f for f, _ in cls._fields_] == list(d.names)
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in d.names] == want, name
        assert [d.itemsize] + [d.fields[f][1] for f in d.names] == want, name
        seen.add(name)
    assert seen == set(structs)
    mirrors = {"orbfe_keypoint": _ffi.KP_DTYPE, "orbfe_proj_query": _ffi.PROJ_QUERY_DTYPE, "orbfe_track_proj": _ffi.TRACK_PROJ_DTYPE,
               "orbfe_sim3_model": sim3.MODEL_DTYPE, "orbfe_sim3_state": sim3.STATE_DTYPE, "orbfe_sim3_result": sim3.RESULT_DTYPE,
               "orbfe_sim3_set": sim3.SET_DTYPE, "orbfe_sim3_iter": sim3.ITER_DTYPE, "orbfe_pnp_params": pnp.PARAMS_DTYPE,
               "orbfe_pnp_state": pnp.STATE_DTYPE, "orbfe_pnp_result": pnp.RESULT_DTYPE, "orbfe_pnp_set": pnp.SET_DTYPE,
               "orbfe_pnp_iter": pnp.ITER_DTYPE, "orbfe_initializer_result": initializer.RESULT_DTYPE,
               "orbfe_initializer_pair": initializer.PAIR_DTYPE, "orbfe_initializer_iter": initializer.ITER_DTYPE,
               "orbfe_cloud_point": cloud.REC_DTYPE, "orbfe_object": cloud.OBJECT_DTYPE, "orbfe_filter_stat": cloud.FILTER_DTYPE,
               "orbfe_knn_plan": cloud.PLAN_DTYPE, "orbfe_cluster": cloud.CLUSTER_DTYPE}
    for name, m in mirrors.items():
        d = _ffi.dtype(name)
        assert (m.names, m.itemsize) == (d.names, d.itemsize), name
        for f in d.names:   # a mirror may only give a member another shape: same place, same scalar type, same bytes
            assert m.fields[f][1] == d.fields[f][1] and m.fields[f][0].itemsize == d.fields[f][0].itemsize, (name, f)
            assert m.fields[f][0].names or m.fields[f][0].base == d.fields[f][0].base, (name, f)
    for cls, name in zip((_ffi.OrbfeParams, _ffi.OrbfeCamera, _ffi.TrackCamera, _ffi.TrackFrames, _ffi.TrackLast, _ffi.TrackMap,
                          _ffi.TrackOut, _ffi.InitSearchFirst, _ffi.InitSearchOut), _ffi.BYREF):
        assert cls is structs[name]


def test_host_hamming_without_device(oracle):
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    rng = np.random.default_rng(0)
    for _ in range(100):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = rng.integers(0, 256, 32, dtype=np.uint8)
        assert ORBmatcher.DescriptorDistance(a, b) == oracle.hamming(a, b)


def test_no_cpu_fallback(have_gpu):
    """Without a GPU the product must fail loudly (ORBFE_ERR_NODEVICE), never compute on the CPU."""
    from orb_slam2_ssd_semantic_amd import ORBextractor, ORBmatcher, OrbfeError, _ffi
    if have_gpu:
        e = ORBextractor()
        assert e.capacity() >= 1000 + 16
        return
    for ctor in (ORBextractor, ORBmatcher):
        try:
            ctor()
        except OrbfeError as err:
            assert err.status == _ffi.ORBFE_ERR_NODEVICE
        else:
            raise AssertionError("constructed without a HIP device")


def test_bad_params_rejected():
    from orb_slam2_ssd_semantic_amd import _ffi
    L = _ffi.lib()
    h = C.c_void_p()
    bad = _ffi.OrbfeParams(1000, 1.2, 0, 20, 7, 640, 480, 1, -1, 0)  # nlevels = 0
    assert L.orbfe_create(C.byref(bad), C.byref(h)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_create(None, C.byref(h)) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_get_scales(None, None, None, None, None) == _ffi.ORBFE_ERR_ARG
    assert L.orbfe_extract(None, None, 0, 0, 0, None, None, 0, None) == _ffi.ORBFE_ERR_ARG


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: no file of the product package may reference it."""
    pkg = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd")
    for dp, _, files in os.walk(pkg):
        if os.path.basename(dp) == "build":
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".cc", ".inc")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "oracle_ffi" not in txt and "orb_oracle" not in txt and "liborb_oracle" not in txt, f
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f
