"""The extractor's launch plan (csrc/orbfe_plan.hip) without a GPU, through the test hook orbfe_internal_plan_table.

(a) byte identity: the tables of every case of the matrix hash to tests/golden/plan_digests.json, recorded from the release
    planner of the last commit that carried the fused kernel variants (profiles/HISTORY.md), its plan table re-packed field by
    field without the fields that went with them; the -DORBFE_DEVELOPER build gives the same tables;
(b) the contracts the FAST, blur and pyramid kernels rely on, checked on the tables themselves;
(c) the planner's errors: status and text;
(d) the planner alone under AddressSanitizer / UBSan (tests/cpp/test_plan_sanitize.cpp, a child process).

The matrix: the shapes and run lengths of tests/test_gpu_launch_options.py (imported, not copied); max_batch 1 / 8 / 9 (default
runs of 8 / 16 / 40 rows); rows 512; blur_pieces x blur_updown.  max_batch only chooses the default run length,
so it is crossed with the options that leave the run length to it; an explicit ROWS_FAST / ROWS_BLUR value is taken at 9."""
import ctypes as C
import hashlib
import json
import os
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd import _ffi
from test_gpu_launch_options import EDGE, ROWS_BLUR, ROWS_FAST, SHAPES, default_rows, fast_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
TABLES = ("plan", "cells", "tabs", "flanes", "clanes", "blanes", "fast_row_steps")
KNOBS = ("rows", "rows_fast", "rows_blur", "blur_pieces", "blur_updown", "debug")
DEFAULT = dict(rows=0, rows_fast=0, rows_blur=0, blur_pieces=1, blur_updown=1, debug=0)
BLUR_LAYOUTS = [dict(blur_pieces=p, blur_updown=u) for p in (0, 1) for u in (0, 1, 2)]


@lru_cache(maxsize=None)
def cases():
    """[(max_batch, knob dict)], the same list for every shape"""
    out = []
    for mb in (1, 8, 9):
        out.append((mb, dict(DEFAULT, rows=512)))
        out += [(mb, dict(DEFAULT, **lay)) for lay in BLUR_LAYOUTS]   # holds the all-default case
    out += [(9, dict(DEFAULT, rows_fast=r)) for r in ROWS_FAST]
    out += [(9, dict(DEFAULT, rows_blur=r, **lay)) for r in ROWS_BLUR for lay in BLUR_LAYOUTS]
    return out


def case_line(shape, mb, knobs, ini=20, mn=7):
    """a case as the stand-alone programs read it"""
    w, h, nl, sf, nf = SHAPES[shape]
    return " ".join(map(str, [nf, sf, nl, w, h, mb, ini, mn] + [knobs[k] for k in KNOBS]))


# ---- the tables --------------------------------------------------------------------------------------------------------------
LANE = np.dtype([("x", "<u2"), ("ys", "<u2"), ("nrows", "<u2"), ("flags", "<u2")])
TAB = np.dtype([("c0", "<i2"), ("c1", "<i2"), ("s", "<i2"), ("pad", "<i2")])
_i = "<i4"
LEVEL = np.dtype([(n, _i) for n in ("w", "h", "pitch", "off", "ncols", "nrows", "wcell", "hcell", "cell0", "ncells", "ncc", "nfeat", "nini")] +
                 [("hx", "<f4")] + [(n, _i) for n in ("key_off", "key_cap", "sel_off", "sel_cap", "xtab", "ytab")] +
                 [("scale", "<f4"), ("patch_size", "<f4"), ("root_x", _i, 9), ("ix1", _i), ("iy1", _i)])
PLAN = np.dtype([(n, _i) for n in ("nlevels", "w", "h", "ncells", "cell_cap", "max_ncells", "keys_per_frame", "sel_per_frame", "node_cap",
                                   "max_nini", "ini_th", "min_th", "blur_rounding", "dbg", "nfwaves", "nfwaves_c", "fast_cellrows")] +
                [("fwave_off", _i, 17), ("nbwaves", _i), ("bwave_off", _i, 17), ("pyr_frame_bytes", "<i8"),
                 ("lv", LEVEL, 16), ("blur_wt", "<u4", (16, 4, 12))])


def hook(L):
    f = L.orbfe_internal_plan_table
    f.argtypes = [C.POINTER(_ffi.OrbfeParams), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                  C.POINTER(C.c_size_t)]
    f.restype = C.c_int32
    return f


_BUF = C.create_string_buffer(8 << 20)


def params(shape, mb, ini=20, mn=7, **kw):
    w, h, nl, sf, nf = SHAPES[shape]
    d = dict(nfeatures=nf, scale_factor=sf, nlevels=nl, ini_th_fast=ini, min_th_fast=mn, max_width=w, max_height=h, max_batch=mb,
             device=-1, blur_rounding=0)
    d.update(kw)
    return _ffi.OrbfeParams(**d)


def table(L, p, knobs, w, h, which):
    """(status, bytes) of one table"""
    n = C.c_size_t(0)
    s = hook(L)(C.byref(p), (C.c_int32 * 6)(*[knobs[k] for k in KNOBS]), w, h, which, _BUF, len(_BUF), C.byref(n))
    return s, C.string_at(_BUF, n.value) if s == 0 else b""


def tables(L, shape, mb, knobs):
    w, h = SHAPES[shape][:2]
    p = params(shape, mb)
    out = []
    for which in range(len(TABLES)):
        s, b = table(L, p, knobs, w, h, which)
        assert s == 0, (shape, mb, knobs, which, L.orbfe_last_error())
        out.append(b)
    return out


class Plan:
    """the tables of one case as arrays"""

    def __init__(self, L, shape, mb, knobs):
        raw = tables(L, shape, mb, knobs)
        assert len(raw[0]) == PLAN.itemsize
        self.P = np.frombuffer(raw[0], PLAN)[0]
        self.nl = int(self.P["nlevels"])
        self.lv = self.P["lv"][:self.nl]
        self.tabs = np.frombuffer(raw[2], TAB)
        self.flanes, self.clanes, self.blanes = (np.frombuffer(raw[k], LANE) for k in (3, 4, 5))
        self.fast_row_steps = int(np.frombuffer(raw[6], "<i8")[0])


# ---- (a) byte identity -------------------------------------------------------------------------------------------------------
def digests(fetch):
    """{shape: {table: sha256 over the table's bytes of every case, in the order of cases(), each prefixed with its length}};
    fetch(shape, max_batch, knobs) -> the tables"""
    out = {}
    for shape in SHAPES:
        hs = [hashlib.sha256() for _ in TABLES]
        for mb, knobs in cases():
            for hsh, b in zip(hs, fetch(shape, mb, knobs)):
                hsh.update(len(b).to_bytes(8, "little"))
                hsh.update(b)
        out[shape] = {t: hsh.hexdigest() for t, hsh in zip(TABLES, hs)}
    return out


def check_digests(L):
    want = json.load(open(GOLDEN))["release"]
    got = digests(lambda shape, mb, knobs: tables(L, shape, mb, knobs))
    bad = [(s, t) for s in SHAPES for t in TABLES if got[s][t] != want[s][t]]
    assert not bad, bad


def test_tables_are_byte_identical_release():
    check_digests(_ffi.lib())


def test_tables_are_byte_identical_developer(dev_lib):
    """the developer build plans exactly what the release build plans"""
    check_digests(dev_lib)


def test_sizing_call_and_capacity():
    L = _ffi.lib()
    p, n = params("tiny", 1), C.c_size_t(0)
    k = (C.c_int32 * 6)(*[DEFAULT[x] for x in KNOBS])
    for which in range(len(TABLES)):
        assert hook(L)(C.byref(p), k, 209, 155, which, None, 0, C.byref(n)) == 0
        s, b = table(L, p, DEFAULT, 209, 155, which)
        assert s == 0 and len(b) == n.value > 0
        assert hook(L)(C.byref(p), k, 209, 155, which, _BUF, n.value - 1, C.byref(n)) == _ffi.ORBFE_ERR_CAP
    assert hook(L)(C.byref(p), k, 209, 155, len(TABLES), None, 0, C.byref(n)) == _ffi.ORBFE_ERR_ARG
    assert hook(L)(C.byref(p), k, 0, 155, 0, None, 0, C.byref(n)) == _ffi.ORBFE_ERR_ARG


# ---- (b) what the kernels rely on ---------------------------------------------------------------------------------------------
def levels_of_waves(lanes, what):
    """per wave its level; every wave is single-level"""
    lv = (lanes["flags"] >> 8).reshape(-1, 64)
    assert (lv == lv[:, :1]).all(), what
    return lv[:, 0]


def assert_fast_coverage(pl, lanes, what):
    """the non-halo lanes cover each (level, column x = 16, 20, ... < ix1, row in [19, iy1)) exactly once"""
    live = lanes[(lanes["flags"] & 1) == 0]
    lvl = live["flags"] >> 8
    for l, L in enumerate(pl.lv):
        ncol = (int(L["ix1"]) - 16 + 3) // 4
        m = live[lvl == l]
        assert ((m["x"] >= 16) & (m["x"] % 4 == 0) & ((m["x"] - 16) // 4 < ncol)).all(), (what, l)
        assert ((m["ys"] >= EDGE) & (m["nrows"] > 0) & (m["ys"].astype(int) + m["nrows"] <= L["iy1"])).all(), (what, l)
        d = np.zeros((max(ncol, 1), int(L["iy1"]) + 1), np.int32)
        ci = (m["x"].astype(int) - 16) // 4
        np.add.at(d, (ci, m["ys"].astype(int)), 1)
        np.add.at(d, (ci, m["ys"].astype(int) + m["nrows"]), -1)
        cov = np.cumsum(d, axis=1)[:ncol, :int(L["iy1"])]
        assert (cov[:, EDGE:] == 1).all() and (cov[:, :EDGE] == 0).all(), (what, l)


def check_dense(pl, shape, rows_fast):
    P, f = pl.P, pl.flanes
    assert len(f) == 64 * P["nfwaves"]
    wl = levels_of_waves(f, "dense")
    off = P["fwave_off"]
    assert off[0] == 0 and (np.diff(off) >= 0).all() and (off[pl.nl:] == P["nfwaves"]).all()
    for l in range(pl.nl):
        assert (wl[off[l]:off[l + 1]] == l).all(), l
    assert_fast_coverage(pl, f, "dense")
    # halo rules: the neighbour columns of a non-halo lane sit next to it in its wave
    x, ys, nr = f["x"].astype(int), f["ys"].astype(int), f["nrows"].astype(int)
    slot = np.arange(len(f)) % 64
    live = (f["flags"] & 1) == 0
    ix1 = pl.lv["ix1"][f["flags"] >> 8]
    left, right = live & (x > 16), live & (x + 4 < ix1)
    assert (slot[left] > 0).all() and (slot[right] < 63).all()
    il, ir = np.flatnonzero(left), np.flatnonzero(right)
    assert ((x[il - 1] == x[il] - 4) & (ys[il - 1] == ys[il]) & (nr[il - 1] == nr[il])).all()
    assert ((x[ir + 1] == x[ir] + 4) & (ys[ir + 1] == ys[ir]) & (nr[ir + 1] == nr[ir])).all()
    assert P["fast_cellrows"] == (rows_fast >= 24)
    if P["fast_cellrows"]:   # one run length per wave, dead lanes included; runs start on a cell row
        n64 = f["nrows"].reshape(-1, 64)
        assert (n64 == n64[:, :1]).all()
        assert ((ys[live] - EDGE) % pl.lv["hcell"][f["flags"][live] >> 8] == 0).all()
    assert (pl.fast_row_steps, int(P["nfwaves"])) == fast_work(shape, rows_fast)


def check_compacting(pl):
    c = pl.clanes
    assert len(c) == 64 * pl.P["nfwaves_c"]
    levels_of_waves(c, "compacting")
    assert_fast_coverage(pl, c, "compacting")
    # every maximal run of non-halo lanes: step 4 in x, one ys, a halo lane at x - 4 before and one at x + 4 behind it
    x, ys = c["x"].astype(int), c["ys"].astype(int)
    live = ((c["flags"] & 1) == 0).reshape(-1, 64)
    assert not live[:, 0].any() and not live[:, 63].any()
    live = live.ravel()
    inner = np.flatnonzero(live[1:] & live[:-1]) + 1     # a live lane behind a live lane
    assert ((x[inner] == x[inner - 1] + 4) & (ys[inner] == ys[inner - 1])).all()
    first = np.flatnonzero(live[1:] & ~live[:-1]) + 1
    last = np.flatnonzero(live[:-1] & ~live[1:])
    assert ((x[first - 1] == x[first] - 4) & (ys[first - 1] == ys[first])).all()
    assert ((x[last + 1] == x[last] + 4) & (ys[last + 1] == ys[last])).all()


def assert_rows_once(idx, r0, n, ncol, nrow, what):
    """the row ranges [r0, r0 + n) of columns idx cover an ncol x nrow grid exactly once"""
    assert ((idx >= 0) & (idx < ncol) & (r0 >= 0) & (r0 + n <= nrow)).all(), what
    d = np.zeros((ncol, nrow + 1), np.int32)
    np.add.at(d, (idx, r0), 1)
    np.add.at(d, (idx, r0 + n), -1)
    assert (np.cumsum(d, axis=1)[:, :nrow] == 1).all(), what


def check_blur(pl):
    P, b = pl.P, pl.blanes
    assert len(b) == 64 * P["nbwaves"]
    wl = levels_of_waves(b, "blur")
    off = P["bwave_off"]
    assert off[0] == 0 and off[pl.nl] == P["nbwaves"] and (np.diff(off[:pl.nl + 1]) >= 0).all()
    for l in range(pl.nl):
        assert (wl[off[l]:off[l + 1]] == l).all(), l
    fl = b["flags"].astype(int)
    kind = (fl & 0xE).reshape(-1, 64)
    assert (kind == kind[:, :1]).all()      # a wave is uniform in flag bits 1, 2 and 3
    assert not (fl & 4).any()               # (bit 2 is not in use)
    lvl = fl >> 8
    x, ys, nr = b["x"].astype(int), b["ys"].astype(int), b["nrows"].astype(int)
    inner = (fl & 2) != 0
    assert ((x[inner] >= 4) & (x[inner] + 8 <= pl.lv["w"][lvl[inner]])).all()   # the window [x - 4, x + 8) lies inside the row
    blur = (fl & 1) == 0        # not dead
    for l, L in enumerate(pl.lv):
        m = blur & (lvl == l)
        assert (x[m] % 4 == 0).all()
        assert_rows_once(x[m] // 4, ys[m], nr[m], (int(L["w"]) + 3) // 4, int(L["h"]), ("blur", l))
    # the 12 weight bytes of every (level, lane type, output pixel) are the 7 taps of the kernel
    wt = np.ascontiguousarray(P["blur_wt"][:pl.nl]).view(np.uint8).reshape(pl.nl, 4, 4, 12)
    assert (wt.sum(axis=3) == 257).all()
    assert not P["blur_wt"][pl.nl:].any()


def check_taps(pl):
    t = pl.tabs
    for l in range(1, pl.nl):
        L, S = pl.lv[l], pl.lv[l - 1]
        for at, n, src, is_x in ((int(L["xtab"]), int(L["w"]), int(S["w"]), True), (int(L["ytab"]), int(L["h"]), int(S["h"]), False)):
            assert at % 4 == 0
            e = t[at:at + n]
            assert (e["c0"].astype(int) + e["c1"] == 2048).all(), (l, is_x)
            if is_x:
                assert ((e["s"] >= 0) & (e["s"] <= src - 1)).all(), l
            else:
                assert (np.diff(e["s"].astype(int)) > 0).all() and e["s"][0] >= 0 and e["s"][-1] <= src - 1, l
            assert (t[at + n:at + n + 8] == e[-1]).all(), (l, is_x)


def effective(knob, rows, mb):
    return knob if knob else (rows if rows else default_rows(mb))


@pytest.mark.parametrize("shape", SHAPES)
def test_fast_lane_lists(oracle, shape):
    """dense and lane-compacting FAST lists and the tap tables, for every case that shapes them"""
    L, seen = _ffi.lib(), set()
    for mb, k in cases():
        rf = effective(k["rows_fast"], k["rows"], mb)
        if rf in seen:
            continue
        seen.add(rf)
        pl = Plan(L, shape, mb, k)
        check_dense(pl, shape, rf)
        check_compacting(pl)
        check_taps(pl)
    assert seen >= set(ROWS_FAST) | {16, 512}


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_lane_list(shape):
    """the blur lane list in its layouts and the folded weights, for every case that shapes them"""
    L, seen = _ffi.lib(), set()
    for mb, k in cases():
        key = (effective(k["rows_blur"], k["rows"], mb), k["blur_pieces"], k["blur_updown"])
        if key in seen:
            continue
        seen.add(key)
        check_blur(Plan(L, shape, mb, k))
    assert seen >= {(r, lay["blur_pieces"], lay["blur_updown"]) for r in ROWS_BLUR + (16, 40) for lay in BLUR_LAYOUTS}


def test_updown_split_keeps_the_wave_count(oracle):
    """blur_updown 1 splits a (level, pass) into up and down waves only where that costs no wave: never more waves than 0"""
    L = _ffi.lib()
    for shape in SHAPES:
        n = [int(Plan(L, shape, 9, dict(DEFAULT, blur_updown=u)).P["nbwaves"]) for u in (0, 1, 2)]
        assert n[0] == n[1] <= n[2], (shape, n)


# ---- (c) errors ----------------------------------------------------------------------------------------------------------------
ERRORS = [   # (params, status, text)
    (dict(nfeatures=1000, scale_factor=1.2, nlevels=8, max_width=160, max_height=120), _ffi.ORBFE_ERR_SIZE,
     "level 4 (77x58) is smaller than one 30-px FAST cell plus borders"),
    (dict(nfeatures=1000, scale_factor=2.5, nlevels=8, max_width=640, max_height=480), _ffi.ORBFE_ERR_ARG,
     "scale factor too large: level 1 is less than half as wide as level 0"),
    (dict(nfeatures=1000, scale_factor=1.2, nlevels=8, max_width=640, max_height=480, ini_th_fast=5), _ffi.ORBFE_ERR_ARG,
     "iniThFAST (5) must be >= minThFAST (7)"),
    (dict(nfeatures=200000, scale_factor=1.2, nlevels=8, max_width=640, max_height=480), _ffi.ORBFE_ERR_ARG,
     "nfeatures too large: 43437 quadtree nodes on one level (at most 16383)"),
    (dict(nfeatures=1000, scale_factor=1.0, nlevels=8, max_width=640, max_height=480), _ffi.ORBFE_ERR_ARG,
     "bad orbfe_params (nlevels 1..16, scale_factor > 1, max size <= 4096, max_batch >= 1)"),
]


@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_errors_without_a_device(case):
    kw, status, text = ERRORS[case]
    L = _ffi.lib()
    p = params("vga", 1, **kw)
    for which in (0, 5):
        s, _ = table(L, p, DEFAULT, p.max_width, p.max_height, which)
        assert (s, L.orbfe_last_error().decode()) == (status, text)


# ---- (d) under sanitizers ----------------------------------------------------------------------------------------------------
def test_planner_under_sanitizers(tmp_path):
    """The planner's translation unit alone, host-only with AddressSanitizer and UBSan, walks the matrix and the error cases in a
    child process; every table arrives in a block of exactly its size, and the sizes are the library's."""
    from orb_slam2_ssd_semantic_amd import _build
    exe = str(tmp_path / "test_plan_sanitize")
    subprocess.check_call([_build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "--offload-host-only", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", _build.CSRC, os.path.join(ROOT, "tests", "cpp", "test_plan_sanitize.cpp"),
                           os.path.join(_build.CSRC, "orbfe_plan.hip"), "-o", exe])
    todo = [(shape, mb, k) for shape in SHAPES for mb, k in cases()]
    lines = [case_line(*c) for c in todo]
    for kw, _, _ in ERRORS:
        lines.append(" ".join(map(str, [kw["nfeatures"], kw["scale_factor"], kw["nlevels"], kw["max_width"], kw["max_height"], 1,
                                        kw.get("ini_th_fast", 20), 7] + [DEFAULT[k] for k in KNOBS])))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    out = [tuple(map(int, l.split())) for l in r.stdout.split("\n") if l]
    assert len(out) == len(lines)
    assert [s for s, _ in out[len(todo):]] == [s for _, s, _ in ERRORS]
    L = _ffi.lib()
    for (shape, mb, k), (s, total) in list(zip(todo, out))[::37]:
        assert s == 0 and total == sum(len(b) for b in tables(L, shape, mb, k)), (shape, mb, k)
    assert all(s == 0 for s, _ in out[:len(todo)])
