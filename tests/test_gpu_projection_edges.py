"""The projection-gated searches at their window, gate, decision and slab edges, bit for bit against the CPU oracle.

Inputs come from tests/proj_edge_cases.py (tests/test_proj_edge_cases.py shows on the CPU that every case sits on the edge it
names).  The grid index runs through FrameGrid (k_assign_grid, k_area_count / k_area_write) and through the device-resident
forms on keypoint records (stride 7); the search core through both device forms, the one-launch pair k_proj_fused +
k_proj_rounds and count -> scan -> fill -> resolve; orbfe_window_distances and k_triangulation through their host entry
points.  No tolerances: match, best, second, offsets, candidates, distances, cell_off, cell_idx and n_in_grid are equal or
the test fails."""
import functools

import numpy as np
import pytest

import proj_edge_cases as E
from oracle import oracle_ffi as O

pytestmark = pytest.mark.gpu

F = np.float32
NC = E.COLS * E.ROWS
CORE_TABLES = ["WINDOW_CASES", "DECISION_CASES", "GATE_CASES", "ROUND_CASES", "SLAB_CASES"]


@pytest.fixture(scope="module", params=[0, 1], ids=["one-launch", "four-kernel"])
def mat(request):
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    m.set_projection_kernel(request.param)
    yield m
    m.close()


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    yield m
    m.close()


@functools.lru_cache(maxsize=None)
def ref(table, name):
    """the case and the oracle's answers for it, computed once: per call (match, best, second) and per query the candidates"""
    case = E.TABLES[table][name]()
    if table == "TRI_CASES":
        return case, [E.run_tri(O.search_for_triangulation, c) for c in case["calls"]]
    out = []
    for c in case["calls"]:
        areas = [E.oracle_area(c, i) for i in range(len(c["q"]))]
        core = None if c.get("wd_only") else E.run_core(O.search_by_projection, c)
        for a in areas + list(core or ()):
            a.setflags(write=False)
        out.append((areas, core))
    return case, out


def _ids(tables):
    return [pytest.param(t, n, id="%s-%s" % (t.split("_")[0].lower(), n)) for t in tables for n in E.TABLES[t]]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _areas_csr(areas):
    off = np.concatenate([[0], np.cumsum([len(a) for a in areas])]).astype(np.uint32)
    return off, (np.concatenate(areas) if len(areas) and off[-1] else np.zeros(0, np.uint32)).astype(np.uint32)


def _qxyr(q):
    return np.stack([q["u"], q["v"], q["r"]], 1).astype(F), np.stack([q["min_level"], q["max_level"]], 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the search core
@pytest.mark.parametrize("table,name", _ids(CORE_TABLES))
def test_core_equals_oracle(mat, table, name):
    case, want = ref(table, name)
    for k, c in enumerate(case["calls"]):
        if c.get("wd_only"):
            continue
        got = E.run_core(mat.SearchByProjectionCore, c)
        for key, g, w in zip(("match", "best", "second"), got, want[k][1]):
            assert np.array_equal(g, w), (name, k, key, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("table,name", _ids(["WINDOW_CASES", "SLAB_CASES"]))
def test_window_distances_equal_oracle(mat, table, name):
    case, want = ref(table, name)
    for k, c in enumerate(case["calls"]):
        ci, q = c["ci"], c["q"]
        off, cand, dist = mat.WindowDistances(ci["descF"], ci["xyF"], ci["octF"], ci["grid"], ci["bounds"], q, c["qd"], cap=16)
        roff, rcand = _areas_csr(want[k][0])
        assert np.array_equal(off, roff) and np.array_equal(cand, rcand), (name, k)
        qi = np.repeat(np.arange(len(q)), np.diff(roff.astype(np.int64)))
        rd = np.unpackbits(c["qd"][qi] ^ ci["descF"][rcand], axis=1).sum(1) if len(rcand) else np.zeros(0, np.int64)
        assert np.array_equal(dist.astype(np.int64), rd), (name, k)


# ------------------------------------------------------------------------------------------------ the grid index
@pytest.mark.parametrize("name", list(E.WINDOW_CASES))
def test_window_cases_through_frame_grid(mt, name):
    from orb_slam2_ssd_semantic_amd import FrameGrid
    case, want = ref("WINDOW_CASES", name)
    for k, c in enumerate(case["calls"]):
        ci, q = c["ci"], c["q"]
        g = FrameGrid(mt, ci["xyF"], ci["octF"], *ci["bounds"])
        assert np.array_equal(g.cell_off, ci["grid"][0]) and np.array_equal(g.cell_idx, ci["grid"][1]), (name, k)
        qoff, cand = g.query(*_qxyr(q), cap=4)
        roff, rcand = _areas_csr(want[k][0])
        assert np.array_equal(qoff, roff) and np.array_equal(cand, rcand), (name, k)


def _kp_block(frames, cap):
    """keypoint records [len(frames)][cap] (stride 7 floats) from (xy, octave) pairs; the rows past a frame's count hold a
    keypoint that would land in a cell if it were read"""
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    blk = np.zeros((len(frames), cap), KP_DTYPE)
    blk["x"], blk["y"], blk["octave"] = 100.0, 100.0, 3
    for f, (xy, octv) in enumerate(frames):
        blk["x"][f, :len(xy)], blk["y"][f, :len(xy)], blk["octave"][f, :len(xy)] = xy[:, 0], xy[:, 1], octv
        blk["angle"][f, :len(xy)], blk["size"][f, :len(xy)] = 45.0, 31.0
    return blk


def _grid_batch_device(mt, frames, g):
    """orbfe_assign_grid_batch_device on a block of len(frames) frames with different counts: (block, d_kps, off, idx, nin)"""
    import torch
    cap = max(len(xy) for xy, _ in frames) + 3
    blk = _kp_block(frames, cap)
    dk = torch.from_numpy(blk.view(np.int32).reshape(len(frames), cap, 7).copy()).cuda()
    dn = _dev(np.array([len(xy) for xy, _ in frames], np.int32))
    d_off = torch.full((len(frames), NC + 1), -7, dtype=torch.int32, device="cuda")
    d_idx = torch.full((len(frames), cap), -7, dtype=torch.int32, device="cuda")
    d_nin = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    mt.AssignFeaturesToGrid_batch_device(dk.data_ptr(), dn.data_ptr(), cap, len(frames), *[float(v) for v in g], d_off.data_ptr(),
                                         d_idx.data_ptr(), d_nin.data_ptr(), st)
    torch.cuda.synchronize()
    return cap, dk, d_off, d_idx, d_nin


def _check_grid_batch(frames, g, d_off, d_idx, d_nin, tag):
    off, idx, nin = d_off.cpu().numpy().view(np.uint32), d_idx.cpu().numpy(), d_nin.cpu().numpy()
    for f, (xy, _) in enumerate(frames):
        roff, ridx = O.assign_grid(xy, *[float(v) for v in g])
        assert nin[f] == len(ridx) and np.array_equal(off[f], roff), (tag, f, nin[f], len(ridx))
        assert np.array_equal(idx[f, :nin[f]].view(np.uint32), ridx) and (idx[f, nin[f]:] == -7).all(), (tag, f)


@pytest.mark.parametrize("name", list(E.WINDOW_CASES))
def test_window_cases_device_resident_on_keypoint_records(mt, name):
    """AssignFeaturesToGrid_batch_device + GetFeaturesInArea_device on KP_DTYPE blocks: two frames with different counts (the
    case's keypoints, and all but its last three)"""
    import torch
    case, want = ref("WINDOW_CASES", name)
    c = case["calls"][0]
    ci, q = c["ci"], c["q"]
    g = ci["bounds"]
    n = len(ci["xyF"])
    frames = [(ci["xyF"], ci["octF"]), (ci["xyF"][:max(n - 3, 0)], ci["octF"][:max(n - 3, 0)])]
    cap, dk, d_off, d_idx, d_nin = _grid_batch_device(mt, frames, g)
    _check_grid_batch(frames, g, d_off, d_idx, d_nin, name)
    qxyr, qlv = _qxyr(q)
    dq, dlv = _dev(qxyr), _dev(qlv)
    st = torch.cuda.current_stream().cuda_stream
    for f, (xy, octv) in enumerate(frames):
        if f == 0:
            areas = want[0][0]
        else:
            goff, gidx = O.assign_grid(xy, *[float(v) for v in g])
            areas = [O.features_in_area(xy, octv, goff, gidx, *[float(v) for v in g], *[float(v) for v in qxyr[i]], int(qlv[i, 0]), int(qlv[i, 1]))
                     for i in range(len(q))]
        roff, rcand = _areas_csr(areas)
        ccap = int(roff[-1]) + 5
        c_off = torch.full((len(q) + 1,), -7, dtype=torch.int32, device="cuda")
        c_cand = torch.full((ccap,), -7, dtype=torch.int32, device="cuda")
        mt.GetFeaturesInArea_device(dk[f].data_ptr(), d_off[f].data_ptr(), d_idx[f].data_ptr(), *[float(v) for v in g], dq.data_ptr(),
                                    dlv.data_ptr(), len(q), c_off.data_ptr(), c_cand.data_ptr(), ccap, st)
        torch.cuda.synchronize()
        assert np.array_equal(c_off.cpu().numpy().view(np.uint32), roff), (name, f)
        got = c_cand.cpu().numpy()
        assert np.array_equal(got[:roff[-1]].view(np.uint32), rcand) and (got[roff[-1]:] == -7).all(), (name, f)


@pytest.mark.parametrize("name", list(E.GRID_CASES))
def test_grid_cases_equal_oracle(mt, name):
    """cell_off, cell_idx and n_in_grid of k_assign_grid in both its forms: FrameGrid on packed (x, y), and the batched
    device form on keypoint records with two frames of different counts"""
    from orb_slam2_ssd_semantic_amd import FrameGrid
    case = E.GRID_CASES[name]()
    xy, g = case["xy"], E.grid_params(case["bounds"])
    octv = np.zeros(len(xy), np.int32)
    roff, ridx = O.assign_grid(xy, *[float(v) for v in g])
    fg = FrameGrid(mt, xy, octv, *g)
    assert np.array_equal(fg.cell_off, roff), (name, np.flatnonzero(fg.cell_off != roff)[:8])
    assert len(fg.cell_idx) == len(ridx) == sum(c >= 0 for c in case["cell"]) and np.array_equal(fg.cell_idx, ridx), name
    frames = [(xy, octv), (xy[len(xy) // 3:], octv[len(xy) // 3:])]
    cap, dk, d_off, d_idx, d_nin = _grid_batch_device(mt, frames, g)
    _check_grid_batch(frames, g, d_off, d_idx, d_nin, name)


# ------------------------------------------------------------------------------------------------ slab overflow and size limits
def test_small_call_after_a_slab_overflow_and_both_forms_agree():
    """a call whose query overflows its slab goes to the four-kernel form and leaves the overflow counter at zero: a second,
    small call on the SAME matcher is right again; both device forms equal the oracle and each other"""
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    forms = []
    for kernel in (0, 1):
        m = ORBmatcher(0.9, True)
        m.set_projection_kernel(kernel)
        got = []
        for name in ("candidates_513", "queries_5", "candidates_512", "candidates_513", "queries_65"):
            case, want = ref("SLAB_CASES", name)
            got.append(E.run_core(m.SearchByProjectionCore, case["calls"][0]))
            for g, w in zip(got[-1], want[0][1]):
                assert np.array_equal(g, w), (kernel, name)
        forms.append(got)
        m.close()
    assert all(np.array_equal(a, b) for x, y in zip(*forms) for a, b in zip(x, y))


def test_size_limits_return_err_size_and_the_matcher_still_works(mat):
    from orb_slam2_ssd_semantic_amd import _ffi
    L, p = _ffi.lib(), _ffi.ptr
    small, want = ref("SLAB_CASES", "queries_4")
    q = E.queries([(320, 240, 10)])
    qd = np.zeros((1, 32), np.uint8)
    m, b, s = (np.zeros(1, np.int32) for _ in range(3))
    off, ent = np.zeros(2, np.uint32), np.zeros(64, np.uint32)
    for n, fn in ((E.PJ_MAX_NF + 1, "core"), (E.WD_MAX_NF + 1, "window")):
        xy = np.full((n, 2), 1000.0, F)   # outside the grid: an empty index is consistent with any n
        desc, octv, goff, gidx = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.zeros(NC + 1, np.uint32), np.zeros(1, np.uint32)
        if fn == "core":
            rc = L.orbfe_search_by_projection(mat.handle, p(desc), p(xy), p(octv), n, p(goff), p(gidx), 0.0, 0.0, 0.1, 0.1, None, None, p(q),
                                              p(qd), 1, 100, 0.8, 1, p(m), p(b), p(s))
        else:
            rc = L.orbfe_window_distances(mat.handle, p(desc), p(xy), p(octv), n, p(goff), p(gidx), 0.0, 0.0, 0.1, 0.1, p(q), p(qd), 1, p(off),
                                          p(ent), 64)
        assert rc == _ffi.ORBFE_ERR_SIZE, (fn, rc)
        got = E.run_core(mat.SearchByProjectionCore, small["calls"][0])
        assert all(np.array_equal(g, w) for g, w in zip(got, want[0][1])), fn
    # one below each limit is taken (the two largest tables of SLAB_CASES run in the tests above)
    assert len(ref("SLAB_CASES", "features_15360")[0]["calls"][0]["ci"]["xyF"]) == E.PJ_MAX_NF


# ------------------------------------------------------------------------------------------------ triangulation
@pytest.mark.parametrize("name", list(E.TRI_CASES))
def test_triangulation_equals_oracle(mt, name):
    case, want = ref("TRI_CASES", name)
    for k, c in enumerate(case["calls"]):
        got = E.run_tri(mt.SearchForTriangulationCore, c)
        assert np.array_equal(got, want[k]), (name, k, got[got != want[k]][:8], want[k][got != want[k]][:8])
