"""SearchBySim3 and SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) for a batch of loop candidates on the device
(csrc/orbfe_sim3_search.hip) bit for bit against tests/sim3_search_oracle.py -- which tests/test_sim3_search_oracle.py holds against
the compiled reference -- and, where oracle/_ref is built, against ref_search_by_sim3 / ref_search_by_projection_kf_sim3 themselves.
No tolerances.  The numpy forms of LoopCloser start every output as a sentinel with a guard band behind it and raise if the band
changed."""
import numpy as np
import pytest

import proj_cases as PC
import sim3_search_cases as SC
import sim3_search_checks as CK
import sim3_search_oracle as SO

pytestmark = pytest.mark.gpu

F = np.float32
HAVE_REF = CK.HAVE_REF


@pytest.fixture(scope="module")
def mt():
    from orb_slam2_ssd_semantic_amd import ORBmatcher
    m = ORBmatcher(0.9, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lc(mt):
    from orb_slam2_ssd_semantic_amd import LoopCloser
    return LoopCloser(mt)


# the single-pair comparisons live in tests/sim3_search_checks.py, shared with tests/test_gpu_sim3_search_edges.py
_poses, _oracle_sim3, _pad, _check_sim3_single, _check_proj = CK.poses, CK.oracle_sim3, CK.pad, CK.check_sim3_single, CK.check_proj


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("seed", range(6))
def test_search_by_sim3_parity(lc, seed):
    k1, k2, s12, R12, t12, m_in = PC.sim3_pair_case(np.random.default_rng(9100 + seed), 300, 280)
    # seed 0: n1 == cap == 300, not a multiple of 64; the others leave unused rows behind both keyframes
    _, nf, _, _ = _check_sim3_single(lc, k1, k2, (s12, R12, t12), m_in, cap=None if seed == 0 else 303)
    assert nf > 20


@pytest.mark.parametrize("shape", [(0, 40), (40, 0), (0, 0), (1, 1)])
def test_search_by_sim3_empty_keyframes(lc, shape):
    k1, k2, s12, R12, t12, m_in = PC.sim3_pair_case(np.random.default_rng(9150), *shape)
    _, nf, _, _ = _check_sim3_single(lc, k1, k2, (s12, R12, t12), m_in, cap=45)
    assert nf == 0 or shape == (1, 1)


@pytest.mark.parametrize("seed", range(6))
def test_search_by_projection_sim3_parity(lc, seed):
    kf, Scw, pts, m_in = PC.kf_sim3_case(np.random.default_rng(9300 + seed), 300, 400)
    _, nm = _check_proj(lc, kf, Scw, pts, m_in, cap=None if seed == 0 else 303)
    assert nm > 10


@pytest.mark.parametrize("shape", [(0, 40), (40, 0), (1, 1)])
def test_search_by_projection_sim3_empty(lc, shape):
    kf, Scw, pts, m_in = PC.kf_sim3_case(np.random.default_rng(9350), *shape)
    _check_proj(lc, kf, Scw, pts, m_in, cap=45)


# ------------------------------------------------------------------------------------------------ batch independence
def test_search_by_sim3_batch_is_independent(lc):
    rng = np.random.default_rng(9200)
    A, B, s1, R1, t1, mAB = PC.sim3_pair_case(rng, 130, 150)
    _, C, s2, R2, t2, _ = PC.sim3_pair_case(rng, 130, 97)
    _, _, s3, R3, t3, _ = PC.sim3_pair_case(rng, 3, 3)
    mBA = np.full(150, -1, np.int32)
    mBA[[3, 50, 149]] = [7, -2, 129]
    mAC = np.full(130, -1, np.int32)
    mAC[[0, 64]] = [96, 5]
    kfs = [A, B, C]
    pairs = [(0, 1), (1, 0), (0, 2), (0, 1), (0, 3)]
    sims = [(s1, R1, t1), (s2, R2, t2), (s2, R2, t2), (s3, R3, t3), (s1, R1, t1)]
    m_in = [mAB, mBA, mAC, mAB, np.arange(153, dtype=np.int32) % 7 - 2]
    singles = [lc.search_by_sim3_pairs_device([kfs[a], kfs[b]], [(0, 1)], [sims[p]], 7.5, [m_in[p]], cap=153)[0] for p, (a, b) in enumerate(pairs[:4])]
    for skip in (None, np.array([0, 0, 1, 0, 0], np.uint8)):
        out = lc.search_by_sim3_pairs_device(kfs, pairs, sims, 7.5, m_in, pair_skip=skip, cap=153)
        for p, (a, b) in enumerate(pairs[:4]):
            mo, nf, v1, v2 = out[p]
            if skip is not None and skip[p]:
                assert nf == 0 and np.array_equal(mo, m_in[p]) and (v1 == -1).all() and (v2 == -1).all()
                continue
            wo, wn, w1, w2 = _oracle_sim3(kfs[a], kfs[b], sims[p], 7.5, m_in[p])
            assert np.array_equal(mo, wo) and nf == wn and np.array_equal(v1, _pad(w1, 153)) and np.array_equal(v2, _pad(w2, 153))
            so, sn, s1v, s2v = singles[p]
            assert np.array_equal(mo, so) and nf == sn and np.array_equal(v1, s1v) and np.array_equal(v2, s2v)
        mo, nf, v1, v2 = out[4]   # a keyframe row out of range: nothing found, the row untouched
        assert nf == 0 and np.array_equal(mo, m_in[4][:len(mo)]) and (v1 == -1).all() and (v2 == -1).all()
    assert singles[0][1] > 5 and singles[0][1] != singles[3][1]


def test_search_by_projection_sim3_batch_is_independent(lc):
    rng = np.random.default_rng(9400)
    cases = [PC.kf_sim3_case(rng, 120, 150), PC.kf_sim3_case(rng, 97, 60), PC.kf_sim3_case(rng, 128, 200)]
    cases.append((cases[0][0], cases[2][1], cases[0][2], cases[0][3]))   # the first keyframe again, under another pose
    out, status = lc.search_by_projection_sim3_pairs_device(cases, 10, cap=131)
    assert status[0] == 0
    for (kf, Scw, pts, m_in), (got, nm) in zip(cases, out):
        want, wn = SO.search_by_projection_kf_sim3(kf, Scw, pts, m_in, 10)
        assert np.array_equal(got, want) and nm == wn
    assert out[0][1] > 5


# ------------------------------------------------------------------------------------------------ ties, thresholds, agreement
def test_tie_goes_to_the_first_in_cell_order(lc):
    k1, k2 = SC.tie_pair(np.random.default_rng(77))
    _, nf, v1, v2 = _check_sim3_single(lc, k1, k2, SC.IDENT, np.full(3, -1, np.int32), cap=5)
    assert v1[2] == 1 and v2[2] == 1 and nf == 0


@pytest.mark.parametrize("th_high", [100, 37])
def test_th_high_and_the_octave_window(lc, th_high):
    k1, k2, want = SC.threshold_pair(np.random.default_rng(78), th_high)
    _, _, v1, _ = _check_sim3_single(lc, k1, k2, SC.IDENT, np.full(6, -1, np.int32), cap=7, th_high=th_high)
    assert np.array_equal(v1[:6], want)


def test_agreement_and_preset_entries(lc):
    k1, k2, m_in, (w1, w2, wout, wn) = SC.agreement_pair(np.random.default_rng(79))
    mo, nf, v1, v2 = _check_sim3_single(lc, k1, k2, SC.IDENT, m_in, cap=11, ref=False)   # an index >= N2 is not the mock's to take
    assert np.array_equal(v1[:9], w1) and np.array_equal(v2[:6], w2) and np.array_equal(mo, wout) and nf == wn
    if HAVE_REF:   # the same scenario without the out-of-range preset, against the reference itself
        m2 = m_in.copy()
        m2[7] = -2
        _check_sim3_single(lc, k1, k2, SC.IDENT, m2, cap=11)


# ------------------------------------------------------------------------------------------------ claims
@pytest.mark.parametrize("th_low", [50, 23])
def test_claims_occupied_slots_and_members(lc, th_low):
    kf, Scw, pts, m_in, want, wn = SC.claims_case(np.random.default_rng(80), th_low)
    res = [_check_proj(lc, kf, Scw, pts, m_in, cap=len(want) + 3, th_low=th_low, list_skip=how) for how in ("device", "members", "host")]
    for got, nm in res:
        assert np.array_equal(got, want) and nm == wn


def test_entry_buffer_protocol(lc):
    kf, Scw, pts, m_in, want, wn = SC.claims_case(np.random.default_rng(80))
    case = [(kf, Scw, pts, m_in)]
    out, status = lc.search_by_projection_sim3_pairs_device(case, 10, ent_cap=0)
    need = int(status[0])
    assert need > 0 and out[0][1] == 0 and np.array_equal(out[0][0], m_in)
    out, status = lc.search_by_projection_sim3_pairs_device(case, 10, ent_cap=need - 1)
    assert status[0] == need and out[0][1] == 0 and np.array_equal(out[0][0], m_in)
    out, status = lc.search_by_projection_sim3_pairs_device(case, 10, ent_cap=need)
    assert status[0] == 0 and out[0][1] == wn and np.array_equal(out[0][0], want)


def test_mark_list_members(lc):
    """rows of cap 15360 (the LDS set at its largest), a pair that names another row, a row out of range, negative entries"""
    import torch
    rng = np.random.default_rng(81)
    cap, nrows = 15360, 2
    rows = np.full((nrows, cap), -1, np.int32)
    rows[0] = rng.permutation(40000)[:cap]
    rows[1, ::3] = rng.integers(0, 1 << 30, len(rows[1, ::3]))
    rows[1, 5] = -2
    lists = [np.concatenate([rows[0, :500], rng.integers(40000, 50000, 500), [-1, -2]]), rng.integers(0, 40000, 3000),
             np.concatenate([rows[1, ::3][:700], rows[0, :50]]), rows[0, :20]]
    pair_row = np.array([0, 0, 1, 2], np.int32)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    idx = np.concatenate(lists).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d_rows, d_pr, d_off, d_idx = dev(rows), dev(pair_row), dev(off.view(np.int32)), dev(idx)
    d_skip = torch.full((len(idx) + 64,), 9, dtype=torch.uint8, device="cuda")
    lc.mark_list_members_device(d_rows.data_ptr(), nrows, cap, d_pr.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), len(idx), 4, d_skip.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_skip.cpu().numpy()
    want = np.concatenate([np.isin(x, rows[r][rows[r] >= 0]) & (np.asarray(x) >= 0) if r < nrows else np.zeros(len(x), bool)
                           for x, r in zip(lists, pair_row)]).astype(np.uint8)
    assert np.array_equal(got[:len(idx)], want) and (got[len(idx):] == 9).all()
    assert want[:500].all() and not want[500:1002].any()


# ------------------------------------------------------------------------------------------------ the pose kernel
def test_pair_poses_device_equals_host(lc):
    import torch
    from orb_slam2_ssd_semantic_amd import loopclosing, sim3
    rng = np.random.default_rng(82)
    n = 64
    res = np.zeros(n, sim3.RESULT_DTYPE)
    res["found"] = rng.random(n) < 0.7
    res["found"][:2] = [1, 0]
    for i in range(n):
        res["model"]["R"][i] = PC._rot(rng, 60.0).astype(F)
        res["model"]["t"][i] = rng.normal(0, 2.0, 3).astype(F)
        res["model"]["s"][i] = F(rng.uniform(0.2, 5.0))
    d_res = torch.from_numpy(res.view(np.uint8).reshape(n, -1).copy()).cuda()
    d_T12, d_T21 = (torch.full((n * 12 + 64,), -7.0, dtype=torch.float32, device="cuda") for _ in range(2))
    d_skip = torch.full((n + 64,), 9, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lc.sim3_pair_poses_device(d_res.data_ptr(), res.dtype.itemsize, n, d_T12.data_ptr(), d_T21.data_ptr(), d_skip.data_ptr(), stream=st)
    # the plain [s, R, t] layout: every record counts as found
    srt = np.concatenate([res["model"]["s"][:, None], res["model"]["R"].reshape(n, 9), res["model"]["t"]], 1).astype(F)
    d_srt = torch.from_numpy(srt).cuda()
    d_U12, d_U21 = (torch.zeros((n, 12), dtype=torch.float32, device="cuda") for _ in range(2))
    lc.sim3_pair_poses_device(d_srt.data_ptr(), 52, n, d_U12.data_ptr(), d_U21.data_ptr(), None, loopclosing.POSE_LAYOUT_SRT, st)
    torch.cuda.synchronize()
    T12, T21, skip = d_T12.cpu().numpy(), d_T21.cpu().numpy(), d_skip.cpu().numpy()
    assert (T12[n * 12:] == -7).all() and (T21[n * 12:] == -7).all() and (skip[n:] == 9).all()
    U12, U21 = d_U12.cpu().numpy(), d_U21.cpu().numpy()
    for i in range(n):
        w12, w21 = loopclosing.sim3_pair_pose(res["model"]["s"][i], res["model"]["R"][i], res["model"]["t"][i])
        assert np.array_equal(U12[i].view(np.uint32), w12.view(np.uint32)) and np.array_equal(U21[i].view(np.uint32), w21.view(np.uint32))
        if not res["found"][i]:
            w12, w21 = np.zeros(12, F), np.zeros(12, F)
        assert np.array_equal(T12[i * 12:(i + 1) * 12].view(np.uint32), w12.view(np.uint32))
        assert np.array_equal(T21[i * 12:(i + 1) * 12].view(np.uint32), w21.view(np.uint32))
        assert skip[i] == (0 if res["found"][i] else 1)


def test_bad_arguments_are_refused_before_any_launch(lc, mt):
    from orb_slam2_ssd_semantic_amd import OrbfeError, _ffi, tracking
    fr = tracking.TrackFrames(1, 1, 1, 15361, 1, 1, 0.0, 0.0, 0.1, 0.1, None, None)
    cam = tracking.camera(500, 500, 320, 240, 40, 0, 640, 0, 480)
    tmap = _ffi.TrackMap(None, None, None, None, None, None, None, 0)
    sf = PC.scale_factors()
    with pytest.raises(OrbfeError) as e:
        lc.SearchBySim3_batch_device(fr, 1, 1, 1, tmap, cam, 1, 1, 1, 1, None, 1, 7.5, sf, 0.18, 1, 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    fr.cap = 64
    with pytest.raises(OrbfeError) as e:
        lc.SearchBySim3_batch_device(fr, 1, 1, 1, tmap, cam, 1, 1, 1, 1, None, 1, 7.5, np.ones(17, F), 0.18, 1, 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG
    with pytest.raises(OrbfeError) as e:
        lc.SearchByProjectionSim3_batch_device(fr, 1, 1, 1, cam, tmap, 1, 1, None, 0, 10, np.ones(17, F), 0.18, 4, 16, 1, 1, 1)
    assert e.value.status == _ffi.ORBFE_ERR_ARG


# ------------------------------------------------------------------------------------------------ the chain of a round
def test_compute_sim3_round_chain_equals_the_steps_one_by_one(lc, mt):
    """four candidates on one non-default stream, one synchronize at the end, against: host SearchByBoW, numpy inversion, the
    host-buffer Sim3 iterate on the constructor's points, the inlier filter, the host pose, a single-pair SearchBySim3"""
    import torch
    from orb_slam2_ssd_semantic_amd import Sim3, _ffi, loopclosing, sim3 as S3, tracking
    rng = np.random.default_rng(83)
    shapes = [(260, 240), (200, 260), (180, 180), (40, 30)]
    cases = [SC.chain_case(rng, a, b) for a, b in shapes]
    kfs = [k for c in cases for k in c[:2]]
    P, B = len(cases), len(kfs)
    pairs = [(2 * p, 2 * p + 1) for p in range(P)]
    cap = 263
    n_it, min_inl = 40, 12
    draws = rng.integers(0, 2 ** 31 - 1, (P, 3 * n_it), dtype=np.int64).astype(np.int32)
    k0 = kfs[0]
    sf, ls2, K4 = k0["scale_factors"], k0["level_sigma2"], np.array(k0["K"][:4], F)
    sets = np.zeros(P, S3.SET_DTYPE)
    sets["K1"], sets["K2"], sets["fix_scale"], sets["min_inliers"], sets["max_its"], sets["n_iterations"] = K4, K4, 0, min_inl, n_it, n_it
    sets["draws_offset"] = np.arange(P) * 3 * n_it
    # ---- the device block, the map (every keyframe's own points), the FeatureVector blocks
    blk, desc, ns, _ = loopclosing._keyframe_block(kfs, cap)
    for r, k in enumerate(kfs):
        blk["angle"][r, :ns[r]] = k["angle"]
    base = np.concatenate([[0], np.cumsum(ns)])
    npts = int(base[-1])
    slot, valid, Tcw = np.full((B, cap), -1, np.int32), np.zeros((B, cap), np.uint8), np.zeros((B, 12), F)
    fv_node, fv_off, fv_idx, counts = (np.zeros((B, cap), np.int32), np.zeros((B, cap + 1), np.int32), np.zeros((B, cap), np.int32),
                                       np.zeros((B, 4), np.int32))
    for r, k in enumerate(kfs):
        n = ns[r]
        slot[r, :n] = np.where(k["state"] > 0, base[r] + np.arange(n), -1)
        valid[r, :n] = k["valid"]
        Tcw[r] = SO.pose34(k).reshape(12)
        node, off, idx = k["fv"]
        fv_node[r, :len(node)], fv_off[r, :len(off)], fv_idx[r, :len(idx)] = node, off, idx
        counts[r] = [0, len(node), len(idx), 0]
    cat = lambda key, w=None: np.concatenate([np.asarray(k[key]).reshape((-1,) if w is None else (-1, w)) for k in kfs])   # noqa: E731
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d = dict(kps=dev(blk.view(np.uint8).reshape(B, cap, -1)), desc=dev(desc), n=dev(ns), slot=dev(slot), valid=dev(valid), Tcw=dev(Tcw),
                 fv_node=dev(fv_node), fv_off=dev(fv_off), fv_idx=dev(fv_idx), counts=dev(counts), wp=dev(cat("world_pos", 3).astype(F)),
                 mn=dev(cat("min_dist").astype(F)), mx=dev(cat("max_dist").astype(F)), bad=dev((cat("state") == 2).astype(np.uint8)),
                 mpd=dev(cat("mpdesc", 32)), kf1=dev(np.array([p[0] for p in pairs], np.int32)), kf2=dev(np.array([p[1] for p in pairs], np.int32)),
                 draws=dev(draws.reshape(-1)), off=torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda"),
                 cidx=torch.zeros((B, cap), dtype=torch.int32, device="cuda"), nin=torch.zeros((B,), dtype=torch.int32, device="cuda"))
        st = stream.cuda_stream
        minx, maxx, miny, maxy = [float(v) for v in k0["bounds"]]
        mt.AssignFeaturesToGrid_batch_device(d["kps"].data_ptr(), d["n"].data_ptr(), cap, B, minx, miny, float(k0["gw_inv"]), float(k0["gh_inv"]),
                                             d["off"].data_ptr(), d["cidx"].data_ptr(), d["nin"].data_ptr(), _ffi.stream_arg(None, st))
        frames = tracking.frames_struct(d["kps"], d["desc"], d["n"], cap, d["off"], d["cidx"], minx, miny, k0["gw_inv"], k0["gh_inv"])
        cam = tracking.camera(*[float(v) for v in k0["K"][:5]], minx, maxx, miny, maxy)
        tmap = _ffi.TrackMap(d["wp"].data_ptr(), None, d["mn"].data_ptr(), d["mx"].data_ptr(), d["bad"].data_ptr(), None, d["mpd"].data_ptr(), npts)
        solver = Sim3(max_pairs=cap, max_sets=P)
        bow = dict(kps=d["kps"], desc=d["desc"], valid=d["valid"], fv_node=d["fv_node"], fv_off=d["fv_off"], fv_idx=d["fv_idx"], counts=d["counts"])
        r = lc.compute_sim3_round_device(solver, frames, B, d["n"], d["Tcw"], d["slot"], tmap, cam, bow, d["kf1"], d["kf2"], sets, d["draws"], 7.5, sf,
                                         ls2, k0["log_scale"])
    torch.cuda.synchronize()   # the only one
    got = {k: v.cpu().numpy() for k, v in r.items() if k in ("match12", "nfound", "pair_skip", "bow_match", "nbow", "offsets", "result")}
    res = got["result"].view(S3.RESULT_DTYPE).reshape(P)
    # ---- the same steps one by one
    host_solver = Sim3(max_pairs=cap, max_sets=1)
    found_any = 0
    for p, (k1, k2, _) in enumerate(cases):
        n1, n2 = len(k1["octave"]), len(k2["octave"])
        bm, nb = mt.SearchByBoW(k1["desc"], k1["valid"], k1["angle"], k1["fv"], k2["desc"], k2["valid"], k2["angle"], k2["fv"])
        assert np.array_equal(got["bow_match"][p, :n2], bm) and got["nbow"][p] == nb
        m12 = np.full(n1, -1, np.int32)
        m12[bm[bm >= 0]] = np.flatnonzero(bm >= 0)
        i1 = np.array([i for i in range(n1) if m12[i] >= 0 and k1["state"][i] == 1 and k2["state"][m12[i]] == 1], np.int64)
        assert got["offsets"][p + 1] - got["offsets"][p] == len(i1)
        def cam(W, k):   # the constructor's Rcw * Xw + tcw in float, left to right (Sim3Solver.from_world)
            Rm, t = np.asarray(k["Rcw"], F).reshape(3, 3), np.asarray(k["tcw"], F).reshape(3)
            return np.stack([((Rm[c, 0] * W[:, 0] + Rm[c, 1] * W[:, 1]) + Rm[c, 2] * W[:, 2]) + t[c] for c in range(3)], 1).astype(F)
        X1, X2 = cam(k1["world_pos"][i1], k1), cam(k2["world_pos"][m12[i1]], k2)
        state, best = np.zeros(1, S3.STATE_DTYPE), np.zeros(len(i1), np.uint8)
        hres, hmask = host_solver.iterate(X1, X2, ls2[k1["octave"][i1]], ls2[k2["octave"][m12[i1]]], K4, K4, False, min_inl,
                                          n_it, n_it, draws[p], state, best)
        assert res["found"][p] == hres["found"] and res["n_inliers"][p] == hres["n_inliers"] and got["pair_skip"][p] == (0 if hres["found"] else 1)
        keep = np.zeros(n1, bool)
        keep[i1[hmask.astype(bool)]] = True
        m12 = np.where(keep, m12, -1).astype(np.int32)
        if hres["found"]:
            found_any += 1
            for f in ("R", "t", "s"):
                assert np.array_equal(np.asarray(res["model"][f][p]).view(np.uint32), np.asarray(hres["model"][f]).view(np.uint32))
            sim = (hres["model"]["s"], hres["model"]["R"], hres["model"]["t"])
            mo, nf, _, _ = lc.search_by_sim3_pairs_device([k1, k2], [(0, 1)], [sim], 7.5, [m12], cap=cap, poses_on_device=False)[0]
            assert nf > 0
        else:
            mo, nf = m12, 0
        assert np.array_equal(got["match12"][p, :n1], mo) and (got["match12"][p, n1:] == -1).all() and got["nfound"][p] == nf, p
    assert found_any >= 3
