"""cv::findHomography on the GPU (csrc/orbfe_homography.hip) against tests/homography_oracle.py, bit for bit: the device
primitives (RNG, hypot, RANSACUpdateNumIters, the 9x9 and 8x8 Jacobi), every tap over the case table and real matched
keypoints, the batched device form against host calls, and the chain pairs -> H -> homography-compensated flow mask."""
import numpy as np
import pytest

import flow_oracle as FO
import homography_cases as HC
import homography_oracle as HO
import warp_cases as WC
import warp_oracle as WO
from homography_checks import batch as _batch, bits as _b, check_case as _check_case
from orb_slam2_ssd_semantic_amd import Flow, Homography, ORBextractor, ORBmatcher
from orb_slam2_ssd_semantic_amd import homography as HG
from orb_slam2_ssd_semantic_amd.synth import synth_tum_like

MAX_PAIRS = 2048


@pytest.fixture(scope="module")
def hg():
    h = Homography(MAX_PAIRS, 64)
    yield h
    h.close()


_CASES = HC.table(MAX_PAIRS)


def _hypot_np(a, b):
    """lapack.cpp's hypot, vectorised (elementwise IEEE ops, as homography_oracle.cv_hypot)"""
    a, b = np.abs(a), np.abs(b)
    out = np.zeros_like(a)
    with np.errstate(all="ignore"):
        g = a > b
        q = b[g] / a[g]
        out[g] = a[g] * np.sqrt(1 + q * q)
        k = ~g & (b > 0)
        q = a[k] / b[k]
        out[k] = b[k] * np.sqrt(1 + q * q)
    return out


@pytest.mark.gpu
def test_kat_rng_stream():
    got = HG.kat(HG.KAT_RNG, HO.MASK64, 1_000_000)
    assert np.array_equal(got, HO.rng_stream(1_000_000))
    assert np.array_equal(HG.kat(HG.KAT_RNG, 12345, 1000), HO.rng_stream(1000, 12345))


@pytest.mark.gpu
def test_kat_hypot():
    rng = np.random.default_rng(3)
    n = 10_000_000
    e = rng.uniform(-30, 30, (n, 2))
    ab = np.sign(rng.random((n, 2)) - 0.5) * rng.random((n, 2)) * 10.0 ** e
    ab[:1000] = 0.0
    ab[1000:2000, 0] = ab[1000:2000, 1]
    got = HG.kat(HG.KAT_HYPOT, ab)
    want = _hypot_np(ab[:, 0], ab[:, 1])
    assert np.array_equal(_b(got), _b(want))
    for a, b in ab[::100000]:
        assert HO.cv_hypot(a, b) == want[int(np.flatnonzero((ab[:, 0] == a) & (ab[:, 1] == b))[0])]
    # the template is not the C library's hypot (oracle H3); report how often they differ
    print(f"lapack hypot != C hypot on {np.count_nonzero(want != np.hypot(ab[:, 0], ab[:, 1]))} of {n} pairs")


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [0.99, 0.995, 0.999])
def test_kat_num_iters_exhaustive(conf):
    rows = [(conf, (c - g) / c, 2000.0) for c in range(5, MAX_PAIRS + 1) for g in range(4, c + 1)]
    inp = np.array(rows, np.float64)
    got = HG.kat(HG.KAT_NUMITERS, inp)
    want = np.array([HO.update_num_iters(p, ep, 4, 2000) for p, ep, _ in rows], np.int32)
    assert np.array_equal(got, want)
    edge = np.array([(conf, 0.0, 2000), (conf, 1.0, 2000), (conf, 0.999, 2000), (conf, 0.5, 7)], np.float64)
    assert np.array_equal(HG.kat(HG.KAT_NUMITERS, edge), [HO.update_num_iters(p, ep, 4, int(m)) for p, ep, m in edge])


def _case_matrices():
    """the refit LtL and the first JtJ of every case that gets that far in the oracle"""
    l9, l8 = [], []
    for s, d, kw in _CASES.values():
        if len(s) < 5:
            continue
        H, mask = HO.find_homography(s, d, **kw)
        if H is None:
            continue
        _, L = HO.run_kernel(s[mask.astype(bool)], d[mask.astype(bool)], with_ltl=True)
        if L is not None:
            l9.append(L)
        r, J = HO.refine_compute(s[mask.astype(bool)], d[mask.astype(bool)], H.ravel()[:8])
        l8.append(HO._jtj(J))
    return np.array(l9), np.array(l8)


@pytest.mark.gpu
def test_kat_jacobi_on_case_matrices():
    l9, l8 = _case_matrices()
    assert len(l9) >= 10 and len(l8) >= 10
    for k, mats in ((HG.KAT_JACOBI9, l9), (HG.KAT_JACOBI8, l8)):
        W, V = HG.kat(k, mats)
        for i, A in enumerate(mats):
            w, v = HO.jacobi(A)
            assert np.array_equal(_b(W[i]), _b(w)) and np.array_equal(_b(V[i]), _b(v)), (k, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_case_table_bit_exact_at_every_tap(hg, name):
    s, d, kw = _CASES[name]
    H, t = _check_case(hg, s, d, kw, name)
    if name in ("collinear", "zero_spread_method_0", "zero_spread_n4", "n_3", "n_0"):
        assert H is None
    if name == "ratio_0.1":
        assert t["iters"] == 2000
    if name == "max_iters_5":
        assert t["iters"] == 5


@pytest.mark.gpu
def test_recovers_the_built_homography(hg):
    s, d, inl = HC.planar(300, 0.6, 5, noise=0.0)
    H, mask = hg.find(s, d)
    assert np.abs(H - HC.H_TRUE).max() < 1e-4
    assert np.array_equal(mask.astype(bool), inl)


def real_pairs(seed=5):
    """keypoints of an S_tum frame (last) and of its warp by a known camera motion with a moving patch (current), matched
    current -> last by the library's brute-force matcher"""
    w, h = 640, 480
    a = synth_tum_like(seed)
    G = WC.homography("camera_plane", w, h)
    b = WO.warp(a, G).copy()
    patch = a[100:196, 100:196].copy()
    b = WC.with_patch(b, patch, 330, 210)
    ext = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    mat = ORBmatcher(0.9, True, device=0)
    ka, da = ext(a)
    kb, db = ext(b)
    m = mat.MatchBruteForce(db, da, kb["angle"], ka["angle"], 100)[0]
    q = np.flatnonzero(m >= 0)
    cur = np.c_[kb["x"][q], kb["y"][q]].astype(np.float32)
    last = np.c_[ka["x"][m[q]], ka["y"][m[q]]].astype(np.float32)
    return cur, last, G


@pytest.mark.gpu
def test_real_matched_keypoints(hg):
    cur, last, G = real_pairs()
    assert len(cur) > 100
    H, t = _check_case(hg, cur, last, {}, "real")
    assert H is not None and t["ransac_ok"]


@pytest.mark.gpu
def test_batched_equals_host_calls(hg):
    sizes = [0, 3, 4, 5, 51, 200, 1, 500, 2, 120, 50, 51]
    sets = []
    for i, n in enumerate(sizes):
        s, d, _ = HC.planar(n, 0.6 if n > 5 else 1.0, 200 + i)
        sets.append((s, d))
    H, ok, mask, off = _batch(hg, sets, 50)
    for i, (s, d) in enumerate(sets):
        hH, hm = hg.find(s, d)
        oH, om = HO.find_homography(s, d)
        assert np.array_equal(mask[off[i]:off[i + 1]], hm) and np.array_equal(hm, om), i
        if hH is None:
            assert ok[i] == 0 and not H[i].any(), i
        else:
            assert np.array_equal(_b(H[i]), _b(hH)) and np.array_equal(_b(hH), _b(oH)), i
            assert ok[i] == int(len(s) > 50), (i, len(s))
    # the min_pairs boundary: 50 pairs give ok = 0, 51 give ok = 1 (TrackHomo's size() > 50)
    assert ok[sizes.index(50)] == 0 and ok[sizes.index(51)] == 1


@pytest.mark.gpu
def test_chain_pairs_to_homography_to_flow_mask(hg):
    """pairs -> orbfe_find_homographies_device -> orbfe_flow_compute_masks_homo_device on one stream, no host round trip, against
    the host chain oracle H -> warp_oracle -> flow_oracle"""
    import torch
    w, h = 640, 480
    frames = [synth_tum_like(40 + i) for i in range(3)]
    sets = [HC.planar(200, 0.7, 300 + i, H=WC.camera_homography(w, h, yaw=0.01 * i))[:2] for i in range(3)]
    sets[1] = (sets[1][0][:40], sets[1][1][:40])   # a lost frame: 40 pairs, ok = 0 with min_pairs 50
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    off = np.r_[0, np.cumsum([len(s) for s, _ in sets])].astype(np.int32)
    src = np.concatenate([s for s, _ in sets]).astype(np.float32)
    dst = np.concatenate([d for _, d in sets]).astype(np.float32)
    fl = Flow(w, h, max_batch=3)
    with torch.cuda.stream(st):
        g = torch.from_numpy(np.stack(frames)).to(dev)
        H, ok, _ = hg.find_batch(torch.from_numpy(off).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev),
                                 min_pairs=50)
        masks, ones = fl.compute_masks(g, 40.0, homographies=H, use=ok)
    st.synchronize()
    masks = masks.cpu().numpy()
    of = FO.Flow()
    for i, (s, d) in enumerate(sets):
        oH, _ = HO.find_homography(s, d)
        use = oH is not None and len(s) > 50
        assert int(ok[i]) == int(use), i
        want = WO.compute_mask_homo(of, frames[i], oH, 40.0) if use else of.compute_mask(frames[i], 40.0)
        assert np.array_equal(masks[i], want), i
    fl.close()


@pytest.mark.gpu
def test_invalid_sizes_are_errors(hg):
    from orb_slam2_ssd_semantic_amd import OrbfeError
    s, d, _ = HC.planar(MAX_PAIRS + 1, 1.0, 1)
    with pytest.raises(OrbfeError):
        hg.find(s, d)
    with pytest.raises(OrbfeError):
        hg.find(s[:10], d[:10], method=4)   # LMEDS is not built
    with pytest.raises(OrbfeError):
        hg.find(s[:10], d[:10], confidence=1.0)
    import torch
    dev = torch.device("cuda", 0)
    off = torch.zeros(66, dtype=torch.int32, device=dev)
    z = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    with pytest.raises(OrbfeError):
        hg.find_batch(off, z, z)   # 65 sets > max_sets 64
