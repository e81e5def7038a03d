"""Parity of the HIP extractor (through the C-ABI) against the CPU oracle and the golden fixtures.
Bar: bit-exact keypoints (x, y, size, angle, response, octave, class_id), descriptors and ORDER."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from orb_slam2_ssd_semantic_amd.synth import synth_frame

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb_golden.npz")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def assert_same_output(gk, gd, ok, od):
    assert len(gk) == len(ok), (len(gk), len(ok))
    for f in ok.dtype.names:
        bad = np.nonzero(gk[f].view(np.uint32) != ok[f].view(np.uint32))[0]
        assert len(bad) == 0, (f, bad[:5], gk[f][bad[:5]], ok[f][bad[:5]])
    assert np.array_equal(gd, od)


def cand_array(c):
    return np.stack([c["x"], c["y"], c["response"]], 1) if len(c) else np.zeros((0, 3), np.float32)


@pytest.fixture(scope="module")
def ext():
    from orb_slam2_ssd_semantic_amd import ORBextractor
    return ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=8)


@pytest.mark.parametrize("seed,sparse", [(0, False), (1, False), (2, True), (3, True), (11, False)])
def test_stage_by_stage_parity(oracle, ext, seed, sparse):
    img = synth_frame(seed, sparse=sparse)
    oe = oracle.OracleExtractor()
    ok, od = oe(img)
    gk, gd = ext(img)
    for l in range(8):
        assert np.array_equal(ext.pyramid_level(l), oe.level(l)), f"pyramid level {l}"
        assert np.array_equal(ext.blurred_level(l), oe.blurred(l)), f"blurred level {l}"
        assert np.array_equal(ext.candidates(l), cand_array(oe.candidates(l))), f"FAST candidates level {l}"
        assert np.array_equal(ext.selected(l), cand_array(oe.selected(l))), f"quadtree level {l}"
    assert_same_output(gk, gd, ok, od)


def test_golden_fixtures(ext):
    from orb_slam2_ssd_semantic_amd import ORBextractor
    g = np.load(GOLD)
    cases = [("A_dense_s0", 0, 480, 640, False, 1000), ("A_dense_s1", 1, 480, 640, False, 1000),
             ("A_sparse_s2", 2, 480, 640, True, 1000), ("B_dense_s10000", 10000, 480, 640, False, 2000),
             ("odd_517x389_s7", 7, 389, 517, False, 500)]
    for name, seed, h, w, sparse, nf in cases:
        img = synth_frame(seed, h, w, sparse)
        assert sha(img) == str(g[f"{name}/img_sha"])
        e = ext if nf == 1000 else ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
        gk, gd = e(img)
        assert_same_output(gk, gd, g[f"{name}/kps"], g[f"{name}/desc"])
        assert [sha(e.pyramid_level(l)) for l in range(8)] == g[f"{name}/level_sha"].tolist()
        assert [len(e.candidates(l)) for l in range(8)] == g[f"{name}/ncand"].tolist()


@pytest.mark.parametrize("h,w,nf,nlev,sf,ini,mn", [
    (480, 752, 1200, 8, 1.2, 20, 7),      # EuRoC-like aspect
    (376, 1241, 2000, 8, 1.2, 20, 7),     # KITTI-like: 3 quadtree roots
    (300, 300, 500, 8, 1.2, 20, 7),
    (240, 320, 300, 4, 1.5, 15, 5),
    (480, 640, 1000, 1, 1.2, 20, 7),      # single level
    (480, 640, 60, 8, 1.2, 20, 7),        # tiny N: some levels ask for < 4 features
    (480, 640, 3000, 8, 1.2, 40, 40),     # iniTh == minTh
    (233, 311, 400, 6, 1.3, 12, 3),
    (1400, 800, 800, 8, 1.2, 20, 7),      # tall (aspect just above the reference's limit of one quadtree root): long
                                          # vertical tap tables in the pyramid kernel's LDS, many row runs
    (300, 1000, 800, 6, 1.2, 20, 7),      # wide: four quadtree roots on every level
    (300, 1100, 800, 8, 1.2, 20, 7),      # wider: five roots on the upper levels
    (230, 1500, 600, 4, 1.2, 20, 7),      # panorama strip: seven to eight roots (the most the product carves LDS for)
    (480, 640, 500, 3, 1.95, 20, 7),      # scale factor close to the limit of 2 (source rows skipped by the walk)
    (301, 403, 500, 8, 1.01, 20, 7),      # scale factor close to 1 (almost every source row completes a destination row)
])
def test_parameter_sweep(oracle, h, w, nf, nlev, sf, ini, mn):
    from orb_slam2_ssd_semantic_amd import ORBextractor
    img = synth_frame(100 + h + w, h, w)
    oe = oracle.OracleExtractor(nf, sf, nlev, ini, mn)
    ok, od = oe(img, cap=nf + 16 * nlev + 64)
    e = ORBextractor(nf, sf, nlev, ini, mn, max_width=w, max_height=h)
    gk, gd = e(img)
    assert_same_output(gk, gd, ok, od)
    assert np.array_equal(e.GetScaleFactors(), oe.scales()[0])
    assert np.array_equal(e.GetInverseScaleSigmaSquares(), oe.scales()[3])
    assert np.array_equal(e.mnFeaturesPerLevel, oe.features_per_level())


def test_1080p_4000_features(oracle):
    """BASELINE config 5 frame shape: 1920x1080, 4000 features (one frame against the oracle)."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    img = synth_frame(20000, 1080, 1920)
    oe = oracle.OracleExtractor(4000, 1.2, 8, 20, 7)
    ok, od = oe(img, cap=4200)
    e = ORBextractor(4000, 1.2, 8, 20, 7, max_width=1920, max_height=1080)
    gk, gd = e(img)
    assert_same_output(gk, gd, ok, od)
    for l in (0, 3, 7):
        assert np.array_equal(e.candidates(l), cand_array(oe.candidates(l)))


def test_config5_batched_device_path_1080p_4000(oracle):
    """BASELINE config 5 through the path bench.py times: 32 distinct 1920x1080 frames, 4000 features, ONE
    orbfe_extract_batch_device call (level 0 asks for 869 keypoints: the largest quadtrees the LDS carve-up sees, grouped
    quadtree launches are off below 128 frames, so a second call with 130 frames covers the grouped launch path on a
    subset), every frame against the oracle: count, keypoint bit patterns, descriptors, order."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor
    w, h, nf = 1920, 1080, 4000
    oe = oracle.OracleExtractor(nf, 1.2, 8, 20, 7)
    imgs = [synth_frame(20000 + i, h, w, sparse=(i % 5 == 4)) for i in range(32)]
    ref = [oe(im, cap=4400) for im in imgs]
    e = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=130)
    cap = e.capacity()
    for B, order in ((32, list(range(32))), (130, [(7 * i) % 32 for i in range(130)])):
        d_gray = torch.from_numpy(np.stack([imgs[i] for i in order])).cuda()
        d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
        e.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.overflow() == 0
        n, kps, desc = d_n.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
        for b, i in enumerate(order):
            ok, od = ref[i]
            assert_same_output(kps[b, :n[b]].copy().view(KP_DTYPE).reshape(-1), desc[b, :n[b]], ok, od)
            assert not desc[b, n[b]:].any() and not kps[b, n[b]:].any()   # padding stays zero (all-gather ready)
        del d_gray, d_kps, d_desc, d_n


@pytest.mark.parametrize("seed,box", [(0, (200, 150, 96, 96)), (1, (19, 19, 60, 60)), (2, (500, 380, 120, 80)), (3, (300, 30, 40, 400))])
def test_clustered_corners_deep_quadtree(oracle, ext, seed, box):
    """All corners inside a small box.  Boxes 0-2: the reference quadtree stops as soon as a pass leaves the node count
    unchanged (one non-empty child), so only a couple of keypoints survive per level; box 3 (a tall strip) splits far
    below depth 5, where the kernel's histogram passes end and its streaming key passes take over."""
    x0, y0, bw, bh = box
    img = np.full((480, 640), 128, np.uint8)
    img[y0:y0 + bh, x0:x0 + bw] = synth_frame(900 + seed)[y0:y0 + bh, x0:x0 + bw]
    oe = oracle.OracleExtractor()
    ok, od = oe(img)
    gk, gd = ext(img)
    for l in range(8):
        assert np.array_equal(ext.candidates(l), cand_array(oe.candidates(l))), f"FAST candidates level {l}"
        assert np.array_equal(ext.selected(l), cand_array(oe.selected(l))), f"quadtree level {l}"
    assert_same_output(gk, gd, ok, od)


def test_streaming_quadtree_passes_only(oracle):
    """ORBFE_OPT_DEBUG = 50 disables the histogram passes: every pass streams over the keys (the deep-tree code path)."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    e = ORBextractor(1000, 1.2, 8, 20, 7, options={"debug": 50})
    for seed, sparse in ((0, False), (2, True)):
        img = synth_frame(seed, sparse=sparse)
        ok, od = oracle.OracleExtractor()(img)
        gk, gd = e(img)
        assert_same_output(gk, gd, ok, od)
    e.set_option("debug", 0)   # back to the default passes on the same handle (the plan is rebuilt)
    gk, gd = e(img)
    assert_same_output(gk, gd, ok, od)


@pytest.mark.parametrize("nf,h,w", [(3000, 480, 640), (10000, 480, 640), (20000, 1080, 1920)])
def test_large_nfeatures_node_arrays_beyond_the_lds(oracle, nf, h, w):
    """Any nfeatures the reference accepts (src/ORBextractor.cc:426-439 has no limit): beyond ~2400 features on one level
    the quadtree's node arrays no longer fit the CU's LDS and move to global scratch (k_octree<true>); 3000 is the largest
    LDS case of the three.  Single frame and a batch of 3 (different frames) against the oracle."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor
    imgs = [synth_frame(300 + i, h, w) for i in range(3)]
    oe = oracle.OracleExtractor(nf, 1.2, 8, 20, 7)
    ref = [oe(im, cap=nf + 4096) for im in imgs]
    assert len(ref[0][0]) > 0.9 * min(nf, 9000 if h == 480 else 10 ** 9)
    e = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=3)
    gk, gd = e(imgs[0])
    assert_same_output(gk, gd, *ref[0])
    oe0 = oracle.OracleExtractor(nf, 1.2, 8, 20, 7)   # oe holds the LAST frame's taps: frame 0's come from a handle of its own
    oe0(imgs[0], cap=nf + 4096)
    for l in (0, 7):
        assert np.array_equal(e.selected(l), cand_array(oe0.selected(l))), l
    cap = e.capacity()
    d_gray = torch.from_numpy(np.stack(imgs)).cuda()
    d_kps = torch.zeros((3, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(3, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_gray.data_ptr(), 3, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.overflow() == 0
    n, kps, desc = d_n.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    for b in range(3):
        assert_same_output(kps[b, :n[b]].copy().view(KP_DTYPE).reshape(-1), desc[b, :n[b]], *ref[b])


def test_generic_quadtree_passes_only(oracle):
    """ORBFE_OPT_DEBUG = 51 disables the fused breadth-first pass of the histogram mode: every pass goes through the generic node
    phase (the one the largest-first passes and the deep trees use) and must give the same trees."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    e = ORBextractor(1000, 1.2, 8, 20, 7, options={"debug": 51})
    for seed, sparse in ((0, False), (2, True), (5, False)):
        img = synth_frame(seed, sparse=sparse)
        oe = oracle.OracleExtractor()
        ok, od = oe(img)
        gk, gd = e(img)
        for l in range(8):
            assert np.array_equal(e.selected(l), cand_array(oe.selected(l))), f"quadtree level {l}"
        assert_same_output(gk, gd, ok, od)


def test_edge_cases(oracle, ext):
    from orb_slam2_ssd_semantic_amd import ORBextractor, OrbfeError, _ffi
    # empty image: silent return, outputs untouched (src/ORBextractor.cc:1055-1056)
    assert ext(np.zeros((0, 0), np.uint8)) == (None, None)
    L = _ffi.lib()
    n = C.c_int32(-5)
    assert L.orbfe_extract(ext.handle, None, 0, 0, 0, None, None, 0, C.byref(n)) == 0 and n.value == -5
    # flat image: zero keypoints (descriptors.release(), :1073-1074)
    k, d = ext(np.full((480, 640), 90, np.uint8))
    assert len(k) == 0 and d.shape == (0, 32)
    # non-contiguous rows (stride != width)
    img = synth_frame(5)
    wide = np.zeros((480, 800), np.uint8)
    wide[:, :640] = img
    k1, d1 = ext(img)
    k2, d2 = ext(wide[:, :640])
    assert np.array_equal(k1, k2) and np.array_equal(d1, d2)
    # frame larger than planned / smaller than one FAST cell per level -> ORBFE_ERR_SIZE
    with pytest.raises(OrbfeError) as ei:
        ext(np.zeros((481, 640), np.uint8))
    assert ei.value.status == _ffi.ORBFE_ERR_SIZE
    with pytest.raises(OrbfeError) as ei:
        ext(np.zeros((120, 160), np.uint8))
    assert ei.value.status == _ffi.ORBFE_ERR_SIZE
    # capacity too small -> ORBFE_ERR_CAP and n_out reports the need
    kps = np.zeros(10, _ffi.KP_DTYPE)
    desc = np.zeros((10, 32), np.uint8)
    st = L.orbfe_extract(ext.handle, img.ctypes.data_as(C.c_void_p), 640, 480, 640, kps.ctypes.data_as(C.c_void_p),
                         desc.ctypes.data_as(C.c_void_p), 10, C.byref(n))
    assert st == _ffi.ORBFE_ERR_CAP and n.value == len(k1)
    # smaller frame on the same handle re-plans; then back
    small = synth_frame(6, 300, 400)
    ks, ds = ext(small)
    oks, ods = oracle.OracleExtractor()(small)
    assert_same_output(ks, ds, oks, ods)
    k3, d3 = ext(img)
    assert np.array_equal(k1, k3) and np.array_equal(d1, d3)


def test_padded_pyramid_is_reflect101(oracle, ext):
    """mvImagePyramid with the 19-px BORDER_REFLECT_101 frame (src/ORBextractor.cc:1136-1142)."""
    img = synth_frame(8)
    ext(img)
    oe = oracle.OracleExtractor()
    oe(img)
    for l in (0, 1, 7):
        assert np.array_equal(ext.pyramid_level(l, with_border=True), oracle.copy_make_border101(oe.level(l), 19))
    # all levels in one device-to-host copy (what the extractor shim's mvImagePyramid is made of)
    padded = ext.padded_pyramid()
    for l in range(8):
        assert np.array_equal(padded[l], oracle.copy_make_border101(oe.level(l), 19)), l
    from orb_slam2_ssd_semantic_amd import ORBextractor
    e2 = ORBextractor(300, 1.31, 5, 20, 7, max_width=517, max_height=389, max_batch=3)     # odd sizes, frame 2 of a batch
    frames = np.stack([synth_frame(70 + i, 389, 517) for i in range(3)])
    e2.extract_batch(frames) if hasattr(e2, "extract_batch") else [e2(f) for f in frames]
    o2 = oracle.OracleExtractor(300, 1.31, 5, 20, 7)
    o2(frames[-1])
    padded = e2.padded_pyramid(frame=2 if hasattr(e2, "extract_batch") else 0)
    for l in range(5):
        assert np.array_equal(padded[l], oracle.copy_make_border101(o2.level(l), 19)), l


def test_batch_equals_single_and_is_idempotent(oracle, ext):
    imgs = [synth_frame(40 + i, sparse=(i % 3 == 0)) for i in range(11)]   # > max_batch: exercises chunking
    res = ext.extract_batch(imgs)
    oe = oracle.OracleExtractor()
    for i, (k, d) in enumerate(res):
        if i < 4:
            ok, od = oe(imgs[i])
            assert_same_output(k, d, ok, od)
        ks, ds = ext(imgs[i])
        assert np.array_equal(k, ks) and np.array_equal(d, ds)
    res2 = ext.extract_batch(imgs[::-1])[::-1]                               # order of frames is irrelevant
    for (k, d), (k2, d2) in zip(res, res2):
        assert np.array_equal(k, k2) and np.array_equal(d, d2)


def test_device_api_with_torch_tensors(oracle):
    """HBM-resident batched mode (what bench.py times): torch only provides memory and the stream."""
    import torch
    from orb_slam2_ssd_semantic_amd import ORBextractor
    B, cap = 6, 2112
    e = ORBextractor(2000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=B)
    assert cap >= e.capacity()
    frames = np.stack([synth_frame(10000 + i) for i in range(B)])
    d_gray = torch.from_numpy(frames).cuda()
    d_kps = torch.full((B, cap, 7), -1, dtype=torch.int32, device="cuda")
    d_desc = torch.full((B, cap, 32), 255, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    e.extract_batch_device(d_gray.data_ptr(), B, 640, 480, 640, 640 * 480, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                           d_n.data_ptr(), stream)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy()
    desc = d_desc.cpu().numpy()
    oe = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    from orb_slam2_ssd_semantic_amd import KP_DTYPE
    for i in range(B):
        ok, od = oe(frames[i], cap=cap)
        gk = kps[i, :n[i]].copy().view(KP_DTYPE).reshape(-1)
        assert_same_output(gk, desc[i, :n[i]], ok, od)
        assert not kps[i, n[i]:].any() and not desc[i, n[i]:].any()       # padding zero-filled for the all-gather


def test_batch_multiple_of_eight_xcd_placement(oracle):
    """16 distinct frames in one launch: the XCD-aware frame placement (batches that are a multiple of 8) and the
    level rotation of the quadtree grid must not change any frame's result."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    B = 16
    e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=B)
    imgs = [synth_frame(300 + i, sparse=(i % 4 == 1)) for i in range(B)]
    res = e.extract_batch(imgs)
    oe = oracle.OracleExtractor()
    for i, (k, d) in enumerate(res):
        ok, od = oe(imgs[i])
        assert_same_output(k, d, ok, od)


def test_scale_factor_limits(oracle):
    from orb_slam2_ssd_semantic_amd import ORBextractor, OrbfeError
    img = synth_frame(77, 480, 640)
    oe = oracle.OracleExtractor(500, 1.9, 3, 20, 7)          # just below the kernel's level-ratio limit of 2
    ok, od = oe(img, cap=700)
    gk, gd = ORBextractor(500, 1.9, 3, 20, 7, max_width=640, max_height=480)(img)
    assert_same_output(gk, gd, ok, od)
    with pytest.raises(OrbfeError):                          # a level less than half as wide as its parent
        ORBextractor(500, 2.5, 3, 20, 7, max_width=640, max_height=480)(img)


def test_exact_sized_input_buffer_is_never_overrun(oracle):
    """512 frames of 640x480 are exactly 150 MiB, so the allocation ends on a 2 MiB page boundary and any read past the
    last pixel faults (it did: an 8-byte row window of the pyramid kernel reached 7 bytes past the last row)."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor
    B, cap = 512, 1088
    e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=B)
    assert cap >= e.capacity()
    base = np.stack([synth_frame(900 + i) for i in range(4)])
    frames = np.ascontiguousarray(np.tile(base, (B // 4, 1, 1)))
    assert frames.nbytes % (2 << 20) == 0
    d_gray = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_gray.data_ptr(), B, 640, 480, 640, 640 * 480, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                           d_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    oe = oracle.OracleExtractor()
    for i in (0, 1, B - 2, B - 1):
        ok, od = oe(frames[i])
        gk = d_kps[i, :n[i]].cpu().numpy().copy().view(KP_DTYPE).reshape(-1)
        assert_same_output(gk, d_desc[i, :n[i]].cpu().numpy(), ok, od)


def test_host_batch_pipeline_pageable_and_pinned(oracle):
    """orbfe_extract_batch with more frames than max_batch: the three-stream pipeline over two buffer sets.  Pageable numpy
    frames with a row stride (staged) and page-locked torch tensors in and out (copied directly, padded rows zero-filled)
    must both give, frame by frame, what the oracle gives."""
    import ctypes as C
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor, _ffi
    N, w, h = 19, 640, 480
    frames = np.stack([synth_frame(800 + i, h, w, sparse=(i % 3 == 0)) for i in range(N)])
    oe = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    expect = [oe(f) for f in frames]
    for max_batch in (4, 8):
        e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=max_batch)
        cap = e.capacity()
        # (a) pageable, strided rows
        wide = np.zeros((N, h, w + 24), np.uint8)
        wide[:, :, :w] = frames
        arr = (C.c_void_p * N)(*[wide[i].ctypes.data for i in range(N)])
        kps = np.zeros((N, cap), KP_DTYPE)
        desc = np.zeros((N, cap, 32), np.uint8)
        n = np.zeros(N, np.int32)
        st = _ffi.lib().orbfe_extract_batch(e.handle, arr, N, w, h, w + 24, kps.ctypes.data, desc.ctypes.data, cap, n.ctypes.data)
        _ffi.check(st, "orbfe_extract_batch")
        for i in range(N):
            ok, od = expect[i]
            assert n[i] == len(ok) and np.array_equal(desc[i, :n[i]], od), (max_batch, i)
            assert np.array_equal(kps[i, :n[i]].view(np.uint8), ok.view(np.uint8)), (max_batch, i)
        # (b) page-locked in and out
        pf = torch.from_numpy(frames).pin_memory()
        pk = torch.full((N, cap, 7), -1, dtype=torch.int32).pin_memory()
        pd = torch.full((N, cap, 32), 7, dtype=torch.uint8).pin_memory()
        pn = torch.zeros(N, dtype=torch.int32).pin_memory()
        arr = (C.c_void_p * N)(*[pf[i].data_ptr() for i in range(N)])
        st = _ffi.lib().orbfe_extract_batch(e.handle, arr, N, w, h, w, pk.data_ptr(), pd.data_ptr(), cap, pn.data_ptr())
        _ffi.check(st, "orbfe_extract_batch")
        k2, d2, n2 = pk.numpy().view(KP_DTYPE).reshape(N, cap), pd.numpy(), pn.numpy()
        for i in range(N):
            ok, od = expect[i]
            assert n2[i] == len(ok) and np.array_equal(d2[i, :n2[i]], od), (max_batch, i)
            assert np.array_equal(k2[i, :n2[i]].view(np.uint8), ok.view(np.uint8)), (max_batch, i)
            assert not d2[i, n2[i]:].any() and not k2[i, n2[i]:].view(np.uint8).any()   # padded slots zero-filled
        assert e.overflow() == 0


def test_hip_path_equals_the_compiled_reference_directly():
    """No oracle in between: 48 frames (S, S vignetted, S_tum; 1000 and 2000 features) through one batched device call each,
    compared frame by frame with oracle/_ref -- the UNMODIFIED reference ORBextractor.cc compiled against the cv stub (bump
    allocator = creation-order tie-break, canonical cos/sin): counts, keypoint bit patterns, descriptors, order."""
    import torch
    from oracle import ref_ffi as R
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor
    from orb_slam2_ssd_semantic_amd.synth import synth_tum_like
    if not R.available():
        pytest.skip("oracle/_ref/libref_orb.so not present")
    R.configure(bump=True, canonical_trig=True, blur_mode=0)
    w, h, B = 640, 480, 24
    frames = np.stack([synth_frame(900 + i, h, w, sparse=(i % 3 == 1)) if i % 3 else synth_tum_like(900 + i, h, w) for i in range(B)])
    for nf in (1000, 2000):
        e = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
        cap = e.capacity()
        dg = torch.from_numpy(frames).cuda()
        dk = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        dn = torch.zeros(B, dtype=torch.int32, device="cuda")
        e.extract_batch_device(dg.data_ptr(), B, w, h, w, w * h, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.overflow() == 0
        n, kps, desc = dn.cpu().numpy(), dk.cpu().numpy(), dd.cpu().numpy()
        ref = R.RefExtractor(nf, 1.2, 8, 20, 7)
        for i in range(B):
            rk, rd = ref(frames[i], cap=nf + 128)
            gk = kps[i, :n[i]].copy().view(KP_DTYPE).reshape(-1)
            assert n[i] == len(rk), (nf, i)
            assert np.array_equal(gk.view(np.uint8), rk.view(np.uint8)) and np.array_equal(desc[i, :n[i]], rd), (nf, i)


def test_side_stream_blur_and_grouped_quadtree_equal_the_inline_single_launch_path(oracle, monkeypatch):
    """Batches of >= 128 frames run the blur on the handle's side stream next to the quadtree and launch the quadtree per
    level group; smaller batches (and ORBFE_OPT_OVERLAP = 0) keep one stream / one launch.  All of it must be invisible:
    136 frames through the large-batch path == the same frames in chunks of 8 through the small-batch path == overlap 0 / 1,
    and a sample of them == the oracle."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBextractor
    w, h, B = 640, 480, 136
    frames = np.stack([synth_frame(4000 + i, h, w, sparse=(i % 2 == 1)) for i in range(B)])
    dg = torch.from_numpy(frames).cuda()

    def run(chunk, env):
        e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=chunk,
                         options=None if env is None else {"overlap": int(env)})
        cap = e.capacity()
        dk = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        dn = torch.zeros(B, dtype=torch.int32, device="cuda")
        for i in range(0, B, chunk):
            e.extract_batch_device(dg[i:].data_ptr(), min(chunk, B - i), w, h, w, w * h, dk[i:].data_ptr(), dd[i:].data_ptr(), cap,
                                   dn[i:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.overflow() == 0
        return dn.cpu().numpy(), dk.cpu().numpy(), dd.cpu().numpy()

    n0, k0, d0 = run(B, None)
    for chunk, env in ((8, None), (B, "0"), (B, "1")):
        n1, k1, d1 = run(chunk, env)
        assert np.array_equal(n0, n1) and np.array_equal(k0, k1) and np.array_equal(d0, d1), (chunk, env)
    oe = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    for i in (0, 67, 135):
        ok, od = oe(frames[i], cap=1200)
        assert_same_output(k0[i, :n0[i]].copy().view(KP_DTYPE).reshape(-1), d0[i, :n0[i]], ok, od)


@pytest.mark.parametrize("updown", ["0", "2"])
def test_blur_row_walk_directions_give_the_same_levels(oracle, updown):
    """ORBFE_OPT_BLUR_UPDOWN: odd row blocks of k_blur7 walk upwards (the 7 x 7 kernel is vertically symmetric) so that neighbouring
    blocks read their shared halo rows at the same time; default 1 = only where it adds no wave, 2 = everywhere, 0 = nowhere.
    Every setting gives the oracle's blurred levels byte for byte, in both rounding modes, on sizes whose last row block is short
    and on single frames (short runs) as well as batches (40-row runs)."""
    from orb_slam2_ssd_semantic_amd import ORBextractor
    for (w, h, nf, nlev, sf, mode, mb) in ((640, 480, 1000, 8, 1.2, 0, 16), (517, 389, 700, 6, 1.3, 1, 16), (333, 271, 400, 4, 1.5, 0, 1),
                                           (752, 480, 1200, 8, 1.2, 1, 9)):
        e = ORBextractor(nf, sf, nlev, 20, 7, max_width=w, max_height=h, max_batch=mb, blur_rounding=mode,
                         options={"blur_updown": int(updown)})
        oe = oracle.OracleExtractor(nf, sf, nlev, 20, 7)
        oe.set_blur_mode(mode)
        frames = [synth_frame(900 + i, h, w, sparse=(i == 1)) for i in range(min(mb, 3))]
        res = e.extract_batch(np.stack(frames)) if mb > 1 else [e(frames[0])]
        for i, img in enumerate(frames):
            ok, od = oe(img)
            assert_same_output(res[i][0], res[i][1], ok, od)
        # blurred levels of frame 0 of a fresh single call
        gk, gd = e(frames[0])
        ok, od = oe(frames[0])
        for l in range(nlev):
            if len(oe.selected(l)):
                assert np.array_equal(e.blurred_level(l), oe.blurred(l)), (w, l, updown)
        assert_same_output(gk, gd, ok, od)
