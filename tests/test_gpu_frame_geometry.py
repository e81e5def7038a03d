"""csrc/orbfe_frame.hip on the GPU against tests/undistort_oracle.py, float bit patterns throughout: cv::undistortPoints on a point
table, UndistortKeyPoints + ComputeStereoFromRGBD on real extractor blocks, the depth conversions, the device-resident RGB-D Frame
chain into the grid, the host form against the batch form, and the cv::undistortPoints shim."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import undistort_oracle as U

pytestmark = pytest.mark.gpu
W, H = U.W, U.H
F32 = np.float32


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_class(got, want):
    """bit-equal where the oracle is finite; NaN / +-inf by class elsewhere"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(u32(got[fin]), u32(want[fin]))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])


def point_table(K, seed=0):
    """the integer lattice of the frame, random points inside it and up to 50 px outside, the corners, (cx, cy)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H + 1, 0:W + 1]
    lat = np.stack([xs.ravel(), ys.ravel()], 1)
    inside = rng.uniform([0, 0], [W, H], (20000, 2))
    outside = rng.uniform([-50, -50], [W + 50, H + 50], (20000, 2))
    corners = [[0, 0], [W, 0], [0, H], [W, H], [-50, -50], [W + 50, H + 50]]
    centre = [[K[0, 2], K[1, 2]]]
    return np.concatenate([lat, inside, outside, corners, centre]).astype(F32)


def _synthetic(n):
    d = np.zeros(n, F32)
    d[:5] = (0.1, -0.2, 0.001, -0.002, 0.05)
    d[5:8] = (0.02, -0.01, 0.005)
    if n == 12:
        d[8:] = (0.001, -0.0005, 0.0007, -0.0003)
    return d[:n]


def camera_sets():
    K1, K2 = U.camera_matrix(U.TUM1), U.camera_matrix(U.TUM2)
    tilt = K1.copy()
    tilt[2] = (1e-4, -2e-4, 1.0)   # a P with a non-trivial third row
    sets = []
    for cfg, K in ((U.TUM1, K1), (U.TUM2, K2)):
        for nd in (4, 5):
            sets.append((U.dist_coeffs(cfg, nd), K, K))
    sets += [(_synthetic(8), K1, K1), (_synthetic(12), K2, K2), (U.dist_coeffs(U.TUM1), K1, None), (U.dist_coeffs(U.TUM2), K2, tilt),
             (np.array([], F32), K1, K1), (np.array([0.0, 0.3, 0.0, 0.0], F32), K1, K1)]
    # denominators that cross zero inside the table: 1 + k1 r2 (k1 = -2: at r2 = 0.5), and P's third row (1, 0, 0), whose
    # ww = 1 / x is 1 / 0 at the point (cx, cy) without coefficients -- inf / NaN compared by class
    cross = K1.copy()
    cross[2] = (1.0, 0.0, 0.0)
    sets.append((np.array([-2.0, 0.0, 0.0, 0.0, 0.0], F32), K1, K1))
    sets.append((np.array([-2.0, 0.0, 0.0, 0.0, 0.0], F32), K1, None))
    sets.append((np.array([], F32), K1, cross))
    sets.append((U.dist_coeffs(U.TUM1), K1, cross))
    sets.append((np.array([], F32), K1, np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], F32)))   # 0 * inf at (cx, cy): NaN
    return sets


def test_undistort_points_equal_the_oracle():
    from orb_slam2_ssd_semantic_amd import Camera
    crossed = 0
    for i, (d, K, P) in enumerate(camera_sets()):
        pts = point_table(K, i)
        cam = Camera(K, d, 40.0, P=P)
        got = cam.undistort_points(pts)
        want = U.undistort_points(pts, K, d, P)
        same_class(got, want)
        crossed += int((~np.isfinite(want)).sum())
        cam.close()
    assert crossed > 0


def _extract(frames, nf):
    import torch
    from orb_slam2_ssd_semantic_amd import ORBextractor
    B, h, w = frames.shape
    e = ORBextractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = e.capacity()
    dg = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    dk = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    dn = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(dg.data_ptr(), B, w, h, w, w * h, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert e.overflow() == 0
    e.close()
    return dg, dk, dd, dn, cap


@pytest.fixture(scope="module")
def frames():
    from orb_slam2_ssd_semantic_amd import photos
    from orb_slam2_ssd_semantic_amd.synth import synth_frames_parallel
    tum = synth_frames_parallel("S_tum", 64, H, W, 4100, max_procs=16)
    real = np.stack([g for _, g in photos.vga_gray_frames()])
    return np.concatenate([tum, real])


def _frame_cams():
    k1zero = np.array([0.0, -0.953104, -0.005358, 0.002628, 1.163314], F32)   # k1 = 0, k2 != 0: not undistorted (Frame.cc:752)
    return [("TUM1", U.camera_matrix(U.TUM1), U.dist_coeffs(U.TUM1)), ("TUM2", U.camera_matrix(U.TUM2), U.dist_coeffs(U.TUM2)),
            ("TUM3", U.camera_matrix(U.TUM3), U.dist_coeffs(U.TUM3)), ("k1=0", U.camera_matrix(U.TUM1), k1zero)]


def test_frame_geometry_on_extractor_blocks(frames):
    """64 S_tum frames and the real-photograph set, 1000 and 2000 features, TUM1 / TUM2 / TUM3 and k1 = 0 with k2 != 0: keysUn per
    frame equal to the oracle, every other field untouched, slots >= n zero, no depth plane -> -1 / -1."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera
    B = len(frames)
    undistorted = 0
    for nf in (1000, 2000):
        _, dk, _, dn, cap = _extract(frames, nf)
        kk = dk.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
        nn = dn.cpu().numpy()
        for name, K, d in _frame_cams():
            cam = Camera(K, d, 40.0)
            sentinel = torch.full_like(dk, 0x5A5A5A5A)
            ku, dep, ur = cam.frame_geometry(dk, dn, cap, kps_un=sentinel)
            torch.cuda.synchronize()
            gu = ku.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
            gd, gr = dep.cpu().numpy(), ur.cpu().numpy()
            for i in range(B):
                n = int(nn[i])
                k = kk[i, :n]
                want, wd, wr = U.frame_geometry(k, K, d, 40.0)
                assert np.array_equal(u32(gu[i, :n]["x"]), u32(want["x"])) and np.array_equal(u32(gu[i, :n]["y"]), u32(want["y"])), (nf, name, i)
                for f in ("size", "angle", "response", "octave", "class_id"):
                    assert np.array_equal(gu[i, :n][f].view(np.uint32), k[f].view(np.uint32)), (nf, name, i, f)
                if name in ("TUM3", "k1=0"):
                    assert np.array_equal(gu[i, :n].view(np.uint8), k.view(np.uint8)), (nf, name, i)
                else:
                    undistorted += int((gu[i, :n]["x"] != k["x"]).sum())
                assert np.array_equal(u32(gd[i, :n]), u32(wd)) and np.array_equal(u32(gr[i, :n]), u32(wr))
                assert not gu[i, n:].view(np.uint8).any() and not gd[i, n:].any() and not gr[i, n:].any(), (nf, name, i)
            cam.close()
    assert undistorted > 100000, undistorted


def _depth_planes(rng, h, w):
    holes = rng.random((h, w)) < 0.2
    tum = rng.integers(2500, 40000, (h, w)).astype(np.uint16)   # 0.5 m .. 8 m at 5000 per metre
    tum[holes] = 0
    full = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    full[:2, :8] = (0, 1, 2, 65534, 65535, 32768, 4999, 5000)
    return [("u16_tum", tum), ("u16_full", full)]


def test_depth_and_uright(frames):
    """u16 planes with holes, TUM-like values and the full range at scales 1/5000f, 1/5208f and 1; f32 planes at scale 1 and not 1
    (with zeros, negatives and -0); a plane smaller than the frame (keypoints outside it have no depth); depth / uRight bit-exact."""
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera
    sub = frames[:6]
    B = len(sub)
    _, dk, _, dn, cap = _extract(sub, 1000)
    kk = dk.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    nn = dn.cpu().numpy()
    K, d = U.camera_matrix(U.TUM1), U.dist_coeffs(U.TUM1)
    cam = Camera(K, d, 40.0)
    rng = np.random.default_rng(11)
    planes = []
    for hh, ww in ((H, W), (400, 600)):
        for tag, p in _depth_planes(rng, hh, ww):
            planes.append((tag, np.stack([p] * B)))
        f = rng.uniform(-1, 9, (B, hh, ww)).astype(F32)
        f[rng.random(f.shape) < 0.1] = 0
        f[:, 0, :4] = (-0.0, 0.0, 1e-30, 3e38)
        planes.append(("f32", f))
    seen = 0
    for tag, p in planes:
        scales = (U.depth_scale(U.TUM1), U.depth_scale(U.TUM2), F32(1.0)) if p.dtype == np.uint16 else (F32(1.0), F32(1.0000001), F32(0.25))
        dp = torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).cuda()
        for s in scales:
            ku, dep, ur = cam.frame_geometry(dk, dn, cap, depth=dp, scale=float(s))
            torch.cuda.synchronize()
            gd, gr = dep.cpu().numpy(), ur.cpu().numpy()
            for i in range(B):
                n = int(nn[i])
                _, wd, wr = U.frame_geometry(kk[i, :n], K, d, 40.0, p[i], s)
                assert np.array_equal(u32(gd[i, :n]), u32(wd)) and np.array_equal(u32(gr[i, :n]), u32(wr)), (tag, p.shape, s, i)
                assert not gd[i, n:].any() and not gr[i, n:].any()
                seen += int((wd > 0).sum())
                if p.shape[1] < H:
                    out = (kk[i, :n]["x"] >= p.shape[2]) | (kk[i, :n]["y"] >= p.shape[1])
                    assert out.any() and (gd[i, :n][out] == -1).all() and (gr[i, :n][out] == -1).all()
            # the whole-plane conversion: u.astype(float32) * float32(scale) under Tracking's condition
            got = Camera.depth_to_float(dp, float(s)).cpu().numpy()
            assert np.array_equal(u32(got), u32(U.depth_to_float(p, s))), (tag, s)
            if p.dtype == np.uint16:
                assert np.array_equal(u32(got), u32(p.astype(F32) * F32(s)))
    assert seen > 10000
    # odd widths and padded rows take the element-wise path
    p = rng.integers(0, 65536, (3, 37, 53)).astype(np.uint16)
    big = torch.zeros((3, 37, 64), dtype=torch.int16, device="cuda")
    big[:, :, :53] = torch.from_numpy(p.view(np.int16)).cuda()
    got = Camera.depth_to_float(big[:, :, :53], float(U.depth_scale(U.TUM2))).cpu().numpy()
    assert np.array_equal(u32(got), u32(p.astype(F32) * U.depth_scale(U.TUM2)))
    cam.close()


def test_rgbd_frame_chain_on_one_stream(frames):
    """orbfe_extract_batch_device -> orbfe_flow_compute_masks_device -> orbfe_mask_keypoints_device -> frame geometry ->
    orbfe_assign_grid_batch_device with the orbfe_image_bounds outputs, all on one stream: every frame's grid equals
    oracle_ffi.assign_grid on the oracle's keysUn of the masked keypoints, and depth / uRight equal the oracle's."""
    import torch
    from oracle import oracle_ffi as O
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera, Flow, ORBmatcher
    from orb_slam2_ssd_semantic_amd import flow as FL
    sub = np.ascontiguousarray(frames[:8])
    B = len(sub)
    st = torch.cuda.current_stream().cuda_stream
    dg, dk, dd, dn, cap = _extract(sub, 1000)
    fl = Flow(W, H, max_batch=B)
    masks, ones = fl.compute_masks(dg, 40.0, stream=st)
    FL.mask_keypoints(masks, ones, dk, dd, dn, cap, stream=st)
    rng = np.random.default_rng(5)
    depth = rng.integers(0, 30000, (B, H, W)).astype(np.uint16)
    d_depth = torch.from_numpy(depth.view(np.int16)).cuda()
    for cfg in (U.TUM1, U.TUM2):
        K, d = U.camera_matrix(cfg), U.dist_coeffs(cfg)
        cam = Camera(K, d, cfg["bf"])
        minx, maxx, miny, maxy, gwi, ghi = cam.image_bounds(W, H)
        assert np.array_equal(u32([minx, maxx, miny, maxy, gwi, ghi]), u32(U.image_bounds(K, d, W, H)))
        ku, dep, ur = cam.frame_geometry(dk, dn, cap, depth=d_depth, scale=float(U.depth_scale(cfg)), stream=st)
        g_off = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
        g_idx = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        g_nin = torch.zeros(B, dtype=torch.int32, device="cuda")
        ORBmatcher(0.9, True).AssignFeaturesToGrid_batch_device(ku.data_ptr(), dn.data_ptr(), cap, B, minx, miny, gwi, ghi,
                                                                g_off.data_ptr(), g_idx.data_ptr(), g_nin.data_ptr(), st)
        torch.cuda.synchronize()
        kk = dk.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
        nn = dn.cpu().numpy()
        off, idx, nin = g_off.cpu().numpy().view(np.uint32), g_idx.cpu().numpy().view(np.uint32), g_nin.cpu().numpy()
        gd, gr = dep.cpu().numpy(), ur.cpu().numpy()
        for i in range(B):
            n = int(nn[i])
            want, wd, wr = U.frame_geometry(kk[i, :n], K, d, cfg["bf"], depth[i], U.depth_scale(cfg))
            roff, ridx = O.assign_grid(np.stack([want["x"], want["y"]], 1), float(minx), float(miny), float(gwi), float(ghi))
            assert nin[i] == len(ridx) and np.array_equal(off[i], roff) and np.array_equal(idx[i, :nin[i]], ridx), i
            assert np.array_equal(u32(gd[i, :n]), u32(wd)) and np.array_equal(u32(gr[i, :n]), u32(wr)), i
        cam.close()
    fl.close()


def test_host_form_equals_batch_form(frames):
    import torch
    from orb_slam2_ssd_semantic_amd import KP_DTYPE, Camera
    sub = frames[64:72]
    B = len(sub)
    _, dk, _, dn, cap = _extract(sub, 2000)
    kk = dk.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    nn = dn.cpu().numpy()
    for cfg in (U.TUM1, U.TUM2):
        cam = Camera(U.camera_matrix(cfg), U.dist_coeffs(cfg), 40.0)
        ku, _, _ = cam.frame_geometry(dk, dn, cap)
        torch.cuda.synchronize()
        gu = ku.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
        for i in range(B):
            n = int(nn[i])
            host = cam.undistort_points(np.stack([kk[i, :n]["x"], kk[i, :n]["y"]], 1))
            assert np.array_equal(u32(host[:, 0]), u32(gu[i, :n]["x"])) and np.array_equal(u32(host[:, 1]), u32(gu[i, :n]["y"])), i
        cam.close()


def test_undistort_points_shim_equals_the_oracle(tmp_path):
    from test_undistort_oracle import build_shim
    exe = build_shim(tmp_path / "test_undistort_points")
    for cfg in (U.TUM1, U.TUM2):
        K, d = U.camera_matrix(cfg), U.dist_coeffs(cfg)
        pts = point_table(K, 3)[::7]
        inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(inp, "wb") as f:
            K.astype(F32).tofile(f)
            np.array([len(d)], np.int32).tofile(f)
            d.astype(F32).tofile(f)
            np.array([len(pts)], np.int32).tofile(f)
            pts.tofile(f)
        r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(out, F32).reshape(-1, 2)
        assert np.array_equal(u32(got), u32(U.undistort_points(pts, K, d, K)))
