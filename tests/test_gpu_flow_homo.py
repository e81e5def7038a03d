"""FlowSLAM::Flow::ComputeMask(GrayImg, Homo, mask, th) on the GPU (csrc/orbfe_flow.hip: k_flow_homo_prep, k_flow_warp,
k_flow_pyrdown_sel) against tests/warp_oracle.py + tests/flow_oracle.py, bit for bit: the warped frame over a table of
homographies and frame sizes, every stage of a host call, the device sequence with mixed tracked / lost frames against host
calls and against the plain sequence form, the chain into the masked Frame rule against the compiled reference, and the
shim's homography overload."""
import os
import subprocess

import numpy as np
import pytest

import flow_oracle as FO
import warp_cases as WC
import warp_oracle as WO
from orb_slam2_ssd_semantic_amd import KP_DTYPE, Flow, _ffi
from orb_slam2_ssd_semantic_amd import flow as FL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def camera_pair(w=640, h=480, seed=21):
    """(a, b, H): a planar scene and a moving patch; between a and b the camera moves by G and the patch by its own motion;
    H = G^-1 maps b onto a (TrackHomo's estimate)"""
    canvas = WC.smooth_canvas(seed, w, h)
    s = w // 5
    patch = np.round(WC.smooth_canvas(seed + 1, s, s)[:s, :s]).astype(np.uint8)
    G = WC.motion(w, h)
    x0, y0 = w * 3 // 8, h // 3
    a = WC.with_patch(WC.view(canvas, np.eye(3), w, h), patch, x0, y0)
    b = WC.with_patch(WC.view(canvas, G, w, h), patch, x0 + 14, y0 + 10)
    return a, b, np.linalg.inv(G)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", WC.SIZES)
def test_warp_tap_bit_exact_over_the_table(w, h):
    fl = Flow(w, h)
    bad = []
    for k, name in enumerate(WC.H_NAMES):
        H = WC.homography(name, w, h)
        g = WC.frame(100 + k, w, h)
        fl.reset()
        m = fl.compute_mask(g, 40.0, homography=H)
        want = WO.warp(g, H)
        got = fl.tap(0, FL.TAP_WARP)
        if not np.array_equal(got, want):
            bad.append((name, int(np.count_nonzero(got != want))))
        assert m.all()   # the first frame: all ones
        assert np.array_equal(fl.tap(0, FL.TAP_HALF), FO.pyr_down_u8(want)), name
    fl.close()
    assert not bad, f"{w}x{h}: pixels differing per homography: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("th", [40.0, 100.0])
def test_host_call_with_homography_every_stage_bit_exact(th):
    a, b, H = camera_pair()
    fl, of = Flow(640, 480), FO.Flow()
    assert np.array_equal(fl.compute_mask(a, th), of.compute_mask(a, th))
    m = fl.compute_mask(b, th, homography=H)
    om = WO.compute_mask_homo(of, b, H, th)
    assert np.array_equal(fl.tap(0, FL.TAP_WARP), of.taps["warp"]), "warp"
    assert np.array_equal(fl.tap(0, FL.TAP_HALF), of.taps["half"]), "half"
    for lv, ofl in enumerate(of.taps["flow_levels"][::-1]):
        got = fl.tap(0, FL.TAP_FLOW, lv)
        assert got.shape == ofl.shape and np.array_equal(_bits(got), _bits(ofl)), f"flow level {lv}"
    assert np.array_equal(_bits(fl.tap(0, FL.TAP_FLOW2)), _bits(of.taps["flow2"])), "flow2"
    assert np.array_equal(fl.tap(0, FL.TAP_PRE), of.taps["mask_pre"]), "pre-morphology mask"
    assert np.array_equal(fl.tap(0, FL.TAP_MASK), of.taps["mask"]), "mask"
    assert np.array_equal(m, om)
    assert 0 < (m == 0).mean() < 0.2   # the patch, not the camera motion
    # a float32 matrix is widened exactly, as Mat::convertTo does
    fl.reset()
    of.reset()
    H32 = H.astype(np.float32)
    fl.compute_mask(a, th)
    of.compute_mask(a, th)
    assert np.array_equal(fl.compute_mask(b, th, homography=H32), WO.compute_mask_homo(of, b, H32, th))
    fl.close()


@pytest.mark.gpu
def test_plain_call_after_a_warped_one_continues_from_the_warped_state():
    frames, Hs = WC.planar_sequence(41, 4, 320, 240, k=1.0)
    fl, of = Flow(320, 240), FO.Flow()
    want, got = [], []
    got.append(fl.compute_mask(frames[0], 40.0))
    want.append(of.compute_mask(frames[0], 40.0))
    got.append(fl.compute_mask(frames[1], 40.0, homography=Hs[1]))
    want.append(WO.compute_mask_homo(of, frames[1], Hs[1], 40.0))
    got.append(fl.compute_mask(frames[2], 40.0))                 # lost: the plain overload, against the warped state
    want.append(of.compute_mask(frames[2], 40.0))
    assert np.array_equal(fl.tap(0, FL.TAP_MASK), of.taps["mask"])
    buf = np.zeros(320 * 240, np.uint8)
    assert _ffi.lib().orbfe_flow_tap(fl.h, 0, FL.TAP_WARP, 0, _ffi.ptr(buf), buf.size, None, None) == _ffi.ORBFE_ERR_STATE
    got.append(fl.compute_mask(frames[3], 40.0, homography=Hs[3]))
    want.append(WO.compute_mask_homo(of, frames[3], Hs[3], 40.0))
    for i, (g, e) in enumerate(zip(got, want)):
        assert np.array_equal(g, e), i
    fl.close()


def _sequence(n, w, h):
    """n frames of a planar scene under steady motion with a patch moving on it from frame 40 on; H_i maps frame i onto i-1;
    use: tracked (1) or lost (0) in runs, as TrackHomo succeeds or fails"""
    frames, Hs = WC.planar_sequence(51, n, w, h, k=0.15)
    patch = np.round(WC.smooth_canvas(52, 64, 64)[:64, :64]).astype(np.uint8)
    for i in range(40, n):
        frames[i] = WC.with_patch(frames[i], patch, 100 + 3 * (i - 40), 60 + (i - 40))
    use = np.ones(n, np.int32)
    use[0] = 0
    use[5:8] = 0
    use[30] = 0
    use[62:67] = 0      # around the 64-frame pass boundary
    return frames, np.stack(Hs).astype(np.float64), use


@pytest.mark.gpu
def test_device_sequence_equals_host_calls_with_mixed_use():
    import torch
    n, w, h = 70, 320, 240
    frames, Hs, use = _sequence(n, w, h)
    host = Flow(w, h)
    want = [host.compute_mask(f, 40.0, homography=Hs[i] if use[i] else None) for i, f in enumerate(frames)]
    host.close()
    assert any(not m.all() for m in want[41:])
    fl = Flow(w, h, max_batch=128)
    d = torch.from_numpy(np.stack(frames)).cuda()
    dH = torch.from_numpy(Hs).cuda()
    du = torch.from_numpy(use).cuda()

    def check(got, ones, lo, label):
        got, ones = got.cpu().numpy(), ones.cpu().numpy()
        for i in range(len(got)):
            assert np.array_equal(got[i], want[lo + i]), (label, lo + i)
            assert ones[i] == int(want[lo + i].sum()), (label, lo + i)

    m, o = fl.compute_masks(d, 40.0, homographies=dH, use=du)     # one call: two internal passes (64 + 6)
    torch.cuda.synchronize()
    check(m, o, 0, "one call")
    assert use[69] and not use[66]   # the taps hold the last pass: frames 64..69 of the call
    assert np.array_equal(fl.tap(69, FL.TAP_WARP), WO.warp(frames[69], Hs[69]))
    buf = np.zeros(w * h, np.uint8)
    assert _ffi.lib().orbfe_flow_tap(fl.h, 66, FL.TAP_WARP, 0, _ffi.ptr(buf), buf.size, None, None) == _ffi.ORBFE_ERR_STATE
    fl.reset()
    m1, o1 = fl.compute_masks(d[:37], 40.0, homographies=dH[:37], use=du[:37])
    m2, o2 = fl.compute_masks(d[37:], 40.0, homographies=dH[37:], use=du[37:])   # the state crosses the calls
    torch.cuda.synchronize()
    check(m1, o1, 0, "first of two")
    check(m2, o2, 37, "second of two")
    # after reset: frame 10 has no previous frame; the rest as host calls from there
    fl.reset()
    m3, _ = fl.compute_masks(d[10:20], 40.0, homographies=dH[10:20], use=du[10:20])
    torch.cuda.synchronize()
    host = Flow(w, h)
    for i in range(10, 20):
        e = host.compute_mask(frames[i], 40.0, homography=Hs[i] if use[i] else None)
        assert np.array_equal(m3[i - 10].cpu().numpy(), e), ("after reset", i)
    host.close()
    # use = None: every frame warped
    fl.reset()
    host = Flow(w, h)
    m4, _ = fl.compute_masks(d[:5], 40.0, homographies=dH[:5])
    torch.cuda.synchronize()
    for i in range(5):
        assert np.array_equal(m4[i].cpu().numpy(), host.compute_mask(frames[i], 40.0, homography=Hs[i])), ("use None", i)
    host.close()
    fl.close()


@pytest.mark.gpu
def test_device_sequence_with_use_all_zero_equals_the_plain_form():
    import torch
    n, w, h = 70, 320, 240
    frames, Hs, _ = _sequence(n, w, h)
    d = torch.from_numpy(np.stack(frames)).cuda()
    dH = torch.from_numpy(Hs).cuda()
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    a, b = Flow(w, h, max_batch=128), Flow(w, h, max_batch=128)
    ma, oa = a.compute_masks(d, 40.0, homographies=dH, use=zero)
    mb, ob = b.compute_masks(d, 40.0)
    torch.cuda.synchronize()
    assert torch.equal(ma, mb) and torch.equal(oa, ob)
    buf = np.zeros(w * h, np.uint8)
    for f in (a, b):   # no frame was warped (frame 69: in the last pass, which the taps hold)
        assert _ffi.lib().orbfe_flow_tap(f.h, 69, FL.TAP_WARP, 0, _ffi.ptr(buf), buf.size, None, None) == _ffi.ORBFE_ERR_STATE
    a.close()
    b.close()


@pytest.mark.gpu
def test_homo_entry_points_reject_bad_arguments():
    import torch
    fl = Flow(320, 240, max_batch=4)
    g = np.zeros((240, 320), np.uint8)
    m = np.zeros_like(g)
    L = _ffi.lib()
    assert L.orbfe_flow_compute_mask_homo(fl.h, _ffi.ptr(g), 320, 240, 320, None, 40.0, _ffi.ptr(m), 320) == _ffi.ORBFE_ERR_ARG
    d = torch.zeros((5, 240, 320), dtype=torch.uint8, device="cuda")
    dm = torch.zeros_like(d)
    dH = torch.zeros((5, 3, 3), dtype=torch.float64, device="cuda")
    assert L.orbfe_flow_compute_masks_homo_device(fl.h, d.data_ptr(), 1, 320, 240, 320, 320 * 240, None, None, 40.0, dm.data_ptr(),
                                                  320, 320 * 240, None, None) == _ffi.ORBFE_ERR_ARG
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_masks(d, 40.0, homographies=dH)   # more than max_batch
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    with pytest.raises(_ffi.OrbfeError) as e:
        fl.compute_mask(np.zeros((8, 8), np.uint8), 40.0, homography=np.eye(3))
    assert e.value.status == _ffi.ORBFE_ERR_SIZE
    with pytest.raises(ValueError):
        fl.compute_mask(g, 40.0, homography=np.eye(2))
    with pytest.raises(ValueError):
        fl.compute_masks(d[:2], 40.0, homographies=dH[:2].float())
    fl.close()


@pytest.mark.gpu
def test_chain_extract_warped_masks_keypoints_equals_reference_masked_frame():
    """orbfe_extract_batch_device -> orbfe_flow_compute_masks_homo_device -> orbfe_mask_keypoints_device, against the compiled
    reference's masked Frame constructor given the same frame and the oracle's warped mask"""
    import torch
    from oracle import ref_ffi as R
    from orb_slam2_ssd_semantic_amd import ORBextractor
    R.configure(bump=True, canonical_trig=True, blur_mode=0)
    h, w = 480, 640
    a, b, H = camera_pair(w, h, seed=61)
    frames = np.stack([a, b])
    Hs = np.stack([np.eye(3), H])
    use = np.array([0, 1], np.int32)
    B = len(frames)
    ext = ORBextractor(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=B)
    cap = ext.capacity()
    st = torch.cuda.current_stream().cuda_stream
    d_gray = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    ext.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    fl = Flow(w, h, max_batch=B)
    masks, ones = fl.compute_masks(d_gray, 40.0, homographies=torch.from_numpy(Hs).cuda(), use=torch.from_numpy(use).cuda())
    FL.mask_keypoints(masks, ones, d_kps, d_desc, d_n, cap)
    torch.cuda.synchronize()
    of = FO.Flow()
    omasks = [of.compute_mask(a, 40.0), WO.compute_mask_homo(of, b, H, 40.0)]
    assert np.array_equal(masks.cpu().numpy(), np.stack(omasks))
    assert omasks[0].all() and 0.65 < omasks[1].mean() < 1.0   # the warped mask filters: only the patch goes
    kk = d_kps.cpu().numpy().view(KP_DTYPE).reshape(B, cap)
    dd = d_desc.cpu().numpy()
    nn = d_n.cpu().numpy()
    ref_ext = R.RefExtractor(1000, 1.2, 8, 20, 7)
    depth = np.ones((h, w), np.float32)
    for i in range(B):
        got = R.frame_ctor(R.FRAME_MASKED, frames[i], depth, omasks[i], extractor=ref_ext)
        n = int(nn[i])
        assert got["N"] == n, (i, got["N"], n)
        assert np.array_equal(kk[i, :n].view(np.uint8), got["keys"][:n].view(np.uint8))
        assert np.array_equal(dd[i, :n], got["desc"][:n])
        assert not kk[i, n:].view(np.uint8).any() and not dd[i, n:].any()
    fl.close()


@pytest.mark.gpu
def test_shim_homography_overload_equals_the_oracle(tmp_path):
    """shim/Flow_orbfe.cc built against the stub: ComputeMask(a) then ComputeMask(b, Homo) with a CV_64F and a CV_32F matrix"""
    from orb_slam2_ssd_semantic_amd import _build
    lib = _build.build()
    shim = os.path.join(ROOT, "orb_slam2_ssd_semantic_amd", "shim")
    w, h = 320, 240
    a, b, H = camera_pair(w, h, seed=71)
    (tmp_path / "a.u8").write_bytes(a.tobytes())
    (tmp_path / "b.u8").write_bytes(b.tobytes())
    (tmp_path / "h.f64").write_bytes(H.astype(np.float64).tobytes())
    main = tmp_path / "main.cpp"
    main.write_text('#include <cstdio>\n#include "Flow.h"\n'
                    'static void rd(const char *p, void *d, size_t n) { FILE *f = fopen(p, "rb"); if (!f || fread(d, 1, n, f) != n) throw 1; fclose(f); }\n'
                    'static void wr(const char *p, const cv::Mat &m) { FILE *f = fopen(p, "wb");\n'
                    '    for (int r = 0; r < m.rows; r++) fwrite(m.ptr(r), 1, m.cols, f); fclose(f); }\n'
                    'int main(int argc, char **argv) {\n'
                    '    const int w = %d, h = %d;\n'
                    '    cv::Mat a(h, w, CV_8U), b(h, w, CV_8U), H(3, 3, CV_64F), H32(3, 3, CV_32F), m;\n'
                    '    rd(argv[1], a.ptr(0), (size_t)w * h); rd(argv[2], b.ptr(0), (size_t)w * h); rd(argv[3], H.ptr(0), 72);\n'
                    '    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) H32.at<float>(r, c) = (float)H.at<double>(r, c);\n'
                    '    FlowSLAM::Flow f, g;\n'
                    '    f.ComputeMask(a, m, 40.f); f.ComputeMask(b, H, m, 40.f); wr(argv[4], m);\n'
                    '    g.ComputeMask(a, m, 40.f); g.ComputeMask(b, H32, m, 40.f); wr(argv[5], m);\n'
                    '    return 0;\n'
                    '}\n' % (w, h))
    exe = tmp_path / "flow_shim_homo"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", shim, str(main),
                           os.path.join(shim, "Flow_orbfe.cc"), "-L", os.path.dirname(lib), "-lorbfe",
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    outs = [tmp_path / "m64.u8", tmp_path / "m32.u8"]
    r = subprocess.run([str(exe), str(tmp_path / "a.u8"), str(tmp_path / "b.u8"), str(tmp_path / "h.f64")] + [str(o) for o in outs],
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for o, Hm in zip(outs, (H, H.astype(np.float32))):
        of = FO.Flow()
        of.compute_mask(a, 40.0)
        want = WO.compute_mask_homo(of, b, Hm, 40.0)
        got = np.frombuffer(o.read_bytes(), np.uint8).reshape(h, w)
        assert np.array_equal(got, want), o.name
