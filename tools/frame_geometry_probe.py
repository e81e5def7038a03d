"""The RGB-D Frame's per-frame geometry on the GPU (csrc/orbfe_frame.hip): HIP-event times of orbfe_frame_geometry_batch_device
(TUM1 camera, u16 depth plane, real extractor blocks of S_tum frames at 1000 features) for B = 1, 64 and 1024 frames, and of
orbfe_depth_to_float_device on B 640 x 480 u16 planes next to a device copy of the same bytes (tools/hbm_rate.py measures the
copy rate on its own).  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    import undistort_oracle as U
    from orb_slam2_ssd_semantic_amd import Camera, ORBextractor
    from orb_slam2_ssd_semantic_amd.synth import synth_frames_parallel
    W, H = 640, 480
    base = synth_frames_parallel("S_tum", 64, H, W, 4100, max_procs=16)
    cam = Camera(U.camera_matrix(U.TUM1), U.dist_coeffs(U.TUM1), 40.0)
    scale = float(U.depth_scale(U.TUM1))
    rng = np.random.default_rng(1)
    for B in (1, 64, 1024):
        frames = torch.from_numpy(base[np.arange(B) % 64]).cuda()
        e = ORBextractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
        cap = e.capacity()
        dk = torch.zeros((B, cap, 7), dtype=torch.int32, device="cuda")
        dd = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
        dn = torch.zeros(B, dtype=torch.int32, device="cuda")
        e.extract_batch_device(frames.data_ptr(), B, W, H, W, W * H, dk.data_ptr(), dd.data_ptr(), cap, dn.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        depth = torch.from_numpy(rng.integers(0, 30000, (B, H, W)).astype(np.uint16).view(np.int16)).cuda()
        ku, dep, ur = torch.empty_like(dk), torch.empty((B, cap), device="cuda"), torch.empty((B, cap), device="cuda")
        torch.cuda.synchronize()
        med, best = timed(lambda: cam.frame_geometry(dk, dn, cap, depth=depth, scale=scale, kps_un=ku, depth_out=dep, uright=ur), a.reps)
        print(json.dumps(dict(what="frame_geometry_batch_device", frames=B, cap=cap, keypoints=int(dn.sum().item()),
                              ms_median=round(med, 4), ms_min=round(best, 4), us_per_frame=round(med * 1e3 / B, 3))), flush=True)
        out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        med, best = timed(lambda: Camera.depth_to_float(depth, scale, out=out), a.reps)
        copy = torch.empty_like(depth)
        cmed, _ = timed(lambda: copy.copy_(depth), a.reps)
        nbytes = depth.numel() * 6   # 2 read + 4 written
        print(json.dumps(dict(what="depth_to_float_device", frames=B, ms_median=round(med, 4), ms_min=round(best, 4),
                              gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1), copy_u16_ms=round(cmed, 4),
                              copy_gb_per_s=round(depth.numel() * 4 / (cmed * 1e-3) / 1e9, 1))), flush=True)
        e.close()
        del frames, dk, dd, dn, depth, out, copy, ku, dep, ur
        torch.cuda.empty_cache()
    cam.close()


if __name__ == "__main__":
    main()
