"""Times orbfe_cloud_insert_device for one 640 x 480 keyframe: into an empty map and into a map of a few million voxels, next to
the CPU oracle's time for the same keyframe (PCL itself is on no machine of the project, so the oracle is the only comparison).

    python tools/cloud_times.py [--reps 30] [--warmup 5] [--voxels 3000000] [--out profiles/cloud_times.json]

Warm-up first, device events round every call, the median and the spread over the repetitions.  The depth plane holds zero-depth
pixels (a sixth of it), as real frames do: they all fall into the one voxel at the camera centre, the longest serial walk of
k_cloud_centroids.  Each repetition restores the map first (outside the timed span), so every insert sees the same map."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from orb_slam2_ssd_semantic_amd import PointCloudMap  # noqa: E402

W, H, LEAF = 640, 480, 0.01


def keyframe(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (2.0 + 0.8 * np.sin(xx / 90.0) + 0.5 * np.cos(yy / 70.0) + rng.normal(scale=0.01, size=(H, W))).astype(np.float32)
    d[rng.random((H, W)) < 1 / 6] = 0
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    K = np.array([525.0, 525.0, 319.5, 239.5], np.float32)
    return d, bgr, K, np.eye(4)


def background(n, seed):
    """n voxel-sized records scattered over a hall, as a map of earlier keyframes would be"""
    rng = np.random.default_rng(seed)
    p = torch.empty((n, 4), dtype=torch.int32)
    xyz = rng.uniform(-6, 6, (n, 3)).astype(np.float32)
    xyz[:, 1] = rng.uniform(-1.5, 1.5, n)
    p[:, :3] = torch.from_numpy(xyz.view(np.int32))
    p[:, 3] = -1
    return p.cuda()


def time_insert(m, frame, base, reps, warmup):
    d, c = torch.from_numpy(frame[0]).cuda(), torch.from_numpy(frame[1]).cuda()
    ms = []
    for k in range(warmup + reps):
        m.load(base)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        n = m.insert(d, c, frame[3], frame[2])
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=reps, map_before=int(base.shape[0]), map_after=int(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--voxels", type=int, default=3000000)
    ap.add_argument("--oracle", type=int, default=1, help="0: skip the CPU oracle's time")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    frame = keyframe(1)
    res = dict(date=time.strftime("%Y-%m-%d"), device=torch.cuda.get_device_name(0), w=W, h=H, leaf=LEAF,
               zero_depth_pixels=int((frame[0] == 0).sum()))
    with PointCloudMap(LEAF, W, H, max_points=a.voxels + 2 * W * H, max_frames=1) as m:
        res["empty_map"] = time_insert(m, frame, torch.empty((0, 4), dtype=torch.int32, device="cuda"), a.reps, a.warmup)
        big = background(a.voxels, 2)
        m.load(big)
        m.voxel_filter()
        res["large_map"] = time_insert(m, frame, m.device_cloud(), a.reps, a.warmup)
    if a.oracle:
        import cloud_oracle as CO
        t = time.perf_counter()
        om = CO.Map(LEAF)
        om.insert([frame])
        res["oracle_cpu_empty_map_s"] = time.perf_counter() - t
        res["oracle_map_after"] = len(om.pts)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
