"""Times orbfe_cloud_objects_device for one 640 x 480 keyframe with three boxes of different sizes, the cell grid against brute
force (mode 2 against mode 1), and the outlier filter alone on the largest box's points.

    python tools/object_times.py [--reps 20] [--warmup 3] [--out profiles/object_times.json]

Warm-up first, device events round every call, the median and the spread over the repetitions.  There is no CPU comparison: PCL
is on no machine of the project, and the numpy oracle's brute force is not one."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_ssd_semantic_amd import PointCloudMap  # noqa: E402
from orb_slam2_ssd_semantic_amd import cloud as CL  # noqa: E402

W, H, LEAF = 640, 480, 0.01
BOXES = np.array([[40, 40, 560, 400], [120, 100, 200, 160], [400, 300, 60, 50]], np.float32)   # 222 642, 31 482 and 2 842 pixels at most
COLORS = np.array([[255, 0, 255], [255, 0, 0], [0, 0, 255]], np.uint8)


def keyframe(seed):
    """a wavy wall at about 2 m (inside the paint's 0.4 m band round each box's mean), noise of a centimetre, a few zeros"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (2.0 + 0.15 * np.sin(xx / 90.0) + 0.1 * np.cos(yy / 70.0) + rng.normal(scale=0.01, size=(H, W))).astype(np.float32)
    d[rng.random((H, W)) < 0.02] = 0
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return d, bgr, np.array([525.0, 525.0, 319.5, 239.5], np.float32), np.eye(4)


def timed(fn, reps, warmup):
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), reps=reps), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d, bgr, K, T = keyframe(1)
    res = dict(date=time.strftime("%Y-%m-%d"), device=torch.cuda.get_device_name(0), w=W, h=H, leaf=LEAF, mean_k=50)
    with PointCloudMap(LEAF, W, H, max_points=16, max_frames=1) as m:
        painted, idx = m.paint_boxes(d, bgr, BOXES, COLORS)
        dd = torch.from_numpy(d).cuda()
        res["indices"] = [int(len(ix)) for ix in idx]
        objs = {}
        for name, mode in (("grid", CL.KNN_GRID), ("brute", CL.KNN_BRUTE)):
            res["objects_" + name], objs[name] = timed(lambda: m.build_objects(dd, painted, T, K, idx, mode=mode), a.reps, a.warmup)
        assert objs["grid"].tobytes() == objs["brute"].tobytes()
        res["n_kept"] = objs["grid"]["n_kept"].tolist()
        res["n_voxels"] = objs["grid"]["n_voxels"].tolist()
        cloud, _ = m.generate(dd, painted, T, K)
        big = cloud[:res["indices"][0]].contiguous()
        for name, mode in (("grid", CL.KNN_GRID), ("brute", CL.KNN_BRUTE)):
            res["filter_" + name], _ = timed(lambda: m.outlier_filter(big, None, 50, 1.0, mode), a.reps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
