"""Times of the multi-view geometry mask (csrc/orbfe_geometry.hip) on the box scene of tests/geometry_cases.py scaled to 640 x 480
with a 200 x 200 box (a 40 000-pixel region), GPU box.

Per stage, wall clock around synchronous host calls, median of the repeats after one warm-up:
  extract      orbfe_geometry_correct on the scene WITHOUT the box: upload, ExtractDynPoints over 5 x N reference keypoints, no
               dynamic point, dilation of an empty union, mask download
  dilate       orbfe_geometry_depth_region_growing with no seed: upload, dilation, mask, download
  grow_<n>     the same with n seeds inside the box (1, 16, 128; max_seeds 128, so one pass): all n regions are grown at once and
               the first is accepted; minus `dilate` it is the serial chain of one seed, reported as steps per second
  correct      orbfe_geometry_correct on the scene with the box
  batch_64     orbfe_geometry_correct_batch_device on 64 device frames (stream events), per frame
Prints one JSON line; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import geometry_cases as GC  # noqa: E402
from orb_slam2_ssd_semantic_amd import Geometry  # noqa: E402
from orb_slam2_ssd_semantic_amd import geometry as GE  # noqa: E402

W, H, BOX = 640, 480, (220, 140, 200, 200)


def median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    sc = GC.box_scene(W, H, BOX, 6, (40, 25), 11)
    nkp = len(sc["key_frames"][0]["keys"])
    g = Geometry(W, H, nkp, 128)
    for f in sc["key_frames"]:
        g.update_db(f["Tcw"], f["depth"], f["keys"], f["keys_un"])
    K, T, depth = sc["K"], sc["cur_T"], sc["cur_depth"]
    flat = np.full_like(depth, 3.0)
    out = dict(size=[W, H], region_pixels=BOX[2] * BOX[3], keypoints_per_reference=nkp, max_seeds=128, chunk=g.chunk)
    out["extract_ms"] = median_ms(lambda: g.correct(flat, T, *K), a.repeats)
    out["dilate_ms"] = median_ms(lambda: g.depth_region_growing(np.zeros((0, 2), np.int32), depth), a.repeats)
    rng = np.random.RandomState(0)
    for n in (1, 16, 128):
        seeds = np.stack([rng.randint(BOX[0] + 5, BOX[0] + BOX[2] - 5, n), rng.randint(BOX[1] + 5, BOX[1] + BOX[3] - 5, n)], 1)
        out[f"grow_{n}_ms"] = median_ms(lambda: g.depth_region_growing(seeds, depth), a.repeats)
        steps = int(GE.depth_region_growing(g, seeds, depth)[2].sum())   # pixels of the union: one step each, nearly
        out[f"grow_{n}_union_pixels"] = steps
    out["seed_steps_per_s"] = out["grow_1_union_pixels"] / ((out["grow_1_ms"] - out["dilate_ms"]) * 1e-3)
    out["correct_ms"] = median_ms(lambda: g.correct(depth, T, *K), a.repeats)
    out["counts"] = g.counts()
    dev = torch.from_numpy(np.repeat(depth[None], a.batch, 0)).cuda()
    poses = np.repeat(T[None], a.batch, 0)
    masks = torch.empty((a.batch, H, W), dtype=torch.uint8, device="cuda")
    ones = torch.empty(a.batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    t = []
    for i in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        g.correct_batch_device(dev, poses, *K, masks=masks, ones=ones)
        e1.record(st)
        e1.synchronize()
        if i:
            t.append(e0.elapsed_time(e1))
    out[f"batch_{a.batch}_ms_per_frame"] = float(np.median(t)) / a.batch
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
