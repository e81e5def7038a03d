"""findHomography on the GPU (csrc/orbfe_homography.hip): the latency of one host call (orbfe_find_homography: copies in,
RANSAC + refit + LM, copies out, synchronised) and the per-set time of the batched device form (orbfe_find_homographies_device,
B sets of n pairs on one stream, HIP-event timing), for n in {100, 500, 2000} and inlier ratio in {0.9, 0.6, 0.3}.
Prints one JSON line per (n, ratio)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import homography_cases as HC
    from orb_slam2_ssd_semantic_amd import Homography
    dev = torch.device("cuda", 0)
    hg = Homography(4096, a.batch)
    for n in (100, 500, 2000):
        for ratio in (0.9, 0.6, 0.3):
            s, d, _ = HC.planar(n, ratio, n + int(ratio * 10))
            for _ in range(3):
                H, m = hg.find(s, d)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                hg.find(s, d)
                t.append(time.perf_counter() - t0)
            sets = [HC.planar(n, ratio, 1000 * k + n)[:2] for k in range(a.batch)]
            off = torch.tensor(np.r_[0, np.cumsum([n] * a.batch)].astype(np.int32), device=dev)
            src = torch.from_numpy(np.concatenate([x for x, _ in sets])).to(dev)
            dst = torch.from_numpy(np.concatenate([y for _, y in sets])).to(dev)
            Hb, ok, mask = hg.find_batch(off, src, dst, min_pairs=50)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            bt = []
            for _ in range(max(3, a.reps // 4)):
                e0.record()
                hg.find_batch(off, src, dst, min_pairs=50, H=Hb, ok=ok, mask=mask)
                e1.record()
                e1.synchronize()
                bt.append(e0.elapsed_time(e1))
            print(json.dumps(dict(n=n, inlier_ratio=ratio, host_call_ms_median=round(float(np.median(t)) * 1e3, 3),
                                  host_call_ms_min=round(min(t) * 1e3, 3), batch=a.batch,
                                  batched_ms_per_set=round(float(np.median(bt)) / a.batch, 4),
                                  ok_sets=int(ok.sum().item()))), flush=True)
    hg.close()


if __name__ == "__main__":
    main()
