"""Time of FlowSLAM::Flow::ComputeMask on the GPU at 640x480: the single-frame host call (host frame in, host mask out,
synchronous) and the device sequence form (orbfe_flow_compute_masks_device) at B = 1, 64 and 1024 frames per call, each next to
its homography-compensated twin (ComputeMask(GrayImg, Homo, ...): orbfe_flow_compute_mask_homo /
orbfe_flow_compute_masks_homo_device, every frame warped), run side by side in the same process.  Prints one JSON line: ms per
frame for each ("..._homo_..." for the warped legs).  Device events around the timed calls; every shape is warmed up first."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,64,1024")
    args = ap.parse_args()
    import torch
    from orb_slam2_ssd_semantic_amd import Flow
    from orb_slam2_ssd_semantic_amd.synth import synth_frame
    import scipy.ndimage as ndi
    torch.cuda.set_device(0)
    h, w = 480, 640
    base = synth_frame(1, h=h + 64, w=w + 64).astype(np.float64)
    seq = [np.clip(np.round(ndi.shift(base, (0.7 * i, 1.1 * i), order=1, mode="nearest")[32:32 + h, 32:32 + w]), 0, 255).astype(np.uint8)
           for i in range(16)]
    # the homography that maps frame i onto frame i-1 of the sequence (a translation by -(1.1, 0.7) px)
    H = np.array([[1.0, 0.0, -1.1], [0.0, 1.0, -0.7], [0.0, 0.0, 1.0]])
    out = {"shape": [w, h]}
    for tag, hom in (("", None), ("_homo", H)):
        fl = Flow(w, h)
        for f in seq[:4]:
            fl.compute_mask(f, 40.0, homography=hom)
        t = time.perf_counter()
        for r in range(args.reps):
            fl.compute_mask(seq[r % 16], 40.0, homography=hom)
        out[f"host_single{tag}_ms_per_frame"] = (time.perf_counter() - t) * 1e3 / args.reps
        fl.close()
    for B in [int(x) for x in args.batches.split(",")]:
        d = torch.from_numpy(np.stack([seq[i % 16] for i in range(B)])).cuda()
        dH = torch.from_numpy(np.stack([H] * B)).cuda()
        masks = torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
        ones = torch.empty(B, dtype=torch.int32, device="cuda")
        reps = max(2, args.reps // max(1, B // 16))
        for tag, hom in (("", None), ("_homo", dH)):
            fl = Flow(w, h, max_batch=B)
            fl.compute_masks(d, 40.0, masks, ones, homographies=hom)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fl.compute_masks(d, 40.0, masks, ones, homographies=hom)
            e1.record()
            torch.cuda.synchronize()
            out[f"device_B{B}{tag}_ms_per_frame"] = e0.elapsed_time(e1) / (reps * B)
            fl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
