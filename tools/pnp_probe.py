"""PnPsolver's EPnP RANSAC on the GPU (csrc/orbfe_pnp.hip): the latency of one host call (orbfe_pnp_iterate: copies in, one
iterate(5) of a fresh solver with Relocalization's parameters, copies out, synchronised) and the per-set time of the batched
device form (orbfe_pnp_iterate_device, 1 / 8 / 64 candidate sets of n correspondences in one launch, HIP-event timing), for n
in {50, 200, 1000} and inlier ratio in {0.9, 0.5}.  Every timed call starts from a zeroed state, so it runs the same iterations.
Prints one JSON line per (n, ratio, candidates)."""
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
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import pnp_cases as PC
    from orb_slam2_ssd_semantic_amd import PnP
    from orb_slam2_ssd_semantic_amd import pnp as PN
    dev = torch.device("cuda", 0)
    pn = PnP(64 * 1000, 64)
    t8 = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev).view(dt)   # noqa: E731
    for n in (50, 200, 1000):
        for ratio in (0.9, 0.5):
            scenes = [PC.scene(1000 * k + n, n, inlier_ratio=ratio) for k in range(64)]
            params = PN.ransac_params(0.99, 10, 300, 4, 0.5, n=n)
            its = PN.iterations(np.zeros(1, PN.STATE_DTYPE), params, 5)
            draws = [PC.draws_for(k, its) for k in range(64)]
            sc = scenes[0]
            t, ran = [], 0
            for rep in range(a.reps + 3):
                state, best = np.zeros(1, PN.STATE_DTYPE), np.zeros(n, np.uint8)
                t0 = time.perf_counter()
                res, _ = pn.iterate(sc["P3Dw"], sc["P2D"], sc["sigma2"], PC.K, params, 5, draws[0], state, best)
                if rep >= 3:
                    t.append(time.perf_counter() - t0)
                ran = int(res["iterations_run"])
            for cand in (1, 8, 64):
                sets = np.zeros(cand, PN.SET_DTYPE)
                sets["K"] = PC.K
                sets["params"] = params[0]
                sets["n_iterations"] = 5
                sets["draws_offset"] = np.arange(cand) * 4 * its
                off = t8(np.arange(cand + 1, dtype=np.int32) * n, torch.int32)
                P3 = t8(np.concatenate([s["P3Dw"] for s in scenes[:cand]]), torch.float32).view(-1, 3)
                P2 = t8(np.concatenate([s["P2D"] for s in scenes[:cand]]), torch.float32).view(-1, 2)
                sg = t8(np.concatenate([s["sigma2"] for s in scenes[:cand]]), torch.float32)
                dsets, dd = t8(sets, torch.uint8), t8(np.concatenate(draws[:cand]), torch.int32)
                state = torch.zeros(cand * PN.STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                best = torch.zeros(cand * n, dtype=torch.uint8, device=dev)
                res, mask = pn.iterate_device(off, P3, P2, sg, dsets, dd, state, best)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                bt = []
                for _ in range(max(3, a.reps // 4)):
                    state.zero_()
                    best.zero_()
                    e0.record()
                    pn.iterate_device(off, P3, P2, sg, dsets, dd, state, best, result=res, mask=mask)
                    e1.record()
                    e1.synchronize()
                    bt.append(e0.elapsed_time(e1))
                r = res.cpu().numpy().reshape(-1).view(PN.RESULT_DTYPE)
                print(json.dumps(dict(n=n, inlier_ratio=ratio, candidates=cand, host_call_ms_median=round(float(np.median(t)) * 1e3, 3),
                                      host_call_iterations=ran, batched_ms=round(float(np.median(bt)), 4),
                                      batched_ms_per_set=round(float(np.median(bt)) / cand, 4), found_sets=int(r["found"].sum()),
                                      iterations_mean=round(float(r["iterations_run"].mean()), 1))), flush=True)
    pn.close()


if __name__ == "__main__":
    main()
