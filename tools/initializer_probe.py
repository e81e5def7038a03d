"""The monocular Initializer on the GPU (csrc/orbfe_initializer.hip): the latency of one host call (orbfe_initializer_initialize:
copies in, the three launches, copies out, synchronised) at N = 100, 300 and 1000 matches with 200 iterations, and the time of the
batched device form (orbfe_initializer_initialize_device, 1 / 16 / 256 pairs of 300 matches in one call, HIP-event timing).
Writes profiles/initializer_probe.json and prints one JSON line per measurement."""
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "initializer_probe.json"))
    a = ap.parse_args()
    import torch
    import initializer_cases as IC
    from orb_slam2_ssd_semantic_amd import InitializerHandle
    from orb_slam2_ssd_semantic_amd import initializer as IN
    dev = torch.device("cuda", 0)
    rows = []
    with InitializerHandle(256 * 400, 256) as h:
        for n in (100, 300, 1000):
            c = IC.general(n, 900 + n, iterations=200, extra1=n // 10, extra2=n // 8)
            t = []
            for rep in range(a.reps + 3):
                t0 = time.perf_counter()
                res, _, _ = h.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], 1.0, 200, c["draws"])
                if rep >= 3:
                    t.append(time.perf_counter() - t0)
            rows.append(dict(form="host", matches=n, iterations=200, ms_median=round(float(np.median(t)) * 1e3, 4),
                             ms_min=round(float(np.min(t)) * 1e3, 4), ok=int(res["ok"]), model=int(res["model"])))
            print(json.dumps(rows[-1]), flush=True)
        cs = [IC.general(300, 2000 + k, iterations=200, extra1=30, extra2=40) for k in range(16)]
        t8 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
        for npairs in (1, 16, 256):
            use = [cs[k % 16] for k in range(npairs)]
            off1 = np.cumsum([0] + [len(c["keys1"]) for c in use]).astype(np.int32)
            off2 = np.cumsum([0] + [len(c["keys2"]) for c in use]).astype(np.int32)
            pairs = np.zeros(npairs, IN.PAIR_DTYPE)
            pairs["K"], pairs["sigma"], pairs["iterations"] = use[0]["K"], 1.0, 200
            pairs["draws_offset"] = np.arange(npairs) * 1600
            args = dict(offsets1=t8(off1), offsets2=t8(off2), keys1=t8(np.concatenate([c["keys1"] for c in use])),
                        keys2=t8(np.concatenate([c["keys2"] for c in use])), matches12=t8(np.concatenate([c["matches12"] for c in use])),
                        pairs=t8(pairs.view(np.uint8).reshape(npairs, -1)), draws=t8(np.concatenate([c["draws"] for c in use])))
            res, P3D, tri = h.initialize_device(**args)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            bt = []
            for _ in range(max(5, a.reps // 3)):
                e0.record()
                h.initialize_device(**args, result=res, P3D=P3D, triangulated=tri)
                e1.record()
                e1.synchronize()
                bt.append(e0.elapsed_time(e1))
            r = res.cpu().numpy().reshape(-1).view(IN.RESULT_DTYPE)
            rows.append(dict(form="device", pairs=npairs, matches=300, iterations=200, ms_median=round(float(np.median(bt)), 4),
                             ms_per_pair=round(float(np.median(bt)) / npairs, 4), ok_pairs=int(r["ok"].sum())))
            print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
