"""The all-pairs kernels behind orbfe_match_bf_frames_device alone on the GPU (GPU box): B pairs of 1004 x 1004 descriptors, k_match_bf
with 4, 2 and 1 query tiles per wave and k_match_popc, matcher + rotation prune, mean of CALLS calls.  Prints one JSON object.
usage: [B=1024] [CALLS=100] [ORBFE_LIB=ab/liborbfe_x.so] python tools/match_times.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from orb_slam2_ssd_semantic_amd import ORBmatcher, _ffi

B, calls = int(os.environ.get("B", "1024")), int(os.environ.get("CALLS", "100"))
cap, n = 1088, 1004
rng = np.random.default_rng(0)
desc = torch.from_numpy(rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)).cuda()
kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
dn = torch.full((B,), n, dtype=torch.int32, device="cuda")
qf = torch.arange(B, dtype=torch.int32, device="cuda")
tf = (qf + B - 1) % B
L = _ffi.lib()
out = {"lib": os.environ.get("ORBFE_LIB", "default"), "pairs": B, "queries": n, "train": n, "calls": calls,
       "distance_evaluations_per_call": B * n * n}
res = []
for kern, tiles, name in ((0, 4, "k_match_bf<4> (matrix cores)"), (0, 2, "k_match_bf<2>"), (0, 1, "k_match_bf<1>"),
                          (1, 4, "k_match_popc (xor + v_bcnt_u32_b32)")):
    mt = ORBmatcher(0.9, True)
    mt.set_bf_kernel(kern)
    mt.set_bf_tiles(tiles)
    dm = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    nm = torch.zeros(B, dtype=torch.int32, device="cuda")

    def run():
        rc = L.orbfe_match_bf_frames_device(mt.handle, kps.data_ptr(), desc.data_ptr(), dn.data_ptr(), cap, qf.data_ptr(),
                                            tf.data_ptr(), B, 0.9, 100, 1, dm.data_ptr(), nm.data_ptr(), None)
        assert rc == 0
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls if kern == 0 else max(1, calls // 10)):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / (calls if kern == 0 else max(1, calls // 10))
    out[name] = {"ms_per_call_incl_rot_prune": round(ms, 4), "Gdist_per_s": round(B * n * n / (ms * 1e-3) / 1e9, 1)}
    res.append(dm.cpu().numpy().copy())
out["identical_results"] = bool(all(np.array_equal(res[0], r) for r in res[1:]))
print(json.dumps(out))
