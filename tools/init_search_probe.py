"""Time of the device-resident SearchForInitialization against the path a caller had before, on identical inputs (GPU box).

1, 16 and 256 pairs of the 2000 x 2000, window 100 case of tests/proj_cases.py (16 distinct seeded pairs, repeated to fill the
batch).  orbfe_search_for_initialization_batch_device (gate -> count -> scan -> fill -> resolve -> finish, one call) is timed with
stream events: 3 warm-ups, then the median of the repeats.  The earlier path for ONE pair is timed with the wall clock, median of
5: orbfe_window_distances (upload, lists, download) + orbfe_initialization_resolve on the host, through ctypes, queries prepared.
Both paths' accepted features are compared before anything is timed.  Prints one JSON line; --out FILE also writes it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import proj_cases as PC  # noqa: E402
from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBmatcher, Tracker, _ffi, tracking  # noqa: E402

F = np.float32
NC = PC.GRID_COLS * PC.GRID_ROWS
DISTINCT, NFEAT, WINDOW, TH_LOW, NNRATIO = 16, 2000, 100, 50, 0.9


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_inputs(mat, f1, f2, prev):
    """what the earlier path needs prepared: frame 2's grid and one query per level-0 feature of frame 1"""
    minx, _, miny, _ = f2["bounds"]
    bounds = (minx, miny, f2["gw_inv"], f2["gh_inv"])
    from orb_slam2_ssd_semantic_amd import FrameGrid
    g = FrameGrid(mat, f2["xy"], f2["octave"], *bounds)
    src = np.flatnonzero(f1["octave"] == 0)
    q = np.zeros(len(src), _ffi.PROJ_QUERY_DTYPE)
    q["u"], q["v"], q["r"] = prev[src, 0], prev[src, 1], F(WINDOW)
    return dict(grid=(g.cell_off, g.cell_idx), bounds=bounds, q=q, qd=np.ascontiguousarray(f1["desc"][src]), src=src)


def host_path(mat, f2, h, cap):
    off, cand, dist = mat.WindowDistances(f2["desc"], f2["xy"], f2["octave"], h["grid"], h["bounds"], h["q"], h["qd"], cap=cap)
    ent = (cand | (dist << 16)).astype(np.uint32)
    nq, n2 = len(h["q"]), len(f2["octave"])
    acc, hold = np.zeros(max(nq, 1), np.int32), np.zeros(max(n2, 1), np.int32)
    _ffi.check(mat._L.orbfe_initialization_resolve(_ffi.ptr(off), _ffi.ptr(ent), nq, n2, TH_LOW, C.c_float(NNRATIO), _ffi.ptr(acc), _ffi.ptr(hold)),
               "orbfe_initialization_resolve")
    return acc[:nq], hold[:n2], int(off[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    cases = [PC.initialization_case(np.random.default_rng(31_000 + k), NFEAT, NFEAT) for k in range(DISTINCT)]
    mat = ORBmatcher(NNRATIO, False)   # the orientation check is off in both paths: the earlier path leaves it to the caller
    trk = Tracker(mat)
    f20 = cases[0][1]
    g = (float(f20["bounds"][0]), float(f20["bounds"][2]), float(f20["gw_inv"]), float(f20["gh_inv"]))
    res = dict(features=NFEAT, window=WINDOW, distinct_cases=DISTINCT, repeats=a.repeats, batches={})
    host = []
    for f1, f2, prev in cases:
        h = host_inputs(mat, f1, f2, prev)
        acc, hold, need = host_path(mat, f2, h, 1 << 18)
        m = np.full(NFEAT, -1, np.int32)
        st = np.flatnonzero(hold >= 0)
        m[h["src"][hold[st]]] = st
        host.append((h, m, need))
    res["level0_queries"] = float(np.mean([len(h[0]["q"]) for h in host]))
    res["entries_per_pair"] = float(np.mean([h[2] for h in host]))
    hs = []
    for it in range(2 + 5):   # ONE pair by the earlier path
        t0 = time.perf_counter()
        host_path(mat, cases[0][1], host[0][0], host[0][2])
        if it >= 2:
            hs.append((time.perf_counter() - t0) * 1e3)
    res["host_path_ms_one_pair"] = float(np.median(hs))
    for B in a.batches:
        idx = [k % DISTINCT for k in range(B)]
        cap = NFEAT
        b1, b2 = np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap), KP_DTYPE)
        d1, d2 = np.zeros((B, cap, 32), np.uint8), np.zeros((B, cap, 32), np.uint8)
        prev = np.zeros((B, cap, 2), F)
        for p, k in enumerate(idx):
            f1, f2, pv = cases[k]
            b1["x"][p], b1["y"][p], b1["octave"][p], b1["angle"][p] = f1["xy"][:, 0], f1["xy"][:, 1], f1["octave"], f1["angle"]
            b2["x"][p], b2["y"][p], b2["octave"][p], b2["angle"][p] = f2["xy"][:, 0], f2["xy"][:, 1], f2["octave"], f2["angle"]
            d1[p], d2[p], prev[p] = f1["desc"], f2["desc"], pv
        i32 = dict(dtype=torch.int32, device="cuda")
        t = dict(k1=dev(b1.view(np.int32).reshape(B, cap, 7)), k2=dev(b2.view(np.int32).reshape(B, cap, 7)), d1=dev(d1), d2=dev(d2), prev=dev(prev),
                 n=dev(np.full(B, NFEAT, np.int32)), off=torch.zeros((B, NC + 1), **i32), idx=torch.zeros((B, cap), **i32), nin=torch.zeros((B,), **i32),
                 m=torch.zeros((B, cap), **i32), nm=torch.zeros((B,), **i32), st=torch.zeros((2,), **i32),
                 pout=torch.zeros((B, cap, 2), dtype=torch.float32, device="cuda"))
        mat.AssignFeaturesToGrid_batch_device(t["k2"].data_ptr(), t["n"].data_ptr(), cap, B, *g, t["off"].data_ptr(), t["idx"].data_ptr(),
                                              t["nin"].data_ptr(), None)
        sec = tracking.frames_struct(t["k2"], t["d2"], t["n"], cap, t["off"], t["idx"], *g)
        first, out = tracking.init_search_structs(t["k1"], t["d1"], t["n"], cap, t["m"], t["nm"], t["st"], t["pout"])

        def call(ent_cap):
            trk.SearchForInitialization_batch_device(first, sec, B, t["prev"].data_ptr(), WINDOW, out, th_low=TH_LOW, nnratio=NNRATIO,
                                                     check_ori=False, ent_cap=ent_cap)
        call(1)
        torch.cuda.synchronize()
        ent_cap = int(t["st"][0].item())   # the exact need
        call(ent_cap)
        torch.cuda.synchronize()
        assert int(t["st"][0].item()) == 0
        m = t["m"].cpu().numpy()
        for p, k in enumerate(idx[:DISTINCT]):   # the two paths agree before anything is timed
            assert np.array_equal(m[p], host[k][1]), (B, p)
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(3 + a.repeats):
            e0.record()
            call(ent_cap)
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        res["batches"][str(B)] = dict(entries=ent_cap, batched_ms=float(np.median(ms)), batched_ms_per_pair=float(np.median(ms)) / B,
                                      batched_ms_min=float(min(ms)), rounds=int(t["st"][1].item()),
                                      nmatches_mean=float(t["nm"].float().mean().item()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
