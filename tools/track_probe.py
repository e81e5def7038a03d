"""Per-frame time of the device-resident last-frame tracker against the host-buffer path, on identical inputs (GPU box).

B = 1, 16 and 256 frames of 1000 features and ~800 valid last-frame points (16 distinct seeded cases, repeated to fill the
batch).  The batched chain orbfe_track_last_frame_batch_device (gating -> search -> replay, one call) is timed with stream
events: warm-up, then the median of the repeats.  The host-buffer path is what a caller had before: per frame, the host
gating (orbfe_project_points + the level-window rule) and one orbfe_search_by_projection call, timed with the wall clock.
Both paths' matches are compared before anything is timed.  Prints one JSON line; --out FILE also writes it."""
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
import proj_cases as PC  # noqa: E402
from orb_slam2_ssd_semantic_amd import KP_DTYPE, ORBmatcher, Tracker, _ffi, tracking  # noqa: E402

F = np.float32
NC = PC.GRID_COLS * PC.GRID_ROWS
DISTINCT, NFEAT, TH, TH_HIGH = 16, 1000, 15.0, 100


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host_queries(L, cur, last):
    """the host gating of the last-frame form through the product's orbfe_project_points (:1620-1656)"""
    p = _ffi.ptr
    Tc, Tl = np.asarray(cur["Tcw"], F), np.asarray(last["Tcw"], F)
    R, t = np.ascontiguousarray(Tc[:3, :3]), np.ascontiguousarray(Tc[:3, 3])
    fx, fy, cx, cy, bf, mb = cur["K"]
    minx, maxx, miny, maxy = cur["bounds"]
    twc = -(R.T @ t)
    tlc = Tl[:3, :3] @ twc + Tl[:3, 3]
    fwd, bwd = tlc[2] > mb, -tlc[2] > mb
    valid = np.flatnonzero(last["has_mp"].astype(bool) & ~last["outlier"].astype(bool))
    wp = np.ascontiguousarray(last["world_pos"][valid], F)
    n = len(valid)
    u, v, invz, ur, ok = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint8)
    rc = L.orbfe_project_points(p(R), p(t), None, None, None, fx, fy, cx, cy, bf, minx, maxx, miny, maxy, 2 | 4 | 8, n, p(wp), None, None, None,
                                p(u), p(v), p(invz), None, p(ur), p(ok))
    assert rc == 0
    keep = np.flatnonzero(ok)
    octv = last["octave"][valid][keep]
    q = np.zeros(len(keep), _ffi.PROJ_QUERY_DTYPE)
    q["u"], q["v"], q["ur"] = u[keep], v[keep], ur[keep]
    q["r"] = F(TH) * cur["scale_factors"][octv]
    q["min_level"] = octv if fwd else 0 if bwd else octv - 1
    q["max_level"] = -1 if fwd else octv if bwd else octv + 1
    q["flags"] = 2 | last["obs_gt0"][valid][keep].astype(np.int32)
    return q, valid[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(2027)
    cases = [PC.last_frame_case(rng, NFEAT, NFEAT, ("small", "forward", "backward")[k % 3]) for k in range(DISTINCT)]
    mat = ORBmatcher(0.9, True)
    trk = Tracker(mat)
    L = mat._L
    cur0 = cases[0][0]
    minx, maxx, miny, maxy = cur0["bounds"]
    cam = tracking.camera(*cur0["K"][:5], minx, maxx, miny, maxy)
    res = dict(features=NFEAT, distinct_cases=DISTINCT, repeats=a.repeats, batches={})
    # host path, frame by frame
    host = []
    for cur, last in cases:
        ci = PC.core_inputs(cur)
        q, src = host_queries(L, cur, last)
        m = mat.SearchByProjectionCore(queries=q, qdesc=last["mpdesc"][src], th=TH_HIGH, nnratio=0.0, ratio_rule=0, **ci)[0]
        host.append((ci, q, src, m))
    res["valid_last_points"] = float(np.mean([len(h[1]) for h in host]))
    for B in a.batches:
        idx = [k % DISTINCT for k in range(B)]
        cap = NFEAT
        blk, lblk = np.zeros((B, cap), KP_DTYPE), np.zeros((B, cap), KP_DTYPE)
        desc, mpdesc = np.zeros((B, cap, 32), np.uint8), np.zeros((B, cap, 32), np.uint8)
        ur, slot = np.zeros((B, cap), F), np.zeros((B, cap), np.uint8)
        valid, obs, wp = np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), np.zeros((B, cap, 3), F)
        Tc, Tl = np.zeros((B, 12), F), np.zeros((B, 12), F)
        for f, k in enumerate(idx):
            cur, last = cases[k]
            blk["x"][f], blk["y"][f], blk["octave"][f], blk["angle"][f] = cur["xy"][:, 0], cur["xy"][:, 1], cur["octave"], cur["angle"]
            lblk["octave"][f], lblk["angle"][f] = last["octave"], last["angle"]
            desc[f], mpdesc[f], ur[f], slot[f] = cur["desc"], last["mpdesc"], cur["uRight"], cur["state"]
            valid[f] = last["has_mp"].astype(bool) & ~last["outlier"].astype(bool)
            obs[f], wp[f] = last["obs_gt0"], last["world_pos"]
            Tc[f], Tl[f] = np.asarray(cur["Tcw"], F)[:3, :4].reshape(12), np.asarray(last["Tcw"], F)[:3, :4].reshape(12)
        t = dict(kps=dev(blk.view(np.int32).reshape(B, cap, 7)), lkps=dev(lblk.view(np.int32).reshape(B, cap, 7)), desc=dev(desc), mpdesc=dev(mpdesc),
                 ur=dev(ur), slot=dev(slot), valid=dev(valid), obs=dev(obs), wp=dev(wp), Tc=dev(Tc), Tl=dev(Tl),
                 n=dev(np.full(B, NFEAT, np.int32)), off=torch.zeros((B, NC + 1), dtype=torch.int32, device="cuda"),
                 idx=torch.zeros((B, cap), dtype=torch.int32, device="cuda"), nin=torch.zeros((B,), dtype=torch.int32, device="cuda"))
        g = (minx, miny, float(cur0["gw_inv"]), float(cur0["gh_inv"]))
        mat.AssignFeaturesToGrid_batch_device(t["kps"].data_ptr(), t["n"].data_ptr(), cap, B, *g, t["off"].data_ptr(), t["idx"].data_ptr(),
                                              t["nin"].data_ptr(), None)
        fr = tracking.frames_struct(t["kps"], t["desc"], t["n"], cap, t["off"], t["idx"], *g, d_uright=t["ur"], d_slot=t["slot"])
        last_s = _ffi.TrackLast(t["lkps"].data_ptr(), t["n"].data_ptr(), cap, t["valid"].data_ptr(), t["wp"].data_ptr(), t["obs"].data_ptr(),
                                t["mpdesc"].data_ptr(), t["Tl"].data_ptr())
        out = trk.alloc_out(B, cap, cap)
        r = trk.track_last_frame(fr, t["Tc"].data_ptr(), last_s, cam, cur0["K"][5], False, TH, cur0["scale_factors"], B, ent_cap=1, out=out)
        torch.cuda.synchronize()
        nq, match = r["nq"].cpu().numpy(), r["match"].cpu().numpy()
        for f, k in enumerate(idx[:DISTINCT]):   # the two paths agree before anything is timed
            assert nq[f] == len(host[k][1]) and np.array_equal(match[f, :nq[f]], host[k][3]), (B, f)
        ent_cap = r["ent_cap"]   # the exact need, found by the wrapper's second call
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for it in range(3 + a.repeats):
            e0.record()
            trk.TrackLastFrame_batch_device(fr, t["Tc"].data_ptr(), last_s, cam, cur0["K"][5], False, TH, cur0["scale_factors"], TH_HIGH, True,
                                            ent_cap, B, out[1], None)
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        assert int(r["status"][0].item()) == 0
        hs = []
        for it in range(2 + min(a.repeats, 5)):
            t0 = time.perf_counter()
            for k in idx:
                cur, last = cases[k]
                q, src = host_queries(L, cur, last)
                mat.SearchByProjectionCore(queries=q, qdesc=last["mpdesc"][src], th=TH_HIGH, nnratio=0.0, ratio_rule=0, **host[k][0])
            if it >= 2:
                hs.append((time.perf_counter() - t0) * 1e3)
        cs = []
        for it in range(2 + min(a.repeats, 5)):   # the search calls alone, queries prepared
            t0 = time.perf_counter()
            for k in idx:
                mat.SearchByProjectionCore(queries=host[k][1], qdesc=cases[k][1]["mpdesc"][host[k][2]], th=TH_HIGH, nnratio=0.0, ratio_rule=0, **host[k][0])
            if it >= 2:
                cs.append((time.perf_counter() - t0) * 1e3)
        res["batches"][str(B)] = dict(host_search_ms_per_frame=float(np.median(cs)) / B, entries=int(ent_cap), batched_ms=float(np.median(ms)), batched_ms_per_frame=float(np.median(ms)) / B, batched_ms_min=float(min(ms)),
                                      host_ms_per_frame=float(np.median(hs)) / B, rounds=int(r["status"][1].item()),
                                      nmatches_mean=float(r["nmatches"].float().mean().item()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
