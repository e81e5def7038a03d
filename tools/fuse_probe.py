"""Time of the batched Fuse (orbfe_fuse_batch_device) against the two forms it could have taken (GPU box).  Workloads, 1000 features a
keyframe, proj_cases.fuse_case data (every target with a 1000-point list that projects onto its keypoints):
  targets20     1000 points into each of 20 target keyframes (SearchInNeighbors, first + second neighbours)
  targets100    the same into 100 targets
  cands30000    30 000 candidates into one keyframe (SearchAndFuse's list, or the last Fuse of a large SearchInNeighbors)
each in the plain and in the Sim3 mode.  Per workload:
  fuse          search + replay, one call                       stream events, 3 warm-ups, median of the repeats with min - max
  search        orbfe_fuse_search_batch_device alone            the same
  b_core        (b) a lower bound of "gate kernel + the shared core": orbfe_search_by_projection_batch_device alone on queries that
                were gated beforehand -- the gate kernel it would need is not even counted        the same
  a_loop        (a) the loop it replaces: per keyframe the host gate (orbfe_fuse_gate_points: orbfe_project_points' arithmetic plus
                the query, in C) and one orbfe_search_by_projection_chi2 call on host buffers     wall clock, same repeats
b_equal says that (b)'s matches equal the fused kernel's.  Prints one JSON line; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import fuse_cases as FC  # noqa: E402
import fuse_oracle as FO  # noqa: E402
import proj_cases as PC  # noqa: E402
from oracle import oracle_ffi as O  # noqa: E402
from orb_slam2_ssd_semantic_amd import KP_DTYPE, LocalMapper, ORBmatcher, Tracker, _ffi, mapping, tracking  # noqa: E402

F = np.float32
NFEAT = 1000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    mt = ORBmatcher(0.6, True)
    lm, trk = LocalMapper(mt), Tracker(mt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ms = []
        for it in range(3 + a.repeats):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        return dict(ms=float(np.median(ms)), ms_min_max=[float(min(ms)), float(max(ms))])

    def wall(fn):
        ms = []
        for it in range(3 + a.repeats):
            t0 = time.perf_counter()
            fn()
            if it >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        return dict(ms=float(np.median(ms)), ms_min_max=[float(min(ms)), float(max(ms))])

    def workload(ntargets, nmp, seed):
        rng = np.random.default_rng(seed)
        cases = [PC.fuse_case(rng, NFEAT, nmp) for _ in range(ntargets)]
        B, cap = ntargets, NFEAT
        blk = np.zeros((B, cap), KP_DTYPE)
        for b, (kf, _) in enumerate(cases):
            blk["x"][b], blk["y"][b], blk["octave"][b] = kf["xy"][:, 0], kf["xy"][:, 1], kf["octave"]
        k0 = cases[0][0]
        minx, maxx, miny, maxy = [float(v) for v in k0["bounds"]]
        i32 = dict(dtype=torch.int32, device="cuda")
        t = dict(kps=dev(blk.view(np.int32).reshape(B, cap, 7)), desc=dev(np.stack([c[0]["desc"] for c in cases])), n=dev(np.full(B, cap, np.int32)),
                 ur=dev(np.stack([c[0]["uRight"] for c in cases])), off=torch.zeros((B, 64 * 48 + 1), **i32), idx=torch.zeros((B, cap), **i32),
                 nin=torch.zeros((B,), **i32))
        mt.AssignFeaturesToGrid_batch_device(t["kps"].data_ptr(), t["n"].data_ptr(), cap, B, minx, miny, float(k0["gw_inv"]), float(k0["gh_inv"]),
                                             t["off"].data_ptr(), t["idx"].data_ptr(), t["nin"].data_ptr(), None)
        frames = tracking.frames_struct(t["kps"], t["desc"], t["n"], cap, t["off"], t["idx"], minx, miny, k0["gw_inv"], k0["gh_inv"], d_uright=t["ur"])
        cam = tracking.camera(*[float(v) for v in k0["K"][:5]], minx, maxx, miny, maxy)
        tabs = [FC.tables(kf, mps) for kf, mps in cases]
        base = np.concatenate([[0], np.cumsum([len(tb[0]["bad"]) for tb in tabs])])
        tmap = {k: np.concatenate([tb[0][k] for tb in tabs]) for k in tabs[0][0]}
        npts = int(base[-1])
        slot = np.stack([np.where(tb[3] >= 0, tb[3] + base[b], -1) for b, tb in enumerate(tabs)]).astype(np.int32)
        d = dict(wp=dev(tmap["world_pos"]), nr=dev(tmap["normal"]), mn=dev(tmap["min_dist"]), mx=dev(tmap["max_dist"]), bad=dev(tmap["bad"]),
                 desc=dev(tmap["desc"]), nobs=dev(np.concatenate([tb[4] for tb in tabs])), slot=dev(slot))
        tm = _ffi.TrackMap(d["wp"].data_ptr(), d["nr"].data_ptr(), d["mn"].data_ptr(), d["mx"].data_ptr(), d["bad"].data_ptr(), None,
                           d["desc"].data_ptr(), npts)
        idx = np.concatenate([np.where(tb[1] >= 0, tb[1] + base[b], -1) for b, tb in enumerate(tabs)]).astype(np.int32)
        skip = np.concatenate([tb[2] for tb in tabs])
        ne = len(idx)
        off = (np.arange(B + 1) * nmp).astype(np.int32)
        sf, s2, log_sf = k0["scale_factors"], k0["inv_sigma2"], k0["log_scale"]
        res = dict(targets=ntargets, points_per_list=nmp, entries=ne)
        for mode, name in ((FO.PLAIN, "plain"), (FO.SIM3, "sim3")):
            poses = [FC.pose_of(kf, mode, FC.scw_of(kf, 1.0)) for kf, _ in cases]
            L = [dev(np.arange(B, dtype=np.int32)), dev(np.array([p[0].reshape(12) for p in poses], F)), dev(np.array([p[1] for p in poses], F)), dev(off),
                 dev(idx), dev(skip)]
            lists = mapping.fuse_lists_struct(L[0], L[1], L[2], L[3], L[4], ne, B, L[5])
            ten, out = lm.alloc_fuse_out(ne, B, cap)
            r = dict()
            r["fuse"] = timed(lambda: lm.Fuse_batch_device(frames, B, lists, cam, tm, d["nobs"].data_ptr(), d["slot"].data_ptr(), 3.0, sf, s2, log_sf,
                                                           out, mode))
            r["search"] = timed(lambda: lm.FuseSearch_batch_device(frames, B, lists, cam, tm, 3.0, sf, s2, log_sf, ten["match"].data_ptr(),
                                                                   ten["dist"].data_ptr(), mode))
            torch.cuda.synchronize()
            match = ten["match"].cpu().numpy()
            r["fused"] = int((match >= 0).sum())
            # the host gate of every pair: (a) runs it inside its loop, (b) gets its queries from it beforehand
            gated = []
            for b, (kf, mps) in enumerate(cases):
                q, _, ok = mapping.fuse_gate_points(poses[b][0], poses[b][1], cam, 3.0, sf, log_sf, mps["world_pos"], mps["normal"], mps["min_dist"],
                                                    mps["max_dist"], mode)
                live = ok.astype(bool) & (tabs[b][1] >= 0) & ~tabs[b][2].astype(bool) & ~np.asarray(mps["bad"]).astype(bool)
                gated.append((q[live], np.flatnonzero(live)))
            qcap = max(max(len(g[1]) for g in gated), 1)
            hq, hsrc = np.zeros((B, qcap), _ffi.PROJ_QUERY_DTYPE), np.zeros((B, qcap), np.int32)
            for b, (q, src) in enumerate(gated):
                hq[b, :len(src)], hsrc[b, :len(src)] = q, src + base[b]
            c = dict(q=dev(hq.view(np.int32).reshape(B, qcap, 8)), src=dev(hsrc), nq=dev(np.array([len(g[1]) for g in gated], np.int32)),
                     match=torch.zeros((B, qcap), **i32), best=torch.zeros((B, qcap), **i32), second=torch.zeros((B, qcap), **i32),
                     status=torch.zeros((2,), **i32))
            ent_cap = B * qcap * 64

            def core():
                trk.SearchByProjection_batch_device(frames, B, c["q"].data_ptr(), c["src"].data_ptr(), c["nq"].data_ptr(), qcap, d["desc"].data_ptr(),
                                                    npts, 0, 50, 0.0, 0, ent_cap, c["match"].data_ptr(), c["best"].data_ptr(), c["second"].data_ptr(),
                                                    c["status"].data_ptr(), s2)
            core()
            torch.cuda.synchronize()
            need = int(c["status"][0].item())
            if need:
                ent_cap = need
            r["b_core"] = timed(core)
            r["b_ent_cap"], r["b_rounds"] = ent_cap, int(c["status"][1].item())
            cm = c["match"].cpu().numpy()
            r["b_equal"] = bool(all(np.array_equal(cm[b, :len(g[1])], match[b * nmp + g[1]]) for b, g in enumerate(gated)))
            grids = [O.assign_grid(kf["xy"], minx, miny, kf["gw_inv"], kf["gh_inv"]) for kf, _ in cases]

            def loop():
                for b, (kf, mps) in enumerate(cases):
                    q, _, ok = mapping.fuse_gate_points(poses[b][0], poses[b][1], cam, 3.0, sf, log_sf, mps["world_pos"], mps["normal"],
                                                        mps["min_dist"], mps["max_dist"], mode)
                    live = ok.astype(bool) & (tabs[b][1] >= 0) & ~tabs[b][2].astype(bool) & ~np.asarray(mps["bad"]).astype(bool)
                    mt.SearchByProjectionCore(kf["desc"], kf["xy"], kf["octave"], grids[b], (minx, miny, kf["gw_inv"], kf["gh_inv"]), kf["uRight"], None,
                                              q[live], np.asarray(mps["mpdesc"])[live], 50, 0.0, 0, inv_level_sigma2=s2)
            r["a_loop"] = wall(loop)
            r["speedup_vs_a"], r["speedup_vs_b"] = r["a_loop"]["ms"] / r["fuse"]["ms"], r["b_core"]["ms"] / r["search"]["ms"]
            res[name] = r
        return res

    res = dict(features=NFEAT, repeats=a.repeats, targets20=workload(20, 1000, 1), targets100=workload(100, 1000, 2), cands30000=workload(1, 30000, 3))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
