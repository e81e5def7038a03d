"""Time of the device-resident CreateNewMapPoints (orbfe_create_new_map_points_batch_device) on the scene and vocabulary of
tools/tri_probe.py (GPU box): 2000 features a keyframe, the k = 10, L = 6 vocabulary at levelsup 4.
  one_kf_10_neighbours   keyframe 0 against 10 neighbours, 10 rounds of one pair (the reference's loop for one keyframe)
  kf16_x_16_rounds       16 keyframes x 16 neighbours, 16 rounds of 16 pairs
  pairs256_one_round     the same 256 pairs in one round (the static batch)
Every workload: the slot state is reset (outside the timed span), then the call between two stream events; 3 warm-ups, the median
of the repeats with min - max.  The split of a workload = its pieces as separate calls on all its pairs at once, on the initial
state: search (orbfe_triangulation_pairs_batch_device + orbfe_search_for_triangulation_batch_device), triangulate
(orbfe_triangulate_pairs_batch_device on the matches found), claim = the one-round call minus the two.  Prints one JSON line;
--out FILE also writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tri_probe as TP  # noqa: E402
from orb_slam2_ssd_semantic_amd import KP_DTYPE, LocalMapper, ORBmatcher, ORBVocabulary, mapping  # noqa: E402
from orb_slam2_ssd_semantic_amd._ffi import NewptOut, NewptState, TriOut  # noqa: E402

F = np.float32
BF = 40.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    frames, Tcw, Ow = TP.scene(rng)
    sf = TP.scale_factors()
    s2 = (sf * sf).astype(F)
    B, cap = TP.NKF, TP.NFEAT
    kps = np.zeros((B, cap), KP_DTYPE)
    for b, f in enumerate(frames):
        kps["x"][b], kps["y"][b], kps["octave"][b], kps["angle"][b] = f["xy"][:, 0], f["xy"][:, 1], f["octave"], f["angle"]
    ur = np.stack([f["uRight"] for f in frames])
    with np.errstate(divide="ignore"):
        depth = np.where(ur >= 0, F(BF) / (np.stack([f["xy"][:, 0] for f in frames]) - ur), F(-1)).astype(F)
    mt = ORBmatcher(0.6, True)
    lm = LocalMapper(mt)
    V = ORBVocabulary(mt, **TP.vocabulary(7, 10, 6))
    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    t = dict(kps=TP.dev(kps.view(np.int32).reshape(B, cap, 7)), desc=TP.dev(np.stack([f["desc"] for f in frames])), n=TP.dev(np.full(B, cap, np.int32)),
             ur=TP.dev(ur), depth=TP.dev(depth), mp0=TP.dev(np.stack([f["has_mp"] for f in frames])),
             f_word=torch.zeros((B, cap), **i32), f_node=torch.zeros((B, cap), **i32), f_weight=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
             bow_id=torch.zeros((B, cap), **i32), bow_val=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
             fv_node=torch.zeros((B, cap), **i32), fv_off=torch.zeros((B, cap + 1), **i32), fv_idx=torch.zeros((B, cap), **i32),
             counts=torch.zeros((B, 4), **i32), Tcw=TP.dev(Tcw.reshape(B, 12)), Ow=TP.dev(Ow))
    t["mp"], t["xyz"], t["id"] = t["mp0"].clone(), torch.zeros((B, cap, 3), **f32), torch.full((B, cap), -1, **i32)
    V.transform_batch_device(t["desc"].data_ptr(), t["n"].data_ptr(), B, cap, 4, t["f_word"].data_ptr(), t["f_node"].data_ptr(),
                             t["f_weight"].data_ptr(), t["bow_id"].data_ptr(), t["bow_val"].data_ptr(), t["fv_node"].data_ptr(),
                             t["fv_off"].data_ptr(), t["fv_idx"].data_ptr(), t["counts"].data_ptr(), None)
    kf = mapping.keyframes_struct(t["kps"], t["desc"], t["n"], cap, B, t["fv_node"], t["fv_off"], t["fv_idx"], t["counts"], t["ur"], t["mp"])
    cam = mapping.camera(*TP.K, BF, 0.0, 640.0, 0.0, 480.0)
    mb = BF / TP.K[0]
    geom = mapping.geometry_struct(t["Tcw"], t["Ow"], cam, mb, 1.2, t["depth"])
    state = NewptState(t["mp"].data_ptr(), t["xyz"].data_ptr(), t["id"].data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def reset():
        t["mp"].copy_(t["mp0"])
        t["xyz"].zero_()
        t["id"].fill_(-1)

    def timed(fn):
        ms = []
        for it in range(3 + a.repeats):
            reset()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        return dict(ms=float(np.median(ms)), ms_min_max=[float(min(ms)), float(max(ms))])

    def workload(pairs, round_off):
        P = len(pairs)
        d = dict(kf1=TP.dev(np.array([p[0] for p in pairs], np.int32)), kf2=TP.dev(np.array([p[1] for p in pairs], np.int32)),
                 F12=torch.zeros((P, 9), **f32), epi=torch.zeros((P, 2), **f32), skip=torch.zeros((P,), dtype=torch.uint8, device="cuda"),
                 m12=torch.zeros((P, cap), **i32), nm=torch.zeros((P,), **i32), pr=torch.zeros((P, cap, 2), **i32), npr=torch.zeros((P,), **i32),
                 ver=torch.zeros((P, cap), dtype=torch.uint8, device="cuda"), idx=torch.zeros((P, cap, 2), **i32), xyz=torch.zeros((P, cap, 3), **f32),
                 nnew=torch.zeros((P,), **i32))
        tri = TriOut(d["m12"].data_ptr(), d["nm"].data_ptr(), d["pr"].data_ptr(), d["npr"].data_ptr())
        out = NewptOut(d["ver"].data_ptr(), d["idx"].data_ptr(), d["xyz"].data_ptr(), d["nnew"].data_ptr())

        def loop(ro):
            lm.CreateNewMapPoints_batch_device(kf, geom, state, 0, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P, ro, sf, s2, tri, out,
                                               TP.TH_LOW, False, True, 0, d["skip"].data_ptr())

        def search():
            lm.TriangulationPairs_batch_device(t["Tcw"].data_ptr(), t["Ow"].data_ptr(), B, cam, mb, 0, None, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P,
                                               d["F12"].data_ptr(), d["epi"].data_ptr(), d["skip"].data_ptr())
            lm.SearchForTriangulation_batch_device(kf, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P, d["F12"].data_ptr(), d["epi"].data_ptr(),
                                                   d["skip"].data_ptr(), sf, s2, tri, TP.TH_LOW, False, True)

        def triangulate():
            lm.TriangulatePairs_batch_device(kf, geom, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P, d["pr"].data_ptr(), d["npr"].data_ptr(), sf, s2, out)

        res = dict(pairs=P, rounds=len(round_off) - 1)
        res["loop"] = timed(lambda: loop(round_off))
        torch.cuda.synchronize()
        res["matches_per_pair"], res["new_points_per_pair"] = float(d["npr"].float().mean()), float(d["nnew"].float().mean())
        res["new_points"] = int(d["nnew"].sum())
        res["per_round_ms"] = res["loop"]["ms"] / res["rounds"]
        res["one_round"] = timed(lambda: loop([0, P]))
        res["search"] = timed(search)
        res["triangulate"] = timed(triangulate)      # on the matches the search just before it left
        res["claim_ms"] = res["one_round"]["ms"] - res["search"]["ms"] - res["triangulate"]["ms"]
        return res

    nk, nn = TP.NKF, TP.NNEIGH
    by_round = [(i, (i + 1 + j) % nk) for j in range(nn) for i in range(nk)]   # round j: every keyframe against its j-th neighbour
    res = dict(features=cap, keyframes=nk, levelsup=4, repeats=a.repeats, stereo_mb=mb,
               one_kf_10_neighbours=workload([(0, 1 + j) for j in range(10)], list(range(11))),
               kf16_x_16_rounds=workload(by_round, [16 * r for r in range(17)]),
               pairs256_one_round=workload(by_round, [0, 256]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
