"""Time of the batched, device-resident SearchForTriangulation against the path a caller had before, on identical inputs (GPU box).

256 pairs = 16 keyframes x 16 neighbours of one seeded scene, 2000 features each, FeatureVectors made on the device by
orbfe_bow_transform_batch_device from a synthetic k = 10, L = 6 vocabulary at levelsup 4 (about 100 nodes of about 20 features, as
ORBvoc gives) and, to see the node-list length at work, at levelsup 5 (about 10 nodes of about 200).
  batch   orbfe_triangulation_pairs_batch_device + orbfe_search_for_triangulation_batch_device, ONE call each for all pairs, timed
          with stream events: 3 warm-ups, then the median of the repeats; with the LDS-tiled kernel and with the one-thread-per-
          feature kernel, alternating in the same loop.
  before  per pair: orbfe_search_for_triangulation on host buffers (upload, host merge walk, k_triangulation, wait) with its
          arrays prepared, timed with the wall clock around the call (it ends in a synchronise), + the replay on the host
          (rotation histogram, ComputeThreeMaxima, pairs; vectorised numpy here, C++ in the shim), timed separately.
The batch form's pairs are compared with the earlier path's before anything is timed.  Prints one JSON line; --out FILE also writes it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from orb_slam2_ssd_semantic_amd import KP_DTYPE, LocalMapper, ORBmatcher, ORBVocabulary, mapping  # noqa: E402
from orb_slam2_ssd_semantic_amd._ffi import TriOut  # noqa: E402

F = np.float32
NKF, NNEIGH, NFEAT, LEVELSUPS, TH_LOW = 16, 16, 2000, (4, 5), 50
K = (535.4, 539.2, 320.1, 247.6)


def scale_factors(nlevels=8, sf=1.2):
    s = np.ones(nlevels, F)
    for i in range(1, nlevels):
        s[i] = F(s[i - 1] * F(sf))   # mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor, in float
    return s


def rotation(rng, deg):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(rng.normal(0, deg))
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def noisy_copy(rng, desc, max_flips):
    bits = np.unpackbits(desc, axis=1)
    for i in range(len(desc)):
        k = int(rng.integers(0, max_flips + 1))
        if k:
            bits[i, rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def vocabulary(seed, k, L):
    """a full k-ary tree of depth L in DBoW2's creation order (breadth first), random node descriptors, weights in [0.1, 9)"""
    rng = np.random.default_rng(seed)
    inner = (k ** L - 1) // (k - 1)
    nodes = inner + k ** L
    child_off = np.minimum(np.arange(nodes + 1, dtype=np.int64), inner) * k
    word_id = np.zeros(nodes, np.uint32)
    word_id[inner:] = np.arange(k ** L, dtype=np.uint32)
    return dict(child_off=child_off.astype(np.uint32), child_idx=np.arange(1, nodes, dtype=np.uint32),
                node_desc=rng.integers(0, 256, (nodes, 32), dtype=np.uint8), word_id=word_id, weight=rng.uniform(0.1, 9.0, nodes), L=L)


def three_maxima(hist):
    """ComputeThreeMaxima (src/ORBmatcher.cc:1912-1957) with its float 0.1f * max1 rules: the bins that stay"""
    m, i = [0, 0, 0], [-1, -1, -1]
    for b, s in enumerate(int(v) for v in hist):
        if s > m[0]:
            m, i = [s, m[0], m[1]], [b, i[0], i[1]]
        elif s > m[1]:
            m, i = [m[0], s, m[1]], [i[0], b, i[1]]
        elif s > m[2]:
            m[2], i[2] = s, b
    if F(m[1]) < F(0.1) * F(m[0]):
        i[1] = i[2] = -1
    elif F(m[2]) < F(0.1) * F(m[0]):
        i[2] = -1
    return [b for b in i if b >= 0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(rng):
    """NKF keyframes of one scene: poses a few centimetres apart, each sees NFEAT of the scene's points"""
    fx, fy, cx, cy = K
    npts = NFEAT * 13 // 10
    z = rng.uniform(1.0, 8.0, npts)
    p0 = np.stack([rng.uniform(-100, 740, npts), rng.uniform(-80, 560, npts)], 1)
    Xw = np.stack([(p0[:, 0] - cx) / fx * z, (p0[:, 1] - cy) / fy * z, z], 1)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    frames, Tcw, Ow = [], [], []
    for j in range(NKF):
        R = rotation(rng, 3.0)
        t = np.array([0.12 * j + rng.normal(0, 0.02), rng.normal(0, 0.03), rng.normal(0, 0.03)])
        Xc = Xw @ R.T + t
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
        inside = np.flatnonzero((uv[:, 0] > 5) & (uv[:, 0] < 635) & (uv[:, 1] > 5) & (uv[:, 1] < 475))
        sel = rng.permutation(np.concatenate([inside, np.setdiff1d(np.arange(npts), inside)])[:NFEAT])
        xy = (uv[sel] + rng.normal(0, 0.6, (NFEAT, 2))).astype(F)
        frames.append(dict(desc=noisy_copy(rng, base[sel], 20), xy=xy, octave=rng.integers(0, 8, NFEAT).astype(np.int32),
                           angle=((rng.choice([10.0, 10.0, 10.0, 200.0], NFEAT) + rng.normal(0, 5, NFEAT)) % 360).astype(F),
                           uRight=np.where(rng.random(NFEAT) < 0.5, xy[:, 0] - rng.uniform(2, 40, NFEAT), -1).astype(F),
                           has_mp=(rng.random(NFEAT) < 0.3).astype(np.uint8)))
        Tcw.append(np.concatenate([R, t[:, None]], 1).astype(F))
        Ow.append((-(R.T @ t)).astype(F))
    return frames, np.stack(Tcw), np.stack(Ow)


def replay_numpy(a1, a2, m12):
    """rotation histogram + ComputeThreeMaxima + pairs, vectorised (the host half of the earlier path)"""
    i = np.flatnonzero(m12 >= 0)
    rot = (a1[i] - a2[m12[i]]).astype(F)
    rot = np.where(rot < 0, rot + F(360), rot).astype(F)
    b = np.rint(np.floor(np.abs(rot * F(1.0 / 30)) + F(0.5))).astype(np.int64)   # roundf for non-negative arguments
    b[b == 30] = 0
    hist = np.bincount(b, minlength=30)
    ok = np.isin(b, three_maxima(hist[:30]))
    return np.stack([i[ok], m12[i[ok]]], 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    frames, Tcw, Ow = scene(rng)
    sf = scale_factors()
    s2 = (sf * sf).astype(F)
    B, cap = NKF, NFEAT
    kps = np.zeros((B, cap), KP_DTYPE)
    for b, f in enumerate(frames):
        kps["x"][b], kps["y"][b], kps["octave"][b], kps["angle"][b] = f["xy"][:, 0], f["xy"][:, 1], f["octave"], f["angle"]
    mt = ORBmatcher(0.6, True)
    lm = LocalMapper(mt)
    voc = vocabulary(7, 10, 6)
    V = ORBVocabulary(mt, **voc)
    i32 = dict(dtype=torch.int32, device="cuda")
    t = dict(kps=dev(kps.view(np.int32).reshape(B, cap, 7)), desc=dev(np.stack([f["desc"] for f in frames])), n=dev(np.full(B, NFEAT, np.int32)),
             ur=dev(np.stack([f["uRight"] for f in frames])), mp=dev(np.stack([f["has_mp"] for f in frames])),
             f_word=torch.zeros((B, cap), **i32), f_node=torch.zeros((B, cap), **i32), f_weight=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
             bow_id=torch.zeros((B, cap), **i32), bow_val=torch.zeros((B, cap), dtype=torch.float64, device="cuda"),
             fv_node=torch.zeros((B, cap), **i32), fv_off=torch.zeros((B, cap + 1), **i32), fv_idx=torch.zeros((B, cap), **i32),
             counts=torch.zeros((B, 4), **i32))
    out_all = dict(pairs=NKF * NNEIGH, keyframes=NKF, neighbours=NNEIGH, features=NFEAT, shapes={})

    def measure(levelsup):
        V.transform_batch_device(t["desc"].data_ptr(), t["n"].data_ptr(), B, cap, levelsup, t["f_word"].data_ptr(), t["f_node"].data_ptr(),
                                 t["f_weight"].data_ptr(), t["bow_id"].data_ptr(), t["bow_val"].data_ptr(), t["fv_node"].data_ptr(),
                                 t["fv_off"].data_ptr(), t["fv_idx"].data_ptr(), t["counts"].data_ptr(), None)
        kf = mapping.keyframes_struct(t["kps"], t["desc"], t["n"], cap, B, t["fv_node"], t["fv_off"], t["fv_idx"], t["counts"], t["ur"], t["mp"])
        pairs = [(i, (i + 1 + j) % NKF) for i in range(NKF) for j in range(NNEIGH)]   # the 16th neighbour of a keyframe is itself
        P = len(pairs)
        cam = mapping.camera(*K, 40.0, 0.0, 640.0, 0.0, 480.0)
        d = dict(kf1=dev(np.array([p[0] for p in pairs], np.int32)), kf2=dev(np.array([p[1] for p in pairs], np.int32)), Tcw=dev(Tcw.reshape(B, 12)),
                 Ow=dev(Ow), F12=torch.zeros((P, 9), dtype=torch.float32, device="cuda"), epi=torch.zeros((P, 2), dtype=torch.float32, device="cuda"),
                 skip=torch.zeros((P,), dtype=torch.uint8, device="cuda"), m12=torch.zeros((P, cap), **i32), nm=torch.zeros((P,), **i32),
                 pr=torch.zeros((P, cap, 2), **i32), npr=torch.zeros((P,), **i32))
        out = TriOut(d["m12"].data_ptr(), d["nm"].data_ptr(), d["pr"].data_ptr(), d["npr"].data_ptr())

        def batch_call():
            lm.TriangulationPairs_batch_device(d["Tcw"].data_ptr(), d["Ow"].data_ptr(), B, cam, 0.0, 0, None, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P,
                                               d["F12"].data_ptr(), d["epi"].data_ptr(), d["skip"].data_ptr())
            lm.SearchForTriangulation_batch_device(kf, d["kf1"].data_ptr(), d["kf2"].data_ptr(), P, d["F12"].data_ptr(), d["epi"].data_ptr(),
                                                   d["skip"].data_ptr(), sf, s2, out, TH_LOW, False, True)

        batch_call()
        torch.cuda.synchronize()
        counts = t["counts"].cpu().numpy()
        fv = [(t["fv_node"][b, :counts[b, 1]].cpu().numpy().view(np.uint32), t["fv_off"][b, :counts[b, 1] + 1].cpu().numpy().view(np.uint32),
               t["fv_idx"][b, :counts[b, 2]].cpu().numpy().view(np.uint32)) for b in range(B)]
        F12, epi = d["F12"].cpu().numpy(), d["epi"].cpu().numpy()
        npr, pr, nm = d["npr"].cpu().numpy(), d["pr"].cpu().numpy(), d["nm"].cpu().numpy()

        def side(b):
            f = frames[b]
            st = (f["uRight"] >= 0).astype(np.uint8)
            return dict(desc=f["desc"], xy=f["xy"], elig=(f["has_mp"] == 0).astype(np.uint8), stereo=st, fv=fv[b], octave=f["octave"], scale_factors=sf,
                        level_sigma2=s2)
        sides = [side(b) for b in range(B)]

        def host_core(p):
            i1, i2 = pairs[p]
            return mt.SearchForTriangulationCore(sides[i1], sides[i2], F12[p], epi[p, 0], epi[p, 1], TH_LOW)

        for p in range(0, P, 15):   # the two paths agree before anything is timed
            i1, i2 = pairs[p]
            want = replay_numpy(frames[i1]["angle"], frames[i2]["angle"], host_core(p))
            assert np.array_equal(pr[p, :npr[p]], want) and nm[p] == len(want), p
        res = dict(pairs=P, keyframes=NKF, neighbours=NNEIGH, features=NFEAT, levelsup=levelsup, repeats=a.repeats,
                   nodes_per_keyframe=float(counts[:, 1].mean()), matches_per_pair=float(nm.mean()), info=mapping.tri_search_info())
        # the earlier path: every pair twice, the second round timed
        core_us, replay_us = [], []
        for rnd in range(2):
            for p in range(P):
                t0 = time.perf_counter()
                m = host_core(p)
                t1 = time.perf_counter()
                replay_numpy(frames[pairs[p][0]]["angle"], frames[pairs[p][1]]["angle"], m)
                t2 = time.perf_counter()
                if rnd:
                    core_us.append((t1 - t0) * 1e6)
                    replay_us.append((t2 - t1) * 1e6)
        res["before_core_us_per_pair"] = float(np.median(core_us))
        res["before_replay_numpy_us_per_pair"] = float(np.median(replay_us))
        res["before_us_per_pair"] = res["before_core_us_per_pair"] + res["before_replay_numpy_us_per_pair"]
        # the batch form, both search kernels alternating
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {0: [], 1: []}
        for it in range(3 + a.repeats):
            for kernel in (0, 1):
                lm.set_triangulation_kernel(kernel)
                e0.record()
                batch_call()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    ms[kernel].append(e0.elapsed_time(e1))
        lm.set_triangulation_kernel(0)
        for kernel, name in ((0, "lds_tiles"), (1, "thread_per_feature")):
            res["batch_%s_ms" % name] = float(np.median(ms[kernel]))
            res["batch_%s_ms_min_max" % name] = [float(min(ms[kernel])), float(max(ms[kernel]))]
            res["batch_%s_us_per_pair" % name] = float(np.median(ms[kernel])) * 1e3 / P
        return res

    for levelsup in LEVELSUPS:   # about 100 nodes of about 20 features (what ORBvoc gives), then about 10 nodes of about 200
        out_all["shapes"]["levelsup_%d" % levelsup] = measure(levelsup)
    res = out_all
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
