"""Cases for the batched Fuse (tests/test_fuse_oracle.py, tests/test_gpu_fuse.py): the flat tables of a proj_cases.fuse_case, the
planted edges of the gate, and hand-built keyframes under the identity pose whose projections are exact.  Test support only."""
import math

import numpy as np

import fuse_oracle as FO
import proj_cases as PC

F = np.float32
K0 = (512.0, 512.0, 320.0, 240.0, 40.0)        # fx, fy, cx, cy, mbf: powers of two, so u = fx * X + cx is exact for the X below
BOUNDS0 = (0.0, 640.0, 0.0, 480.0)
SF = PC.scale_factors()
LOG_SF = F(math.log(F(1.2)))
IDENTITY = np.concatenate([np.eye(3, dtype=F), np.zeros((3, 1), F)], 1)
SIZES_KF, SIZES_MP = (1, 30, 300, 1000), (1, 40, 400, 1500)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


EFF_MIN, EFF_MAX = F(F(0.8) * F(1.25)), F(F(1.2) * F(2.5))   # GetMinDistanceInvariance() of 1.25, GetMaxDistanceInvariance() of 2.5


def seed_case(seed):
    """fuse_case number `seed`: the sizes cycle through nKF in {1, 30, 300, 1000} x nmp in {1, 40, 400, 1500}"""
    rng = np.random.default_rng(41_000 + seed)
    kf, mps = PC.fuse_case(rng, SIZES_KF[seed % 4], SIZES_MP[(seed // 4) % 4])
    return kf, mps, float([3.0, 3.0, 5.0][seed % 3])


def scw_of(kf, s):
    """a Sim3 whose decomposition is (about) the keyframe's pose: [s * Rcw | s * tcw]"""
    S = np.eye(4, dtype=F)
    S[:3, :3] = (np.asarray(kf["Rcw"], np.float64) * s).astype(F)
    S[:3, 3] = (np.asarray(kf["tcw"], np.float64) * s).astype(F)
    return S


def tables(kf, mps, mode=FO.PLAIN):
    """the flat tables of one fuse_case: the map = the list's points followed by the keyframe's own (the point of feature j has
    index nmp + j) -> (tmap, list_idx, list_skip, slot_mp [nKF], nobs)"""
    nKF, nmp = len(np.asarray(kf["octave"])), len(np.asarray(mps["bad"]))
    state = np.asarray(kf["state"])

    def both(a, width, dt, own=None):
        o = np.zeros((nmp + nKF,) + ((width,) if width else ()), dt)
        o[:nmp] = np.asarray(a, dt).reshape(o[:nmp].shape)
        if own is not None:
            o[nmp:] = own
        return o
    tmap = dict(world_pos=both(mps["world_pos"], 3, F), normal=both(mps["normal"], 3, F), min_dist=both(mps["min_dist"], 0, F),
                max_dist=both(mps["max_dist"], 0, F), bad=both(mps["bad"], 0, np.uint8, (state == 2).astype(np.uint8)),
                desc=both(mps["mpdesc"], 32, np.uint8))
    nobs = both(mps["obs"] if "obs" in mps else np.zeros(nmp), 0, np.int32, np.asarray(kf["obs"], np.int32))
    list_idx = np.where(np.asarray(mps["null"]).astype(bool), -1, np.arange(nmp)).astype(np.int32)
    skip = np.asarray(mps["in_kf"], np.uint8) if (mode == FO.PLAIN and "in_kf" in mps) else np.zeros(nmp, np.uint8)
    slot = np.where(state > 0, nmp + np.arange(nKF), -1).astype(np.int32)
    return tmap, list_idx, skip, slot, nobs


def pose_of(kf, mode=FO.PLAIN, Scw=None):
    if mode == FO.SIM3:
        return FO.decompose_sim3(Scw)
    return FO.pose34(kf["Rcw"], kf["tcw"]), np.asarray(kf["Ow"], F).reshape(3)


# ------------------------------------------------------------------------------------------------ hand-built keyframes
def mini_kf(xy, octave, desc=None, uRight=None, state=None, obs=None):
    """a keyframe under the identity pose with camera K0: xy [n][2], octave [n]; descriptors default to zeros"""
    n = len(octave)
    return dict(desc=np.zeros((n, 32), np.uint8) if desc is None else np.asarray(desc, np.uint8).reshape(n, 32),
                xy=np.asarray(xy, F).reshape(n, 2), octave=np.asarray(octave, np.int32),
                uRight=np.full(n, -1, F) if uRight is None else np.asarray(uRight, F),
                state=np.zeros(n, np.uint8) if state is None else np.asarray(state, np.uint8),
                obs=np.zeros(n, np.int32) if obs is None else np.asarray(obs, np.int32), Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F),
                Ow=np.zeros(3, F), K=K0, bounds=BOUNDS0, gw_inv=F(64) / F(640), gh_inv=F(48) / F(480), scale_factors=SF,
                inv_sigma2=(F(1) / (SF * SF)).astype(F), log_scale=LOG_SF)


def bits(k):
    """a descriptor with the first k bits set: Hamming distance k from the zero descriptor"""
    d = np.zeros(256, np.uint8)
    d[:k] = 1
    return np.packbits(d)


def point(u, v, level=0, z=1.0, desc=None, bad=0, obs=0):
    """a map point that projects exactly to (u, v) under the identity pose (u, v multiples of 1/8, z = 1) and whose predicted level
    is `level`: max_dist = dist * 1.2^level * 0.95, seen head on"""
    P = np.array([(u - K0[2]) / K0[0] * z, (v - K0[3]) / K0[1] * z, z], F)
    d = float(np.linalg.norm(P.astype(np.float64)))
    return dict(world_pos=P, normal=(P / d).astype(F), max_dist=F(d * 1.2 ** level * 0.95), min_dist=F(0), bad=bad,
                mpdesc=np.zeros(32, np.uint8) if desc is None else np.asarray(desc, np.uint8), obs=obs)


def points(plist):
    """a mps dict from point() records"""
    n = len(plist)
    return dict(null=np.zeros(n, np.uint8), bad=np.array([p["bad"] for p in plist], np.uint8), in_kf=np.zeros(n, np.uint8),
                world_pos=np.array([p["world_pos"] for p in plist], F).reshape(n, 3), normal=np.array([p["normal"] for p in plist], F).reshape(n, 3),
                max_dist=np.array([p["max_dist"] for p in plist], F), min_dist=np.array([p["min_dist"] for p in plist], F),
                mpdesc=np.array([p["mpdesc"] for p in plist], np.uint8).reshape(n, 32), obs=np.array([p["obs"] for p in plist], np.int32))


# ------------------------------------------------------------------------------------------------ the gate's planted edges
def planted_gate():
    """[(name, P, Pn, min_dist, max_dist, expected ok, expected level or None)] under the identity pose, Ow = 0, camera K0"""
    z1 = (0.0, 0.0, 1.0)
    head = (0.0, 0.0, 1.0)
    out = [
        ("z < 0", (0.0, 0.0, -1.0), head, 0.0, 10.0, 0, None),
        ("z == 0, X != 0: u infinite", (0.1, 0.0, 0.0), (1.0, 0.0, 0.0), 0.0, 10.0, 0, None),
        ("z == 0, X == 0: u NaN", (0.0, 0.0, 0.0), head, 0.0, 10.0, 0, None),
        ("u == minx", (-0.625, 0.0, 1.0), head, 0.0, 10.0, 1, None),
        ("u == maxx", (0.625, 0.0, 1.0), head, 0.0, 10.0, 0, None),
        ("u just below maxx", (0.6249, 0.0, 1.0), head, 0.0, 10.0, 1, None),
        ("v == miny", (0.0, -0.46875, 1.0), head, 0.0, 10.0, 1, None),
        ("v == maxy", (0.0, 0.46875, 1.0), head, 0.0, 10.0, 0, None),
        # the distance gate is the getters': [0.8f * mfMinDistance, 1.2f * mfMaxDistance], both ends in
        ("dist == min", (0.0, 0.0, float(EFF_MIN)), head, 1.25, 10.0, 1, None),
        ("dist one ulp below min", (0.0, 0.0, float(dn(EFF_MIN))), head, 1.25, 10.0, 0, None),
        ("dist == max: ratio < 1, level clamped at 0", (0.0, 0.0, float(EFF_MAX)), head, 0.0, 2.5, 1, 0),
        ("dist one ulp above max", (0.0, 0.0, float(up(EFF_MAX))), head, 0.0, 2.5, 0, None),
        ("ratio 1: level 0 unclamped", z1, head, 0.0, 1.0, 1, 0),
        ("dot == 0.5 * dist", (0.0, 0.0, 2.0), (0.0, 0.0, 0.5), 0.0, 10.0, 1, None),
        ("dot one ulp below 0.5 * dist", (0.0, 0.0, 2.0), (0.0, 0.0, float(dn(0.5))), 0.0, 10.0, 0, None),
        ("level just above 0", z1, head, 0.0, float(up(1.0)), 1, 1),
        ("level clamped at nlevels - 1", z1, head, 0.0, 100.0, 1, 7),
        ("level nlevels - 1 unclamped", z1, head, 0.0, float(F(1.2) ** 7 * F(0.99)), 1, 7),
    ]
    return [(n, np.array(P, F), np.array(Pn, F), F(mn), F(mx), ok, lv) for n, P, Pn, mn, mx, ok, lv in out]


# ------------------------------------------------------------------------------------------------ pair lookup, scan carry
PAIR_LOOKUP_LENGTHS = (0, 1, 0, 0, 3, 1025, 0, 5, 0)   # empty pairs between full ones; boundaries 1, 1029, 1034: no multiples of 4
PAIR_LOOKUP_STRIDE = 1024                               # the replay's workgroup: positions 0 and 1024 are one thread's


def pair_lookup(mode, th=3.0):
    """Nine (keyframe, list) pairs over the two keyframes of seed_case(10) / seed_case(11) (300 and 1000 features, 400 points each),
    rows alternating, for the bisection that finds an entry's pair in list_off: dict(rows [9], sels [9] = selections of the row's
    400-point list, S [2] = the rows' Sim3s).  The short lists hold entries the oracle says match (plus some that do not and, in
    the 5-entry list, one entry twice).  The 1025-entry list walks the 400 points round and round, rotated so that position 1024
    -- the second entry of the replay's thread 0 -- holds a point that matches and therefore stood at 224 and 624 already."""
    cases = [seed_case(10)[:2], seed_case(11)[:2]]
    S = [scw_of(c[0], 0.9) for c in cases]
    hit, miss = [], []
    for (kf, mps), s in zip(cases, S):
        tmap, idx, skip, _, _ = tables(kf, mps, mode)
        T, Ow = pose_of(kf, mode, s)
        m = FO.fuse_search(kf, T, Ow, tmap, idx, skip, th, mode)[0]
        hit.append(np.flatnonzero(m >= 0))
        miss.append(np.flatnonzero(m < 0))
    rows = [i % 2 for i in range(len(PAIR_LOOKUP_LENGTHS))]
    n = len(cases[1][1]["bad"])
    sels = []
    for row, length in zip(rows, PAIR_LOOKUP_LENGTHS):
        h, x = hit[row], miss[row]
        if length > PAIR_LOOKUP_STRIDE:
            r = (int(h[len(h) // 2]) - PAIR_LOOKUP_STRIDE) % n
            sel = (np.arange(length) + r) % n
        else:
            sel = {0: [], 1: [h[0]], 3: [h[1], x[0], h[2]], 5: [h[3], x[1], h[4], x[2], h[3]]}[length]
        sels.append(np.asarray(sel, np.int64))
    return dict(rows=rows, sels=sels, S=S, cases=cases)


CAND_NPOINTS = 300_000
CAND_BLOCK = 256                                         # positions per workgroup of the candidates kernels
CAND_SCAN = 1024                                         # block counts the scan takes per chunk


def candidates_case(ntargets, cap, seed=0):
    """vpFuseCandidates over ntargets * cap positions, for the scan of the per-block counts where it carries from one chunk of 1024
    blocks into the next: dict(slot [ntargets + 1][cap] (the last row is the current keyframe), n, targets, bad, cur).  ~300 000
    points, 5 % bad; row 3 holds fewer than cap points.  Behind position 1024 * 256 every other slot repeats a point that
    occurred before it, the others hold points that occur nowhere before."""
    rng = np.random.default_rng(7700 + seed + ntargets * 10_000 + cap)
    total, edge = ntargets * cap, CAND_SCAN * CAND_BLOCK
    low = min(total, edge)
    fresh = rng.permutation(CAND_NPOINTS)
    flat = np.full(total, -1, np.int64)
    flat[:low] = fresh[rng.integers(0, 200_000, low)]                 # with repeats among themselves
    if total > low:
        k = total - low
        flat[low:] = np.where(np.arange(k) % 2 == 0, flat[rng.integers(0, low, k)], fresh[200_000 + rng.permutation(100_000)[:k]])
    flat[rng.random(total) < 0.03] = -1                               # empty slots
    slot = np.concatenate([flat.reshape(ntargets, cap), fresh[rng.integers(0, CAND_NPOINTS, cap)].reshape(1, cap)]).astype(np.int32)
    n = np.full(ntargets + 1, cap, np.int32)
    n[3] = cap - 37
    bad = (rng.random(CAND_NPOINTS) < 0.05).astype(np.uint8)
    return dict(slot=slot, n=n, targets=np.arange(ntargets, dtype=np.int32), bad=bad, cur=ntargets)
