"""A numpy restatement of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1334-1558) and of SearchByProjection(pKF, Scw, vpPoints,
vpMatched, th) (:378-498) in the flat layout of the device calls, under the rules of DESIGN.md 8q: one binary32 operation per float
operation of the reference, matrix products summed left to right from 0, norms in double, serial loops in the reference's order.
Pinned by the compiled reference wherever oracle/_ref is built (tests/test_sim3_search_oracle.py).  Test support only."""
import math

import numpy as np

import fuse_oracle as FO

F = np.float32
TH_HIGH, TH_LOW = 100, 50
_POP = FO._POP


def pair_pose(s12, R12, t12):
    """(T12, T21) float32 [3, 4]: :1355-1357 on the stub's cv::Mat -- scalar products in double rounded to float, t21 = (-sR21) * t12"""
    R, t = np.asarray(R12, F).reshape(3, 3), np.asarray(t12, F).reshape(3)
    s, inv = float(F(s12)), 1.0 / float(F(s12))
    T12, T21 = np.zeros((3, 4), F), np.zeros((3, 4), F)
    for r in range(3):
        for c in range(3):
            T12[r, c] = F(float(R[r, c]) * s)
            T21[r, c] = F(float(R[c, r]) * inv)
        T12[r, 3] = t[r]
    for r in range(3):
        acc = F(0)
        for c in range(3):
            acc = F(acc + F(F(-T21[r, c]) * t[c]))
        T21[r, 3] = acc
    return T12, T21


def affine(T, x):
    """A * x + b: the product's accumulator starts at 0, then one add"""
    T = np.asarray(T, F).reshape(3, 4)
    out = np.zeros(3, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(3):
            acc = F(0)
            for c in range(3):
                acc = F(acc + F(T[k, c] * x[c]))
            out[k] = F(acc + T[k, 3])
    return out


def gate_point(T_own, T_to, K, bounds, th, sf, log_sf, P, min_dist, max_dist):
    """:1400-1431 / :1476-1503 for one point: None where the reference `continue`s, else dict(u, v, r, ur, level)"""
    fx, fy, cx, cy, bf = (F(v) for v in K[:5])
    minx, maxx, miny, maxy = (F(v) for v in bounds)
    po = affine(T_to, affine(T_own, np.asarray(P, F)))
    if po[2] < 0:
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F(F(1) / po[2])
        x, y = F(po[0] * invz), F(po[1] * invz)
        u, v = F(F(fx * x) + cx), F(F(fy * y) + cy)
    if not (u >= minx and u < maxx and v >= miny and v < maxy):
        return None
    d = [float(c) for c in po]
    dist = F(math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))     # cv::norm(p3Dc): the camera-frame point
    if dist < F(F(0.8) * F(min_dist)) or dist > F(F(1.2) * F(max_dist)):
        return None
    lv = FO.predict_scale(max_dist, dist, log_sf, len(sf))
    return dict(u=u, v=v, r=F(F(th) * F(sf[lv])), ur=F(u - F(bf * invz)), level=lv)


def gate_points(T_own, T_to, K, bounds, th, sf, log_sf, world_pos, min_dist, max_dist):
    """the layout of orbfe_sim3_gate_points: (q [n][8] uint32 bit patterns, level, ok)"""
    n = len(min_dist)
    q, level, ok = np.zeros((n, 8), np.uint32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for i in range(n):
        g = gate_point(T_own, T_to, K, bounds, th, sf, log_sf, world_pos[i], min_dist[i], max_dist[i])
        if g is None:
            continue
        fl = np.array([g["u"], g["v"], g["r"], 0, 0, g["ur"]], F).view(np.uint32)
        it = np.array([g["level"] - 1, g["level"], 0, 0], np.int32).view(np.uint32)
        q[i] = [fl[0], fl[1], fl[2], it[0], it[1], fl[5], it[2], it[3]]
        level[i], ok[i] = g["level"], 1
    return q, level, ok


def search_point(kf, g, d, blocked=None):
    """the candidate loop: (bestIdx or -1, bestDist; 256 = no candidate), the first in GetFeaturesInArea order wins a tie"""
    octv, desc = np.asarray(kf["octave"]), np.asarray(kf["desc"], np.uint8).reshape(-1, 32)
    best, best_idx = 256, -1
    for k in FO.features_in_area(kf, g["u"], g["v"], g["r"]):
        if blocked is not None and blocked[k]:
            continue
        lv = int(octv[k])
        if lv < g["level"] - 1 or lv > g["level"]:
            continue
        dist = int(_POP[desc[k] ^ d].sum())
        if dist < best:
            best, best_idx = dist, k
    return best_idx, best


def pose34(k):
    return FO.pose34(k["Rcw"], k["tcw"])


def search_by_sim3(k1, k2, T12, T21, th, matches_in, th_high=TH_HIGH):
    """SearchBySim3 in index form: (matches_out [N1], nFound, vnMatch1 [N1], vnMatch2 [N2]).  k: the keyframe dicts of
    proj_cases.sim3_pair_case; T12 / T21 from orbfe_sim3_pair_pose or pair_pose()."""
    n1, n2 = len(np.asarray(k1["octave"])), len(np.asarray(k2["octave"]))
    m12 = np.asarray(matches_in, np.int32).reshape(-1)[:n1].copy()
    already1 = m12 != -1
    already2 = np.zeros(n2, bool)
    for j in m12:
        if 0 <= j < n2:
            already2[j] = True

    def direction(ks, ko, T_to, already):
        ns = len(np.asarray(ks["octave"]))
        vn = np.full(ns, -1, np.int32)
        T_own = pose34(ks)
        state, mpdesc = np.asarray(ks["state"]), np.asarray(ks["mpdesc"], np.uint8).reshape(-1, 32)
        for i in range(ns):
            if state[i] != 1 or already[i]:
                continue
            g = gate_point(T_own, T_to, ko["K"], ko["bounds"], th, ko["scale_factors"], ko["log_scale"], np.asarray(ks["world_pos"], F).reshape(-1, 3)[i],
                           ks["min_dist"][i], ks["max_dist"][i])
            if g is None:
                continue
            bi, bd = search_point(ko, g, mpdesc[i])
            if bd <= th_high:
                vn[i] = bi
        return vn

    vn1 = direction(k1, k2, T21, already1)
    vn2 = direction(k2, k1, T12, already2)
    nfound = 0
    for i1 in range(n1):
        j = int(vn1[i1])
        if j >= 0 and vn2[j] == i1:
            m12[i1] = j
            nfound += 1
    return m12, nfound, vn1, vn2


def search_by_projection_kf_sim3(kf, Scw, pts, matched_in, th, th_low=TH_LOW, list_skip=None):
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) in the encoding of ref_search_by_projection_kf_sim3: matched [nKF] = -1
    NULL, k >= 0 point k of the list, -2 another point.  -> (matched_out, nmatches)"""
    T, Ow = FO.decompose_sim3(Scw)
    matched = np.asarray(matched_in, np.int32).copy()
    n = len(np.asarray(pts["bad"]))
    found = set(int(v) for v in matched if v >= 0)
    wp, nr = np.asarray(pts["world_pos"], F).reshape(-1, 3), np.asarray(pts["normal"], F).reshape(-1, 3)
    d = np.asarray(pts["mpdesc"], np.uint8).reshape(-1, 32)
    nm = 0
    for i in range(n):
        if pts["bad"][i] or (list_skip[i] if list_skip is not None else i in found):
            continue
        g = FO.gate_point(T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], wp[i], nr[i], pts["min_dist"][i], pts["max_dist"][i], False)
        if g is None:
            continue
        bi, bd = search_point(kf, g, d[i], blocked=matched != -1)
        if bd <= th_low:
            matched[bi] = i
            nm += 1
    return matched, nm
