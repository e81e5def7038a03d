"""A numpy restatement of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1334-1558) and of SearchByProjection(pKF, Scw, vpPoints,
vpMatched, th) (:378-498) in the flat layout of the device calls, under the rules of DESIGN.md 8q: one binary32 operation per float
operation of the reference, matrix products summed left to right from 0, norms in double, serial loops in the reference's order.
Pinned by the compiled reference wherever oracle/_ref is built (tests/test_sim3_search_oracle.py).  Test support only.

Every member takes an optional `trace` list and appends (comparison, outcome) for each decision it makes: outcome is the sign of
left - right (-1, 0, 1; 2 when unordered) for a numeric comparison, a bool or a word otherwise.  SIM3S_BREAK breaks exactly one
rule of SIM3S_RULES at a time, so that a test can show which cases a kernel with that rule wrong would fail
(tests/test_sim3_search_edge_cases.py).  With the switch unset the results are those of the version without either
(tests/golden/sim3_search_oracle_digests.json)."""
import math

import numpy as np

import fuse_oracle as FO

F = np.float32
TH_HIGH, TH_LOW = 100, 50
_POP = FO._POP

SIM3S_RULES = {
    # the gate of SearchBySim3
    "z_le": "pc'.z <= 0 is out, not < 0",
    "u_min_open": "u > minx, not >=", "u_max_closed": "u <= maxx, not <", "v_min_open": "v > miny, not >=", "v_max_closed": "v <= maxy, not <",
    "d08_le": "dist <= 0.8 * min is out, not <", "d08_factor": "dist < min, without the 0.8",
    "d12_ge": "dist >= 1.2 * max is out, not >", "d12_factor": "dist > max, without the 1.2",
    "clamp0": "no clamp of the level at 0", "clampN": "no clamp of the level at nlevels - 1", "r_no_sf": "r = th, not th * sf[level]",
    "fused_pose": "(T_to * T_own) * P with the product of the poses in float, not T_to * (T_own * P)",
    # the candidate loop
    "oct_lo_wide": "octave level - 2 is a candidate", "oct_lo_narrow": "octave level - 1 is not", "oct_hi_wide": "octave level + 1 is",
    "oct_hi_narrow": "octave level is not", "first_min_le": "<= for the minimum: the last of a tie wins", "th_high_lt": "< th_high, not <=",
    # SearchBySim3's bookkeeping
    "already1_ge0": "vbAlreadyMatched1 is >= 0, not != -1", "already2_clip": "an index >= N2 marks feature N2 - 1",
    "agree_off": "vnMatch1 alone decides, vnMatch2[j] == i1 is not asked",
    # the projection form
    "found_live": "spAlreadyFound grows with every claim", "found_off": "spAlreadyFound is empty", "blocked_ge0": "a slot is blocked iff >= 0 at entry",
    "claim_open": "a claimed slot stays a candidate", "th_low_lt": "< th_low, not <=", "bad_kept": "a bad point is searched",
    "angle_off": "no viewing-angle gate", "angle_le": "dot <= 0.5 * dist is out, not <",
}
SIM3S_BREAK = frozenset()


def _b(rule):
    return rule in SIM3S_BREAK


def _sgn(a, b):
    return 2 if (a != a or b != b) else int(a > b) - int(a < b)


def _t(trace, key, val):
    if trace is not None:
        trace.append((key, val))


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


def _fused(T_to, T_own):
    """the broken rule "fused_pose": one pose (A_to * A_own | A_to * b_own + b_to), every product in float from 0"""
    A, B = np.asarray(T_to, F).reshape(3, 4), np.asarray(T_own, F).reshape(3, 4)
    out = np.zeros((3, 4), F)
    for c in range(3):
        out[:, c] = affine(np.concatenate([A[:, :3], np.zeros((3, 1), F)], 1), B[:, c])
    out[:, 3] = affine(A, B[:, 3])
    return out


def predict_level(max_dist, dist, log_sf, nlevels, trace=None):
    """fuse_oracle.predict_scale with its two clamps traced: (level, level of the search radius)"""
    ratio = F(F(max_dist) / F(dist))
    lg = F(math.log(float(ratio))) if ratio > 0 else F(-np.inf)
    n = int(math.ceil(F(lg / F(log_sf))))
    _t(trace, "clamp0", _sgn(n, 0))
    _t(trace, "clampN", _sgn(n, nlevels - 1))
    lv = min(max(n, 0), nlevels - 1)
    if n < 0 and _b("clamp0"):
        return n, lv
    if n >= nlevels and _b("clampN"):
        return n, lv
    return lv, lv


def gate_point(T_own, T_to, K, bounds, th, sf, log_sf, P, min_dist, max_dist, trace=None):
    """:1400-1431 / :1476-1503 for one point: None where the reference `continue`s, else dict(u, v, r, ur, level)"""
    fx, fy, cx, cy, bf = (F(v) for v in K[:5])
    minx, maxx, miny, maxy = (F(v) for v in bounds)
    po = affine(_fused(T_to, T_own), np.asarray(P, F)) if _b("fused_pose") else affine(T_to, affine(T_own, np.asarray(P, F)))
    _t(trace, "z", _sgn(po[2], 0))
    if po[2] <= 0 if _b("z_le") else po[2] < 0:
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F(F(1) / po[2])
        x, y = F(po[0] * invz), F(po[1] * invz)
        u, v = F(F(fx * x) + cx), F(F(fy * y) + cy)
    for key, a, b in (("u_min", u, minx), ("u_max", u, maxx), ("v_min", v, miny), ("v_max", v, maxy)):
        _t(trace, key, _sgn(a, b))
    if not ((u > minx if _b("u_min_open") else u >= minx) and (u <= maxx if _b("u_max_closed") else u < maxx) and
            (v > miny if _b("v_min_open") else v >= miny) and (v <= maxy if _b("v_max_closed") else v < maxy)):
        return None
    d = [float(c) for c in po]
    dist = F(math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))     # cv::norm(p3Dc): the camera-frame point
    lo = F(min_dist) if _b("d08_factor") else F(F(0.8) * F(min_dist))
    hi = F(max_dist) if _b("d12_factor") else F(F(1.2) * F(max_dist))
    _t(trace, "d08", _sgn(dist, lo))
    _t(trace, "d08_band", bool(F(F(0.8) * F(min_dist)) <= dist < F(min_dist)))
    _t(trace, "d12", _sgn(dist, hi))
    _t(trace, "d12_band", bool(F(max_dist) < dist <= F(F(1.2) * F(max_dist))))
    if (dist <= lo if _b("d08_le") else dist < lo) or (dist >= hi if _b("d12_ge") else dist > hi):
        return None
    lv, rlv = predict_level(max_dist, dist, log_sf, len(sf), trace)
    r = F(th) if _b("r_no_sf") else F(F(th) * F(sf[rlv]))
    return dict(u=u, v=v, r=r, ur=F(u - F(bf * invz)), level=lv)


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


def gate_point_proj(T, Ow, K, bounds, th, sf, log_sf, P, Pn, min_dist, max_dist, trace=None):
    """fuse_oracle.gate_point without chi2 (the gate of the projection form, Fuse's Sim3 gate) with its viewing-angle comparison
    traced and breakable; the other comparisons are Fuse's own tests' business"""
    fx, fy, cx, cy, bf = (F(v) for v in K[:5])
    minx, maxx, miny, maxy = (F(v) for v in bounds)
    P, Pn = np.asarray(P, F), np.asarray(Pn, F)
    pc = np.zeros(3, F)
    for k in range(3):
        acc = F(T[k, 0] * P[0])
        acc = F(acc + F(T[k, 1] * P[1]))
        acc = F(acc + F(T[k, 2] * P[2]))
        pc[k] = F(acc + T[k, 3])
    if pc[2] < 0:
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F(F(1) / pc[2])
        x, y = F(pc[0] * invz), F(pc[1] * invz)
        u, v = F(F(fx * x) + cx), F(F(fy * y) + cy)
    if not (u >= minx and u < maxx and v >= miny and v < maxy):
        return None
    po = [float(F(P[k] - Ow[k])) for k in range(3)]
    dist = F(math.sqrt(po[0] * po[0] + po[1] * po[1] + po[2] * po[2]))
    if dist < F(F(0.8) * F(min_dist)) or dist > F(F(1.2) * F(max_dist)):
        return None
    dot = po[0] * float(Pn[0]) + po[1] * float(Pn[1]) + po[2] * float(Pn[2])
    _t(trace, "angle", _sgn(dot, 0.5 * float(dist)))
    if not _b("angle_off") and (dot <= 0.5 * float(dist) if _b("angle_le") else dot < 0.5 * float(dist)):
        return None
    lv = FO.predict_scale(max_dist, dist, log_sf, len(sf))
    return dict(u=u, v=v, r=F(F(th) * F(sf[lv])), ur=F(u - F(bf * invz)), level=lv, flags=0)


def search_point(kf, g, d, blocked=None, trace=None, claimed=None):
    """the candidate loop: (bestIdx or -1, bestDist; 256 = no candidate), the first in GetFeaturesInArea order wins a tie"""
    octv, desc = np.asarray(kf["octave"]), np.asarray(kf["desc"], np.uint8).reshape(-1, 32)
    best, best_idx = 256, -1
    lo = g["level"] - (2 if _b("oct_lo_wide") else 0 if _b("oct_lo_narrow") else 1)
    hi = g["level"] + (1 if _b("oct_hi_wide") else -1 if _b("oct_hi_narrow") else 0)
    for k in FO.features_in_area(kf, g["u"], g["v"], g["r"]):
        if blocked is not None:
            _t(trace, "slot_blocked", bool(blocked[k]))
            if claimed is not None:
                _t(trace, "slot_claimed", bool(claimed[k]))
            if blocked[k]:
                continue
        lv = int(octv[k])
        _t(trace, "oct_lo", _sgn(lv, g["level"] - 1))
        _t(trace, "oct_hi", _sgn(lv, g["level"]))
        if lv < lo or lv > hi:
            continue
        dist = int(_POP[desc[k] ^ d].sum())
        _t(trace, "first_min", _sgn(dist, best))
        if dist <= best if _b("first_min_le") else dist < best:
            best, best_idx = dist, k
    return best_idx, best


def pose34(k):
    return FO.pose34(k["Rcw"], k["tcw"])


def search_by_sim3(k1, k2, T12, T21, th, matches_in, th_high=TH_HIGH, trace=None):
    """SearchBySim3 in index form: (matches_out [N1], nFound, vnMatch1 [N1], vnMatch2 [N2]).  k: the keyframe dicts of
    proj_cases.sim3_pair_case; T12 / T21 from orbfe_sim3_pair_pose or pair_pose()."""
    n1, n2 = len(np.asarray(k1["octave"])), len(np.asarray(k2["octave"]))
    m12 = np.asarray(matches_in, np.int32).reshape(-1)[:n1].copy()
    already1 = m12 >= 0 if _b("already1_ge0") else m12 != -1
    already2 = np.zeros(n2, bool)
    for j in m12:
        _t(trace, "preset", "null" if j == -1 else "other" if j < 0 else "in" if j < n2 else "past")
        if 0 <= j < n2:
            already2[j] = True
        elif j >= n2 > 0 and _b("already2_clip"):
            already2[n2 - 1] = True

    def direction(ks, ko, T_to, already, tag):
        ns = len(np.asarray(ks["octave"]))
        vn = np.full(ns, -1, np.int32)
        T_own = pose34(ks)
        state, mpdesc = np.asarray(ks["state"]), np.asarray(ks["mpdesc"], np.uint8).reshape(-1, 32)
        for i in range(ns):
            _t(trace, "slot" + tag, "empty" if state[i] == 0 else "bad" if state[i] != 1 else "already" if already[i] else "live")
            if state[i] != 1 or already[i]:
                continue
            g = gate_point(T_own, T_to, ko["K"], ko["bounds"], th, ko["scale_factors"], ko["log_scale"], np.asarray(ks["world_pos"], F).reshape(-1, 3)[i],
                           ks["min_dist"][i], ks["max_dist"][i], trace)
            if g is None:
                continue
            bi, bd = search_point(ko, g, mpdesc[i], trace=trace)
            if bi >= 0:
                _t(trace, "th_high", _sgn(bd, th_high))
            if bd < th_high if _b("th_high_lt") else bd <= th_high:
                vn[i] = bi
        return vn

    vn1 = direction(k1, k2, T21, already1, "1")
    vn2 = direction(k2, k1, T12, already2, "2")
    nfound = 0
    for i1 in range(n1):
        j = int(vn1[i1])
        if j >= 0:
            _t(trace, "agree", bool(vn2[j] == i1))
        if j >= 0 and (vn2[j] == i1 or _b("agree_off")):
            m12[i1] = j
            nfound += 1
    return m12, nfound, vn1, vn2


def search_by_projection_kf_sim3(kf, Scw, pts, matched_in, th, th_low=TH_LOW, list_skip=None, trace=None, ids=None):
    """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) in the encoding of ref_search_by_projection_kf_sim3: matched [nKF] = -1
    NULL, k >= 0 point k of the list, -2 another point.  -> (matched_out, nmatches).  ids [n]: the MapPoint behind each list entry
    where a point stands in the list more than once (the default: entry i is point i); matched then holds ids."""
    T, Ow = FO.decompose_sim3(Scw)
    matched = np.asarray(matched_in, np.int32).copy()
    n = len(np.asarray(pts["bad"]))
    ids = np.arange(n) if ids is None else np.asarray(ids)
    found = set() if _b("found_off") else set(int(v) for v in matched if v >= 0)
    entry = matched >= 0 if _b("blocked_ge0") else matched != -1
    claimed = np.zeros(len(matched), bool)
    wp, nr = np.asarray(pts["world_pos"], F).reshape(-1, 3), np.asarray(pts["normal"], F).reshape(-1, 3)
    d = np.asarray(pts["mpdesc"], np.uint8).reshape(-1, 32)
    nm = 0
    for i in range(n):
        skip = bool(list_skip[i]) if list_skip is not None else int(ids[i]) in found
        _t(trace, "entry", "bad" if pts["bad"][i] else "found" if skip else "live")
        if (pts["bad"][i] and not _b("bad_kept")) or skip:
            continue
        g = gate_point_proj(T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], wp[i], nr[i], pts["min_dist"][i], pts["max_dist"][i],
                            trace)
        if g is None:
            continue
        bi, bd = search_point(kf, g, d[i], blocked=entry if _b("claim_open") else entry | claimed, trace=trace, claimed=claimed)
        if bi >= 0:
            _t(trace, "th_low", _sgn(bd, th_low))
        if bd < th_low if _b("th_low_lt") else bd <= th_low:
            matched[bi] = ids[i]
            claimed[bi] = True
            nm += 1
            if _b("found_live"):
                found.add(int(ids[i]))
    return matched, nm
