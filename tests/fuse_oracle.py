"""A numpy restatement of ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:1031-1182, :1198-1318), under the numbered rules of
DESIGN.md 8p: one binary32 operation per float operation of the reference, 3x3 * 3x1 products summed left to right, norms and dot
products in double, serial loops in the reference's order.  The gate and the search are pinned by the compiled reference wherever
oracle/_ref is built (tests/test_fuse_oracle.py holds the whole Fuse against ref_fuse / ref_fuse_sim3 on the mock objects of
oracle/refbuild/ref_mocks.h).  Also the entry-state action codes of the device replay, the serial replay on the mock's Replace /
AddObservation, and vpFuseCandidates.  Test support only."""
import math

import numpy as np

from oracle import oracle_ffi as O

F = np.float32
GRID_COLS, GRID_ROWS = 64, 48
TH_LOW = 50
PLAIN, SIM3 = 0, 1
NONE, ADD, REPLACE_SLOT, REPLACE_POINT, COUNTED, DEFERRED, REPLACE_CANDIDATE = range(7)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def pose34(Rcw, tcw):
    return np.concatenate([np.asarray(Rcw, F).reshape(3, 3), np.asarray(tcw, F).reshape(3, 1)], 1)


def decompose_sim3(Scw):
    """F0 (Sim3 overload, :1209-1213; the caller's expressions): scw = (float)sqrt(row 0 . row 0) with the dot product in double,
    Rcw = sRcw / scw and tcw = Scw.col(3) / scw per element in double rounded to float, Ow = -Rcw.t() * tcw left to right in float"""
    S = np.asarray(Scw, F).reshape(4, 4)
    r0 = [float(v) for v in S[0, :3]]
    scw = F(math.sqrt(r0[0] * r0[0] + r0[1] * r0[1] + r0[2] * r0[2]))
    T = np.zeros((3, 4), F)
    for r in range(3):
        for c in range(4):
            T[r, c] = F(float(S[r, c]) / float(scw))
    Ow = np.zeros(3, F)
    for k in range(3):
        acc = F(F(-T[0, k]) * T[0, 3])
        acc = F(acc + F(F(-T[1, k]) * T[1, 3]))
        acc = F(acc + F(F(-T[2, k]) * T[2, 3]))
        Ow[k] = acc
    return T, Ow


def predict_scale(max_dist, dist, log_sf, nlevels):
    """MapPoint::PredictScale(dist, KeyFrame*): ceil(log(max / dist) / mfLogScaleFactor), float ratio, float log, float quotient"""
    ratio = F(F(max_dist) / F(dist))
    lg = F(math.log(float(ratio))) if ratio > 0 else F(-np.inf)
    n = int(math.ceil(F(lg / F(log_sf))))
    return min(max(n, 0), nlevels - 1)


def gate_point(T, Ow, K, bounds, th, sf, log_sf, P, Pn, min_dist, max_dist, chi2):
    """F2 .. F8 for one point: None where the reference `continue`s, else dict(u, v, r, ur, level, flags)"""
    fx, fy, cx, cy, bf = (F(v) for v in K[:5])
    minx, maxx, miny, maxy = (F(v) for v in bounds)
    P, Pn = np.asarray(P, F), np.asarray(Pn, F)
    pc = np.zeros(3, F)
    for k in range(3):                                   # F2: p3Dc = Rcw * p3Dw + tcw
        acc = F(T[k, 0] * P[0])
        acc = F(acc + F(T[k, 1] * P[1]))
        acc = F(acc + F(T[k, 2] * P[2]))
        pc[k] = F(acc + T[k, 3])
    if pc[2] < 0:                                        # F3
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = F(F(1) / pc[2])                           # F4 (the Sim3 body's 1.0 / z in double rounds to the same float)
        x, y = F(pc[0] * invz), F(pc[1] * invz)
        u, v = F(F(fx * x) + cx), F(F(fy * y) + cy)
    if not (u >= minx and u < maxx and v >= miny and v < maxy):   # F5: KeyFrame::IsInImage; NaN is out
        return None
    po = [float(F(P[k] - Ow[k])) for k in range(3)]     # F6: PO in float, the norm in double
    dist = F(math.sqrt(po[0] * po[0] + po[1] * po[1] + po[2] * po[2]))
    # min_dist / max_dist are mfMinDistance / mfMaxDistance: the getters scale them, PredictScale reads mfMaxDistance itself
    if dist < F(F(0.8) * F(min_dist)) or dist > F(F(1.2) * F(max_dist)):
        return None
    dot = po[0] * float(Pn[0]) + po[1] * float(Pn[1]) + po[2] * float(Pn[2])
    if dot < 0.5 * float(dist):                          # F7: in double, against 0.5 * (double)dist3D
        return None
    lv = predict_scale(max_dist, dist, log_sf, len(sf))  # F8
    return dict(u=u, v=v, r=F(F(th) * F(sf[lv])), ur=F(u - F(bf * invz)), level=lv, flags=4 if chi2 else 0)


def gate_points(T, Ow, K, bounds, th, sf, log_sf, world_pos, normal, min_dist, max_dist, chi2):
    """the layout of orbfe_fuse_gate_points: (q [n] of (u, v, r, min_level, max_level, ur, flags, pad) as uint32 bit patterns, level, ok)"""
    n = len(min_dist)
    q, level, ok = np.zeros((n, 8), np.uint32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for i in range(n):
        g = gate_point(T, Ow, K, bounds, th, sf, log_sf, world_pos[i], normal[i], min_dist[i], max_dist[i], chi2)
        if g is None:
            continue
        fl = np.array([g["u"], g["v"], g["r"], 0, 0, g["ur"]], F).view(np.uint32)
        it = np.array([g["level"] - 1, g["level"], g["flags"], 0], np.int32).view(np.uint32)
        q[i] = [fl[0], fl[1], fl[2], it[0], it[1], fl[5], it[2], it[3]]
        level[i], ok[i] = g["level"], 1
    return q, level, ok


_grids = {}


def grid_of(kf):
    key = id(kf["xy"])
    if key not in _grids:
        minx, _, miny, _ = kf["bounds"]
        _grids[key] = (kf["xy"], O.assign_grid(kf["xy"], minx, miny, kf["gw_inv"], kf["gh_inv"]))
    return _grids[key][1]


def features_in_area(kf, x, y, r):
    """F9: KeyFrame::GetFeaturesInArea(x, y, r) -- cells ix outer, iy inner, a cell's features in index order, the box test strict"""
    off, idx = grid_of(kf)
    minx, _, miny, _ = (F(v) for v in kf["bounds"])
    gwi, ghi = F(kf["gw_inv"]), F(kf["gh_inv"])
    x0 = max(0, int(math.floor(F(F(F(x - minx) - r) * gwi))))
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(math.ceil(F(F(F(x - minx) + r) * gwi))))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(F(F(F(y - miny) - r) * ghi))))
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(math.ceil(F(F(F(y - miny) + r) * ghi))))
    if y1 < 0:
        return []
    xy = np.asarray(kf["xy"], F).reshape(-1, 2)
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = ix * GRID_ROWS + iy
            for k in idx[off[c]:off[c + 1]]:
                if abs(F(xy[k, 0] - x)) < r and abs(F(xy[k, 1] - y)) < r:
                    out.append(int(k))
    return out


def search_point(kf, g, d, chi2):
    """F9 .. F12 for one gated point with descriptor d: (bestIdx or -1, bestDist; 256 = no candidate)"""
    xy, octv = np.asarray(kf["xy"], F).reshape(-1, 2), np.asarray(kf["octave"])
    uR, is2, desc = np.asarray(kf["uRight"], F), np.asarray(kf["inv_sigma2"], F), np.asarray(kf["desc"], np.uint8).reshape(-1, 32)
    best, best_idx = 256, -1
    for k in features_in_area(kf, g["u"], g["v"], g["r"]):
        lv = int(octv[k])
        if lv < g["level"] - 1 or lv > g["level"]:       # F10
            continue
        if lv < 0 or lv >= len(is2):                     # this library: never a candidate (the reference would index out of bounds)
            continue
        if chi2:                                         # F11 (plain overload only)
            ex, ey = F(g["u"] - xy[k, 0]), F(g["v"] - xy[k, 1])
            e2 = F(F(ex * ex) + F(ey * ey))
            bound = 5.99
            if uR[k] >= 0:
                er = F(g["ur"] - uR[k])
                e2 = F(e2 + F(er * er))
                bound = 7.8
            if float(F(e2 * is2[lv])) > bound:
                continue
        dist = int(_POP[desc[k] ^ d].sum())
        if dist < best:                                  # F12: strict, so the first in order wins a tie
            best, best_idx = dist, k
    return best_idx, best


def fuse_search(kf, T, Ow, tmap, list_idx, list_skip, th, mode, th_low=TH_LOW):
    """F1 .. F13 for one (keyframe, list) pair: (match [n], dist [n]).  tmap: dict(world_pos, normal, min_dist, max_dist, bad, desc)"""
    n = len(list_idx)
    match, dist = np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    npts = len(tmap["bad"])
    for i in range(n):
        p = int(list_idx[i])
        if p < 0 or p >= npts or (list_skip is not None and list_skip[i]) or tmap["bad"][p]:   # F1
            continue
        g = gate_point(T, Ow, kf["K"], kf["bounds"], th, kf["scale_factors"], kf["log_scale"], tmap["world_pos"][p], tmap["normal"][p],
                       tmap["min_dist"][p], tmap["max_dist"][p], mode == PLAIN)
        if g is None:
            continue
        bi, bd = search_point(kf, g, np.asarray(tmap["desc"], np.uint8).reshape(-1, 32)[p], mode == PLAIN)
        dist[i] = bd
        if bd <= th_low:                                 # F13
            match[i] = bi
    return match, dist


def actions(mode, match, list_idx, slot_mp, bad, nobs, cap):
    """F14: the action of every entry from the slot state AT ENTRY: (action uint8 [n], other [n], nfused, first [cap])"""
    n = len(match)
    action, other, first = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(cap, -1, np.int32)
    npts = len(bad)
    for i in range(n):
        m = int(match[i])
        if m >= 0 and first[m] < 0:
            first[m] = i
    for i in range(n):
        m = int(match[i])
        if m < 0:
            continue
        s = int(slot_mp[m]) if slot_mp is not None else -1
        if s < 0 or s >= npts:
            s = -1
        f = int(first[m])
        if s >= 0 and bad[s]:
            action[i] = COUNTED
        elif mode == SIM3:
            if s >= 0:
                action[i], other[i] = REPLACE_CANDIDATE, s
            elif f == i:
                action[i] = ADD
            else:
                action[i], other[i] = REPLACE_CANDIDATE, list_idx[f]
        elif f != i:
            action[i], other[i] = DEFERRED, f
        elif s < 0:
            action[i] = ADD
        else:
            action[i] = REPLACE_POINT if nobs[s] > nobs[list_idx[i]] else REPLACE_SLOT
            other[i] = s
    return action, other, int((np.asarray(match) >= 0).sum()), first


def fuse_pair(kf, T, Ow, tmap, list_idx, list_skip, slot_mp, nobs, th, mode, th_low=TH_LOW, cap=None):
    """what orbfe_fuse_batch_device leaves for one pair"""
    match, dist = fuse_search(kf, T, Ow, tmap, list_idx, list_skip, th, mode, th_low)
    cap = cap if cap is not None else max(len(np.asarray(kf["octave"])), 1)
    action, other, nfused, first = actions(mode, match, list_idx, slot_mp, tmap["bad"], nobs, cap)
    return dict(match=match, dist=dist, action=action, other=other, nfused=nfused, first=first)


# ------------------------------------------------------------------------------------------------ the serial replays on the mock
def mock_replay_plain(kf, mps, match):
    """Fuse(pKF, vpMapPoints, th) :1154-1179 in list order on the mock objects (oracle/refbuild/ref_mocks.h: Replace(p) sets `replaced`
    and mbBad, AddObservation increments nObs for a keyframe the point does not observe yet), driven by the per-entry bestIdx.  In
    the encoding of ref_fuse: (kf_assigned [nKF], mp_replaced [nmp], own_replaced [nKF], return value) and, per entry, what the loop
    did: (serial_action, serial_other) with `other` in map indices (list point i = i, the keyframe's own point of feature j = nmp + j)."""
    nKF, nmp = len(np.asarray(kf["octave"])), len(np.asarray(mps["bad"]))
    state = np.asarray(kf["state"])
    assigned = np.where(state > 0, -2, -1).astype(np.int32)
    own_bad, own_obs = (state == 2).copy(), np.asarray(kf["obs"]).astype(np.int64).copy()
    mp_bad, mp_obs = np.asarray(mps["bad"]).astype(bool).copy(), np.asarray(mps["obs"]).astype(np.int64).copy()
    mp_replaced, own_replaced = np.full(nmp, -1, np.int32), np.full(nKF, -1, np.int32)
    s_action, s_other = np.zeros(nmp, np.uint8), np.full(nmp, -1, np.int32)
    nf = 0
    for i in range(nmp):
        m = int(match[i])
        if m < 0:
            continue
        a = int(assigned[m])
        if a == -1:
            mp_obs[i] += 1
            assigned[m] = i
            s_action[i] = ADD
        else:
            bad, obs = (own_bad[m], own_obs[m]) if a == -2 else (mp_bad[a], mp_obs[a])
            if bad:
                s_action[i] = COUNTED
            elif obs > mp_obs[i]:
                mp_replaced[i] = -(m + 2) if a == -2 else a
                mp_bad[i] = True
                s_action[i], s_other[i] = REPLACE_POINT, (nmp + m if a == -2 else a)
            else:
                if a == -2:
                    own_replaced[m], own_bad[m] = i, True
                else:
                    mp_replaced[a], mp_bad[a] = i, True
                s_action[i], s_other[i] = REPLACE_SLOT, (nmp + m if a == -2 else a)
        nf += 1
    return assigned, mp_replaced, own_replaced, nf, s_action, s_other


def sim3_result(kf, nmp, match, action, other):
    """the outputs of ref_fuse_sim3 from the action codes: (kf_assigned [nKF], replace_point [nmp], return value)"""
    state = np.asarray(kf["state"])
    assigned = np.where(state > 0, -2, -1).astype(np.int32)
    rep = np.full(nmp, -1, np.int32)
    for i in range(nmp):
        if action[i] == ADD:
            assigned[match[i]] = i
        elif action[i] == REPLACE_CANDIDATE:
            rep[i] = other[i] - nmp if other[i] >= nmp else -(int(other[i]) + 2)
    return assigned, rep, int((np.asarray(action) != NONE).sum())


# ------------------------------------------------------------------------------------------------ vpFuseCandidates
def candidates(slot_mp, n, targets, bad, cur_kf=-1):
    """LocalMapping::SearchInNeighbors :705-725 as written: a loop with the mnFuseCandidateForKF stamp -> (cand, skip)"""
    nkf, cap = slot_mp.shape
    stamp = np.zeros(len(bad), bool)
    out = []
    for t in targets:
        if t < 0 or t >= nkf:
            continue
        for s in range(min(max(int(n[t]), 0), cap)):
            p = int(slot_mp[t, s])
            if p < 0 or p >= len(bad) or bad[p] or stamp[p]:
                continue
            stamp[p] = True
            out.append(p)
    in_cur = set()
    if cur_kf >= 0:
        in_cur = {int(p) for p in slot_mp[cur_kf, :min(max(int(n[cur_kf]), 0), cap)] if 0 <= p < len(bad)}
    return np.array(out, np.int32), np.array([p in in_cur for p in out], np.uint8)
