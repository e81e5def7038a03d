"""ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651) restated in numpy, line for line, and the model of what the
device does instead of the sequential loop (csrc/orbfe_init_search.hip): relaxation rounds over per-feature claim
lists, plus the two one-word-per-feature shortcuts that are NOT equivalent.  Test support only; Frame::GetFeaturesInArea and
the grid come from the C oracle (pinned to the reference by tests/test_ref_pin.py).

Frames are the dicts of tests/proj_cases.py: desc uint8 [n, 32], xy float32 [n, 2], octave int32 [n], angle float32 [n],
bounds = (minx, maxx, miny, maxy), gw_inv, gh_inv."""
import numpy as np

from oracle import oracle_ffi as O

F = np.float32
INT_MAX = 2 ** 31 - 1
TH_LOW = 50          # src/ORBmatcher.cc:40
HISTO_LENGTH = 30    # src/ORBmatcher.cc:41
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    """DescriptorDistance (:1968-1984) of row a against the rows b"""
    return _POP[np.bitwise_xor(np.asarray(b, np.uint8).reshape(-1, 32), np.asarray(a, np.uint8).reshape(1, 32))].sum(1)


def frame_grid(f):
    minx, _, miny, _ = f["bounds"]
    return O.assign_grid(f["xy"], minx, miny, f["gw_inv"], f["gh_inv"])


def candidate_lists(f1, f2, prev, window):
    """(qsrc, lists): the level-0 features of f1 in index order and, for each, (candidates, distances) of
    F2.GetFeaturesInArea(prev.x, prev.y, window, 0, 0) in the cell-walk order (:539-564)"""
    off, idx = frame_grid(f2)
    minx, _, miny, _ = f2["bounds"]
    prev = np.asarray(prev, F).reshape(-1, 2)
    qsrc, lists = [], []
    for i1 in range(len(f1["octave"])):
        if f1["octave"][i1] != 0:   # :540-542 and GetFeaturesInArea's level filter for level1 < 0
            continue
        c = O.features_in_area(f2["xy"], f2["octave"], off, idx, minx, miny, f2["gw_inv"], f2["gh_inv"], float(prev[i1, 0]), float(prev[i1, 1]),
                               float(window), 0, 0).astype(np.int64)
        qsrc.append(i1)
        lists.append((c, descriptor_distance(f1["desc"][i1], f2["desc"][c]) if len(c) else np.zeros(0, np.int32)))
    return np.asarray(qsrc, np.int64), lists


def entries(lists):
    """the lists as orbfe_window_distances lays them out: off uint32 [nq + 1], ent = candidate | distance << 16"""
    off = np.zeros(len(lists) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c, _ in lists])
    ent = np.concatenate([(c | (d.astype(np.int64) << 16)) for c, d in lists] + [np.zeros(0, np.int64)]).astype(np.uint32)
    return off, ent


def rot_bin(a1, a2):
    """:602-607: float arithmetic, round() half away from zero"""
    rot = F(a1) - F(a2)
    if rot < 0.0:
        rot = F(rot + F(360.0))
    v = F(rot * (F(1.0) / F(HISTO_LENGTH)))
    b = int(np.floor(v + F(0.5))) if v >= 0 else int(np.ceil(v - F(0.5)))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(counts):
    """ComputeThreeMaxima (:1912-1957) on the bins' sizes"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if F(max2) < F(0.1) * F(max1):
        i2 = i3 = -1
    elif F(max3) < F(0.1) * F(max1):
        i3 = -1
    return i1, i2, i3


def _accepts(best, second, th_low, nnratio):
    """:583-587: bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio"""
    return best <= th_low and F(best) < F(F(second) * F(nnratio))


def search_for_initialization(f1, f2, prev, window, th_low=TH_LOW, nnratio=0.9, check_ori=True, details=False):
    """-> (matches12 int32 [n1], prev_out float32 [n1, 2], nmatches); details=True adds a dict with the accepted feature per
    level-0 query, the take-overs and how many candidates the skip of :566 removed"""
    n1, n2 = len(f1["octave"]), len(f2["octave"])
    qsrc, lists = candidate_lists(f1, f2, prev, window)
    nmatches = 0
    vnMatches12 = np.full(n1, -1, np.int32)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    vMatchedDistance = np.full(n2, INT_MAX, np.int64)
    vnMatches21 = np.full(n2, -1, np.int64)
    accepted, takeovers, skipped = np.full(len(qsrc), -1, np.int64), 0, 0
    for q, i1 in enumerate(qsrc):
        vIndices2, dists = lists[q]
        if len(vIndices2) == 0:
            continue
        bestDist, bestDist2, bestIdx2 = INT_MAX, INT_MAX, -1
        for i2, dist in zip(vIndices2, dists):
            if vMatchedDistance[i2] <= dist:
                skipped += 1
                continue
            if dist < bestDist:
                bestDist2, bestDist, bestIdx2 = bestDist, dist, i2
            elif dist < bestDist2:
                bestDist2 = dist
        if bestDist <= th_low:
            if F(bestDist) < F(F(bestDist2) * F(nnratio)):
                if vnMatches21[bestIdx2] >= 0:
                    vnMatches12[vnMatches21[bestIdx2]] = -1
                    nmatches -= 1
                    takeovers += 1
                vnMatches12[i1] = bestIdx2
                vnMatches21[bestIdx2] = i1
                vMatchedDistance[bestIdx2] = bestDist
                nmatches += 1
                accepted[q] = bestIdx2
                if check_ori:
                    rotHist[rot_bin(f1["angle"][i1], f2["angle"][bestIdx2])].append(i1)
    if check_ori:
        ind = three_maxima([len(h) for h in rotHist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rotHist[i]:
                if vnMatches12[idx1] >= 0:
                    vnMatches12[idx1] = -1
                    nmatches -= 1
    prev_out = np.array(prev, F).reshape(-1, 2).copy()
    for i1 in range(n1):
        if vnMatches12[i1] >= 0:
            prev_out[i1] = f2["xy"][vnMatches12[i1]]
    if details:
        return vnMatches12, prev_out, nmatches, dict(qsrc=qsrc, accepted=accepted, takeovers=takeovers, skipped=skipped)
    return vnMatches12, prev_out, nmatches


# ---- the device's algorithm as a model ----------------------------------------------------------------------------------------
def relaxation(lists, n2, th_low=TH_LOW, nnratio=0.9, table="lists"):
    """Rounds to a fixed point: in every round each query decides against the claims (feature, distance) the queries made in
    the round BEFORE; stop after a round that changes no claim.  -> (accepted [nq] (feature or -1), dist [nq], rounds run)
      table = "lists"         every claimant k < i with d_k <= d blocks (what the reference's vMatchedDistance amounts to)
      table = "min_distance"  one word per feature, the smallest claimed distance: blocks when that is <= d (a later query's
                              closer claim blocks an earlier query: wrong)
      table = "lowest_query"  one word per feature, the lowest claiming query: blocks when it is < i and holds d_k <= d (a
                              closer claim of a query in between is not seen: wrong)"""
    nq = len(lists)
    acc, dist = np.full(nq, -1, np.int64), np.zeros(nq, np.int64)
    rounds = 0
    while rounds <= nq + 1:
        rounds += 1
        claims = [[] for _ in range(n2)]
        for k in range(nq):
            if acc[k] >= 0:
                claims[acc[k]].append((k, dist[k]))

        def blocked(i, j, d):
            cl = claims[j]
            if table == "lists":
                return any(k < i and dk <= d for k, dk in cl)
            if table == "min_distance":
                other = [dk for k, dk in cl if k != i]
                return bool(other) and min(other) <= d
            k, dk = min(cl) if cl else (nq, 0)
            return k < i and dk <= d

        new_acc, new_dist = acc.copy(), dist.copy()
        for i, (cand, dd) in enumerate(lists):
            best, second, arg = INT_MAX, INT_MAX, -1
            for j, d in zip(cand, dd):
                if blocked(i, j, d):
                    continue
                if d < best:
                    second, best, arg = best, d, j
                elif d < second:
                    second = d
            ok = arg >= 0 and _accepts(best, second, th_low, nnratio)
            new_acc[i], new_dist[i] = (arg, best) if ok else (-1, 0)
        changed = not (np.array_equal(new_acc, acc) and np.array_equal(new_dist, dist))
        acc, dist = new_acc, new_dist
        if not changed:
            break
    return acc, dist, rounds


def finish(f1, f2, prev, qsrc, accepted, check_ori=True):
    """what the loop leaves behind, from the accepted feature of every query: the last query accepted on a feature holds it, all
    accepted queries vote, a vote in a dropped bin clears an entry that still stands -> (matches12, prev_out, nmatches)"""
    n1, n2 = len(f1["octave"]), len(f2["octave"])
    holder = np.full(n2, -1, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    for q, j in enumerate(accepted):
        if j >= 0:
            holder[j] = q
            if check_ori:
                hist[rot_bin(f1["angle"][qsrc[q]], f2["angle"][j])].append(q)
    m = np.full(n1, -1, np.int32)
    for q, j in enumerate(accepted):
        if j >= 0 and holder[j] == q:
            m[qsrc[q]] = j
    if check_ori:
        ind = three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b not in ind:
                for q in hist[b]:
                    m[qsrc[q]] = -1
    prev_out = np.array(prev, F).reshape(-1, 2).copy()
    st = m >= 0
    prev_out[st] = f2["xy"][m[st]]
    return m, prev_out, int(st.sum())


def model(f1, f2, prev, window, th_low=TH_LOW, nnratio=0.9, check_ori=True, table="lists"):
    """the device's result by its own algorithm -> (matches12, prev_out, nmatches, rounds)"""
    qsrc, lists = candidate_lists(f1, f2, prev, window)
    acc, _, rounds = relaxation(lists, len(f2["octave"]), th_low, nnratio, table)
    return finish(f1, f2, prev, qsrc, acc, check_ori) + (rounds,)
