"""Matcher inputs whose answers are known by construction: descriptor sets with PLANTED Hamming distances, angle pairs on
exact float boundaries of the rotation bin, histograms on the ComputeThreeMaxima edges, and hand-built SearchByBoW feature
vectors.  numpy only (CPU); tests/test_hamming_cases.py checks every builder, tests/test_gpu_matcher_edges.py feeds them to
the HIP kernels.

Hamming distances of random 256-bit rows cluster around 128, so random inputs almost never sit on a tie, a threshold or a
float-rounding boundary.  Here a train row is set at an exact distance from a query by flipping that many chosen bits, and
rows that must not compete are either independent random rows (>= ~80 from a random query in practice, checked where it
matters) or `far_rows` of a query base (>= 200 from every query built by `near_rows` of the same base).

Float boundaries (all in IEEE binary32, as the reference computes them):
  * ratio test `(float)best < nnratio * (float)second`: 0.6f * 5 rounds to exactly 3.0f, so (3, 5) is rejected, while in
    double 3 < 3.0000001 would accept it; the same at RATIO_EDGES.
  * ComputeThreeMaxima `(float)max2 < 0.1f * (float)max1`: 0.1f * 10 rounds to 1.0f, so (10, 1) keeps the second maximum.
  * rot_bin `round(rot * (1.0f / 30))`: rot = 15, 135, 255 (and 254.99998) land exactly on 0.5, 4.5, 8.5, where roundf
    (half away from zero) and rintf (half to even) differ.
"""
import numpy as np

POPC = np.array([bin(i).count("1") for i in range(256)], np.uint8)

# (best, second) pairs where the float32 ratio test and a double one disagree (float rejects, double would accept)
RATIO_EDGES = {0.6: [(3, 5), (6, 10), (9, 15), (12, 20)], 0.8: [(4, 5), (8, 10), (12, 15), (16, 20)]}
# (max1, max2) pairs where 0.1f * max1 in float32 equals max2 exactly (double would drop max2)
MAXIMA_EDGES = [(10, 1), (20, 2), (30, 3), (40, 4), (50, 5)]
# rotation = a1 - a2 (+360 when negative) on an exact half bin: (a1, a2, bin under roundf, bin under rintf)
HALF_BIN_ANGLES = [(15.0, 0.0, 1, 0), (135.0, 0.0, 5, 4), (255.0, 0.0, 9, 8), (254.99998, 0.0, 9, 8),
                   (100.0, 85.0, 1, 0), (10.0, 355.0, 1, 0), (0.0, 225.0, 5, 4), (45.0, 150.0, 9, 8)]


def distances(a, b):
    """Hamming distance matrix [len(a), len(b)] (int32), by a byte popcount table."""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
    out = np.empty((len(a), len(b)), np.int32)
    for i in range(0, len(a), 256):
        out[i:i + 256] = POPC[a[i:i + 256, None, :] ^ b[None, :, :]].sum(2, dtype=np.int32)
    return out


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(row, bits):
    """`row` (32 bytes) with the listed bit positions (0..255) inverted."""
    out = np.array(row, np.uint8).reshape(32).copy()
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def at_distance(rng, row, d, lo=0, hi=256):
    """`row` with exactly d distinct bits inverted, chosen from positions [lo, hi)."""
    return flip(row, rng.choice(np.arange(lo, hi), size=int(d), replace=False))


def near_rows(rng, base, n, max_flips=16):
    """n queries around `base`: each inverts up to max_flips bits of [0, 128)"""
    return np.stack([at_distance(rng, base, rng.integers(0, max_flips + 1), 0, 128) for _ in range(n)]) if n else \
        np.zeros((0, 32), np.uint8)


def far_rows(rng, base, n, flips=4):
    """n filler rows: ~base with `flips` bits of [128, 256) inverted back.  Distance 256 - flips - k >= 200 from any
    near_rows(base, max_flips=k) query (k + flips <= 56)."""
    inv = np.bitwise_not(np.asarray(base, np.uint8).reshape(32))
    return np.stack([at_distance(rng, inv, flips, 128, 256) for _ in range(n)]) if n else np.zeros((0, 32), np.uint8)


def plant(rng, q, t, plants):
    """t[row] = q[qi] with exactly d bits inverted, for every (qi, row, d) in `plants` (in place; returns t)."""
    for qi, row, d in plants:
        t[row] = at_distance(rng, q[qi], d)
    return t


def planted_bf(rng, nq, nt, plants):
    """Independent random queries and filler rows, plus planted train rows: (q, t)."""
    q, t = random_rows(rng, nq), random_rows(rng, nt)
    return q, plant(rng, q, t, plants)


# ------------------------------------------------------------------------------------------------ plain references
def best2(drow):
    """The reference's sequential update idiom over one row of distances: (best, index, second), initial 256 / -1."""
    b1, b2, bi = 256, 256, -1
    for j, d in enumerate(drow):
        d = int(d)
        if d < b1:
            b2, b1, bi = b1, d, j
        elif d < b2:
            b2 = d
    return b1, bi, b2


def best2_np(D):
    """best2 for every row of a distance matrix, vectorised: the first minimum wins, second keeps multiplicity."""
    nq, nt = D.shape
    if nt == 0:
        return np.full(nq, 256, np.int32), np.full(nq, -1, np.int32), np.full(nq, 256, np.int32)
    idx = D.argmin(1).astype(np.int32)
    b1 = D[np.arange(nq), idx]
    rest = D.copy()
    rest[np.arange(nq), idx] = 256
    b2 = np.minimum(rest.min(1), 256).astype(np.int32)
    idx = np.where(b1 < 256, idx, -1).astype(np.int32)   # d < 256 is needed to take the first row
    return b1.astype(np.int32), idx, b2


def ratio_pass(best, second, nnratio):
    """`(float)best < nnratio * (float)second` in binary32 (no FMA), elementwise"""
    f = np.float32
    return np.asarray(best, f) < (f(nnratio) * np.asarray(second, f)).astype(f)


def rot_bin(a1, a2):
    """ORBmatcher.cc:308-313 in binary32: rot = a1 - a2 (+360 if < 0), bin = round(rot * (1.0f / 30)), 30 -> 0"""
    f = np.float32
    rot = f(f(a1) - f(a2))
    if rot < 0:
        rot = f(rot + f(360))
    x = f(rot * (f(1) / f(30)))
    b = int(np.floor(np.float64(x) + 0.5))   # roundf: half away from zero (x >= 0); exact in double
    return 0 if b == 30 else b


def three_maxima(counts):
    """ComputeThreeMaxima (ORBmatcher.cc:1912-1957) with its binary32 0.1f * max1 rules"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(counts):
        s = int(s)
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    f = np.float32
    lim = f(f(0.1) * f(max1))
    if f(max2) < lim:
        i2 = i3 = -1
    elif f(max3) < lim:
        i3 = -1
    return i1, i2, i3


def match_bf(q, t, qa, ta, nnratio, th, check_ori):
    """Plain numpy restatement of the all-pairs matcher (oracle.match_bf): (match, best, second, nmatches)."""
    b1, idx, b2 = best2_np(distances(q, t))
    ok = (idx >= 0) & (b1 <= th) & ratio_pass(b1, b2, nnratio)
    m = np.where(ok, idx, -1).astype(np.int32)
    if check_ori and qa is not None and ta is not None:
        prune_by_rotation(m, [(i, rot_bin(qa[i], ta[m[i]])) for i in np.flatnonzero(m >= 0)])
    return m, b1, b2, int((m >= 0).sum())


def prune_by_rotation(m, key_bins):
    """The rotation histogram (:308-316, :338-360): keys whose bin is not one of the three maxima lose their match."""
    counts = np.zeros(30, np.int64)
    for _, b in key_bins:
        counts[b] += 1
    keep = three_maxima(counts)
    for k, b in key_bins:
        if b not in keep:
            m[k] = -1
    return m


# ------------------------------------------------------------------------------------------------ angles / histograms
def rotation_for_bin(b, jitter=0.0):
    """a rotation (degrees) inside bin b = 0..12, |jitter| < 6 away from the middle of the part of the bin that [0, 360)
    holds (bin 0 is [0, 15), bin 12 is [345, 360))"""
    assert 0 <= b <= 12 and abs(jitter) < 6
    return (7.5 if b == 0 else 352.5 if b == 12 else 30.0 * b) + jitter


def angles_for_histogram(rng, counts, base=None):
    """(a1, a2) float32 arrays, sum(counts) pairs, whose rot_bin histogram over bins 0..12 equals `counts` (len <= 13);
    pairs are shuffled; a2 random in [0, 360) unless given, so that about half of the differences wrap through +360."""
    bins = np.repeat(np.arange(len(counts)), counts)
    rng.shuffle(bins)
    n = len(bins)
    a2 = rng.uniform(0, 360, n).astype(np.float32) if base is None else np.asarray(base, np.float32)
    rot = np.array([rotation_for_bin(int(b), rng.uniform(-5, 5)) for b in bins], np.float64)
    a1 = np.mod(a2.astype(np.float64) + rot, 360.0).astype(np.float32)
    return a1, a2, bins


# ------------------------------------------------------------------------------------------------ SearchByBoW
def csr(lists):
    """{node id: [feature indices]} -> (node, off, idx) uint32 with ascending node ids"""
    nodes = sorted(lists)
    off = np.zeros(len(nodes) + 1, np.uint32)
    idx = []
    for i, k in enumerate(nodes):
        idx.extend(int(v) for v in lists[k])
        off[i + 1] = len(idx)
    return np.asarray(nodes, np.uint32), off, np.asarray(idx, np.uint32)


def search_by_bow(descKF, validKF, angKF, fvKF, descF, validF, angF, fvF, nnratio, th_low, strict_lt, check_ori):
    """Plain restatement of SearchByBoW (src/ORBmatcher.cc:217-363 / :665-812, oracle.search_by_bow): node merge, greedy
    claim of F features, TH_LOW (strict for KF-KF), ratio, rotation histogram keyed by the F feature.  (match, n)."""
    nodeK, offK, idxK = fvKF
    nodeF, offF, idxF = fvF
    D = distances(descKF, descF)
    m = np.full(len(descF), -1, np.int32)
    keys = []
    posF = {int(v): i for i, v in enumerate(nodeF)}
    for a, node in enumerate(nodeK):
        b = posF.get(int(node))
        if b is None:
            continue
        for rk in idxK[offK[a]:offK[a + 1]]:
            if validKF is not None and not validKF[rk]:
                continue
            b1, b2, bi = 256, 256, -1
            for rf in idxF[offF[b]:offF[b + 1]]:
                if m[rf] >= 0 or (validF is not None and not validF[rf]):
                    continue
                d = int(D[rk, rf])
                if d < b1:
                    b2, b1, bi = b1, d, int(rf)
                elif d < b2:
                    b2 = d
            ok = b1 < th_low if strict_lt else b1 <= th_low
            if ok and bi >= 0 and ratio_pass(b1, b2, nnratio):
                m[bi] = rk
                keys.append(bi)
    if check_ori:
        prune_by_rotation(m, [(k, rot_bin(angKF[m[k]], angF[k])) for k in keys])
    return m, int((m >= 0).sum())


def bow_node(rng, node_id, nK, nF, plants, shuffle=True):
    """One vocabulary node with nK KeyFrame and nF Frame features, independent random rows except for the PLANTED pairs,
    applied in order: (k, f, d) rewrites F feature f to sit at distance d from KF feature k, ("K", k, f, d) rewrites KF
    feature k from F feature f.  k and f are positions in the node's lists (the order the matcher walks them); with
    `shuffle` the lists hold the node's local rows in a random order, so that an earlier position is not a lower index.
    Returns (node_id, dK, dF, kf_order, f_order) for bow_frame_pair."""
    dK, dF = random_rows(rng, nK), random_rows(rng, nF)
    ko = rng.permutation(nK) if shuffle else np.arange(nK)
    fo = rng.permutation(nF) if shuffle else np.arange(nF)
    for p in plants:
        if p[0] == "K":
            _, k, f, d = p
            dK[ko[k]] = at_distance(rng, dF[fo[f]], d)
        else:
            k, f, d = p
            dF[fo[f]] = at_distance(rng, dK[ko[k]], d)
    return node_id, dK, dF, ko, fo


def bow_frame_pair(nodes):
    """Pack several `bow_node` nodes into one (KeyFrame, Frame) pair.  nodes: list of (node id, dK, dF, kf_order, f_order)
    where the orders permute the node's local features (the list order the matcher walks).  Feature indices are assigned
    node after node; returns ((descKF, fvKF), (descF, fvF)) with ascending node ids."""
    dKs, dFs, lk, lf = [], [], {}, {}
    nk = nf = 0
    for node_id, dK, dF, ko, fo in sorted(nodes, key=lambda x: x[0]):
        lk[node_id] = [nk + int(i) for i in ko]
        lf[node_id] = [nf + int(i) for i in fo]
        dKs.append(dK)
        dFs.append(dF)
        nk += len(dK)
        nf += len(dF)
    descK = np.concatenate(dKs) if dKs else np.zeros((0, 32), np.uint8)
    descF = np.concatenate(dFs) if dFs else np.zeros((0, 32), np.uint8)
    return (descK, csr(lk)), (descF, csr(lf))
