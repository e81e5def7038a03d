"""Hand-made cases for the batched SearchBySim3 and the loop's SearchByProjection (tests/test_sim3_search_oracle.py,
tests/test_gpu_sim3_search.py): keyframes at the identity pose under the identity similarity, so a point's world coordinates are its
coordinates in both cameras and every scenario can be placed by pixel.  Seeded cases come from proj_cases.  Test support only."""
import numpy as np

import proj_cases as PC

F = np.float32
FX, FY, CX, CY, BF = 500.0, 500.0, 320.0, 240.0, 40.0
W, H = 640, 480
SF = PC.scale_factors()
LOG_SF = F(np.log(F(1.2)))
IDENT = (1.0, np.eye(3, dtype=F), np.zeros(3, F))


def flips(rng, d, k):
    """a copy of descriptor d with exactly k bits flipped"""
    bits = np.unpackbits(np.asarray(d, np.uint8))
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def point_at(u, v, z, level):
    """(world, max_dist, min_dist) of a point that projects to (u, v) at depth z and is predicted at `level`"""
    X = np.array([(u - CX) / FX * z, (v - CY) / FY * z, z], F)
    dist = float(np.linalg.norm(X.astype(np.float64)))
    maxd = F(dist * 1.2 ** (level - 0.5))
    return X, maxd, F(maxd / 1.2 ** 7)


class KfBuilder:
    """features (pixel, octave, descriptor) and the MapPoint each holds (state 0 none, 1 good, 2 bad), in index order"""

    def __init__(self):
        self.xy, self.octave, self.desc, self.state, self.world, self.maxd, self.mind, self.mpdesc = [], [], [], [], [], [], [], []

    def add(self, xy, octave, desc, point=None, mpdesc=None, state=None):
        """point = (u, v, z, level) in the OTHER keyframe's image (or the own one for the projection search); -> the feature's index"""
        self.xy.append(xy)
        self.octave.append(octave)
        self.desc.append(np.asarray(desc, np.uint8))
        if point is None:
            X, mx, mn = np.zeros(3, F), F(1), F(0.1)
        else:
            X, mx, mn = point_at(*point)
        self.state.append((1 if point is not None else 0) if state is None else state)
        self.world.append(X)
        self.maxd.append(mx)
        self.mind.append(mn)
        self.mpdesc.append(np.asarray(mpdesc if mpdesc is not None else np.zeros(32), np.uint8))
        return len(self.xy) - 1

    def build(self):
        n = len(self.xy)
        return dict(desc=np.array(self.desc, np.uint8).reshape(n, 32), xy=np.array(self.xy, F).reshape(n, 2), octave=np.array(self.octave, np.int32),
                    uRight=np.full(n, -1, F), K=(FX, FY, CX, CY, BF), bounds=(0.0, float(W), 0.0, float(H)),
                    gw_inv=F(PC.GRID_COLS) / F(W), gh_inv=F(PC.GRID_ROWS) / F(H), scale_factors=SF, inv_sigma2=(1.0 / (SF * SF)).astype(F),
                    log_scale=LOG_SF, state=np.array(self.state, np.uint8), world_pos=np.array(self.world, F).reshape(n, 3),
                    max_dist=np.array(self.maxd, F), min_dist=np.array(self.mind, F), mpdesc=np.array(self.mpdesc, np.uint8).reshape(n, 32),
                    Rcw=np.eye(3, dtype=F), tcw=np.zeros(3, F))


def pts_of(points, descs, bad=None):
    """the list dict of the projection search from [(u, v, z, level)] and descriptors; normals look at the camera"""
    n = len(points)
    X = np.zeros((n, 3), F)
    mx, mn = np.zeros(n, F), np.zeros(n, F)
    for i, p in enumerate(points):
        X[i], mx[i], mn[i] = point_at(*p)
    nr = (X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-9)).astype(F)   # PO / |PO| with Ow = 0
    return dict(bad=np.zeros(n, np.uint8) if bad is None else np.asarray(bad, np.uint8), world_pos=X, normal=nr, max_dist=mx, min_dist=mn,
                mpdesc=np.array(descs, np.uint8).reshape(n, 32))


def tie_pair(rng):
    """both directions: two features with one descriptor in one window, the higher index in the earlier grid column.  The winner
    is feature 1 on either side (cell order), not feature 0 (index order)."""
    D, E = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    a, b = KfBuilder(), KfBuilder()
    # keyframe 1: features 0 / 1 share E; feature 2 carries the point that lands between keyframe 2's pair
    a.add((415.0, 300.0), 2, E)
    a.add((400.0, 300.0), 2, E)
    a.add((100.0, 100.0), 0, rng.integers(0, 256, 32, dtype=np.uint8), point=(307.0, 200.0, 2.0, 2), mpdesc=flips(rng, D, 9))
    b.add((315.0, 200.0), 2, D)
    b.add((300.0, 200.0), 2, D)
    b.add((500.0, 400.0), 0, rng.integers(0, 256, 32, dtype=np.uint8), point=(407.0, 300.0, 2.0, 2), mpdesc=flips(rng, E, 9))
    return a.build(), b.build()


def threshold_pair(rng, th):
    """keyframe 1's points against isolated candidates of keyframe 2: distance exactly th / th + 1, and the octaves level - 2 ..
    level + 1 at distance 0 around a point of level 3.  -> (k1, k2, expected vnMatch1)"""
    a, b = KfBuilder(), KfBuilder()
    want = []
    spots = [(60.0 + 90.0 * i, 120.0) for i in range(6)]
    for i, (dist, octave, ok) in enumerate([(th, 3, True), (th + 1, 3, False), (0, 1, False), (0, 2, True), (0, 3, True), (0, 4, False)]):
        D = rng.integers(0, 256, 32, dtype=np.uint8)
        j = b.add(spots[i], octave, D)
        a.add((50.0 + 10 * i, 400.0), 0, rng.integers(0, 256, 32, dtype=np.uint8), point=(spots[i][0] + 1.0, spots[i][1] - 1.0, 3.0, 3),
              mpdesc=flips(rng, D, dist))
        want.append(j if ok else -1)
    return a.build(), b.build(), np.array(want, np.int32)


def agreement_pair(rng):
    """-> (k1, k2, matches_in, notes): the agreement rules of :1542-1555 and the three kinds of preset entry"""
    a, b = KfBuilder(), KfBuilder()
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)   # noqa: E731
    A = [(60.0 + 60.0 * i, 100.0) for i in range(9)]        # keyframe 1's features
    B = [(60.0 + 60.0 * i, 300.0) for i in range(6)]        # keyframe 2's features
    dA, dB = [rd() for _ in A], [rd() for _ in B]
    lv = 1

    def aim(spot, d):
        return dict(point=(spot[0] + 0.5, spot[1] + 0.5, 2.5, lv), mpdesc=flips(rng, d, 7))
    # 0: i1 = 0 -> j = 0, but j = 0 -> i1' = 1.  1: aims at nothing.
    a.add(A[0], lv, dA[0], **aim(B[0], dB[0]))
    a.add(A[1], lv, dA[1], point=(600.0, 450.0, 2.5, lv), mpdesc=rd())
    # 2, 3: both -> j = 1, which answers 3
    a.add(A[2], lv, dA[2], **aim(B[1], dB[1]))
    a.add(A[3], lv, dA[3], **aim(B[1], dB[1]))
    # 4: preset to j = 2.  5: -> j = 2, still a candidate, but j = 2 is already matched and asks nothing
    a.add(A[4], lv, dA[4], **aim(B[2], dB[2]))
    a.add(A[5], lv, dA[5], **aim(B[2], dB[2]))
    # 6 / 7 / 8: preset -2, an index >= N2, the index of an empty slot: each blocks only its own query
    a.add(A[6], lv, dA[6], **aim(B[3], dB[3]))
    a.add(A[7], lv, dA[7], **aim(B[4], dB[4]))
    a.add(A[8], lv, dA[8], **aim(B[5], dB[5]))
    b.add(B[0], lv, dB[0], **aim(A[1], dA[1]))
    b.add(B[1], lv, dB[1], **aim(A[3], dA[3]))
    b.add(B[2], lv, dB[2], **aim(A[5], dA[5]))
    b.add(B[3], lv, dB[3], **aim(A[6], dA[6]))
    b.add(B[4], lv, dB[4], **aim(A[7], dA[7]))
    b.add(B[5], lv, dB[5])                                   # an empty slot
    m = np.full(9, -1, np.int32)
    m[4], m[6], m[7], m[8] = 2, -2, 6 + 5, 5
    want_vn1 = np.array([0, -1, 1, 1, -1, 2, -1, -1, -1], np.int32)
    want_vn2 = np.array([1, 3, -1, 6, 7, -1], np.int32)
    want_out = m.copy()
    want_out[3] = 1
    return a.build(), b.build(), m, (want_vn1, want_vn2, want_out, 1)


def claims_case(rng, th_low=50):
    """-> (kf, Scw, pts, matched_in, want_matched, want_n) for the projection search: claims, occupied slots, spAlreadyFound, th_low
    and the octave window"""
    k = KfBuilder()
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)   # noqa: E731
    S = [(60.0 + 70.0 * i, 150.0) for i in range(8)] + [(60.0 + 70.0 * i, 330.0) for i in range(8)]
    lv = 2
    pts, descs = [], []

    def lp(spot, d, level=lv):
        pts.append((spot[0] + 0.5, spot[1] - 0.5, 3.0, level))
        descs.append(d)
        return len(pts) - 1
    # two (three) list points with one best feature: the earlier takes it, the next gets its second candidate, the third none
    D = rd()
    f0 = k.add(S[0], lv, D)
    f1 = k.add((S[0][0] + 3.0, S[0][1]), lv, flips(rng, D, th_low // 2))   # within th_low of every copy of D below
    p0, p1, p2 = lp(S[0], flips(rng, D, 2)), lp(S[0], flips(rng, D, 3)), lp(S[0], flips(rng, D, 4))
    # a slot occupied at entry by a point that is in no list: never a candidate
    D2 = rd()
    f2 = k.add(S[1], lv, D2)
    p3 = lp(S[1], D2)
    # a list point that stands in vpMatched at entry is skipped, although its feature is free
    D3 = rd()
    f3 = k.add(S[2], lv, rd())
    f4 = k.add(S[3], lv, D3)
    p4 = lp(S[3], D3)
    # th_low: exactly at it, one above
    D4, D5 = rd(), rd()
    f5, f6 = k.add(S[4], lv, D4), k.add(S[5], lv, D5)
    p5, p6 = lp(S[4], flips(rng, D4, th_low)), lp(S[5], flips(rng, D5, th_low + 1))
    # octaves level - 2 .. level + 1 around points of level 3
    want_oct = []
    for i, octave in enumerate((1, 2, 3, 4)):
        Dk = rd()
        f = k.add(S[8 + i], octave, Dk)
        want_oct.append((f, lp(S[8 + i], Dk, 3), octave in (2, 3)))
    kf = k.build()
    n = len(kf["octave"])
    matched = np.full(n, -1, np.int32)
    matched[f2], matched[f3] = -2, p4
    want = matched.copy()
    want[f0], want[f1], want[f5] = p0, p1, p5
    for f, p, ok in want_oct:
        if ok:
            want[f] = p
    Scw = np.eye(4, dtype=F)
    return kf, Scw, pts_of(pts, descs), matched, want, 3 + 2


def chain_case(rng, n1, n2, nnodes=40):
    """(k1, k2, (s12, R12, t12)) for a whole ComputeSim3 round: a share of the features are the two views of one physical point
    under a true similarity -- correlated descriptors, angles and octaves, most of them in one vocabulary node (SearchByBoW finds
    those, SearchBySim3 the rest) --, the others carry unrelated points.  Keyframe dicts as proj_cases.sim3_pair_case builds them,
    plus angle, fv = (node, off, idx) and valid (a good MapPoint)."""
    c1, c2 = PC.current_frame(rng, n1, stereo=False), PC.current_frame(rng, n2, stereo=False)
    fx, fy, cx, cy = 535.4, 539.2, 320.1, 247.6
    T1, T2 = PC._pose(rng, 5.0, rng.normal(0, 0.2, 3)).astype(np.float64), PC._pose(rng, 5.0, rng.normal(0, 0.2, 3)).astype(np.float64)
    s12, R12, t12 = float(rng.uniform(0.9, 1.1)), PC._rot(rng, 3.0), rng.normal(0, 0.05, 3)

    def unrelated(c, n, T):
        z = rng.uniform(0.5, 8.0, n)
        Xc = np.stack([(c["xy"][:, 0] - cx) / fx * z, (c["xy"][:, 1] - cy) / fy * z, z], 1)
        return ((Xc - T[:3, 3]) @ T[:3, :3]), np.linalg.norm(Xc, axis=1) * 1.2 ** c["octave"] * 0.96

    w1, mx1 = unrelated(c1, n1, T1)
    w2, mx2 = unrelated(c2, n2, T2)
    node1, node2 = rng.integers(0, nnodes, n1), rng.integers(0, nnodes, n2)
    st1, st2 = rng.choice([0, 1, 1, 2], n1).astype(np.uint8), rng.choice([0, 1, 1, 2], n2).astype(np.uint8)
    mp1, mp2 = rng.integers(0, 256, (n1, 32), dtype=np.uint8), rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    m = min(n1, n2) * 3 // 5
    for a, b in zip(rng.permutation(n1)[:m], rng.permutation(n2)[:m]):
        z = rng.uniform(1.0, 6.0)
        X2 = np.array([(c2["xy"][b, 0] - cx) / fx * z, (c2["xy"][b, 1] - cy) / fy * z, z]) + rng.normal(0, 0.002, 3)
        X1 = s12 * (R12 @ X2) + t12
        u, v = fx * X1[0] / X1[2] + cx, fy * X1[1] / X1[2] + cy
        if X1[2] <= 0.1 or not (1 <= u < 639 and 1 <= v < 479):
            continue
        c1["xy"][a] = (u + rng.normal(0, 0.5), v + rng.normal(0, 0.5))
        c1["octave"][a] = c2["octave"][b]
        c1["angle"][a] = (c2["angle"][b] + rng.normal(0, 2.0)) % 360
        c1["desc"][a] = PC.noisy_copy(rng, c2["desc"][b][None], 20)[0]
        w1[a], w2[b] = (X1 - T1[:3, 3]) @ T1[:3, :3], (X2 - T2[:3, 3]) @ T2[:3, :3]
        mx1[a], mx2[b] = np.linalg.norm(X2) * 1.2 ** c2["octave"][b] * 0.96, np.linalg.norm(X1) * 1.2 ** c1["octave"][a] * 0.96
        mp1[a], mp2[b] = PC.noisy_copy(rng, c2["desc"][b][None], 30)[0], PC.noisy_copy(rng, c1["desc"][a][None], 30)[0]
        st1[a] = st2[b] = 1
        if rng.random() < 0.7:
            node1[a] = node2[b]
    sf = c1["scale_factors"]

    def kf(c, n, T, w, mx, st, mp, node):
        return dict(desc=c["desc"], xy=c["xy"].astype(F), octave=c["octave"], angle=c["angle"].astype(F), uRight=np.full(n, -1, F),
                    K=(fx, fy, cx, cy, 40.0), bounds=c["bounds"], gw_inv=c["gw_inv"], gh_inv=c["gh_inv"], scale_factors=sf,
                    inv_sigma2=(1.0 / (sf * sf)).astype(F), level_sigma2=(sf * sf).astype(F), log_scale=LOG_SF, state=st,
                    world_pos=w.astype(F), max_dist=mx.astype(F), min_dist=(mx / 1.2 ** 7).astype(F), mpdesc=mp, Rcw=T[:3, :3].astype(F),
                    tcw=T[:3, 3].astype(F), fv=PC._fv_csr(node, np.ones(n, bool)), valid=(st == 1).astype(np.uint8))
    return kf(c1, n1, T1, w1, mx1, st1, mp1, node1), kf(c2, n2, T2, w2, mx2, st2, mp2, node2), (s12, R12.astype(F), t12.astype(F))
