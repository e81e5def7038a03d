"""Edge cases for the batched SearchBySim3 and the loop's SearchByProjection (tests/test_sim3_search_edge_cases.py checks the table
on the CPU, tests/test_gpu_sim3_search_edges.py runs it on the device), and the inputs the older tests use, by name, so that the
oracle's digests and the report of what the older tables miss speak of the same runs.  A case is a dict: kind "sim3" (k1, k2, sim,
th, m_in, th_high) or "proj" (kf, Scw, pts, m_in, th, th_low and, optionally, ids: the MapPoint behind each list entry).  Planted
cases use identity poses and, where a comparison must be met exactly, a camera with fx = fy = 1, cx = cy = 0 and points at z = 1,
so that u = x and v = y without rounding.  Test support only."""
import math

import numpy as np

import fuse_oracle as FO
import proj_cases as PC
import sim3_search_cases as SC
import sim3_search_oracle as SO

F = np.float32
SHAPES = ((0, 0), (0, 40), (1, 1), (300, 280))


def sim3_case(k1, k2, sim, m_in, th=7.5, th_high=100):
    return dict(kind="sim3", k1=k1, k2=k2, sim=sim, m_in=np.asarray(m_in, np.int32), th=th, th_high=th_high)


def proj_case(kf, Scw, pts, m_in, th=10, th_low=50, ids=None):
    return dict(kind="proj", kf=kf, Scw=Scw, pts=pts, m_in=np.asarray(m_in, np.int32), th=th, th_low=th_low, ids=ids)


def run(c, trace=None):
    """the oracle's outputs for a case: sim3 (matches_out, nfound, vnMatch1, vnMatch2), proj (matched_out, nmatches)"""
    kw = {} if trace is None else dict(trace=trace)
    if c["kind"] == "sim3":
        T12, T21 = SO.pair_pose(*c["sim"])
        return SO.search_by_sim3(c["k1"], c["k2"], T12, T21, c["th"], c["m_in"], c["th_high"], **kw)
    if c.get("ids") is not None:
        kw["ids"] = c["ids"]
    return SO.search_by_projection_kf_sim3(c["kf"], c["Scw"], c["pts"], c["m_in"], c["th"], c["th_low"], **kw)


def compared(out):
    """the bytes a GPU test compares"""
    return b"".join(np.asarray(v, np.int32).tobytes() for v in out)


def with_break(rule, fn):
    old = SO.SIM3S_BREAK
    SO.SIM3S_BREAK = frozenset([rule])
    try:
        return fn()
    finally:
        SO.SIM3S_BREAK = old


def _shape(seed):
    return SHAPES[seed % len(SHAPES)] if seed < 8 else SHAPES[3]


_old = {}


def old_inputs():
    """name -> case: every oracle run of tests/test_sim3_search_oracle.py and tests/test_gpu_sim3_search.py (the chain test's
    SearchBySim3 inputs come out of the solver and are not restated here)"""
    if _old:
        return _old
    rng = lambda s: np.random.default_rng(s)   # noqa: E731
    for seed in range(12):
        n1, n2 = _shape(seed)
        k1, k2, s, R, t, m = PC.sim3_pair_case(rng(9100 + seed), n1, n2)
        _old[f"sim3_oracle_{seed}"] = sim3_case(k1, k2, (s, R, t), m)
        kf, Scw, pts, m = PC.kf_sim3_case(rng(9300 + seed), n1, n2)
        _old[f"proj_oracle_{seed}"] = proj_case(kf, Scw, pts, m)
    for seed in range(6):
        k1, k2, s, R, t, m = PC.sim3_pair_case(rng(9100 + seed), 300, 280)
        _old[f"sim3_parity_{seed}"] = sim3_case(k1, k2, (s, R, t), m)
        kf, Scw, pts, m = PC.kf_sim3_case(rng(9300 + seed), 300, 400)
        _old[f"proj_parity_{seed}"] = proj_case(kf, Scw, pts, m)
    for shape in ((0, 40), (40, 0), (0, 0), (1, 1)):
        k1, k2, s, R, t, m = PC.sim3_pair_case(rng(9150), *shape)
        _old[f"sim3_empty_{shape[0]}_{shape[1]}"] = sim3_case(k1, k2, (s, R, t), m)
        if shape != (0, 0):
            kf, Scw, pts, m = PC.kf_sim3_case(rng(9350), *shape)
            _old[f"proj_empty_{shape[0]}_{shape[1]}"] = proj_case(kf, Scw, pts, m)
    r = rng(9200)
    A, B, s1, R1, t1, mAB = PC.sim3_pair_case(r, 130, 150)
    _, C, s2, R2, t2, _ = PC.sim3_pair_case(r, 130, 97)
    _, _, s3, R3, t3, _ = PC.sim3_pair_case(r, 3, 3)
    mBA = np.full(150, -1, np.int32)
    mBA[[3, 50, 149]] = [7, -2, 129]
    mAC = np.full(130, -1, np.int32)
    mAC[[0, 64]] = [96, 5]
    _old["sim3_batch_0"] = sim3_case(A, B, (s1, R1, t1), mAB)
    _old["sim3_batch_1"] = sim3_case(B, A, (s2, R2, t2), mBA)
    _old["sim3_batch_2"] = sim3_case(A, C, (s2, R2, t2), mAC)
    _old["sim3_batch_3"] = sim3_case(A, B, (s3, R3, t3), mAB)
    r = rng(9400)
    cs = [PC.kf_sim3_case(r, 120, 150), PC.kf_sim3_case(r, 97, 60), PC.kf_sim3_case(r, 128, 200)]
    cs.append((cs[0][0], cs[2][1], cs[0][2], cs[0][3]))
    for i, c in enumerate(cs):
        _old[f"proj_batch_{i}"] = proj_case(*c)
    k1, k2 = SC.tie_pair(rng(77))
    _old["tie_pair"] = sim3_case(k1, k2, SC.IDENT, np.full(3, -1, np.int32))
    for th_high in (100, 37):
        k1, k2, _ = SC.threshold_pair(rng(78), th_high)
        _old[f"threshold_pair_{th_high}"] = sim3_case(k1, k2, SC.IDENT, np.full(6, -1, np.int32), th_high=th_high)
    k1, k2, m, _ = SC.agreement_pair(rng(79))
    _old["agreement_pair"] = sim3_case(k1, k2, SC.IDENT, m)
    m2 = m.copy()
    m2[7] = -2
    _old["agreement_pair_ref"] = sim3_case(k1, k2, SC.IDENT, m2)
    for th_low in (50, 23):
        kf, Scw, pts, m, _, _ = SC.claims_case(rng(80), th_low)
        _old[f"claims_case_{th_low}"] = proj_case(kf, Scw, pts, m, th_low=th_low)
    return _old


# ---------------------------------------------------------------------------------------------------------------- the planted table
K1 = (1.0, 1.0, 0.0, 0.0, 40.0)   # u = x / z, v = y / z: exact for z = 1
up = lambda x: np.nextafter(F(x), F(np.inf))      # noqa: E731
down = lambda x: np.nextafter(F(x), F(-np.inf))   # noqa: E731
TINY = F(-1e-30)                                  # a normal float just below 0 (no denormal, so no flush can move it)


class Pair:
    """two keyframes at the identity pose under the identity similarity; query(): a point of keyframe 1 given in camera
    coordinates with its distance range, and the feature of keyframe 2 it should find if nothing gates it out"""

    def __init__(self, rng, K):
        self.rng, self.K, self.a, self.b = rng, K, SC.KfBuilder(), SC.KfBuilder()

    def rd(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def point(self, kb, P, mn, mx, mpdesc, state=1):
        i = kb.add((5.0 + 3.0 * len(kb.xy) % 600, 470.0), 0, self.rd())
        kb.state[i], kb.world[i], kb.mind[i], kb.maxd[i], kb.mpdesc[i] = state, np.asarray(P, F), F(mn), F(mx), np.asarray(mpdesc, np.uint8)
        return i

    def query(self, P, mn, mx, off=(0.25, 0.25), octave=None, nflip=0):
        """-> (index in keyframe 1, index of its target in keyframe 2)"""
        P = np.asarray(P, F)
        fx, fy, cx, cy = self.K[:4]
        z = float(P[2]) if P[2] != 0 else 1.0
        u, v = fx * float(P[0]) / z + cx, fy * float(P[1]) / z + cy
        dist = F(math.sqrt(float(P[0]) ** 2 + float(P[1]) ** 2 + float(P[2]) ** 2))
        lv = FO.predict_scale(mx, dist, SC.LOG_SF, len(SC.SF)) if dist > 0 else 0
        D = self.rd()
        j = self.b.add((min(max(u, 0.0), 639.0) + off[0], min(max(v, 0.0), 479.0) + off[1]), lv if octave is None else octave, D)
        return self.point(self.a, P, mn, mx, SC.flips(self.rng, D, nflip)), j

    def build(self, m_in=None, th=7.5, th_high=100):
        k1, k2 = self.a.build(), self.b.build()
        for k in (k1, k2):
            k["K"] = self.K
        m = np.full(len(k1["octave"]), -1, np.int32) if m_in is None else m_in
        return sim3_case(k1, k2, SC.IDENT, m, th, th_high)


def rng_range(dist, level):
    """(min_dist, max_dist) that predict `level` at distance dist"""
    mx = F(dist * 1.2 ** (level - 0.5))
    return F(mx / 1.2 ** 7), mx


def gate_exact():
    """every comparison of the gate met exactly and from either side; -> (case, vnMatch1 expected: 1 = finds its target)"""
    p = Pair(np.random.default_rng(9601), K1)
    want = []

    def q(P, mn, mx, ok, **kw):
        i, j = p.query(P, mn, mx, **kw)
        want.append(j if ok else -1)
    for (u, v), ok in ((((0, 100), True), ((TINY, 100), False), ((640, 100), False), ((down(640), 100), True), ((100, 0), True), ((100, TINY), False),
                        ((100, 480), False), ((100, down(480)), True))):
        d = math.sqrt(float(u) ** 2 + float(v) ** 2 + 1)
        # PosInGrid rounds: a feature right of x = 635 or below y = 475 is in no cell, so the targets of the far edges stand 6 px inside
        q((u, v, 1), *rng_range(d, 2), ok, off=(-6.0 if u > 600 else 0.25, -6.0 if v > 400 else 0.25))
    q((3, 3, 0), 0.1, 100.0, False)           # z == 0: u is not a number
    q((3, 3, -1), *rng_range(math.sqrt(19), 2), False)
    mn = F(1.7)
    lo = F(F(0.8) * mn)
    for z, ok in ((lo, True), (down(lo), False), (F(0.9) * mn, True), (mn, True)):   # the level clamps at nlevels - 1
        q((0, 0, z), mn, 1000.0, ok)
    mx = F(9.3)
    hi = F(F(1.2) * mx)
    for z, ok in ((hi, True), (up(hi), False), (F(1.1) * mx, True), (mx, True)):     # the level clamps at 0 (n = -1) or is 0
        q((0, 0, z), 0.1, mx, ok)
    mx = F(25.83517)                                     # one of the values for which log(mx / (1.2f * mx)) / log(1.2f) rounds to -1: n = -1
    q((0, 0, F(F(1.2) * mx)), 0.1, mx, True)
    q((0, 0, 2.0), 0.1, F(2.0 * 1.2 ** 7.5), True)      # n = 8: clamped; unclamped the window would be [7, 8]
    q((0, 0, 2.0), 0.1, F(2.0 * 1.2 ** 9.5), True)      # n = 10: unclamped the window [9, 10] holds no octave
    q((0, 0, 2.0), 0.1, F(2.0 * 1.2 ** 6.5), True)      # n = 7 exactly at the clamp
    q((300, 200, 1), *rng_range(math.sqrt(300 ** 2 + 200 ** 2 + 1), 4), True, off=(10.0, 0.0))   # inside th * sf[4], outside th
    q((300, 300, 1), *rng_range(math.sqrt(300 ** 2 + 300 ** 2 + 1), 4), False, off=(16.0, 0.0))  # outside th * sf[4] = 15.55
    return p.build(), np.array(want, np.int32)


def search_exact(th_high=100):
    """the candidate loop: the octaves level - 2 .. level + 1 around points of level 3, th_high met exactly and from above and
    below, a tie of two features in one window (the first in cell order wins: the higher index)"""
    p = Pair(np.random.default_rng(9602), (SC.FX, SC.FY, SC.CX, SC.CY, SC.BF))
    want = []
    for i, (octave, nflip, ok) in enumerate(((1, 0, False), (2, 0, True), (3, 0, True), (4, 0, False), (3, th_high, True), (3, th_high + 1, False),
                                             (3, max(th_high - 1, 0), True))):
        u, v, z = 60.0 + 80.0 * i, 120.0, 3.0
        X, mx, mn = SC.point_at(u, v, z, 3)
        _, j = p.query(X, mn, mx, octave=octave, nflip=nflip)
        want.append(j if ok else -1)
    X, mx, mn = SC.point_at(307.0, 300.0, 2.0, 2)
    D = p.rd()
    p.b.add((315.0, 300.0), 2, D)
    tie = p.b.add((300.0, 300.0), 2, D)     # the earlier grid column
    p.point(p.a, X, mn, mx, D)
    want.append(tie)
    return p.build(th_high=th_high), np.array(want, np.int32)


def bookkeeping():
    """SearchBySim3's presets and agreement: SC.agreement_pair's scenario plus a preset >= N2 whose wrong reading (clipped to
    N2 - 1) would silence a live query of keyframe 2, and a preset that names the last feature of keyframe 2"""
    p = Pair(np.random.default_rng(9603), (SC.FX, SC.FY, SC.CX, SC.CY, SC.BF))
    A = [(60.0 + 60.0 * i, 100.0) for i in range(6)]
    B = [(60.0 + 60.0 * i, 300.0) for i in range(6)]
    dA, dB = [p.rd() for _ in A], [p.rd() for _ in B]

    def aim(spot, d):
        X, mx, mn = SC.point_at(spot[0] + 0.5, spot[1] + 0.5, 2.5, 1)
        return dict(P=X, mn=mn, mx=mx, mpdesc=SC.flips(p.rng, d, 7))

    def feat(kb, spot, d, tgt=None, state=1):
        i = kb.add(spot, 1, d)
        if tgt is not None:
            t = aim(*tgt)
            kb.state[i], kb.world[i], kb.mind[i], kb.maxd[i], kb.mpdesc[i] = state, t["P"], t["mn"], t["mx"], t["mpdesc"]
        return i
    # keyframe 1: 0 <-> 0 mutual; 1 preset to feature 1 of keyframe 2, which therefore asks nothing; 2 -> 1, unanswered; 3 preset -2
    # (its partner 3 still asks and finds it); 4 preset 9 >= N2 (its partner 4 still asks); 5 <-> 5 mutual, 5 being N2 - 1: a preset
    # >= N2 read as N2 - 1 would silence it
    for i, t in enumerate((0, 1, 1, 3, 4, 5)):
        feat(p.a, A[i], dA[i], (B[t], dB[t]))
    for j, t in enumerate((0, 2, None, 3, 4, 5)):
        feat(p.b, B[j], dB[j], None if t is None else (A[t], dA[t]))
    p.b.state[2] = 2
    feat(p.a, (500.0, 100.0), p.rd(), (B[0], dB[0]), state=2)     # a bad point of keyframe 1
    m = np.array([-1, 1, -1, -2, 9, -1, -1], np.int32)
    return p.build(m)


def fused_pose():
    """real poses and points that project within rounding of u = minx: at least one is in the image under T_to * (T_own * P) and
    out under (T_to * T_own) * P or the other way round, so the two-stage product is not a matter of taste"""
    rng = np.random.default_rng(9604)
    K = (SC.FX, SC.FY, SC.CX, SC.CY, SC.BF)
    T_own = np.concatenate([PC._rot(rng, 20.0), rng.normal(0, 0.3, (3, 1))], 1)
    s12, R12, t12 = 1.3, PC._rot(rng, 10.0).astype(F), rng.normal(0, 0.2, 3).astype(F)
    T12, T21 = SO.pair_pose(s12, R12, t12)
    A = T21.astype(np.float64)[:, :3] @ T_own[:, :3]
    b = T21.astype(np.float64)[:, :3] @ T_own[:, 3] + T21.astype(np.float64)[:, 3]
    p = Pair(rng, K)
    differ = 0
    T_own32 = T_own.astype(F)
    for _ in range(400):
        u, v, z = rng.uniform(-4e-5, 4e-5), rng.uniform(50, 400), rng.uniform(1, 5)
        Xo = np.array([(u - SC.CX) / SC.FX * z, (v - SC.CY) / SC.FY * z, z])
        W = np.linalg.solve(A, Xo - b).astype(F)
        mn, mx = rng_range(float(np.linalg.norm(Xo)), 2)
        g0 = SO.gate_point(T_own32, T21, K, (0.0, 640.0, 0.0, 480.0), 7.5, SC.SF, SC.LOG_SF, W, mn, mx)
        g1 = with_break("fused_pose", lambda: SO.gate_point(T_own32, T21, K, (0.0, 640.0, 0.0, 480.0), 7.5, SC.SF, SC.LOG_SF, W, mn, mx))
        if (g0 is None) != (g1 is None) and differ < 6 or len(p.a.xy) < 6:
            differ += (g0 is None) != (g1 is None)
            D = p.rd()
            p.b.add((0.3, v + 0.2), 2, D)
            p.point(p.a, W, mn, mx, D)
    c = p.build()
    c["k1"]["Rcw"], c["k1"]["tcw"] = T_own32[:, :3].copy(), T_own32[:, 3].copy()
    c["sim"] = (s12, R12, t12)
    return c, differ


def proj_exact(th_low=50):
    """the projection form: SC.claims_case's scenario (claims, a slot occupied by -2, a list point that stands in the row at
    entry, th_low, the octave window) plus bad points with a free feature in reach, the viewing-angle gate met exactly and from
    either side, th_low from below"""
    rng = np.random.default_rng(9605)
    kf, Scw, pts, m_in, _, _ = SC.claims_case(rng, th_low)
    k = SC.KfBuilder()
    for i in range(len(kf["octave"])):
        k.add(tuple(kf["xy"][i]), int(kf["octave"][i]), kf["desc"][i])
    P = {key: list(np.asarray(pts[key])) for key in ("bad", "world_pos", "normal", "max_dist", "min_dist", "mpdesc")}

    def lp(u, v, z, level, d, normal=None, bad=0):
        X, mx, mn = SC.point_at(u, v, z, level)
        nr = X / np.linalg.norm(X) if normal is None else normal
        for key, val in zip(("bad", "world_pos", "normal", "max_dist", "min_dist", "mpdesc"), (bad, X, np.asarray(nr, F), mx, mn, d)):
            P[key].append(val)
    rd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)   # noqa: E731
    D = rd()
    k.add((600.5, 60.5), 2, D)
    lp(600.0, 60.0, 3.0, 2, D, bad=1)                          # bad: its free feature stays free
    D = rd()
    k.add((600.5, 420.5), 2, D)
    lp(600.0, 420.0, 3.0, 2, SC.flips(rng, D, max(th_low - 1, 0)))
    # on the optical axis PO = (0, 0, z) and dist = z exactly: dot = z * n_z against 0.5 * z
    for nz in (0.5, 0.4, 0.6):
        D = rd()
        k.add((SC.CX + 0.5, SC.CY + 0.5), 2, D)
        lp(SC.CX, SC.CY, 3.0, 2, D, normal=(0.0, 0.0, nz))
    kf2 = k.build()
    n = len(kf2["octave"])
    m = np.full(n, -1, np.int32)
    m[:len(m_in)] = m_in
    pts2 = dict(bad=np.array(P["bad"], np.uint8), world_pos=np.array(P["world_pos"], F), normal=np.array(P["normal"], F),
                max_dist=np.array(P["max_dist"], F), min_dist=np.array(P["min_dist"], F), mpdesc=np.array(P["mpdesc"], np.uint8))
    return proj_case(kf2, Scw, pts2, m, th_low=th_low)


def cascade(nlist=9, nfeat=8):
    """a claim cascade: nlist list points with one descriptor at one spot, nfeat features in the window at increasing distance:
    entry k ends on its k-th choice, the ninth gets none.  -> (case, expected row)"""
    rng = np.random.default_rng(9606)
    k = SC.KfBuilder()
    D = rng.integers(0, 256, 32, dtype=np.uint8)
    order = rng.permutation(nfeat)   # feature index order is not distance order
    f = {}
    for i in range(nfeat):
        rank = int(order[i])
        f[rank] = k.add((300.0 + 1.5 * i, 200.0 + (i % 3)), 2, SC.flips(rng, D, 3 * rank))
    pts = SC.pts_of([(302.0, 201.0, 3.0, 2)] * nlist, [D] * nlist)
    want = np.full(nfeat, -1, np.int32)
    for rank in range(min(nlist, nfeat)):
        want[f[rank]] = rank
    return proj_case(k.build(), np.eye(4, dtype=F), pts, np.full(nfeat, -1, np.int32)), want


def dup_point():
    """one MapPoint twice in a list: spAlreadyFound is taken at entry, so the second entry searches again and, its first choice
    claimed, takes its second"""
    rng = np.random.default_rng(9607)
    k = SC.KfBuilder()
    D, E = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
    k.add((300.0, 200.0), 2, D)
    k.add((303.0, 200.0), 2, SC.flips(rng, D, 20))
    k.add((100.0, 100.0), 2, E)
    pts = SC.pts_of([(301.0, 200.5, 3.0, 2), (100.5, 100.5, 3.0, 2), (301.0, 200.5, 3.0, 2)], [D, E, D])
    return proj_case(k.build(), np.eye(4, dtype=F), pts, np.full(3, -1, np.int32), ids=np.array([0, 1, 0]))


_table = {}


def table():
    """name -> case; the planted cases and two small seeded ones for the breadth no planting gives"""
    if _table:
        return _table
    _table["gate_exact"] = gate_exact()[0]
    _table["search_exact"] = search_exact()[0]
    _table["search_exact_th0"] = search_exact(0)[0]
    _table["search_exact_th255"] = search_exact(255)[0]
    _table["bookkeeping"] = bookkeeping()
    _table["fused_pose"] = fused_pose()[0]
    _table["proj_exact"] = proj_exact()
    _table["proj_exact_th0"] = proj_exact(0)
    _table["proj_exact_th255"] = proj_exact(255)
    _table["cascade"] = cascade()[0]
    _table["dup_point"] = dup_point()
    k1, k2, s, R, t, m = PC.sim3_pair_case(np.random.default_rng(9501), 70, 60)
    _table["seeded_sim3"] = sim3_case(k1, k2, (s, R, t), m)
    kf, Scw, pts, m = PC.kf_sim3_case(np.random.default_rng(9502), 70, 90)
    _table["seeded_proj"] = proj_case(kf, Scw, pts, m)
    return _table


# what the census asks of the trace of the whole table: comparison -> the outcomes that must all occur
CENSUS = {
    "z": {-1, 0, 1}, "u_min": {-1, 0, 1}, "u_max": {-1, 0, 1}, "v_min": {-1, 0, 1}, "v_max": {-1, 0, 1},
    "d08": {-1, 0, 1}, "d08_band": {True, False}, "d12": {-1, 0, 1}, "d12_band": {True, False}, "clamp0": {-1, 0, 1}, "clampN": {-1, 0, 1},
    "oct_lo": {-1, 0, 1}, "oct_hi": {-1, 0, 1}, "first_min": {-1, 0, 1}, "th_high": {-1, 0, 1},
    "preset": {"null", "other", "in", "past"}, "slot1": {"empty", "bad", "already", "live"}, "slot2": {"empty", "bad", "already", "live"},
    "agree": {True, False},
    "entry": {"bad", "found", "live"}, "slot_blocked": {True, False}, "slot_claimed": {True, False}, "th_low": {-1, 0, 1}, "angle": {-1, 0, 1},
}
