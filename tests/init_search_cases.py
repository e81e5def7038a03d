"""Planted cases for ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651) on the device (csrc/orbfe_init_search.hip):
take-overs and skips on one feature, ties, dependency chains, the ratio / threshold edges, votes of lost matches, contended
random frames and the batch edges.  Descriptors are a base row with chosen bits flipped, so every Hamming distance is exact:
d(flip(r, S), flip(r, T)) = |S xor T|.  The random cases of tests/proj_cases.py (initialization_case) never take a match over
(several second-frame features copy one first-frame feature there, not the other way round), so contention is planted here.
Test support only.

A case is dict(f1, f2, prev, window, check_ori); frames are the dicts of proj_cases.current_frame, on a 1000 x 480 image
for the planted ones (a chain of 70 needs the width)."""
import functools

import numpy as np

import proj_cases as PC

F = np.float32
W, H = 1000, 480
WINDOW = 15


def geometry(w=W, h=H):
    return dict(bounds=(0.0, float(w), 0.0, float(h)), gw_inv=F(PC.GRID_COLS) / F(w), gh_inv=F(PC.GRID_ROWS) / F(h))


def flip(row, bits):
    """row (uint8 [32]) with the given bit positions flipped"""
    b = np.unpackbits(np.asarray(row, np.uint8))
    b[np.asarray(list(bits), np.int64)] ^= 1
    return np.packbits(b)


class Builder:
    """collects the features of both frames of a planted pair"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.a, self.b = [], []   # (x, y, desc, angle, octave)

    def row(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def bits(self, k, avoid=()):
        free = np.setdiff1d(np.arange(256), np.asarray(list(avoid), np.int64))
        return [int(v) for v in self.rng.choice(free, k, replace=False)]

    def f1(self, x, y, desc, angle=0.0, octave=0):
        self.a.append((x, y, desc, angle, octave))
        return len(self.a) - 1

    def f2(self, x, y, desc, angle=0.0, octave=0):
        self.b.append((x, y, desc, angle, octave))
        return len(self.b) - 1

    def case(self, window=WINDOW, check_ori=False):
        return dict(f1=_frame(self.a), f2=_frame(self.b), prev=_frame(self.a)["xy"].copy(), window=window, check_ori=check_ori)


def _frame(items, w=W, h=H):
    n = len(items)
    f = dict(xy=np.array([[it[0], it[1]] for it in items], F).reshape(n, 2), desc=np.array([it[2] for it in items], np.uint8).reshape(n, 32),
             angle=np.array([it[3] for it in items], F), octave=np.array([it[4] for it in items], np.int32), uRight=np.full(n, -1, F),
             state=np.zeros(n, np.uint8), Tcw=np.eye(4, dtype=F), K=(535.4, 539.2, 320.1, 247.6, 40.0, 40.0 / 535.4),
             scale_factors=PC.scale_factors())
    f.update(geometry(w, h))
    return f


# ---- three queries on one feature ------------------------------------------------------------------------------------------------
def takeover_20_15_10():
    """queries at 20, 15, 10 from feature A: each takes it over.  Query 1 also sees C at 30: it is accepted on A (15 < 27) and
    loses it, so its entry ends -1; a table of the smallest claimed distance (10, by the LATER query 2) makes it skip A and stand
    on C"""
    B = Builder(1)
    r = B.row()
    A = B.f2(100, 100, r)
    s1 = B.bits(15)
    q1row = flip(r, s1)
    C = B.f2(88, 100, flip(q1row, B.bits(30, avoid=s1)))
    B.f1(106, 100, flip(r, B.bits(20)))      # sees A only (C is 18 px away)
    B.f1(100, 100, q1row)                    # sees A and C
    B.f1(108, 100, flip(r, B.bits(10)))      # sees A only
    c = B.case()
    c["expect"] = dict(matches12=[-1, -1, A], nmatches=1, takeovers=2)
    return c


def skip_20_12_15():
    """queries at 20, 12, 15 from A: the second takes it over, the third is skipped on A (12 <= 15) and falls to B at 16, alone
    and so accepted; unskipped it would have been rejected (15 < 16 * 0.9 is false).  A table of the lowest claiming query
    (query 0 at 20) lets it take A"""
    B = Builder(2)
    r = B.row()
    A = B.f2(100, 100, r)
    s2 = B.bits(15)
    q2row = flip(r, s2)
    Bf = B.f2(120, 100, flip(q2row, B.bits(16, avoid=s2)))
    B.f1(94, 100, flip(r, B.bits(20)))       # sees A only
    B.f1(96, 100, flip(r, B.bits(12)))       # sees A only
    B.f1(110, 100, q2row)                    # sees A (15) and B (16)
    c = B.case()
    c["expect"] = dict(matches12=[-1, A, Bf], nmatches=2, takeovers=1)
    return c


def tie_is_skipped():
    """a later query at d == held (15, 15) is skipped (:566 is <=) and has nothing else"""
    B = Builder(3)
    r = B.row()
    A = B.f2(100, 100, r)
    B.f1(98, 100, flip(r, B.bits(15)))
    B.f1(102, 100, flip(r, B.bits(15)))
    c = B.case()
    c["expect"] = dict(matches12=[A, -1], nmatches=1, takeovers=0)
    return c


# ---- a dependency chain ------------------------------------------------------------------------------------------------------------
def chain(L, with_query0=True):
    """features A_1 .. A_L, 10 px apart; query m sits between A_m and A_m+1 at distances 11 and 10: rejected by the ratio
    (10 < 9.9 is false) unless A_m is held at 10 by query m - 1.  Query 0 sees A_1 only.  With query 0 every query is accepted,
    one round after its predecessor; without it none is"""
    B = Builder(100 + L)
    rows = [B.row()]
    flips = []
    for m in range(L):
        s = B.bits(21)
        flips.append(s)
        rows.append(flip(rows[-1], s))
    for m in range(1, L + 1):               # A_m = rows[m] at x = 20 + 10 m
        B.f2(20 + 10 * m, 100, rows[m])
    for m in range(L):                      # query m = rows[m + 1] with 10 of its 21 bits flipped back
        if m == 0 and not with_query0:
            B.f1(25, 100, B.row(), octave=1)   # keeps the indices; not level 0, no query
            continue
        B.f1(25 + 10 * m, 100, flip(rows[m + 1], flips[m][:10]))
    c = B.case()
    c["expect"] = dict(matches12=list(range(L)) if with_query0 else [-1] * L, nmatches=L if with_query0 else 0, takeovers=0,
                       min_rounds=L + 1 if with_query0 else 1)
    return c


# ---- ratio and threshold edges: independent queries 60 px apart ----------------------------------------------------------
def decision_edges():
    B = Builder(4)
    want = []

    def spot(k, dists):
        x, r = 40 + 60 * k, B.row()
        used, first = [], None
        for j, d in enumerate(dists):
            s = B.bits(d, avoid=used) if d + len(used) <= 256 else B.bits(d)
            used += s
            f = B.f2(x + 2 * j, 200, flip(r, s))
            first = f if first is None else first
        B.f1(x, 200, r)
        return first

    for k, (dists, ok) in enumerate([((50,), True), ((51,), False), ((30,), True), ((45, 50), False), ((44, 50), True), ((9, 10), False),
                                     ((8, 10), True), ((50, 56), True), ((50, 55), False), ((0, 1), True)]):
        f = spot(k, dists)
        want.append(f if ok else -1)
    c = B.case()
    c["expect"] = dict(matches12=want, nmatches=sum(1 for w in want if w >= 0), takeovers=0)
    return c


# ---- votes of lost matches -------------------------------------------------------------------------------------------------------
def _votes(seed, standing, takeovers):
    """standing: bins of isolated matches; takeovers: (bin of the query that loses, bin of the one that takes).  Angles: frame
    2 at 0, frame 1 at 30 * bin, so rot * (1 / 30) rounds to bin."""
    B = Builder(seed)
    k = 0
    spots = []
    for b in standing:
        x, y, r = 30 + 40 * (k % 24), 60 + 60 * (k // 24), B.row()
        k += 1
        f = B.f2(x, y, r)
        spots.append(("s", B.f1(x + 1, y, flip(r, B.bits(5)), angle=30.0 * b), f, b))
    for lost, taker in takeovers:
        x, y, r = 30 + 40 * (k % 24), 60 + 60 * (k // 24), B.row()
        k += 1
        f = B.f2(x, y, r)
        i = B.f1(x + 1, y, flip(r, B.bits(20)), angle=30.0 * lost)
        j = B.f1(x + 2, y, flip(r, B.bits(10)), angle=30.0 * taker)
        spots.append(("t", (i, j), f, (lost, taker)))
    return B, spots


def _votes_expect(B, spots, kept):
    m = [-1] * len(B.a)
    for kind, q, f, b in spots:
        if kind == "s" and b in kept:
            m[q] = f
        if kind == "t" and b[1] in kept:
            m[q[1]] = f
    return dict(matches12=m, nmatches=sum(1 for v in m if v >= 0), takeovers=sum(1 for s in spots if s[0] == "t"))


def lost_votes_change_the_bins():
    """votes: bin 0 = 3 (1 + 2 takers), bin 1 = 2, bin 2 = 1 standing + 2 LOST = 3, bin 3 = 2.  With the lost votes the three
    maxima are bins 0, 2, 1 and bin 3's two matches go; counting only standing matches would keep 0, 1, 3 and drop bin 2"""
    B, spots = _votes(5, [0, 1, 1, 2, 3, 3], [(2, 0), (2, 0)])
    c = B.case(check_ori=True)
    c["expect"] = _votes_expect(B, spots, kept={0, 1, 2})
    return c


def dropped_bin_of_lost_votes_only():
    """bins 0, 1, 2 hold 5, 3, 2 votes; bin 5 holds ONE vote, of a match that was taken over (by a bin-0 query): it is dropped
    and nmatches must not move; bin 6 holds one vote, of a TAKER: it is dropped, the feature it took ends unmatched"""
    B, spots = _votes(6, [0, 0, 0, 1, 1, 1, 2, 2], [(5, 0), (0, 6)])
    c = B.case(check_ori=True)
    c["expect"] = _votes_expect(B, spots, kept={0, 1, 2})
    return c


PLANTED = dict(takeover_20_15_10=takeover_20_15_10, skip_20_12_15=skip_20_12_15, tie_is_skipped=tie_is_skipped,
               chain_40=functools.partial(chain, 40), chain_70=functools.partial(chain, 70),
               chain_40_without_query0=functools.partial(chain, 40, False), chain_70_without_query0=functools.partial(chain, 70, False),
               decision_edges=decision_edges, lost_votes_change_the_bins=lost_votes_change_the_bins,
               dropped_bin_of_lost_votes_only=dropped_bin_of_lost_votes_only)
CHAINS = {"chain_40": 40, "chain_70": 70}


# ---- contended random frames -------------------------------------------------------------------------------------------------------
def contended(rng, n1, n2, k, window=100, check_ori=True):
    """frame-1 features are noisy copies (<= 45 flipped bits, +-8 px) of k hot level-0 features of frame 2: many queries want the
    same feature, so matches are taken over and the skip of :566 changes decisions"""
    f2 = PC.current_frame(rng, n2, stereo=False, dense_states=False)
    f2["octave"] = rng.choice([0, 0, 0, 1, 3], n2).astype(np.int32)
    hot = rng.choice(n2, k, replace=False)
    f2["octave"][hot] = 0
    f1 = PC.current_frame(rng, n1, stereo=False, dense_states=False)
    f1["octave"] = rng.choice([0, 0, 0, 0, 1, 2], n1).astype(np.int32)
    src = hot[rng.integers(0, k, n1)]
    f1["xy"] = np.clip(f2["xy"][src] + rng.uniform(-8, 8, (n1, 2)), [0, 0], [639.9, 479.9]).astype(F)
    f1["desc"] = PC.noisy_copy(rng, f2["desc"][src], 45)
    f1["angle"] = ((f2["angle"][src] + rng.choice([0, 0, 0, 40, 150], n1) + rng.normal(0, 3, n1)) % 360).astype(F)
    return dict(f1=f1, f2=f2, prev=f1["xy"].copy(), window=window, check_ori=check_ori)


CONTENDED = [(64, 64, 4, 100), (300, 300, 20, 100), (600, 300, 40, 30), (1200, 1000, 60, 100)]


def contended_case(i):
    n1, n2, k, win = CONTENDED[i]
    return contended(np.random.default_rng(52_000 + i), n1, n2, k, win)


# ---- the random cases of the existing tests --------------------------------------------------------------------------------------
def random_case(seed):
    """seed 0..59: sizes 1 / 50 / 500 / 2000, windows 30 / 100, orientation check on / off"""
    rng = np.random.default_rng(29_000 + seed)
    n1, n2 = int(rng.choice([1, 50, 500, 2000])), int(rng.choice([1, 60, 600, 2000]))
    f1, f2, prev = PC.initialization_case(rng, n1, n2)
    return dict(f1=f1, f2=f2, prev=prev, window=int(rng.choice([30, 100])), check_ori=bool(seed % 5))


# ---- batch edges -------------------------------------------------------------------------------------------------------------------
def batch_edges():
    """name -> case on the 640 x 480 geometry, window 30: empty frames, no level-0 feature, every prev outside the image"""
    out = {}
    rng = np.random.default_rng(77)
    f1, f2, prev = PC.initialization_case(rng, 40, 50)
    e1, e2, _ = PC.initialization_case(rng, 0, 0)
    out["n1_0"] = dict(f1=e1, f2=f2, prev=np.zeros((0, 2), F))
    out["n2_0"] = dict(f1=f1, f2=e2, prev=prev)
    g1 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f1.items()}
    g1["octave"] = np.maximum(g1["octave"], 1)
    out["no_level0"] = dict(f1=g1, f2=f2, prev=prev)
    out["prev_outside"] = dict(f1=f1, f2=f2, prev=(prev + F(5000.0)).astype(F))
    out["prev_negative"] = dict(f1=f1, f2=f2, prev=(prev - F(5000.0)).astype(F))
    out["plain"] = dict(f1=f1, f2=f2, prev=prev)
    for c in out.values():
        c.update(window=30, check_ori=True)
    return out
