"""Edge cases of the Sim3 solver beside tests/sim3_cases.py: a count equal to min_inliers, ties of the best count inside a chunk
and across the chunk boundary, one NaN hypothesis among good ones, the iteration clamp on the chunk boundary and with carried
state, pair counts on the 256-lane stride, extreme scales and Rodrigues' identity arm.  Every case keeps the MARGIN acceptance
rule of sim3_cases._accept (searched from a fixed seed), so the libm and canonical oracles take the same decisions.  Sizes: at
most 600 pairs (513 in one case) and 200 iterations per call."""
import functools

import numpy as np

import sim3_cases as SC
import sim3_oracle as SO

F = np.float32
MAX_PAIRS = 513
# the seed each case's search accepts (identity_arm: the step of its scan).  tests/test_sim3_edge_cases.py holds the table to
# them, so that a change in sim3_cases.scene or in the oracle that moves a case to another seed shows up as such
SEEDS = {"count_eq_min": 3000, "count_eq_min_minus_1": 3000, "tie_same_chunk": 3100, "tie_31_32": 3100, "zero_tie_nan_first": 3200,
         "zero_tie_nan_last": 3200, "one_nan_in_chunk": 3300, "clamp_32": 3400, "clamp_33": 3410, "clamp_64": 3420, "clamp_carried": 3430,
         "pairs_255": 3755, "pairs_256": 3756, "pairs_512": 4012, "pairs_513": 4013, "scale_0.05": 3600, "scale_20": 3620,
         "truncation": 3721, "identity_arm": 32}


def _good_triples(inl, k, rng):
    gi = np.flatnonzero(inl)
    return [[int(v) for v in rng.choice(gi, 3, replace=False)] for _ in range(k)]


def _bad_triple(inl, rng):
    n = len(inl)
    o = int(rng.choice(np.flatnonzero(~inl)))
    return [int(v) for v in rng.permutation(np.r_[o, rng.choice(np.setdiff1d(np.arange(n), [o]), 2, replace=False)])]


def _draws(triples, n):
    return np.array([d for t in triples for d in SC.draws_for_triple(t, n)], np.int32)


def _counts(case):
    outs, _ = SC.run(case, "libm")
    return [[it["count"] for it in r["log"]] for r in outs], outs


# ---- count == min_inliers --------------------------------------------------------------------------------------------------------
def count_equals_min():
    """iteration 2 of 5 picks three inliers and counts c.  min_inliers = c: no return, it becomes the best.  min_inliers = c - 1: it
    returns there.  -> (case with c, case with c - 1, c)"""
    for seed in range(3000, 3040):
        X1, X2, s1, s2, inl = SC.scene(100, 30, seed)
        d = SC.steered_draws(inl, 5, (2,), np.random.default_rng(seed + 7919))
        probe = SC.make("probe", X1, X2, s1, s2, [(5, d)], True, 99, max_its=300)
        c = _counts(probe)[0][0][2]
        eq = SC.make("count_eq_min", X1, X2, s1, s2, [(5, d)], True, c, max_its=300, expect=[(False, 5)])
        below = SC.make("count_eq_min_minus_1", X1, X2, s1, s2, [(5, d)], True, c - 1, max_its=300, expect=[(True, 3)])
        if c > 20 and max(_counts(probe)[0][0][3:]) < c and SC._accept(eq) and SC._accept(below):
            eq["seed"] = below["seed"] = seed
            return eq, below, c
    raise AssertionError("no seed for count == min_inliers")


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def tie(name, a, b, nit):
    """iterations a and b pick two different inlier triples that count the same, min_inliers = that count: neither returns, the
    later one is the best after the call"""
    for seed in range(3100, 3160):
        X1, X2, s1, s2, inl = SC.scene(100, 30, seed)
        rng = np.random.default_rng(seed + 1)
        g = _good_triples(inl, 2, rng)
        tri = [g[0] if it == a else g[1] if it == b else _bad_triple(inl, rng) for it in range(nit)]
        d = _draws(tri, 100)
        probe = SC.make("probe", X1, X2, s1, s2, [(nit, d)], True, 99, max_its=300)
        cnt, outs = _counts(probe)
        cnt, log = cnt[0], outs[0]["log"]
        if cnt[a] != cnt[b] or cnt[a] < 20 or max(c for i, c in enumerate(cnt) if i not in (a, b)) >= cnt[a]:
            continue
        if log[a]["T12"].tobytes() == log[b]["T12"].tobytes():
            continue
        c = SC.make(name, X1, X2, s1, s2, [(nit, d)], True, cnt[a], max_its=300, expect=[(False, nit)])
        if SC._accept(c):
            c["tie"], c["seed"] = (a, b), seed
            return c
    raise AssertionError("no seed for " + name)


def planted_scene(seed):
    """an ordinary scene of 64 pairs whose first three are exact-translation pairs (every coordinate a multiple of 3, as
    sim3_cases.translation_case): the triple (0, 1, 2) gives a NaN model"""
    X1, X2, s1, s2, inl = SC.scene(64, 16, seed)
    rng = np.random.default_rng(seed + 5)
    P = 3.0 * rng.integers([-20, -20, 2], [20, 20, 30], (3, 3))
    X2[:3] = P
    X1[:3] = P + [6.0, -3.0, 9.0]
    inl[:3] = False
    return X1, X2, s1, s2, inl


def zero_tie(nan_first):
    """a tie at count 0 between the NaN model and a finite model that counts nothing, in the given order: two iterations"""
    for seed in range(3200, 3260):
        X1, X2, s1, s2, inl = planted_scene(seed)
        rng = np.random.default_rng(seed + 2)
        for _ in range(20):
            bad = _bad_triple(inl, rng)
            if set(bad) & {0, 1, 2}:
                continue
            tri = [[0, 1, 2], bad] if nan_first else [bad, [0, 1, 2]]
            name = "zero_tie_nan_first" if nan_first else "zero_tie_nan_last"
            c = SC.make(name, X1, X2, s1, s2, [(2, _draws(tri, 64))], True, 20, max_its=300, expect=[(False, 2)])
            cnt, outs = _counts(c)
            fin = [it["finite"] for it in outs[0]["log"]]
            if cnt[0] == [0, 0] and fin == ([False, True] if nan_first else [True, False]) and SC._accept(c):
                c["seed"] = seed
                return c
    raise AssertionError("no finite model that counts nothing")


def one_nan_in_chunk():
    """iteration 2 draws the planted triple (a NaN model among finite ones), iteration 6 three inliers: the call returns there"""
    def build(seed):
        X1, X2, s1, s2, inl = planted_scene(seed)
        rng = np.random.default_rng(seed + 3)
        tri = [[0, 1, 2] if it == 2 else _good_triples(inl, 1, rng)[0] if it == 6 else _bad_triple(inl, rng) for it in range(10)]
        return SC.make("one_nan_in_chunk", X1, X2, s1, s2, [(10, _draws(tri, 64))], True, 20, max_its=300, expect=[(True, 7)])
    return SC._search(build, 3300)


# ---- the clamp --------------------------------------------------------------------------------------------------------------------
def clamp(name, max_its, nits, expect, seed0):
    """no iteration picks three inliers: every call runs to what the clamp leaves"""
    def build(seed):
        X1, X2, s1, s2, inl = SC.scene(60, 20, seed)
        rng = np.random.default_rng(seed + 7919)
        calls = [(k, SC.steered_draws(inl, k, (), rng)) for k in nits]
        return SC.make(name, X1, X2, s1, s2, calls, True, 20, max_its=max_its, expect=expect)
    return SC._search(build, seed0)


# ---- pair counts ------------------------------------------------------------------------------------------------------------------
def pairs(n, seed0):
    """n pairs with an inlier at 255, at 256 and at the last index, each beside an outlier (254, 257, n - 2): a tail the
    kernel dropped, or a lane it read twice, changes the count.  Iteration 1 of 3 returns"""
    def build(seed):
        X1, X2, s1, s2, inl = SC.scene(n, n // 4, seed)
        want = {i: True for i in (255, 256, n - 1) if 0 <= i < n}
        want.update({i: False for i in (254, 257, n - 2) if 0 <= i < n and i not in want})
        free = [i for i in range(n) if i not in want]
        for i, w in want.items():
            if inl[i] != w:
                j = next(j for j in free if inl[j] == w)
                free.remove(j)
                for a in (X1, X2, s1, s2, inl):
                    a[[i, j]] = a[[j, i]]
        rng = np.random.default_rng(seed + 7919)
        c = SC.make(f"pairs_{n}", X1, X2, s1, s2, [(3, SC.steered_draws(inl, 3, (1,), rng))], True, 20, max_its=300, expect=[(True, 2)])
        c["inl"] = inl
        return c
    return SC._search(build, seed0)


# ---- scale ------------------------------------------------------------------------------------------------------------------------
def scaled(s, seed0):
    """fix_scale = 0 on data of scale s; the noise scales along, so that the inliers stay inliers"""
    def build(seed):
        X1, X2, s1, s2, inl = SC.scene(100, 30, seed, s=s, noise=0.002 * min(s, 1.0))
        rng = np.random.default_rng(seed + 7919)
        return SC.make(f"scale_{s}", X1, X2, s1, s2, [(5, SC.steered_draws(inl, 5, (2,), rng))], False, 20, max_its=300, expect=[(True, 3)])
    return SC._search(build, seed0)


# ---- the truncated thresholds -------------------------------------------------------------------------------------------------------
def truncation():
    """mvnMaxError is (size_t)(9.210 * sigma2): noise of 0.01 puts errors of true inliers between the truncated threshold and
    9.210 * sigma2 (still MARGIN away from the truncated one); the first seed at which un-truncated thresholds change a count"""
    for seed in range(3700, 3760):
        X1, X2, s1, s2, inl = SC.scene(100, 30, seed, noise=0.01)
        rng = np.random.default_rng(seed + 7919)
        c = SC.make("truncation", X1, X2, s1, s2, [(5, SC.steered_draws(inl, 5, (2,), rng))], True, 20, max_its=300, expect=[(True, 3)])
        if not SC._accept(c):
            continue
        cnt = [lg["count"] for lg in SC.run(c, "canonical")[0][0]["log"]]
        if cnt != [lg["count"] for lg in with_break("max_errors_no_trunc", lambda: SC.run(c, "canonical"))[0][0]["log"]]:
            c["seed"] = seed
            return c
    raise AssertionError("no seed puts an error between the truncated threshold and 9.210 * sigma2")


# ---- Rodrigues' identity arm ----------------------------------------------------------------------------------------------------------
def identity_arm():
    """theta < DBL_EPSILON with a non-zero axis inside iterate.  The float Jacobi stops at |p| <= FLT_EPSILON (absolute), so the
    quaternion's imaginary part is either exactly zero (NaN model) or p / (difference of the diagonal): below 1e-16 only when
    the diagonal of N is past 1e9 while an off-diagonal entry stays near 1e-6.  Pairs that do it: a pure translation of points
    spread over 1e5 in x and y with depths near 1e-7, one depth off by less than 1e-12 (the translation itself is zero).  Not
    a scene a camera sees.  The other 17 pairs are ordinary points with X1 == X2: the identity model counts them and returns.
    -> the case, or None when the bounded scan of the perturbation finds none"""
    base = np.array([[1.0e5, 2.0e5, 1.0e-7], [-2.0e5, 1.0e5, 2.0e-7], [1.0e5, -3.0e5, 3.0e-7]])
    rng = np.random.default_rng(9)
    fill = np.stack([rng.uniform(-2, 2, 17), rng.uniform(-1.5, 1.5, 17), rng.uniform(2, 8, 17)], 1)
    for k in range(1, 400):
        X2 = np.vstack([base, fill]).astype(F)
        X1 = X2.copy()
        X1[0, 2] = np.nextafter(X1[0, 2], F(1), dtype=F) if k == 1 else F(X1[0, 2] * (1 + k * 2.0 ** -22))
        c = SC.make("identity_arm", X1, X2, np.ones(20), np.ones(20), [(1, _draws([[0, 1, 2]], 20))], True, 6, max_its=300)
        outs, _ = SC.run(c, "canonical")
        lg = outs[0]["log"][0]
        if lg["identity"] and lg["finite"] and SC._accept(c):
            c["seed"] = k   # the step of the scan
            return c
    return None


@functools.lru_cache(maxsize=None)
def table():
    """name -> case"""
    t = {}
    eq, below, _ = count_equals_min()
    t["count_eq_min"], t["count_eq_min_minus_1"] = eq, below
    t["tie_same_chunk"] = tie("tie_same_chunk", 3, 7, 12)
    t["tie_31_32"] = tie("tie_31_32", 31, 32, 40)
    t["zero_tie_nan_first"] = zero_tie(True)
    t["zero_tie_nan_last"] = zero_tie(False)
    t["one_nan_in_chunk"] = one_nan_in_chunk()
    t["clamp_32"] = clamp("clamp_32", 32, (100,), [(False, 32)], 3400)
    t["clamp_33"] = clamp("clamp_33", 33, (100,), [(False, 33)], 3410)
    t["clamp_64"] = clamp("clamp_64", 64, (100,), [(False, 64)], 3420)
    t["clamp_carried"] = clamp("clamp_carried", 32, (20, 40, 10), [(False, 20), (False, 12), (False, 0)], 3430)
    for n in (255, 256, 512, 513):
        t[f"pairs_{n}"] = pairs(n, 3500 + n)
    t["scale_0.05"] = scaled(0.05, 3600)
    t["scale_20"] = scaled(20.0, 3620)
    t["truncation"] = truncation()
    c = identity_arm()
    if c is not None:
        t["identity_arm"] = c
    return t


@functools.lru_cache(maxsize=None)
def reference(name, mode="canonical"):
    """the oracle's run of a case, computed once and shared: (list of iterate results, final solver)"""
    return SC.run(table()[name], mode)


def _b(a):
    """the bytes of a float array, every NaN the same one (its sign and payload belong to the processor)"""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def compared(outs):
    """the bytes of everything the GPU test compares of the oracle's run of a case (sim3_cases.run)"""
    out = []
    for o in outs:
        st = o["state"]
        out += [str((o["found"], o["no_more"], o["n_inliers"], o["iterations_run"], st["iterations"], st["best_inliers"])).encode(),
                _b(np.zeros((4, 4), F) if o["T12"] is None else o["T12"]), o["mask"].tobytes(), st["best_mask"].tobytes()]
        if st["best"] is not None:
            out += [_b(st["best"][k]) for k in ("T12", "R", "t")] + [_b(np.array([st["best"]["s"]], F))]
        for lg in o["log"]:
            out += [str(([int(v) for v in lg["triple"]], lg["count"])).encode(), _b(lg["T12"]), _b(lg["err1"]), _b(lg["err2"])]
    return b"".join(out)


def with_break(rule, fn):
    SO.SIM3_BREAK = frozenset([rule])
    try:
        return fn()
    finally:
        SO.SIM3_BREAK = frozenset()
