"""Cases for the Sim3 solver (tests/sim3_oracle.py, csrc/orbfe_sim3.hip): two keyframes' camera-frame points related by a
similarity, a share of outliers, level sigma^2 values, and the draws of every `iterate` call.  The draws are an input of the
solver, so a case can steer which iteration picks three inliers: a return on a chosen lane of a chunk of hypotheses.

Every case is generated so that, under the libm oracle, no finite error of any iteration run lies within a relative MARGIN of
its threshold (a seed that does not meet this is rejected and the next one tried): the inlier decisions then cannot depend
on the last bits of atan2 / sin / cos, which is what lets the canonical oracle and the kernel stand in for the reference."""
import functools

import numpy as np

import sim3_oracle as SO

F = np.float32
MARGIN = 1e-4
K_A = (525.0, 525.0, 319.5, 239.5)
K_B = (517.3, 516.5, 318.6, 255.3)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def scene(n, n_out, seed, s=1.0, noise=0.002, angle=0.3):
    """n pairs with X1 ~ s * R * X2 + t; n_out of them replaced by unrelated points.  -> X1, X2, sigma2_1, sigma2_2, inlier flags"""
    rng = np.random.default_rng(seed)
    X2 = rng.uniform([-2, -1.5, 2], [2, 1.5, 8], (n, 3))
    R = rodrigues(rng.normal(size=3), angle)
    t = rng.uniform(-0.5, 0.5, 3)
    X1 = s * (X2 @ R.T) + t + noise * rng.normal(size=(n, 3))
    inl = np.ones(n, bool)
    inl[rng.permutation(n)[:n_out]] = False
    X1[~inl] = rng.uniform([-2, -1.5, 2], [2, 1.5, 8], (int((~inl).sum()), 3))
    lv = 1.2 ** (2 * rng.integers(0, 8, (2, n)))
    return X1.astype(F), X2.astype(F), lv[0].astype(F), lv[1].astype(F), inl


def draws_for_triple(tri, n):
    """three raw draws that make Sim3Solver's swap-with-back selection pick `tri` out of n"""
    avail = list(range(n))
    out = []
    for v in tri:
        k = avail.index(v)
        out.append(int((k + 0.5) / len(avail) * 2147483648.0))
        avail[k] = avail[-1]
        avail.pop()
    assert SO.triple_from_draws(out, n) == list(tri)
    return out


def steered_draws(inl, total, good_at, rng):
    """3 * total draws: the iterations listed in good_at pick three inliers, every other one at least one outlier"""
    n = len(inl)
    gi, bi = np.flatnonzero(inl), np.flatnonzero(~inl)
    d = []
    for it in range(total):
        if it in good_at:
            tri = rng.choice(gi, 3, replace=False)
        else:
            o = int(rng.choice(bi))
            tri = rng.permutation(np.r_[o, rng.choice(np.setdiff1d(np.arange(n), [o]), 2, replace=False)])
        d += draws_for_triple([int(v) for v in tri], n)
    return np.array(d, np.int32)


def make(name, X1, X2, s1, s2, calls, fix_scale=True, min_inliers=20, K1=K_A, K2=K_B, max_its=None, expect=None):
    n = len(X1)
    if max_its is None:
        max_its = SO.ransac_iterations(0.99, min_inliers, 300, n)
    return dict(name=name, X1=np.ascontiguousarray(X1, F), X2=np.ascontiguousarray(X2, F), sigma2_1=np.ascontiguousarray(s1, F),
                sigma2_2=np.ascontiguousarray(s2, F), K1=K1, K2=K2, fix_scale=fix_scale, min_inliers=min_inliers, max_its=max_its,
                calls=calls, expect=expect)


def run(case, mode):
    """every `iterate` call of the case through the oracle -> (list of iterate results, the solver)"""
    s = SO.Solver(case["X1"], case["X2"], case["sigma2_1"], case["sigma2_2"], case["K1"], case["K2"], case["fix_scale"], mode)
    s.min_inliers = case["min_inliers"]
    s.max_its = case["max_its"]
    outs = []
    for nit, draws in case["calls"]:
        r = s.iterate(nit, draws)
        r["state"] = dict(iterations=s.iterations, best_inliers=s.best_inliers, best=s.best, best_mask=s.best_mask.copy())
        outs.append(r)
    return outs, s


def margin(case, outs):
    """the smallest relative distance of a finite error to its threshold over every iteration run"""
    thr1, thr2 = SO.max_errors(case["sigma2_1"]).astype(np.float64), SO.max_errors(case["sigma2_2"]).astype(np.float64)
    m = np.inf
    for r in outs:
        for it in r["log"]:
            for e, t in ((it["err1"], thr1), (it["err2"], thr2)):
                e = e.astype(np.float64)
                ok = np.isfinite(e)
                if ok.any():
                    m = min(m, float((np.abs(e[ok] - t[ok]) / t[ok]).min()))
    return m


def _accept(case):
    outs, _ = run(case, "libm")
    if margin(case, outs) <= MARGIN:
        return False
    if case["expect"] is not None:
        got = [(bool(r["found"]), r["iterations_run"]) for r in outs]
        if got != case["expect"]:
            return False
    return True


def _search(build, seed0):
    for seed in range(seed0, seed0 + 40):
        c = build(seed)
        if _accept(c):
            c["seed"] = seed
            return c
    raise AssertionError("no seed met the margin / the steering of this case")


def _steered(name, n, n_out, calls_spec, seed0, s=1.0, fix_scale=True, min_inliers=20):
    """calls_spec: list of (n_iterations, iterations of that call that pick three inliers, expected (found, iterations run))"""
    def build(seed):
        X1, X2, s1, s2, inl = scene(n, n_out, seed, s)
        rng = np.random.default_rng(seed + 7919)
        calls = [(nit, steered_draws(inl, nit, good, rng)) for nit, good, _ in calls_spec]
        return make(name, X1, X2, s1, s2, calls, fix_scale, min_inliers, expect=[e for _, _, e in calls_spec])
    return _search(build, seed0)


def _random(name, n, n_out, nits, seed0, s=1.0, fix_scale=True, min_inliers=20):
    def build(seed):
        X1, X2, s1, s2, _ = scene(n, n_out, seed, s)
        rng = np.random.default_rng(seed + 104729)
        calls = [(k, rng.integers(0, 2 ** 31, 3 * k).astype(np.int32)) for k in nits]
        return make(name, X1, X2, s1, s2, calls, fix_scale, min_inliers)
    return _search(build, seed0)


def translation_case(n=40, nits=(5, 5)):
    """pure translation, every coordinate a multiple of 3: centroids, M and N are exact, the quaternion is (1, 0, 0, 0), its
    imaginary part is zero and every model is NaN"""
    rng = np.random.default_rng(5)
    X2 = 3.0 * rng.integers([-20, -20, 2], [20, 20, 30], (n, 3))
    X1 = X2 + [6.0, -3.0, 9.0]
    d = np.random.default_rng(6)
    calls = [(k, d.integers(0, 2 ** 31, 3 * k).astype(np.int32)) for k in nits]
    return make("nan_translation", X1, X2, np.ones(n), np.ones(n), calls, True, 20)


def exact_case(s=2.0):
    """noise-free integer points under s = 2, a quarter turn about z and an integer t"""
    rng = np.random.default_rng(11)
    n = 30
    X2 = rng.integers([-9, -9, 4], [9, 9, 16], (n, 3)).astype(np.float64)
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    X1 = s * (X2 @ R.T) + [1.0, 2.0, 3.0]
    calls = [(1, np.array(draws_for_triple([0, 1, 2], n), np.int32))]
    c = make("exact", X1, X2, np.ones(n), np.ones(n), calls, False, 20)
    c["truth"] = (s, R, np.array([1.0, 2.0, 3.0]))
    return c


def behind_case():
    """some points of keyframe 1 land behind camera 2 under T21, one X2 has z == 0 and one z < 0"""
    def build(seed):
        X1, X2, s1, s2, inl = scene(80, 16, seed)
        o = np.flatnonzero(~inl)
        X1[o[:4], 2] = -X1[o[:4], 2] - 20   # far behind both cameras
        X2[o[4]] = [0.5, 0.25, 0.0]
        X2[o[5], 2] = -3.0
        rng = np.random.default_rng(seed + 13)
        calls = [(5, steered_draws(inl, 5, (3,), rng))]
        return make("behind", X1, X2, s1, s2, calls, True, 20, expect=[(True, 4)])
    return _search(build, 300)


@functools.lru_cache(maxsize=None)
def table():
    """name -> case"""
    c = {}
    for n in (3, 19, 20, 63, 64, 65, 257):
        c[f"n_{n}"] = _random(f"n_{n}", n, n // 4, (5,), 1000 + n)
    c["n_21"] = _random("n_21", 21, 0, (5,), 1021)
    # returns on the first lane, a middle lane and the last lane of a chunk of 32 hypotheses, and in the second chunk
    c["its_1_first"] = _steered("its_1_first", 100, 30, [(1, (0,), (True, 1))], 2000)
    c["its_5_middle"] = _steered("its_5_middle", 100, 30, [(5, (2,), (True, 3))], 2010, s=1.7, fix_scale=False)
    c["its_33_last_lane"] = _steered("its_33_last_lane", 100, 30, [(33, (31,), (True, 32))], 2020)
    c["its_33_second_chunk"] = _steered("its_33_second_chunk", 100, 30, [(33, (32,), (True, 33))], 2030, s=0.6, fix_scale=False)
    c["its_300_second_chunk"] = _steered("its_300_second_chunk", 100, 30, [(300, (45,), (True, 46))], 2040)
    c["its_300_none"] = _steered("its_300_none", 100, 30, [(300, (), (False, 300))], 2050)
    c["scale_free_on_fixed_data"] = _random("scale_free_on_fixed_data", 64, 16, (5,), 2060, fix_scale=False)
    c["fixed_on_scaled_data"] = _random("fixed_on_scaled_data", 64, 16, (5,), 2070, s=1.3, fix_scale=True)
    c["behind"] = behind_case()
    c["nan_translation"] = translation_case()
    c["exact"] = exact_case()

    def outliers(seed):
        X1, X2, s1, s2, _ = scene(64, 64, seed)
        rng = np.random.default_rng(seed + 1)
        return make("all_outliers", X1, X2, s1, s2, [(300, rng.integers(0, 2 ** 31, 900).astype(np.int32))], True, 20)
    c["all_outliers"] = _search(outliers, 2080)
    c["three_calls"] = _steered("three_calls", 100, 30, [(5, (), (False, 5)), (5, (), (False, 5)), (5, (2,), (True, 3))], 2090)
    return c


def second_call_case():
    """a success, then a second call whose iterations pick three inliers twice: it returns only where the count reaches the
    stored best (the `>= best` condition), which the expectation leaves to the oracle"""
    def build(seed):
        X1, X2, s1, s2, inl = scene(100, 30, seed)
        rng = np.random.default_rng(seed + 3)
        calls = [(5, steered_draws(inl, 5, (1,), rng)), (10, steered_draws(inl, 10, (2, 6), rng))]
        return make("second_call", X1, X2, s1, s2, calls, True, 20)

    def good(c):
        outs, _ = run(c, "libm")
        return outs[0]["found"] and outs[0]["iterations_run"] == 2 and outs[1]["found"] and outs[1]["iterations_run"] == 7
    for seed in range(2100, 2200):
        c = build(seed)
        if _accept(c) and good(c):
            c["seed"] = seed
            return c
    raise AssertionError("no seed gave a second call that skips a smaller inlier count")


@functools.lru_cache(maxsize=None)
def full_table():
    c = dict(table())
    c["second_call"] = second_call_case()
    return c


@functools.lru_cache(maxsize=None)
def reference(name, mode="canonical"):
    """the oracle's run of a case, computed once and shared: (list of iterate results, final solver)"""
    return run(full_table()[name], mode)
