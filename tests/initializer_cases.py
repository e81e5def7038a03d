"""Synthetic frame pairs for the monocular Initializer (tests/initializer_oracle.py, csrc/orbfe_initializer.hip): noiseless
general and planar scenes, and the cases steered at one branch each.  A case is a dict: keys1 [n1, 2], keys2 [n2, 2], matches12
int32 [n1], K [3, 3], sigma, iterations, draws [iterations * 8], and the ground truth (R, t, X by index of keys1) where there
is one.  Everything is drawn from seeded generators, so the oracle's answer for a case is a constant of the repository."""
import numpy as np

K0 = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]], np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def project(X, R, t, K=K0):
    Xc = X @ R.T + t
    uv = Xc[:, :2] / Xc[:, 2:3]
    K = K.astype(np.float64)
    return np.stack([K[0, 0] * uv[:, 0] + K[0, 2], K[1, 1] * uv[:, 1] + K[1, 2]], 1)


def points(kind, N, rng):
    """3-D points in the first camera's frame"""
    x = rng.uniform(-2.0, 2.0, N)
    y = rng.uniform(-1.5, 1.5, N)
    if kind == "planar":
        z = 6.0 + 0.45 * x - 0.3 * y
    else:
        z = rng.uniform(4.0, 9.0, N)
    return np.stack([x, y, z], 1)


def draws_for(iterations, seed):
    return np.random.default_rng(1000 + seed).integers(0, 2 ** 31, iterations * 8).astype(np.int32)


def pair_from(X, R, t, extra1=0, extra2=0, seed=0, iterations=16, sigma=1.0, shuffle=True, draws=None, K=K0):
    """keys and matches for the 3-D points X seen from [I | 0] and [R | t]; extra1 / extra2 unmatched keys are interleaved and the
    second frame's keys are permuted, so that n1 != n2 and the match indices are not the identity"""
    rng = np.random.default_rng(seed)
    N = len(X)
    a = project(X, np.eye(3), np.zeros(3), K)
    b = project(X, R, t, K)
    n1, n2 = N + extra1, N + extra2
    pos1 = np.sort(rng.permutation(n1)[:N]) if extra1 else np.arange(N)
    pos2 = rng.permutation(n2)[:N] if (shuffle or extra2) else np.arange(N)
    keys1 = rng.uniform([0, 0], [640, 480], (n1, 2))
    keys2 = rng.uniform([0, 0], [640, 480], (n2, 2))
    keys1[pos1] = a
    keys2[pos2] = b
    m = np.full(n1, -1, np.int32)
    m[pos1] = pos2
    Xk = np.zeros((n1, 3))
    Xk[pos1] = X
    return dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m, K=K.astype(np.float32), sigma=sigma,
                iterations=iterations, draws=draws_for(iterations, seed) if draws is None else draws, R=R, t=t, X=Xk, matched=pos1)


R_GEN, T_GEN = rot(0.02, -0.05, 0.03), np.array([0.6, 0.1, 0.05])


def general(N, seed=0, **kw):
    return pair_from(points("general", N, np.random.default_rng(seed)), R_GEN, T_GEN, seed=seed, **kw)


def planar(N, seed=0, **kw):
    return pair_from(points("planar", N, np.random.default_rng(seed)), R_GEN, T_GEN, seed=seed, **kw)


def tie(N=64, seed=3):
    """every iteration draws the same set: all scores tie and iteration 0 has to win"""
    d = np.tile(draws_for(1, seed), 3)
    return general(N, seed, iterations=3, draws=d)


def pure_rotation(N=80, seed=4):
    """no translation: H = K R K^-1, three equal singular values, the d1/d2 early-out of ReconstructH"""
    X = points("general", N, np.random.default_rng(seed))
    return pair_from(X, rot(0.03, 0.08, -0.02), np.zeros(3), seed=seed)


def two_sided(N=120, seed=5):
    """half of the points lie behind both cameras (their projections are still those of the same epipolar geometry): (R, t) and
    (R, -t) each triangulate one half in front, so nsimilar > 1"""
    X = points("general", N, np.random.default_rng(seed))
    X[::2] *= -1.0
    return pair_from(X, R_GEN, T_GEN, seed=seed)


def too_few(N=30, seed=6):
    """a good F with fewer than minTriangulated = 50 points: maxGood < nMinGood"""
    return general(N, seed)


def low_parallax(N=100, seed=7):
    """a baseline of about 1/90 of the median depth: some 0.6 degrees of parallax, below the 1 degree cut and above the 0.99998
    gate; depths from 3 to 12 keep a homography from explaining the scene"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3, 12, N)], 1)
    return pair_from(X, rot(0.01, -0.01, 0.005), np.array([0.08, 0.01, 0.0]), seed=seed)


def far_point(N=90, seed=8):
    """match 0 is a point 10^6 away: it passes every gate of CheckRT with cosParallax >= 0.99998, so it enters vCosParallax and
    vP3D but neither nGood nor vbTriangulated"""
    X = points("general", N, np.random.default_rng(seed))
    X[0] = [1.0e5, -0.5e5, 1.0e6]
    return pair_from(X, R_GEN, T_GEN, seed=seed, shuffle=False)


def one_behind(N=70, seed=9):
    """match 0 is a point in front of the first camera and behind the second: one of the losing hypotheses triangulates it
    alone, a vCosParallax of size 1"""
    X = points("general", N, np.random.default_rng(seed))
    t = np.array([0.3, 0.05, -3.0])
    X[0] = [0.2, -0.1, 1.5]
    return pair_from(X, rot(0.01, 0.02, -0.01), t, seed=seed, shuffle=False)


def sized(N, seed=10):
    """vCosParallax of exactly N entries for the winner (N = 50, 51, 52 straddle idx = min(50, size - 1))"""
    return general(N, seed + N)


def ambiguous_plane(N=100, seed=11, t=(0.3, 0.0, 0.8)):
    """a fronto-parallel plane approached almost along its normal: the two physically possible decompositions of H are close to
    each other and both put nearly every point in front, secondBest >= 0.75 best"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), np.full(N, 6.0)], 1)
    return pair_from(X, rot(0.0, 0.0, 0.0), np.array(t), seed=seed)


def ambiguous_tie():
    """as ambiguous_plane, with hypotheses 0 and 1 at the same nGood: the lower index stays best"""
    return ambiguous_plane(seed=12, t=(0.15, 0.0, 0.6))


def noisy(kind, N, seed, noise=0.7, outliers=0.2, **kw):
    """pixel noise on the second frame's matched keys and a share of wrong matches: scores without ties, points near every gate
    (not noiseless, so no ground-truth tolerances: parity only)"""
    c = pair_from(points(kind, N, np.random.default_rng(seed)), R_GEN, T_GEN, seed=seed, **kw)
    rng = np.random.default_rng(seed + 7)
    m = c["matches12"]
    first = np.nonzero(m >= 0)[0]
    k2 = c["keys2"].astype(np.float64)
    k2[m[first]] += rng.normal(0, noise, (len(first), 2))
    wrong = first[rng.random(len(first)) < outliers]
    k2[m[wrong]] = rng.uniform([0, 0], [640, 480], (len(wrong), 2))
    c["keys2"] = k2.astype(np.float32)
    return c


# name -> constructor; the sizes the issue names (N = 8, 9, 63, 64, 65, 257; iterations 1, 2, 63, 64, 65, 200; n1 != n2)
TABLE = {
    "general_8": lambda: general(8, 20, iterations=4),
    "general_9": lambda: general(9, 21, iterations=8),
    "general_63": lambda: general(63, 22, iterations=1),
    "general_64": lambda: general(64, 23, iterations=2, extra1=7, extra2=3),
    "general_65": lambda: general(65, 24, iterations=63),
    "general_257": lambda: general(257, 25, iterations=64, extra1=40, extra2=91),
    "general_100_it65": lambda: general(100, 26, iterations=65, extra1=5),
    "general_120_it200": lambda: general(120, 27, iterations=200, extra2=9),
    "planar_64": lambda: planar(64, 30, iterations=8, extra1=3),
    "planar_257": lambda: planar(257, 31, iterations=16, extra2=20),
    "tie": tie,
    "pure_rotation": pure_rotation,
    "two_sided": two_sided,
    "too_few": too_few,
    "low_parallax": low_parallax,
    "far_point": far_point,
    "one_behind": one_behind,
    "sized_50": lambda: sized(50),
    "sized_51": lambda: sized(51),
    "sized_52": lambda: sized(52),
    "ambiguous_plane": ambiguous_plane,
    "ambiguous_tie": ambiguous_tie,
    "noisy_general_200": lambda: noisy("general", 200, 60, iterations=100, extra1=20, extra2=35),
    "noisy_general_sigma": lambda: noisy("general", 130, 61, noise=1.2, iterations=80, sigma=1.5),
    "noisy_planar_150": lambda: noisy("planar", 150, 62, iterations=90, extra2=11),
}

_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = TABLE[name]()
    return _cache[name]


_answers = {}


def answer(name, tap_iteration=0, tap_hypothesis=0):
    """the oracle's answer for a case, computed once per (case, taps)"""
    import initializer_oracle as IO
    key = (name, tap_iteration, tap_hypothesis)
    if key not in _answers:
        c = case(name)
        _answers[key] = IO.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], c["sigma"], c["iterations"], c["draws"],
                                      tap_iteration, tap_hypothesis)
    return _answers[key]


# ---- known-answer inputs ---------------------------------------------------------------------------------------------------------
def kat_points(n, seed=40):
    """n sets of eight normalised point pairs from a general scene -> (vP1 [n, 8, 2], vP2 [n, 8, 2]) float32"""
    import initializer_oracle as IO
    rng = np.random.default_rng(seed)
    c = general(120, seed)
    first = np.nonzero(c["matches12"] >= 0)[0]
    pn1, _ = IO.normalize(c["keys1"])
    pn2, _ = IO.normalize(c["keys2"])
    sets = np.stack([rng.permutation(len(first))[:8] for _ in range(n)])
    return pn1[first[sets]], pn2[c["matches12"][first[sets]]]


def kat_matrices(what, n=6, seed=41):
    """the KAT matrices float32 [n, rows, cols]: the DLT systems of ComputeH21 (16 x 9) and ComputeF21 (8 x 9) on kat_points, a
    rank-2 and four random 3 x 3, Triangulate-like and random 4 x 4"""
    rng = np.random.default_rng(seed)
    p1, p2 = kat_points(n)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    one, zero = np.ones_like(u1), np.zeros_like(u1)
    if what == "16x9":
        r0 = np.stack([zero, zero, zero, -u1, -v1, -one, v2 * u1, v2 * v1, v2], -1)
        r1 = np.stack([u1, v1, one, zero, zero, zero, -u2 * u1, -u2 * v1, -u2], -1)
        return np.stack([r0, r1], 2).reshape(n, 16, 9).astype(np.float32)
    if what == "8x9":
        return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], -1).astype(np.float32)
    if what == "3x3":
        A = rng.normal(size=(n, 3, 3))
        A[0, 2] = A[0, 0] - 2 * A[0, 1]   # rank 2: a null singular value
        return A.astype(np.float32)
    A = rng.normal(size=(n, 4, 4))
    A[0, 3] = A[0, 0] + A[0, 1]
    return A.astype(np.float32)
