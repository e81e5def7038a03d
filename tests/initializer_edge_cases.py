"""Frame pairs for the monocular Initializer (csrc/orbfe_initializer.hip) at the seams of its three kernels: the 256-key passes
of k_init_prepare's compaction, the 256-match LDS stages and the 512-iteration grid of k_init_ransac, the radix selection and the
winner scan of k_init_reconstruct, and the batch form.  Built on initializer_cases.pair_from; a case is the same dict.  numpy
only: tests/test_initializer_edge_cases.py shows with tests/initializer_oracle.py alone that every case sits on the edge it
names, tests/test_gpu_initializer_edges.py runs the kernels on them.  Everything is seeded, so the oracle's answer is a constant
of the repository.  Test support only.

One table per group (name -> constructor, the docstring or the comment names the edge):
  PASSES      1. n1 = 256 .. 2000 with planted layouts of the matched keys over the 256-key passes
  STAGES      2. N = 256 .. 4096 matches over the 256-match stages, general and planar
  ITERATIONS  3. 448 .. 512 iterations with the strict winner of both models in the last one
  PARALLAX    4. converging wide-baseline scenes: negative cosines, the sign change at index 50 / 51, a wide spread, one bit
                 pattern across index 50, a vCosParallax of two entries
  NONFINITE   5. a frame whose keys share their x (every score NaN) and one whose x spread leaves only some iterations finite
  batches     6. batch33(), empties(), exact_fit(), iteration_mix(), reorder(): lists of pairs for initialize_device"""
import numpy as np

import initializer_cases as IC
from initializer_cases import draws_for, pair_from, rot   # noqa: F401  (rot: the converging camera is written out below)

PASS = 256    # IN_T: keys of frame 1 per compaction pass; IN_STAGE: matches per LDS stage
MAXIT = 512   # ORBFE_INIT_MAX_ITERATIONS = ORBFE_INIT_TAP_ITERS


# ---- 1. compaction passes ---------------------------------------------------------------------------------------------------------------
def relayout(c, n1, pos1, n2=None, seed=0):
    """the pair c (made with extra1 = 0, so key i of frame 1 is match i) with its matched keys moved to the ascending positions
    pos1 of a first frame of n1 keys, the others unmatched at random places; n2 >= N pads the second frame behind its keys"""
    rng = np.random.default_rng(7000 + seed)
    pos1 = np.asarray(pos1, np.int64)
    N = len(c["keys1"])
    assert len(pos1) == N and (np.diff(pos1) > 0).all() and 0 <= pos1[0] and pos1[-1] < n1 and (c["matches12"] >= 0).all()
    k1 = rng.uniform([0, 0], [640, 480], (n1, 2)).astype(np.float32)
    k1[pos1] = c["keys1"]
    m = np.full(n1, -1, np.int32)
    m[pos1] = c["matches12"]
    X = np.zeros((n1, 3))
    X[pos1] = c["X"]
    k2 = c["keys2"]
    if n2 is not None:
        assert n2 >= len(k2)
        k2 = np.concatenate([k2, rng.uniform([0, 0], [640, 480], (n2 - len(k2), 2)).astype(np.float32)])
    return dict(c, keys1=k1, keys2=k2, matches12=m, X=X, matched=pos1)


def layout(n1, blocks, seed):
    """ascending positions in [0, n1) from a per-pass recipe: blocks[b] is 0 (no match), "all", "wave3" (keys 192 .. 255 of the
    pass), "last" (the frame's last key only) or a count of random keys of the pass"""
    rng = np.random.default_rng(7100 + seed)
    out = []
    assert len(blocks) == (n1 + PASS - 1) // PASS
    for b, what in enumerate(blocks):
        lo, hi = b * PASS, min(n1, (b + 1) * PASS)
        if isinstance(what, str):
            pos = {"all": np.arange(lo, hi), "wave3": np.arange(lo + 192, hi), "last": np.array([n1 - 1])}[what]
            assert len(pos) and lo <= pos[0]
        else:
            pos = lo + np.sort(rng.permutation(hi - lo)[:what])
        out.append(pos)
    return np.concatenate(out).astype(np.int64)


def passes(n1, blocks, n2, seed, iterations=24, kind="general"):
    pos1 = layout(n1, blocks, seed)
    N = len(pos1)
    c = pair_from(IC.points(kind, N, np.random.default_rng(seed)), IC.R_GEN, IC.T_GEN, seed=seed, iterations=iterations,
                  extra2=max(0, min(n2 - N, 5)))   # a few interleaved keys of frame 2, the rest behind
    return dict(relayout(c, n1, pos1, n2, seed), blocks=blocks)


# name -> constructor; the recipe (`blocks`) is the per-pass histogram of matched keys the case has to show
PASSES = {
    # (e) one pass, matches only in its wave 3; n2 < n1
    "p256_wave3": lambda: passes(256, ["wave3"], 71, 101),
    # (c) the last pass is key 256 alone and it is matched; n2 > n1
    "p257_last_key": lambda: passes(257, [100, "last"], 400, 102),
    # (d) the first pass has no match; n2 < n1
    "p512_first_empty": lambda: passes(512, [0, 150], 173, 103),
    # (b) pass 0 with every key matched, a one-key last pass that is matched; n2 > n1
    "p513_full_pass": lambda: passes(513, ["all", 40, "last"], 600, 104),
    # (a) pass 1 empty between matched passes, (b) pass 3 full, the one-key pass 4 unmatched; n2 < n1
    "p1025_middle_empty": lambda: passes(1025, [90, 0, 60, "all", 0], 450, 105),
    # the workload's size: (a) passes 1, 4, 6 empty, (e) pass 2 wave 3 only, (b) pass 3 full, (c) the last pass (208 keys) holds
    # only key 1999; n2 > n1
    "p2000_mixed": lambda: passes(2000, [120, 0, "wave3", "all", 0, 100, 0, "last"], 2100, 106, iterations=32),
}


def pass_histogram(c):
    """matched keys per 256-key pass of frame 1, and per 64-key wave"""
    m = c["matches12"] >= 0
    pad = np.zeros((-len(m)) % PASS, bool)
    w = np.concatenate([m, pad]).reshape(-1, 4, 64).sum(2)
    return w.sum(1), w


# ---- 2. LDS stages and the size ceiling -------------------------------------------------------------------------------------------------
STAGES = {
    "general_256": lambda: IC.general(256, 201, iterations=16, extra1=9, extra2=4),       # exactly one full stage
    "planar_512": lambda: IC.planar(512, 202, iterations=16, extra2=30),                   # exactly two
    "general_513": lambda: IC.general(513, 203, iterations=16, extra1=30),                 # two and one match
    "general_1000": lambda: IC.general(1000, 204, iterations=24, extra1=700, extra2=411),  # four stages, the last of 232
    "planar_1000": lambda: IC.planar(1000, 205, iterations=24, extra1=24, extra2=900),
    "general_4096": lambda: IC.general(4096, 206, iterations=64, extra2=37),               # n1 = N = the handle's maximum
}


# ---- 3. the iteration ceiling -----------------------------------------------------------------------------------------------------------
def last_wins(iterations, seed, base, target, N=60):
    """a noisy planar scene in which every iteration draws set `base` of a pool of 64 but the last, which draws set `target`:
    that one scores strictly higher in BOTH models and its H score lies above its F score (tie's trick; base and target were
    searched on the oracle).  So iterH = iterF = iterations - 1 and SH > SF: a record of model H that lands in model F's rows,
    or the other way round, changes a winner whichever of the two writes last"""
    c = IC.noisy("planar", N, seed, noise=0.8, outliers=0.15)
    pool = draws_for(64, 5000 + seed).reshape(64, 8)
    d = np.tile(pool[base], iterations)
    d[-8:] = pool[target]
    return dict(c, iterations=iterations, draws=d)


ITERATIONS = {
    "it448": lambda: last_wins(448, 301, 9, 4),     # seven full chunks of 64: the last lane of chunk 6
    "it449": lambda: last_wins(449, 302, 8, 5),     # lane 0 of chunk 7, alone in its workgroup
    "it511": lambda: last_wins(511, 303, 1, 11),    # lane 62 of chunk 7
    "it512": lambda: last_wins(512, 304, 17, 8),    # the last lane of the grid, the last record of the tap
}


# ---- 4. the parallax selection ----------------------------------------------------------------------------------------------------------
C2 = np.array([2.0, 0.0, 2.0])
R_CONV = np.array([[-1, 0, 1], [0, np.sqrt(2.0), 0], [-1, 0, -1]]) / np.sqrt(2.0)   # camera 2 looks along (-1, 0, -1) / sqrt 2
T_CONV = -R_CONV @ C2


def cluster(n, rng):
    """points within 0.25 of (1, 0, 1), between the two cameras: the rays meet at more than 90 degrees, cosParallax < 0"""
    return np.array([1.0, 0.0, 1.0]) + rng.uniform(-0.25, 0.25, (n, 3))


def column(n, rng, lo=2.0, hi=4.0):
    """points (1, d, 1) with some scatter in x and z: in front of both cameras, cosParallax about (d^2 - 2) / (d^2 + 2) > 0"""
    d = rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)
    return np.stack([1.0 + rng.uniform(-0.2, 0.2, n), d, 1.0 + rng.uniform(-0.2, 0.2, n)], 1)


def converging(X, seed, iterations=24, **kw):
    return pair_from(X, R_CONV, T_CONV, seed=seed, iterations=iterations, **kw)


def par_all_negative(seed=401):
    """(a) 120 points between the cameras: every accepted cosine is negative and so is the selected one"""
    return converging(cluster(120, np.random.default_rng(seed)), seed, extra1=6, extra2=11)


def par_split(negatives, seed, positives=30):
    """(b) / (c) `negatives` points between the cameras and 30 in the column: the sign changes inside the sorted list at index
    `negatives`, so 51 selects the largest negative and 50 the smallest non-negative cosine"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([cluster(negatives, rng), column(positives, rng)])
    return converging(X[rng.permutation(len(X))], seed, extra2=5)


def par_spread(seed=404):
    """(d) 40 cosines near -0.97, 70 from the column out to d = 40 (0.3 .. 0.997): the keys of the selection differ from their
    sign bit down, and index 50 lies among the positive ones"""
    rng = np.random.default_rng(seed)
    d = np.geomspace(2.0, 40.0, 70) * rng.choice([-1.0, 1.0], 70)
    col = np.stack([1.0 + rng.uniform(-0.2, 0.2, 70), d, 1.0 + rng.uniform(-0.2, 0.2, 70)], 1)
    X = np.concatenate([cluster(40, rng), col])
    return converging(X[rng.permutation(len(X))], seed, extra1=4)


def par_duplicates(seed=405):
    """(e) 45 points between the cameras, ONE column point under 11 different indices in both frames (the same coordinates, so
    the same triangulation and the same cosine bit for bit), 30 column points further out: the sorted list holds one bit pattern
    at the indices 45 .. 55"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([cluster(45, rng), np.tile([[1.05, 2.0, 0.95]], (11, 1)), column(30, rng, 2.6, 4.0)])
    return converging(X[rng.permutation(len(X))], seed, extra2=7)


def concat(cs, seed, iterations):
    """several pairs as one: the keys of both frames back to back, the matches shifted (pair_from's output concatenated)"""
    off2 = np.cumsum([0] + [len(c["keys2"]) for c in cs])
    m = np.concatenate([np.where(c["matches12"] >= 0, c["matches12"] + o, -1) for c, o in zip(cs, off2)]).astype(np.int32)
    return dict(cs[0], keys1=np.concatenate([c["keys1"] for c in cs]), keys2=np.concatenate([c["keys2"] for c in cs]), matches12=m,
                iterations=iterations, draws=draws_for(iterations, seed), X=np.concatenate([c["X"] for c in cs]),
                matched=np.nonzero(m >= 0)[0])


def par_two(seed=406):
    """(f) eight matches, two for each of the four (R, t) of DecomposeE.  Real points reach only three of them (in front of one
    camera only lands on one twisted hypothesis either way), so the pairs are projected through the four camera pairs that share
    the essential matrix: (R, t), (R, -t), (R', t), (R', -t) with R' = (2 t t^T / |t|^2 - I) R, each seeing its two points in
    front of both of ITS cameras.  Every hypothesis triangulates its own two in front: vCosParallax has two entries everywhere,
    the selection runs with k = 1, maxGood = 2 < 50 and Initialize fails."""
    rng = np.random.default_rng(seed)
    th = T_CONV / np.linalg.norm(T_CONV)
    R_tw = (2.0 * np.outer(th, th) - np.eye(3)) @ R_CONV
    parts = []
    for k, (R, t) in enumerate(((R_CONV, T_CONV), (R_CONV, -T_CONV), (R_tw, T_CONV), (R_tw, -T_CONV))):
        X = []
        for _ in range(20000):   # two points at depths of 0.5 to 8 in front of both cameras of this pair
            x = rng.uniform([-8.0, -2.0, 0.5], [8.0, 2.0, 8.0])
            if 0.5 < (R @ x + t)[2] < 8.0:
                X.append(x)
            if len(X) == 2:
                break
        assert len(X) == 2
        parts.append(pair_from(np.array(X), R, t, seed=seed + k, extra1=k % 2, extra2=1, shuffle=False))
    return concat(parts, seed, 8)


PARALLAX = {
    "all_negative": par_all_negative,
    "negatives_51": lambda: par_split(51, 402),
    "negatives_50": lambda: par_split(50, 403),
    "spread": par_spread,
    "duplicates": par_duplicates,
    "two_entries": par_two,
}


# ---- 5. non-finite scores ---------------------------------------------------------------------------------------------------------------
def same_x(N=40, seed=501):
    """(a) every key of frame 2 at x = 320: meanDev = 0, sX = inf, T2 and every model and score of both kinds NaN"""
    c = IC.general(N, seed, iterations=12, extra1=3, extra2=2)
    c["keys2"][:, 0] = 320.0
    return c


def partly_finite(N=40, seed=503, scale=1.96e36, offset2=20000.0):
    """(b) some iterations of BOTH models non-finite, a finite one wins each.  Shrinking the spread of frame 2's x alone does not
    get there: on the oracle every score stays finite down to a spread of 1e-38 (an overflowed entry gives an infinite chiSquare,
    which is an outlier and adds nothing) and all turn NaN together once sX overflows.  What does: the defect on frame 1 (x
    within 1e-36 of each other, s1X = 2e36, all keys still normal floats), frame 2's x moved out to 20000, a rolling and
    advancing camera and 30 % wrong matches, so that the models differ enough between iterations: where H21(0, 0) or F21's
    first column overflow, inf - inf and 0 * inf make that iteration's score NaN.  Scales and offsets searched on the oracle."""
    X = IC.points("general", N, np.random.default_rng(seed))
    c = pair_from(X, rot(0.05, -0.1, 0.6), np.array([0.3, 0.2, 0.8]), seed=seed, iterations=32, extra1=3, extra2=2)
    rng = np.random.default_rng(5)
    m = c["matches12"]
    first = np.nonzero(m >= 0)[0]
    k2 = c["keys2"].astype(np.float64)
    k2[m[first]] += rng.normal(0, 1.0, (len(first), 2))
    wrong = first[rng.random(len(first)) < 0.3]
    k2[m[wrong]] = rng.uniform([0, 0], [640, 480], (len(wrong), 2))
    c["keys2"] = k2.astype(np.float32)
    c["keys1"][:, 0] = ((c["keys1"][:, 0].astype(np.float64) + 680) / (160 * scale)).astype(np.float32)
    c["keys2"][:, 0] += np.float32(offset2)
    return c


NONFINITE = {"same_x": same_x, "partly_finite": partly_finite}


# ---- 6. the batch form ------------------------------------------------------------------------------------------------------------------
SMALL = {
    "g40": lambda: IC.general(40, 601, iterations=6, extra1=2, extra2=5),
    "p70": lambda: IC.planar(70, 602, iterations=9, extra2=3),
    "g64": lambda: IC.general(64, 603, iterations=5, extra1=7),
    "g63_it1": lambda: IC.general(63, 604, iterations=1, extra1=1),
    "g90_it1": lambda: IC.general(90, 605, iterations=1, extra2=4),
}
TAP_SETS = 32   # ORBFE_INIT_TAP_SETS


def empty_pair(n1, n2, seed=610):
    """a pair with no match: n1 keys all unmatched over n2 keys (either may be 0)"""
    rng = np.random.default_rng(seed)
    return dict(keys1=rng.uniform(0, 480, (n1, 2)).astype(np.float32), keys2=rng.uniform(0, 480, (n2, 2)).astype(np.float32),
                matches12=np.full(n1, -1, np.int32), K=IC.K0.copy(), sigma=1.0, iterations=4, draws=draws_for(4, seed))


def batch33():
    """(a) 33 pairs, three distinct ones in turn: pair 32 lies past ORBFE_INIT_TAP_SETS"""
    return [("SMALL", n) for n in ("g40", "p70", "g64")] * 11


def empties():
    """(b) a pair without keys in frame 1 and a pair of 6 unmatched keys over an EMPTY frame 2, each between good pairs"""
    return [("SMALL", "g40"), ("EMPTY", "n1_0"), ("SMALL", "p70"), ("EMPTY", "n2_0"), ("SMALL", "g64")]


def exact_fit():
    """(c) three pairs; the handle is made for exactly their keys, then for one fewer"""
    return [("SMALL", "g64"), ("PASSES", "p257_last_key"), ("SMALL", "p70")]


def iteration_mix():
    """(d) 1, 512, 1 and 512 iterations side by side"""
    return [("SMALL", "g63_it1"), ("ITERATIONS", "it512"), ("SMALL", "g90_it1"), ("ITERATIONS", "it512")]


def reorder():
    """(e) one batch in two orders on one handle: slot 0 holds 512 iterations and then 5, slot 1 N = 1000 and then 60, slot 2
    N = 64 and then 512 matches over two stages; every later pair is smaller in what its slot's scratch still holds"""
    first = [("ITERATIONS", "it512"), ("STAGES", "general_1000"), ("SMALL", "g64"), ("STAGES", "planar_512")]
    second = [("SMALL", "g64"), ("ITERATIONS", "it512"), ("STAGES", "planar_512"), ("STAGES", "general_1000")]
    return first, second


EMPTY = {"n1_0": lambda: empty_pair(0, 5), "n2_0": lambda: empty_pair(6, 0, 611)}
TABLES = dict(PASSES=PASSES, STAGES=STAGES, ITERATIONS=ITERATIONS, PARALLAX=PARALLAX, NONFINITE=NONFINITE, SMALL=SMALL, EMPTY=EMPTY)

_cache, _answers = {}, {}


def case(table, name):
    if (table, name) not in _cache:
        _cache[table, name] = TABLES[table][name]()
    return _cache[table, name]


def run(c, tap_iteration=0, tap_hypothesis=0):
    import initializer_oracle as IO
    return IO.initialize(c["keys1"], c["keys2"], c["matches12"], c["K"], c["sigma"], c["iterations"], c["draws"], tap_iteration,
                         tap_hypothesis)


def answer(table, name, tap_iteration=0, tap_hypothesis=0):
    """the oracle's answer for a case, computed once per (case, taps) and shared"""
    key = (table, name, tap_iteration, tap_hypothesis)
    if key not in _answers:
        _answers[key] = run(case(table, name), tap_iteration, tap_hypothesis)
    return _answers[key]
