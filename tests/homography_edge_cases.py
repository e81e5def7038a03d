"""Edge cases for cv::findHomography (tests/homography_oracle.py, csrc/orbfe_homography.hip) beside homography_cases.table():
point sets that walk the Levenberg-Marquardt state machine of k_homo_refine (all three R bands, lambda zeroed and kept, the
lambda == 0 inversion with iterations after it, both nu clamps and the open interval, rejected steps, all three exits) and
the partition boundaries of k_homo_ransac (the 32-iteration chunk, the 256-lane stride, max_iters and threshold defaults, a
subset draw that fails after the first iteration).  Each case is (src, dst, kwargs) as in homography_cases; every set has at
most 300 pairs and runs at most 65 RANSAC iterations, so the oracle takes well under a second per case.

Method 0 (the DLT over all points) with a few outliers gives LM a start far from its optimum; the seeds were found by a
bounded search over small planar(..., method=0) sets with the oracle's trace (tests/test_homography_edge_cases.py holds the
census that keeps them honest).  Two findings of that search:
  * the ||r||inf exit is not reachable from pixel-sized coordinates without an exit on ||d||inf first: a DLT start on pairs
    that an H fits to 1e-7 px is itself that good.  It is reached, and proven, by coordinates scaled by 2^-24: every residual
    is then below FLT_EPSILON whatever the noise, while the step on h6 / h7 (units 1 / coordinate) is large;
  * a subset draw can fail after iteration 0 (mostly_one_point below), so k_homo_ransac's `sIdx[h][0] < 0` at it > 0 is
    reachable."""
import numpy as np

import homography_cases as HC

MAX_PAIRS = 300
MAX_RANSAC_ITERS = 65
CHUNK_EDGE_ITERS = (1, 31, 32, 33, 64, 65, 0, -3)   # max_iters around k_homo_ransac's HO_K = 32; <= 0 means 1
TINY = np.float32(2.0 ** -24)


def identity_pixels(n=50, seed=3):
    """src == dst on integer pixels: every subset fits exactly, RANSACUpdateNumIters returns 0 at iteration 0"""
    s, _, _ = HC.planar(n, 1.0, seed, noise=0.0, subpixel=False)
    return s, s.copy()


def duplicated_block(n=60, ratio=0.8, seed=4):
    """ten pairs equal pair 0: subsets that draw two of them are rejected by haveCollinearPoints"""
    s, d, _ = HC.planar(n, ratio, seed)
    s[10:20] = s[0]
    d[10:20] = d[0]
    return s, d


def mostly_one_point(n=264, k=6, seed=1200):
    """pairs k.. all equal pair k, pairs 1, 3, 5 of the first k aimed anywhere: a subset passes haveCollinearPoints only when
    it holds four different locations, about 1e-4 of all draws, so a 10000-attempt getSubset fails about every other time.
    With n = 264 the draw of iteration 0 succeeds (niters becomes 2) and the draw of iteration 1 fails."""
    s, d, _ = HC.planar(n, 1.0, seed, noise=0.0)
    s[k:] = s[k]
    d[k:] = d[k]
    rng = np.random.default_rng(seed)
    d[1:k:2] = (rng.random((len(d[1:k:2]), 2)) * [640, 480]).astype(np.float32)
    return s, d


def table():
    """name -> (src, dst, kwargs for find_homography)"""
    c = {}
    m0 = dict(method=0)

    def planar(name, n, ratio, seed, noise, kw):
        s, d, _ = HC.planar(n, ratio, seed, noise=noise)
        c[name] = (s, d, dict(kw))

    # ---- LM: method 0 over sets with a few outliers
    planar("lm_ten_iterations", 40, 0.9, 500, 0.5, m0)        # 10 iterations; lambda kept 4x, zeroed 3x; 3 inversions with nu > 10
    planar("lm_nu_between", 12, 0.75, 503, 0.2, m0)           # 2 < nu < 10 before an inversion, lc read afterwards
    planar("lm_tenth_step_a", 40, 0.8, 501, 1.0, m0)          # the 10th iteration still moves H
    planar("lm_tenth_step_b", 60, 0.7, 502, 0.3, m0)
    planar("lm_mid_band_last", 100, 0.95, 504, 2.0, m0)       # 0.25 <= R <= 0.75 at iteration 9 (H does not depend on it)
    planar("lm_mid_band", 12, 0.75, 601, 0.5, m0)             # 0.25 <= R <= 0.75 where treating it as R < 0.25 changes H
    planar("lm_clamp2_after_reject", 8, 0.95, 635, 2.0, m0)   # nu clamped at 2 in the iteration after a rejected step
    s, d, _ = HC.planar(40, 1.0, 900, noise=0.3)
    c["lm_residual_exit"] = (s * TINY, d * TINY, dict(m0))    # leaves on ||r||inf with ||d||inf large
    c["lm_residual_exit_ransac"] = (s * TINY, d * TINY, {})
    c["identity_pixels"] = identity_pixels() + ({},)
    c["identity_pixels_method_0"] = identity_pixels() + (dict(m0),)
    # ---- RANSAC: the 32-iteration chunk, max_iters <= 0, threshold <= 0
    s, d, _ = HC.planar(300, 0.1, 7)
    for mi in CHUNK_EDGE_ITERS:
        c[f"max_iters_{mi}"] = (s, d, dict(max_iters=mi))
    s, d, _ = HC.planar(150, 0.7, 21)
    c["threshold_3.0"] = (s, d, {})
    c["threshold_0.0"] = (s, d, dict(threshold=0.0))
    c["threshold_-1.0"] = (s, d, dict(threshold=-1.0))
    # ---- the 256-lane stride of k_homo_ransac; n = 256 also has niters fall below the loop counter at an update
    for n in (255, 256, 257):
        s, d, _ = HC.planar(n, 0.6, 800 + n)
        c[f"n_{n}"] = (s, d, {})
    # ---- subset draws
    c["duplicated_block"] = duplicated_block() + ({},)
    c["subset_fails_at_1"] = mostly_one_point() + ({},)
    return c


def groups(cases):
    """the cases by kwargs, for one find_batch call per group: [(kwargs, [names])]"""
    out = {}
    for name, (_, _, kw) in cases.items():
        out.setdefault(tuple(sorted(kw.items())), []).append(name)
    return [(dict(k), names) for k, names in out.items()]
