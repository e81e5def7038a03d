"""Point-pair cases for cv::findHomography (tests/homography_oracle.py, csrc/orbfe_homography.hip): planar pairs with a
chosen inlier ratio, noise and size, and the degenerate sets.  Each case is (src, dst, kwargs) with src = points_current,
dst = points_last, dst ~ H * src."""
import numpy as np

RANSAC = 8
H_TRUE = np.array([[1.03, 0.02, 12.5], [-0.015, 0.98, -7.25], [2.0e-5, -3.0e-5, 1.0]])


def planar(n, ratio, seed, H=H_TRUE, noise=0.3, w=640, h=480, subpixel=True):
    """n pairs, round(n * ratio) of them on H (with Gaussian noise of `noise` px), the rest uniform outliers; returns
    (src, dst, inlier mask as built)"""
    rng = np.random.default_rng(seed)
    src = rng.random((n, 2)) * [w, h]
    if not subpixel:
        src = np.round(src)
    p = np.c_[src, np.ones(n)] @ np.asarray(H, np.float64).T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0, noise, (n, 2)) * (noise > 0)
    inl = np.zeros(n, bool)
    inl[rng.permutation(n)[:int(round(n * ratio))]] = True
    dst[~inl] = rng.random((int((~inl).sum()), 2)) * [w, h]
    return src.astype(np.float32), dst.astype(np.float32), inl


def threshold_boundary(n_in=150, n_out=300, seed=77, rounds=4):
    """inliers on H_TRUE plus points re-aimed, round after round, at distance 3 px from the prediction of the oracle's RANSAC
    model: their float computeError sits at (float)(3*3) within rounding, so float and double errors give different masks"""
    import homography_oracle as HO
    rng = np.random.default_rng(seed)
    src = rng.random((n_in + n_out, 2)) * [640, 480]
    p = np.c_[src, np.ones(len(src))] @ H_TRUE.T
    aim = p[:, :2] / p[:, 2:]
    th = rng.random(n_out) * 2 * np.pi
    off = 3.0 * np.c_[np.cos(th), np.sin(th)]
    s, d = src.astype(np.float32), aim.astype(np.float32)
    for _ in range(rounds):
        d[n_in:] = (aim[n_in:] + off).astype(np.float32)
        h = HO.ransac(s, d)["H"]
        M = s.astype(np.float64)
        ww = 1 / (h[6] * M[:, 0] + h[7] * M[:, 1] + 1)
        aim = np.c_[(h[0] * M[:, 0] + h[1] * M[:, 1] + h[2]) * ww, (h[3] * M[:, 0] + h[4] * M[:, 1] + h[5]) * ww]
    return s, d


def table(max_pairs):
    """name -> (src, dst, kwargs for find_homography)"""
    c = {}
    for r in (1.0, 0.8, 0.5, 0.25, 0.1):
        s, d, _ = planar(200, r, int(r * 100))
        c[f"ratio_{r}"] = (s, d, {})
    for n in (4, 5, 51, 500, max_pairs):
        s, d, _ = planar(n, 0.7 if n > 5 else 1.0, 1000 + n)
        c[f"n_{n}"] = (s, d, {})
    s, d, _ = planar(300, 0.3, 7)
    c["max_iters_5"] = (s, d, dict(max_iters=5))
    for t in (1.0, 10.0):
        c[f"threshold_{t}"] = (s, d, dict(threshold=t))
    for cf in (0.99, 0.999):
        c[f"confidence_{cf}"] = (s, d, dict(confidence=cf))
    s, d, _ = planar(120, 1.0, 8, noise=0.8)
    c["method_0"] = (s, d, dict(method=0))
    s, d, _ = planar(6, 1.0, 9, noise=0.5)
    c["method_0_n6"] = (s, d, dict(method=0))
    x = np.arange(10, 610, 16, dtype=np.float32)   # exactly on y = x / 2 + 20: every cross product is 0
    line = np.c_[x, 0.5 * x + 20].astype(np.float32)
    c["collinear"] = (line, (line * 1.1).astype(np.float32), {})
    s, d, _ = planar(30, 0.9, 10)
    c["duplicated"] = (np.r_[s, s, s[:10]], np.r_[d, d, d[:10]], {})
    zs = s.copy()
    zs[:, 0] = 100.0
    c["zero_spread_method_0"] = (zs, d, dict(method=0))
    c["zero_spread_n4"] = (zs[:4], d[:4], {})
    s, d, _ = planar(150, 0.75, 11, noise=0.05)
    c["subpixel"] = ((s / 7).astype(np.float32), (d / 7).astype(np.float32), dict(threshold=0.5))
    c["threshold_boundary"] = threshold_boundary() + ({},)
    s, d, _ = planar(3, 1.0, 12)
    c["n_3"] = (s, d, {})
    c["n_0"] = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), {})
    return c
