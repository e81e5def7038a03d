"""Seeded inputs for the point-cloud map tests (tests/test_cloud_oracle.py, tests/test_gpu_cloud.py)."""
import numpy as np

import cloud_oracle as CO

F = np.float32


def pose_tcw(seed):
    """a float32 Tcw: a rotation of a fraction of a radian about a random axis, a translation of a metre or so"""
    rng = np.random.default_rng(1000 + seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(-0.8, 0.8)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(-1.5, 1.5, 3)
    return T.astype(F)


def intrinsics(w, h, seed):
    rng = np.random.default_rng(2000 + seed)
    f = F(w * rng.uniform(0.8, 1.1))
    return np.array([f, f * F(rng.uniform(0.98, 1.02)), F(w / 2 - 0.5 + rng.uniform(-2, 2)), F(h / 2 - 0.5 + rng.uniform(-2, 2))], F)


SPECIALS = (np.nan, np.inf, 0.0, 3e38)   # 3e38: d is finite, x = (c - cx) * d is not


def frame(w, h, seed, kind="mixed"):
    """-> (depth float32 [h, w], bgr uint8 [h, w, 3], K float32 [4], T float64 [4, 4]).  kind: "mixed" (depths of 0.3 .. 7 m,
    a tenth of them 0, the four special values at pixels 63, 64, 255, 256 and the last one), "clean" (no invalid point) or
    "invalid" (every point dropped: NaN and infinities, 3e38 in the four corners)."""
    rng = np.random.default_rng(seed)
    n = w * h
    d = rng.uniform(0.3, 7.0, n).astype(F)
    if kind == "mixed":
        d[rng.random(n) < 0.1] = 0
        for k, p in enumerate((63, 64, 255, 256, n - 1)):
            if p < n:
                d[p] = F(SPECIALS[(k + seed) % 4])
        for k, p in enumerate((62, 65, 254, 257)):   # and each special value somewhere near a wave / workgroup edge
            if p < n:
                d[p] = F(SPECIALS[(k + 1 + seed) % 4])
    elif kind == "invalid":
        d[:] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), n)
        d[[0, w - 1, n - w, n - 1]] = F(3e38)   # only in the corners: next to the principal point (c - cx) * 3e38 stays finite
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    K = intrinsics(w, h, seed)
    T = CO.pose_matrix(pose_tcw(seed))
    return d.reshape(h, w), bgr, K, T


def random_cloud(n, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(3000 + seed)
    xyz = rng.uniform(lo, hi, (n, 3)).astype(F)
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return CO.records(xyz, rgba)


def one_voxel_cloud(n, seed, white=False):
    """n points inside the voxel [0.05, 0.1)^3 of a 0.05 grid, plus one point at the origin so that min_b is 0"""
    rng = np.random.default_rng(4000 + seed)
    xyz = rng.uniform(0.055, 0.095, (n, 3)).astype(F)
    rgba = np.full(n, 0xffffffff, np.uint32) if white else rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    pts = CO.records(xyz, rgba)
    return np.concatenate([CO.records(np.zeros((1, 3), F), np.array([0xff102030], np.uint32)), pts])


def paint_frame(w, h, seed):
    """depth with an object at about 2 m in front of a background at 3 .. 5 m, a few zeros"""
    rng = np.random.default_rng(5000 + seed)
    d = rng.uniform(3.0, 5.0, (h, w)).astype(F)
    d[h // 4:3 * h // 4, w // 4:3 * w // 4] = rng.uniform(1.7, 2.5, (3 * h // 4 - h // 4, 3 * w // 4 - w // 4)).astype(F)
    d[rng.random((h, w)) < 0.05] = 0
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return d, bgr
