"""Inputs of the DynaSLAM::Geometry tests (tests/test_geometry_oracle.py on the CPU, tests/test_gpu_geometry*.py on the device):
poses, the box-on-a-plane scene, single-reference scenes whose one point sits at an edge of ExtractDynPoints, the hand-worked
region-growing planes and the seed lists of DepthRegionGrowing.  Everything is deterministic; nothing here calls the library."""
import functools

import numpy as np

import geometry_oracle as GO

F = np.float32


def pose(rx=0., ry=0., rz=0., tx=0., ty=0., tz=0.):
    """mTcw, 4x4 float32: R = Rz Ry Rx, t"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (tx, ty, tz)
    return T.astype(F)


def key_poses(n, seed=7, rot=0.02, trans=0.08):
    """n distinct key-frame poses: small rotations about all three axes, translations of a few centimetres"""
    rng = np.random.RandomState(seed)
    return [pose(*(rng.uniform(-rot, rot, 3)), *(rng.uniform(-trans, trans, 3))) for _ in range(n)]


def lattice(w, h, nx, ny, seed, margin=4.0):
    """nx * ny keypoints on a jittered lattice, (x, y) float32, row by row"""
    rng = np.random.RandomState(seed)
    xs = np.linspace(margin, w - 1 - margin, nx)
    ys = np.linspace(margin, h - 1 - margin, ny)
    xy = np.array([(x, y) for y in ys for x in xs]) + rng.uniform(-1.5, 1.5, (nx * ny, 2))
    return xy.astype(F)


def intrinsics(w, h):
    return float(0.75 * w), float(0.75 * w), float(w / 2), float(h / 2)


@functools.lru_cache(maxsize=None)
def box_scene(w=160, h=120, box=(48, 32, 64, 56), nkf=6, grid=(14, 10), seed=0):
    """A plane at 3 m in every key frame; the current frame sees the same plane with a box at 1.5 m in front of it.
    dict(K, key_frames [dict(Tcw, depth, keys, keys_un)], cur_T, cur_depth, box)"""
    frames = []
    for i, T in enumerate(key_poses(nkf, seed + 7)):
        keys = lattice(w, h, grid[0], grid[1], seed + 100 + i)
        frames.append(dict(Tcw=T, depth=np.full((h, w), 3.0, F), keys=keys, keys_un=keys + F(0.25)))
    cur_depth = np.full((h, w), 3.0, F)
    x0, y0, bw, bh = box
    cur_depth[y0:y0 + bh, x0:x0 + bw] = 1.5
    return dict(K=intrinsics(w, h), key_frames=frames, cur_T=pose(0.004, -0.006, 0.003, 0.01, -0.02, 0.015), cur_depth=cur_depth, box=box)


def box_union(w, h, box):
    """what RegionGrowing leaves for any seed inside the box: the box and its 4-neighbour border"""
    x0, y0, bw, bh = box
    u = np.zeros((h, w), np.uint8)
    u[y0:y0 + bh, x0:x0 + bw] = 1
    u[y0 - 1, x0:x0 + bw] = u[y0 + bh, x0:x0 + bw] = 1
    u[y0:y0 + bh, x0 - 1] = u[y0:y0 + bh, x0 + bw] = 1
    return u


def oracle_run(scene, nkf=None):
    """the oracle over a scene: (mask, computed, taps)"""
    g = GO.Geometry()
    for f in scene["key_frames"][:nkf]:
        g.update_db(f["Tcw"], f["depth"], f["keys"], f["keys_un"])
    mask, done = g.correct(scene["cur_depth"], scene["cur_T"], *scene["K"])
    return mask, done, g.taps


# ---- scenes with one active reference -------------------------------------------------------------------------------------------------
W1, H1 = 96, 80
K1 = intrinsics(W1, H1)
ACTIVE_T = pose(0.011, -0.007, 0.005, 0.03, -0.02, 0.04)


def single_ref_scene(keys, kf_depth, cur_depth, cur_T=None, keys_un=None, rank=4, active_T=ACTIVE_T):
    """Five key frames of which only one has keypoints; `rank` is its place in GetRefFrames' order (4 = last: with cur_T None the
    current pose is its pose moved by 2 mm, so it scores lowest).  The other four have no keypoints: references without a
    survivor."""
    keys = np.asarray(keys, F).reshape(-1, 2)
    others = key_poses(4, 31, rot=0.03, trans=0.3)
    if cur_T is None:
        cur_T = active_T.copy()
        cur_T[0, 3] += F(0.002)
    poses = others + [active_T]
    order = GO.select_ref_frames(cur_T, poses)
    at = order.index(4)
    if rank is not None and at != rank:
        raise AssertionError(f"the active frame ranks {at}, not {rank}: pick another pose")
    none = np.zeros((0, 2), F)
    frames = [dict(Tcw=T, depth=np.full((H1, W1), 3.0, F), keys=none, keys_un=none) for T in others]
    frames.append(dict(Tcw=active_T, depth=np.asarray(kf_depth, F), keys=keys, keys_un=keys if keys_un is None else np.asarray(keys_un, F)))
    return dict(K=K1, key_frames=frames, cur_T=cur_T, cur_depth=np.asarray(cur_depth, F))


def plane(v, w=W1, h=H1):
    return np.full((h, w), v, F)


def window_scene(n_near, near=2.3, bg=3.01, at=(48.5, 40.5)):
    """one keypoint of depth 3 re-projected by its own pose (proj = 3 up to rounding) into a plane of `bg` (not below proj) with
    n_near pixels of `near` in its 41x41 window, at distinct offsets: diff = 0.7 > 0.6, variance = n (bg - near)^2 / 1681 nearly"""
    cur = plane(bg)
    cx, cy = int(np.ceil(at[0])), int(np.ceil(at[1]))
    for i in range(n_near):
        cur[cy + 3 + 2 * i, cx - 5 + 3 * i] = near
    return single_ref_scene([at], plane(3.0), cur)


def count_scene(n):
    """n keypoints that all survive every gate of ExtractDynPoints up to the search (the gemm shape depends on n)"""
    keys = [(30.5 + 7 * (i % 6), 28.5 + 9 * (i // 6)) for i in range(n)]
    return single_ref_scene(keys, plane(3.0), plane(2.3))


# ---- RegionGrowing, hand-worked -----------------------------------------------------------------------------------------------------
def plane9(spots=()):
    im = np.full((9, 9), 5.0, F)
    for x, y in spots:
        im[y, x] = 1.0
    return im


def embed(im9, w=47, h=45, x0=20, y0=18):
    """a 9x9 hand-worked plane inside a w x h plane of 5.0 (the library takes no plane smaller than 45 x 45)"""
    im = np.full((h, w), 5.0, F)
    im[y0:y0 + 9, x0:x0 + 9] = im9
    return im, x0, y0


def staircase(w=64, h=48):
    """plateaus of 1.0 (wide), 1.15 (narrow) and 1.3 side by side in a plane of 9: a seed on the wide one stops before the third
    (its mean stays near 1.0), a seed on the narrow one drifts into the third.  Seeds A on the wide plateau, B on the narrow one."""
    im = np.full((h, w), 9.0, F)
    im[10:38, 6:34] = 1.0
    im[10:38, 34:37] = 1.15
    im[10:38, 37:52] = 1.3
    return im, (12, 20), (35, 20)


def seed_grid(n, w=64, h=48):
    """n seeds on separate 1-pixel islands of depth 2 in a plane of 9 (each grows to its island and the 4 neighbours)"""
    im = np.full((h, w), 9.0, F)
    seeds = []
    for i in range(n):
        x, y = 3 + 4 * (i % 15), 3 + 4 * (i // 15)
        im[y, x] = 2.0
        seeds.append((x, y))
    return im, seeds


GRID12 = [(30.5 + 7 * (i % 6), 28.5 + 9 * (i // 6)) for i in range(12)]
# the active reference's place in GetRefFrames' order -> (its pose, the current pose): the four empty references take the others
RANK_POSES = {
    0: (pose(0.011, -0.007, 0.005, 0.03, -0.02, 0.5), pose(-0.01, 0.02, 0., 0., 0., -0.2)),
    2: (pose(0.011, -0.007, 0.005, 0.03, -0.02, 0.5), pose(0., 0.01, 0., 0., 0., 0.)),
    1: (ACTIVE_T, pose(0., 0.01, 0., 0., 0., -0.4)),
    3: (ACTIVE_T, pose(0., 0.01, 0., -0.3, 0., 0.)),
    4: (ACTIVE_T, pose(0., 0.01, 0., 0.3, 0., 0.)),
}


def rank_scene(rank):
    """twelve keypoints in the reference GetRefFrames puts at `rank`; the current plane is near enough for every one to be dynamic"""
    active_T, cur_T = RANK_POSES[rank]
    return single_ref_scene(GRID12, plane(3.0), plane(1.5), cur_T=cur_T, rank=rank, active_T=active_T)


def nan_scene():
    """the current translation equals the reference's: both rays are the same vector, and the ratio dot / (|a| |a|) lands a
    rounding above 1 for some points (acos: NaN, the point is dropped) and at or below 1 for others (angle 0, kept)"""
    keys = GRID12 + [(48.5, 40.5), (52.25, 33.75), (61.5, 47.0), (40.75, 52.5)]
    return single_ref_scene(keys, plane(3.0), plane(2.3), cur_T=ACTIVE_T)


def parallax_scene():
    """translation columns of +1.2 m (reference) and -1.2 m (current): the angle between (mp - tRef) and (mp - tCur) runs from
    about 22 degrees at one side of the image to about 43 in the middle"""
    active_T = pose(0.011, -0.007, 0.005, 1.2, -0.02, 0.04)
    keys = [(6.5 + 8 * i, 20.5 + 13 * j) for j in range(4) for i in range(11)]
    return single_ref_scene(keys, plane(3.0), plane(2.3), cur_T=pose(0., 0.01, 0., -1.2, 0., 0.), rank=None, active_T=active_T)


def flip_depth(fn, lo, hi):
    """adjacent float32 (a, b), lo <= a < b <= hi, with fn(a) true and fn(b) false (fn true at lo, false at hi), by bisection"""
    lo, hi = F(lo), F(hi)
    assert fn(lo) and not fn(hi)
    while np.nextafter(lo, F(np.inf)) < hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        if fn(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def depth7_scene():
    """the current camera 1.5 m further back: two keypoints whose reference depths are adjacent floats, one projecting to a depth
    just below 7 and one to 7 or just above (found with the oracle's own arithmetic)"""
    cur_T = ACTIVE_T.copy()
    cur_T[2, 3] += F(1.5)
    cur_T[0, 3] += F(0.002)
    Kinv = GO.geo_inv3(GO.geo_make_K(*K1))
    lu = GO.LU4(ACTIVE_T)
    at = (48.5, 40.5)

    def below7(d):
        return bool(GO.geo_to_current(cur_T, lu.solve(GO.geo_backproject(Kinv, at[0], at[1], d)))[2] < 7)

    a, b = flip_depth(below7, 5.0, 5.9)
    kf = plane(3.0)
    keys = [(20.5, 30.5), (60.5, 30.5)]
    kf[30, 20], kf[30, 60] = a, b
    sc = single_ref_scene(keys, kf, plane(2.3), cur_T=cur_T, keys_un=[at, at], rank=None)
    sc["flip"] = (a, b)
    return sc
