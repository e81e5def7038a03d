"""Seeded inputs for the point-cloud map at its real-size seams (tests/test_cloud_objects_edge_cases.py checks on the CPU that every
case reaches its seam, tests/test_gpu_cloud_edges.py runs them on the device).  The seam is derived, not chosen: k_cloud_scan
walks its input 1024 entries at a time, one entry is one workgroup of 256 items, so the scan's carry and k_cloud_minmax's second
grid-stride trip both begin at item 1024 * 256 = 262 144.  Numpy only.  Test support only."""
import numpy as np

import cloud_cases as CC
import cloud_oracle as CO

F = np.float32
WG = 256                    # CL_T
SCAN = 1024                 # CL_SCAN_T: entries the scan takes per chunk; also the most workgroups k_cloud_minmax launches
SEAM = SCAN * WG            # 262 144


def blocks_of(n):
    return (n + WG - 1) // WG


# ---- the ordered compaction as the kernels do it (count per workgroup, exclusive scan, offset + rank) -----------------------------
def block_counts(flags):
    """kept items of every workgroup of 256 over one flag array"""
    f = np.asarray(flags, bool)
    pad = np.zeros(blocks_of(len(f)) * WG, bool)
    pad[:len(f)] = f
    return pad.reshape(-1, WG).sum(1).astype(np.int64)


def exclusive_scan(counts, reset_at=None):
    """the scan of the workgroup counts; reset_at = an entry at which a broken scan would lose its carry"""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(len(counts), np.int64)
    carry = 0
    for a in range(0, len(counts), SCAN):
        if reset_at is not None and a == reset_at:
            carry = 0
        c = counts[a:a + SCAN]
        out[a:a + SCAN] = carry + np.cumsum(c) - c
        carry += int(c.sum())
    return out


def placement(flag_segments, reset_at=None):
    """where every kept item is written: flag_segments = one flag array per keyframe (each starts a new workgroup), or one array.
    -> int64 [kept]"""
    segs = flag_segments if isinstance(flag_segments, (list, tuple)) else [flag_segments]
    counts = np.concatenate([block_counts(s) for s in segs])
    offs = exclusive_scan(counts, reset_at)
    out, e = [], 0
    for s in segs:
        f = np.asarray(s, bool)
        for b in range(blocks_of(len(f))):
            k = int(f[b * WG:(b + 1) * WG].sum())
            out.append(offs[e] + np.arange(k))
            e += 1
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def kept_flags(frame):
    """the pixels of a frame that generate_point_cloud keeps (a point finite after the transform)"""
    import objects_oracle as OO
    c = OO.organised_cloud(*frame)
    return np.isfinite(c["x"]) & np.isfinite(c["y"]) & np.isfinite(c["z"])


# ---- A1, A2: frames -----------------------------------------------------------------------------------------------------------------
BIG_W, BIG_H = 512, 513     # 262 656 pixels, 1026 workgroups


def holes(frame, seed, p):
    """the frame with a fraction p of its depths NaN, so that the workgroup counts differ from one another"""
    d, bgr, K, T = frame
    rng = np.random.default_rng(8000 + seed)
    d = d.copy()
    d[rng.random(d.shape) < p] = np.nan
    return d, bgr, K, T


def big_frame(kind):
    """"mixed": cloud_cases.frame as it is (seed 61: the last pixel is dropped, so the last workgroup holds 255).  "rows": runs of
    whole rows invalid (a row is two workgroups: counts of 0 and 256) and a third of the last three rows' pixels NaN (the counts of
    entries 1020 .. 1025 all differ)"""
    f = CC.frame(BIG_W, BIG_H, 61)
    if kind == "mixed":
        return f
    d = f[0].copy()
    for a, b in ((0, 3), (100, 137), (255, 256), (400, 431), (505, 508)):
        d[a:b] = np.nan
    rng = np.random.default_rng(8100)
    tail = d[BIG_H - 3:]
    tail[rng.random(tail.shape) < 1 / 3] = np.inf
    return d, f[1], f[2], f[3]


# (w, h, frames): blocks_of(w * h) * frames entries in the scan
STRADDLE = (352, 256, 3)                    # 352 workgroups each, 1056 entries: the third keyframe's segment straddles entry 1024
BATCH_TOTALS = {1023: (343, 254, 3),        # 87 122 pixels, 341 workgroups each
                1024: (257, 255, 4),        # 65 535 pixels, 256 each: the scan's input ends with its first chunk
                1025: (229, 229, 5),        # 52 441 pixels, 205 each: one entry in the second chunk
                2049: (418, 418, 3)}        # 174 724 pixels, 683 each: one entry in the third chunk


def batch(w, h, B, seed):
    return [holes(CC.frame(w, h, seed + b), seed + b, 0.2) for b in range(B)]


# ---- A3, A4: clouds ------------------------------------------------------------------------------------------------------------------
VOXEL_N = SEAM + WG         # 262 400 points: the sorted positions fill 1025 workgroups of k_cloud_heads


def voxel_cloud(not_finite=False):
    """cloud_cases.random_cloud in [0, 1)^3 with the last point in the corner (1, 1, 1): a voxel of its own with the largest key, so
    the last workgroup of k_cloud_heads, entry 1024 of the scan, holds a head at either leaf (8001 voxels at 0.05, 65 at 0.25)"""
    pts = CC.random_cloud(VOXEL_N, 70)
    pts["x"][-1] = pts["y"][-1] = pts["z"][-1] = 1.0
    if not_finite:          # about 50 records on both sides of position 262 144: the 32-bit sort path, nfin still above the seam
        rng = np.random.default_rng(8200)
        at = np.unique(np.r_[rng.integers(0, SEAM, 24), rng.integers(SEAM, VOXEL_N - 1, 24), [SEAM - 1, SEAM, VOXEL_N - 2]])
        for k, i in enumerate(at):
            pts["xyz"[k % 3]][i] = (np.nan, np.inf, -np.inf)[k % 3]
    return pts


def head_flags(pts, leaf):
    """over the sorted finite points: the first of every voxel (what k_cloud_heads compacts)"""
    idx = CO.voxel_keys(pts, CO.voxel_plan(pts, leaf))
    keys = np.sort(idx[idx >= 0])
    return np.r_[True, keys[1:] != keys[:-1]]


def bounds(pts):
    """getMinMax3D over the finite points -> (min float32 [3], max float32 [3], how many)"""
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
    fin = np.isfinite(xyz).all(1)
    return xyz[fin].min(0), xyz[fin].max(0), int(fin.sum())


EXTREMES = ((0, -0.35), (0, 1.3), (1, -0.2), (1, 1.15), (2, 0.02), (2, 1.4))   # axis, value: min and max per axis, outside [0.1, 0.9]
TAIL = 300


def second_trip_cloud(mirror=False):
    """262 144 points strictly inside [0.1, 0.9]^3, then 300 more.  mirror = False: six of the 300 hold the six extremes (in both
    workgroups of the second trip) and two are not finite.  mirror = True: the extremes sit in the first 256 items instead"""
    rng = np.random.default_rng(8300)
    xyz = rng.uniform(0.1, 0.9, (SEAM + TAIL, 3)).astype(F)
    rgba = rng.integers(0, 2 ** 32, SEAM + TAIL, dtype=np.uint64).astype(np.uint32)
    where = (7, 70, 133, 200, 260, 299)       # 260 and 299 fall into the second workgroup of the trip
    base = 3 if mirror else SEAM
    for (ax, v), p in zip(EXTREMES, where):
        xyz[base + (p if not mirror else p % 250), ax] = F(v)
    xyz[SEAM + 50, 1] = np.nan
    xyz[SEAM + 280, 2] = np.inf
    return CO.records(xyz, rgba)


# ---- A5, B: inserts ------------------------------------------------------------------------------------------------------------------
INSERT_LEAF = 0.25          # a few thousand voxels: the oracle's per-voxel loop stays short


def big_inserts():
    return [[CC.frame(BIG_W, BIG_H, 63)], [CC.frame(BIG_W, BIG_H, 65)]]


OVERFLOW_LEAF = 1e-4        # ten metres of depth are 10^5 cells an axis: dx * dy * dz > INT_MAX


def overflow_inserts():
    return [[CC.frame(37, 23, 300 + k)] for k in range(3)]


# ---- C: paint ------------------------------------------------------------------------------------------------------------------------
PAINT_W, PAINT_H = 64, 48
CHUNK_BOXES = {(2, 3, 34, 9): 256, (2, 3, 34, 17): 512, (2, 3, 35, 9): 264}      # on a constant plane: box -> recorded indices
NOTHING_BOXES = ((10, 8, 2, 10), (10, 8, 10, 1), (10, 8, 3, 1), (10, 8, 0, 0))
ORDINARY_BOXES = ((12, 10, 20, 12), (30, 20, 25, 18))
EDGE_BOX = (50, 8, 30, 10)  # columns 49 .. 76 of a 64-wide plane: the rows run on into columns 0 .. 12 of the next ones
EDGE_SEED = 6               # cloud_cases.paint_frame(64, 48, 6): 97 indices, some in columns 0, 1 and 2


def constant_plane():
    rng = np.random.default_rng(8400)
    return np.full((PAINT_H, PAINT_W), 2.0, F), rng.integers(0, 256, (PAINT_H, PAINT_W, 3), dtype=np.uint8)


def paint_need(boxes):
    """the indices the boxes can record: what idx_cap has to hold"""
    return sum((int(b[2]) - 2) * (int(b[3]) - 1) for b in boxes if int(b[2]) > 2 and int(b[3]) > 1)
