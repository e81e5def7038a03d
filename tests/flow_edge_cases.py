"""Planted inputs for the optical-flow mask (csrc/orbfe_flow.hip) at the sizes, level plans and contents its stage tests never
reach, and for the masked-Frame keypoint rule alone.  numpy + synth_frame only; tests/test_flow_edge_cases.py checks with the
CPU oracle that every case reaches the edge its tag names, tests/test_gpu_flow_edges.py feeds them to the HIP kernels.  Test
support only.

SIZES is the table: dict(w, h, gen, tag, levels), `levels` the Farneback level sizes of the half-size image written out by
hand, level 0 (the half-size image) first.  `gen` is chosen per size so that the pre-morphology mask at threshold 40 holds
both values (zero share in [0.02, 0.98]); FLOW_ONLY names the sizes where none does (none today).

The level rule (calcOpticalFlowFarneback): level k exists while w2 * 0.5^k >= 32 and h2 * 0.5^k >= 32, at most 3 beyond level
0; its size is cvRound(w2 * 0.5^k), round half to even: 64.5 -> 64, 65.5 -> 66."""
import numpy as np

from orb_slam2_ssd_semantic_amd import KP_DTYPE
from orb_slam2_ssd_semantic_amd.synth import synth_frame

F32 = np.float32


def _u8(a):
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ frame pairs
def gen_shift(w, h):
    """a synth_frame crop and the same crop displaced by (14, -10) px"""
    bg = synth_frame(w * 1000 + h, h=h + 64, w=w + 64)
    return bg[32:32 + h, 32:32 + w].copy(), bg[42:42 + h, 18:18 + w].copy()


def gen_noise(w, h):
    """two independent uniform u8 frames"""
    rng = np.random.default_rng(w * 1000 + h)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)


def _wave(w, h, L, ox, oy):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return _u8(127.5 + 60 * np.sin(2 * np.pi * (x - ox) / L) + 60 * np.sin(2 * np.pi * (y - oy) / (1.25 * L)))


def gen_wave(L, d):
    """127.5 + 60 sin(2 pi x / L) + 60 sin(2 pi y / 1.25 L), and the same shifted by (d, d / 2)"""
    return lambda w, h: (_wave(w, h, L, 0.0, 0.0), _wave(w, h, L, d, d / 2.0))


def gen_bowl(w, h, k=0.3, d=28.0):
    """a quadratic bowl k ((x - x0)^2 + (y - y0)^2) about (-6, -6), and the same translated by d on both axes: a pure
    translation of a quadratic, which the polynomial expansion recovers where the u8 range does not clip it"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x0 = y0 = -6.0
    return _u8(k * ((x - x0) ** 2 + (y - y0) ** 2)), _u8(k * ((x - x0 - d) ** 2 + (y - y0 - d) ** 2))


GENERATORS = {"shift": gen_shift, "noise": gen_noise, "wave96": gen_wave(96.0, 22.0), "wave80": gen_wave(80.0, 18.0),
              "bowl": gen_bowl}


def pair(case):
    return GENERATORS[case["gen"]](case["w"], case["h"])


def _c(w, h, gen, tag, *levels):
    return dict(w=w, h=h, gen=gen, tag=tag, levels=list(levels))


SIZES = [
    # minimum and tiny one-level: w2 < 10 (the border test of UpdateMatrices wraps), h2 < 15 and w2 < 7 (the box filter's
    # clamps act in the initial sums), w, h < 21 (the ellipse hangs outside on every side)
    _c(16, 16, "bowl", "min 8x8", (8, 8)),
    _c(17, 16, "bowl", "min 8x8, odd width strip", (8, 8)),
    _c(16, 17, "bowl", "min 8x8, odd height strip", (8, 8)),
    _c(19, 23, "bowl", "tiny 9x11, both odd", (9, 11)),
    _c(40, 22, "bowl", "tiny 20x11: h2 < 15 only", (20, 11)),
    _c(64, 20, "bowl", "tiny 32x10: one morph tile wide", (32, 10)),
    # thin
    _c(16, 300, "wave80", "thin 8x150", (8, 150)),
    _c(300, 16, "wave80", "thin 150x8", (150, 8)),
    _c(512, 16, "wave96", "thin 256x8: one full PolyExp segment", (256, 8)),
    _c(514, 16, "wave96", "thin 257x8: a one-pixel PolyExp tail", (257, 8)),
    # level steps, each axis limiting
    _c(127, 200, "wave96", "step 1|2, width limits: 63 * 0.5 < 32", (63, 100)),
    _c(128, 200, "shift", "step 1|2, width on the step", (64, 100), (32, 50)),
    _c(200, 127, "wave96", "step 1|2, height limits", (100, 63)),
    _c(200, 128, "shift", "step 1|2, height on the step", (100, 64), (50, 32)),
    _c(255, 300, "shift", "step 2|3, width limits; 63.5 -> 64 (tie up)", (127, 150), (64, 75)),
    _c(256, 300, "noise", "step 2|3, width on the step; 37.5 -> 38 (tie up)", (128, 150), (64, 75), (32, 38)),
    _c(300, 255, "shift", "step 2|3, height limits; 63.5 -> 64", (150, 127), (75, 64)),
    _c(300, 256, "noise", "step 2|3, height on the step; 37.5 -> 38", (150, 128), (75, 64), (38, 32)),
    _c(511, 512, "noise", "step 3|4, width limits; 127.5 -> 128, 63.75 -> 64", (255, 256), (128, 128), (64, 64)),
    _c(512, 511, "noise", "step 3|4, height limits", (256, 255), (128, 128), (64, 64)),
    _c(512, 512, "noise", "the smallest four-level frame", (256, 256), (128, 128), (64, 64), (32, 32)),
    # cvRound ties and mixed resize modes
    _c(258, 256, "bowl", "64.5 -> 64 (tie down) in x, exact 2x in y", (129, 128), (64, 64), (32, 32)),
    _c(262, 256, "noise", "65.5 -> 66 (tie up) in x, exact 2x in y", (131, 128), (66, 64), (33, 32)),
    _c(256, 258, "noise", "64.5 -> 64 in y, exact 2x in x", (128, 129), (64, 64), (32, 32)),
    _c(256, 262, "noise", "65.5 -> 66 in y, exact 2x in x", (128, 131), (64, 66), (32, 33)),
    _c(260, 258, "noise", "level 1 = 65x64: exact 2x in x only; 32.5 -> 32", (130, 129), (65, 64), (32, 32)),
    _c(259, 263, "noise", "odd both: 64.5 -> 64, 65.5 -> 66", (129, 131), (64, 66), (32, 33)),
    _c(516, 256, "wave96", "258 * 0.25 = 64.5 -> 64; levels 1 and 2 exact 2x in y only", (258, 128), (129, 64), (64, 32)),
    _c(524, 262, "wave96", "262 * 0.25 = 65.5 -> 66; level 1 exact 2x in x only", (262, 131), (131, 66), (66, 33)),
]

# The sizes whose pre-morphology mask holds one value only, so that only the flow taps carry them.  The bowl moves the flow past
# the clamped threshold at (19, 23), (40, 22) and (64, 20), and the 96 px wave does at (512, 16) and (514, 16), so none is left.
FLOW_ONLY = []
SECOND_THRESHOLD = 45.0    # for the entries with both mask values

# one handle sized for the largest plan runs these one after another (level counts 4, 1, 3, 2, 1, 3, 1)
ONE_HANDLE = [(512, 512), (16, 16), (524, 262), (128, 200), (19, 23), (259, 263), (300, 16)]


def case_of(w, h):
    return next(c for c in SIZES if (c["w"], c["h"]) == (w, h))


# ------------------------------------------------------------------------------------------------------ degenerate contents
def degenerate(name, w, h):
    if name == "constant":
        a = np.full((h, w), 93, np.uint8)
        return a, a.copy()
    if name == "black_to_white":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if name == "identical":
        a = synth_frame(7, h=h, w=w)
        return a, a.copy()
    if name == "checkerboard":
        y, x = np.mgrid[0:h, 0:w]
        a = (((x + y) & 1) * 255).astype(np.uint8)
        return a, (255 - a).astype(np.uint8)
    if name == "step_edge":
        a = np.zeros((h, w), np.uint8)
        b = np.zeros((h, w), np.uint8)
        a[:, w // 2:] = 255
        b[:, w // 2 + 6:] = 255
        return a, b
    raise KeyError(name)


DEGENERATE = ["constant", "black_to_white", "identical", "checkerboard", "step_edge"]
DEGENERATE_SIZES = [(128, 128), (17, 16)]

# ------------------------------------------------------------------------------------------------------ thresholds
THRESHOLD_SIZE = (259, 263)
TH_AS_40 = [float(np.nextafter(F32(40), F32(0))), -1.0, 0.0]                            # clamp to 40
TH_OTHER = [float(np.nextafter(F32(40), F32(np.inf))), 1e30, float("inf"), float("nan")]   # kept as given


# ------------------------------------------------------------------------------------------------------ the keypoint rule
def _records(n, seed):
    """n keypoint records with every field set (so a copy that drops a field shows) and n distinct descriptors"""
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KP_DTYPE)
    for f in KP_DTYPE.names:
        if np.issubdtype(KP_DTYPE[f], np.floating):
            k[f] = rng.uniform(1, 100, n).astype(KP_DTYPE[f])
        else:
            k[f] = rng.integers(1, 8, n).astype(KP_DTYPE[f])
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)   # distinct
    return k, d


KEEP_PATTERNS = ["all", "none", "alternating", "first_of_256", "last_of_256"]
RULE_COUNTS = [0, 1, 255, 256, 257, 513]


def keep_pattern(name, n):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 0, "first_of_256": i % 256 == 0,
            "last_of_256": (i % 256 == 255) | (i == n - 1)}[name]


def rule_case(n, pattern, w=48, h=40):
    """n keypoints at distinct pixels of a w x h mask (w * h >= n); the mask is 1 except under the keypoints the pattern drops
    (at most 513 of 1920 pixels, so more than 65 % stay 1 and the frame is filtered).
    Returns dict(mask, kps, desc, keep = planted keep flags)."""
    assert n <= 640 and w * h * 0.65 < w * h - n
    k, d = _records(n, n * 7 + len(pattern))
    cells = np.random.default_rng(n).permutation(w * h)[:n]
    frac = np.random.default_rng(n + 1).uniform(0.0, 0.99, (2, n)).astype(np.float32)
    k["x"] = (cells % w).astype(np.float32) + frac[0]
    k["y"] = (cells // w).astype(np.float32) + frac[1]
    keep = keep_pattern(pattern, n)
    mask = np.ones((h, w), np.uint8)
    mask[cells[~keep] // w, cells[~keep] % w] = 0
    return dict(mask=mask, kps=k, desc=d, keep=keep)


def ones_mask(w, h, ones):
    """a w x h 0 / 1 mask with exactly `ones` ones, the zeros at the end"""
    m = np.zeros(w * h, np.uint8)
    m[:ones] = 1
    return m.reshape(h, w)


def share_case(w, h, extra):
    """the 65 % comparison: a mask with int(h * w * 0.65) + extra ones and one keypoint on a one, one on a zero.  extra = 0:
    sum <= bound, nothing is filtered; extra = 1: the keypoint on the zero goes."""
    ones = int(h * w * 0.65) + extra
    mask = ones_mask(w, h, ones)
    k, d = _records(2, w * 100 + h + extra)
    k["x"] = [0.5, w - 0.5]
    k["y"] = [0.5, h - 0.5]
    assert mask[0, 0] == 1 and mask[h - 1, w - 1] == 0
    filtered = float(ones) > h * w * 0.65
    return dict(mask=mask, kps=k, desc=d, keep=np.array([True, not filtered]))


def value_case(w=12, h=10):
    """mask values other than 0 and 1 under a keypoint: only == 1 keeps.  ones is the SUM of the values, as the reference sums"""
    mask = np.ones((h, w), np.uint8)
    mask[2, 3], mask[4, 5], mask[6, 7] = 2, 255, 0
    k, d = _records(4, 99)
    k["x"] = [3.5, 5.5, 7.5, 9.5]
    k["y"] = [2.5, 4.5, 6.5, 8.5]
    return dict(mask=mask, kps=k, desc=d, keep=np.array([False, False, False, True]))


def coordinate_case(w=12, h=10):
    """truncation and the plane's edges.  The mask is 1 except column 4, column w - 1 and row h - 1 from column 6 on are 0 and
    (0, 0) is 0, so a keypoint is kept or dropped by the column / row its coordinate truncates to; everything outside the plane
    is dropped.  (x, y, kept)"""
    mask = np.ones((h, w), np.uint8)
    mask[:, 4] = 0
    mask[:, w - 1] = 0
    mask[h - 1, 6:] = 0
    mask[0, 0] = 0
    big, inf, nan = 1e9, float("inf"), float("nan")
    wf, hf = float(w), float(h)
    pts = [
        (4.999, 2.0, False),                      # column 4 (a zero), not 5
        (5.0, 2.0, True),
        (float(np.nextafter(F32(4), F32(0))), 2.0, True),   # column 3
        (-0.5, 2.0, True),                        # (int)-0.5 = 0: column 0, row 2 (a one)
        (2.0, -0.5, True),                        # row 0
        (-0.5, -0.5, False),                      # (0, 0): the planted zero
        (float(np.nextafter(F32(-1), F32(0))), 2.0, True),  # the last value inside
        (wf - 0.001, 2.0, False),                 # column w - 1 (zeros)
        (wf - 1.001, 2.0, True),                  # column w - 2
        (7.0, hf - 0.001, False),                 # row h - 1 (zeros from column 6)
        (2.0, hf - 0.001, True),                  # row h - 1, a one
        (-1.0, 2.0, False), (2.0, -1.0, False), (wf, 2.0, False), (2.0, hf, False),
        (big, 2.0, False), (2.0, big, False), (3e9, 2.0, False), (2.0, 3e9, False), (-3e9, 2.0, False),
        (inf, 2.0, False), (-inf, 2.0, False), (2.0, inf, False), (2.0, -inf, False),
        (nan, 2.0, False), (2.0, nan, False), (nan, nan, False),
        (1.0, 1.0, True),
    ]
    k, d = _records(len(pts), 5)
    k["x"] = np.array([p[0] for p in pts], np.float32)
    k["y"] = np.array([p[1] for p in pts], np.float32)
    assert mask.sum() > w * h * 0.65
    return dict(mask=mask, kps=k, desc=d, keep=np.array([p[2] for p in pts]))


def batch_case(w=20, h=12):
    """three frames: 0 filtered (alternating), 1 not (exactly 65 % ones or fewer: all kept although half sit on zeros),
    2 filtered to zero keypoints"""
    out = []
    for f, n in enumerate((300, 257, 40)):
        k, d = _records(n, 50 + f)
        cells = np.random.default_rng(60 + f).permutation(w * h)[:n] if n <= w * h else np.arange(n) % (w * h)
        k["x"] = (cells % w).astype(np.float32) + np.float32(0.25)
        k["y"] = (cells // w).astype(np.float32) + np.float32(0.75)
        mask = np.ones((h, w), np.uint8)
        if f == 0:
            mask[:, 0:w:4] = 0                                    # 75 % ones
            keep = mask[cells // w, cells % w] == 1
        elif f == 1:
            mask = ones_mask(w, h, int(h * w * 0.65))             # 156 of 240 = the bound exactly: not filtered
            keep = np.ones(n, bool)
        else:
            mask[cells // w, cells % w] = 0                       # 40 holes: 83 % ones
            keep = np.zeros(n, bool)
        out.append(dict(mask=mask, kps=k, desc=d, keep=keep))
    return out
