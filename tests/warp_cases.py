"""Shared inputs of the homography-compensated flow mask tests: the table of homographies and frame sizes the GPU warp is checked
on (tests/test_gpu_flow_homo.py; tests/test_warp_oracle.py shows which edges of warpPerspective it reaches) and planar scenes
moved by known homographies."""
import numpy as np
import scipy.ndimage as ndi

SIZES = [(640, 480), (1241, 376), (641, 481), (127, 96), (129, 96), (16, 16), (100, 17)]


def _about_centre(A, w, h):
    """the 3x3 matrix A applied about the frame centre"""
    c = np.array([[1, 0, (w - 1) / 2.0], [0, 1, (h - 1) / 2.0], [0, 0, 1]])
    return c @ A @ np.linalg.inv(c)


def camera_homography(w, h, yaw=0.02, pitch=-0.015, roll=0.01, t=(0.03, -0.02, 0.01), n=(0.05, -0.1, 1.0), d=2.5):
    """H = K (R - t n^T / d) K^-1 of a plane n.X = d seen by a camera with focal length 0.8 w, normalised to H[2, 2] = 1"""
    f = 0.8 * w
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]])
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]) @ \
        np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    nn = np.asarray(n, np.float64)
    nn = nn / np.linalg.norm(nn)
    H = K @ (R - np.outer(t, nn) / d) @ np.linalg.inv(K)
    return H / H[2, 2]


def homography(name, w, h):
    """One entry of the table, for a w x h frame (float64 3x3, or float32 for 'float32_entries')."""
    if name == "identity":
        return np.eye(3)
    if name == "int_translation":
        return np.array([[1.0, 0, 5], [0, 1, -3], [0, 0, 1]])
    if name == "subpixel_translation":
        return np.array([[1.0, 0, 2.37], [0, 1, -1.61], [0, 0, 1]])
    if name == "rotation_scale":
        a, s = np.deg2rad(7.0), 1.06
        return _about_centre(np.array([[s * np.cos(a), -s * np.sin(a), 0], [s * np.sin(a), s * np.cos(a), 0], [0, 0, 1]]), w, h)
    if name == "camera_plane":
        return camera_homography(w, h)
    if name == "strong_perspective":
        # the inverse map's W = 1 - 2.2 y / h changes sign at y ~ 0.45 h: the horizon crosses the frame, beyond it W < 0, near it
        # |X / W| overflows int and the source cells saturate as shorts
        Minv = np.array([[1.0, 0.3, -0.4 * w], [0.05, 1.2, -0.1 * h], [0.0004 * 64 / max(w, 64), -2.2 / h, 1.0]])
        return np.linalg.inv(Minv)
    if name == "out_of_view":
        return np.array([[1.0, 0, 3.0 * w + 7.5], [0, 1, 0.5], [0, 0, 1]])
    if name == "float32_entries":
        return camera_homography(w, h, yaw=-0.03, pitch=0.02, roll=-0.02, t=(-0.04, 0.01, 0.03)).astype(np.float32)
    if name == "near_ties":
        # an affine map whose inverse puts many 32 * X exactly or within an ulp of a half-integer (65/64 steps) with entries
        # an ulp or so off the dyadic values: the rounding of M0*xb + M0*x1 (the invoker's block split) against M0*x decides
        # cvRound's direction at many pixels
        A = np.array([[65 / 64, 1 / 64, 0.25], [-1 / 64, 63 / 64, 1.5], [0, 0, 1]])
        A[:2, :] *= 1 + np.array([[-4, -4, -3], [3, 1, 4]]) * 2.0 ** -52
        return np.linalg.inv(A)
    if name == "singular":
        return np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    raise KeyError(name)


H_NAMES = ["identity", "int_translation", "subpixel_translation", "rotation_scale", "camera_plane", "strong_perspective",
           "out_of_view", "float32_entries", "near_ties", "singular"]


def frame(seed, w, h):
    """uniform random bytes: every sub-pixel weight and every neighbour shows in the output"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- planar scenes --------------------------------------------------------------------------------------------------------
def smooth_canvas(seed, w, h, cell=12, margin=64):
    """a smooth texture (random cells, cubic zoom) on a canvas `margin` px larger on every side, float64"""
    rng = np.random.default_rng(seed)
    H, W = h + 2 * margin, w + 2 * margin
    low = rng.uniform(0, 255, (H // cell + 4, W // cell + 4))
    big = ndi.zoom(low, cell, order=3)[:H, :W]
    return np.clip(big, 0, 255)


def view(canvas, G, w, h, margin=64):
    """the w x h frame of the planar canvas after the camera motion G (frame coordinates): out(x) = canvas(G^-1 x), cubic
    spline, rounded to u8"""
    Gi = np.linalg.inv(np.asarray(G, np.float64))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    q = Gi @ p
    sx, sy = q[0] / q[2] + margin, q[1] / q[2] + margin
    out = ndi.map_coordinates(canvas, [sy, sx], order=3, mode="nearest").reshape(h, w)
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


def motion(w, h, k=1.0, dx=14.0, dy=-9.0, rot=0.01):
    """a camera motion between two frames: translation (dx, dy) px plus a small rotation and perspective, scaled by k"""
    a = rot * k
    A = np.array([[np.cos(a), -np.sin(a), dx * k], [np.sin(a), np.cos(a), dy * k], [2e-5 * k * 640 / w, -1e-5 * k * 480 / h, 1.0]])
    return _about_centre(A, w, h)


def with_patch(img, patch, x0, y0):
    out = img.copy()
    ph, pw = patch.shape
    out[y0:y0 + ph, x0:x0 + pw] = patch
    return out


def planar_sequence(seed, n, w, h, k=0.6):
    """n frames of a planar scene under a steady camera motion G (frame i = canvas under G^i) and, for each frame i >= 1, the
    homography H_i = G^-1 that maps frame i onto frame i-1 (what TrackHomo's findHomography(points_current, points_last)
    estimates); H_0 is the identity."""
    canvas = smooth_canvas(seed, w, h)
    G = motion(w, h, k)
    frames, Hs = [], []
    Gi = np.eye(3)
    for i in range(n):
        frames.append(view(canvas, Gi, w, h))
        Hs.append(np.linalg.inv(G) if i else np.eye(3))
        Gi = G @ Gi
    return frames, Hs
