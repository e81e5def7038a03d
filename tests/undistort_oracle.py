"""CPU oracle of the RGB-D Frame's per-frame geometry, in numpy: cv::undistortPoints (OpenCV 3.2 cvUndistortPoints,
imgproc/src/undistort.cpp) as Frame::UndistortKeyPoints calls it (perfect/src/Frame.cc:750-781, with its k1 rule),
Frame::ComputeImageBounds (:784-815), Frame::ComputeStereoFromRGBD (:1041-1062) and Tracking's depth convertTo
(perfect/src/Tracking.cc:681-682).

float32 and float64 are used exactly where the C++ uses float and double, one operation at a time in the C++ evaluation
order; numpy's float64 ufuncs neither contract nor reorder.  No fused multiply-add anywhere.

UNPINNED.  OpenCV is not available to this project, so the oracle has never been compared with a real OpenCV build.  One
independent check keeps it honest (tests/test_undistort_oracle.py): the Brown-Conrady forward model (the projectPoints
formula, written separately) maps the oracle's output back to the input point, closer with every iteration.  The points
below rest on knowledge of the OpenCV 3.2 sources and could not be confirmed here:

  U1  3.2 iterates exactly 5 times whenever distortion coefficients are given (iters = 5; no termination criterion -- that
      arrived with 3.4's undistortPoints(..., TermCriteria)), and not at all without them.
  U2  The tilt compensation of 3.1+ (invMatTilt = identity for fewer than 14 coefficients: vecUntilt = I * (x, y, 1),
      x0 = x = (1 / 1) * vecUntilt(0)) changes no bit of a finite value.
  U3  RR = P * I (cvMatMul(&_PP, &_RR, &_RR) through cvGEMM's small-matrix path, in place) is P exactly; without P it is the
      identity, still applied as xx = 1*x + 0*y + 0 and ww = 1 / (0*x + 0*y + 1).
  U4  convertTo(CV_32F, scale) of a u16 plane is cvtScale_<ushort, float, float>: (float)u * scale + 0.0f in float, on the
      scalar and the SSE2 path alike; of a f32 plane the same with v in place of (float)u.
  U5  imDepth.at<float>(v, u) with float v, u truncates both to int (Mat::at(int, int)).
"""
import numpy as np

F32, F64 = np.float32, np.float64

# the fork's RGB-D configs (perfect/Examples/RGB-D/TUM*.yaml): fx, fy, cx, cy, (k1, k2, p1, p2[, k3]), bf, DepthMapFactor
TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, dist=(0.262383, -0.953104, -0.005358, 0.002628, 1.163314),
            bf=40.0, depth_factor=5000.0)
TUM2 = dict(fx=520.908620, fy=521.007327, cx=325.141442, cy=249.701764, dist=(0.231222, -0.784899, -0.003257, -0.000105, 0.917205),
            bf=40.0, depth_factor=5208.0)
TUM3 = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, dist=(0.0, 0.0, 0.0, 0.0), bf=40.0, depth_factor=5000.0)
W, H = 640, 480


def camera_matrix(cfg):
    """mK as Tracking builds it (CV_32F)."""
    K = np.eye(3, dtype=F32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = F32(cfg["fx"]), F32(cfg["fy"]), F32(cfg["cx"]), F32(cfg["cy"])
    return K


def dist_coeffs(cfg, n=None):
    """mDistCoef: 4 coefficients, 5 when k3 != 0 (Tracking.cc:154-165); n forces a count."""
    d = [F32(v) for v in cfg["dist"]]
    if n is None:
        n = 5 if len(d) > 4 and d[4] != 0 else 4
    d = (d + [F32(0)] * 12)[:n]
    return np.array(d, F32)


def depth_scale(cfg):
    """mDepthMapFactor = 1.0f / DepthMapFactor (float)."""
    return F32(1.0) / F32(cfg["depth_factor"])


def undistort_points(xy, K, dist, P=None, iters=None):
    """cv::undistortPoints(src, dst, K, D, noArray(), P) for CV_32FC2 points: float32 [n, 2] -> float32 [n, 2].  P None ->
    normalised coordinates.  iters overrides the iteration count (U1) for the property test."""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    dist = np.asarray(dist, F32).ravel()
    nd = len(dist)
    if nd not in (0, 4, 5, 8, 12):
        raise ValueError("distortion coefficient count")
    k = np.zeros(14, F64)
    k[:nd] = dist.astype(F64)
    if iters is None:
        iters = 5 if nd else 0
    K = np.asarray(K, F32)
    fx, fy, cx, cy = F64(K[0, 0]), F64(K[1, 1]), F64(K[0, 2]), F64(K[1, 2])
    ifx = F64(1.) / fx
    ify = F64(1.) / fy
    RR = np.eye(3, dtype=F64) if P is None else np.asarray(P, F32).astype(F64)
    with np.errstate(all="ignore"):
        x = xy[:, 0].astype(F64)
        y = xy[:, 1].astype(F64)
        x = (x - cx) * ifx
        y = (y - cy) * ify
        x0, y0 = x, y
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - deltaX) * icdist
            y = (y0 - deltaY) * icdist
        xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
        yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
        ww = F64(1.) / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
        return np.stack([(xx * ww).astype(F32), (yy * ww).astype(F32)], 1)


def k1_zero(dist):
    """mDistCoef.at<float>(0) == 0.0 (Frame.cc:752, :786); no coefficients count as k1 = 0."""
    dist = np.asarray(dist, F32).ravel()
    return len(dist) == 0 or dist[0] == F32(0)


def undistort_keypoints(xy, K, dist, P="K"):
    """Frame::UndistortKeyPoints: the positions of mvKeysUn (float32 [n, 2])."""
    xy = np.ascontiguousarray(xy, F32).reshape(-1, 2)
    if k1_zero(dist):
        return xy.copy()
    return undistort_points(xy, K, dist, K if isinstance(P, str) else P)


def _fmin(a, b):
    return b if b < a else a   # std::min


def _fmax(a, b):
    return b if a < b else a   # std::max


def image_bounds(K, dist, w, h, P="K"):
    """Frame::ComputeImageBounds + the grid factors of Frame.cc:401-402: (minX, maxX, minY, maxY, gw_inv, gh_inv), float32."""
    if k1_zero(dist):
        minx, maxx, miny, maxy = F32(0), F32(w), F32(0), F32(h)
    else:
        c = np.array([[0, 0], [w, 0], [0, h], [w, h]], F32)
        u = undistort_points(c, K, dist, K if isinstance(P, str) else P)
        minx = _fmin(u[0, 0], u[2, 0])
        maxx = _fmax(u[1, 0], u[3, 0])
        miny = _fmin(u[0, 1], u[1, 1])
        maxy = _fmax(u[2, 1], u[3, 1])
    with np.errstate(all="ignore"):
        gwi = F32(64) / F32(maxx - minx)
        ghi = F32(48) / F32(maxy - miny)
    return tuple(F32(v) for v in (minx, maxx, miny, maxy, gwi, ghi))


def depth_scaled(fmt_f32, scale):
    """Tracking.cc:681: a u16 plane is always converted; a f32 plane when fabs(scale - 1.0f) > 1e-5."""
    return (not fmt_f32) or float(abs(F32(scale) - F32(1.0))) > 1e-5


def depth_to_float(plane, scale):
    """mImDepth.convertTo(CV_32F, scale) under Tracking's condition (U4): float32 plane."""
    plane = np.asarray(plane)
    f32 = plane.dtype == np.float32
    v = plane.astype(F32)
    if not depth_scaled(f32, scale):
        return v.copy()
    with np.errstate(all="ignore"):
        return v * F32(scale) + F32(0.0)


def stereo_from_rgbd(xy, xy_un, depth_f32, bf):
    """Frame::ComputeStereoFromRGBD on the float depth plane: (mvDepth, mvuRight) float32 [n].  The depth is read at the
    DISTORTED keypoint, truncated (U5); a keypoint outside the plane has no depth (undefined in the reference)."""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    xy_un = np.asarray(xy_un, F32).reshape(-1, 2)
    n = len(xy)
    dep = np.full(n, -1, F32)
    ur = np.full(n, -1, F32)
    h, w = depth_f32.shape
    for i in range(n):
        x, y = xy[i]
        if not (x > -1 and x < w and y > -1 and y < h):
            continue
        d = depth_f32[int(y), int(x)]
        if d > 0:
            dep[i] = d
            ur[i] = F32(xy_un[i, 0] - F32(F32(bf) / d))
    return dep, ur


def frame_geometry(kps, K, dist, bf, depth=None, scale=1.0):
    """The whole per-frame step on one frame's keypoints (a KP_DTYPE array): (mvKeysUn as a KP_DTYPE array, mvDepth, mvuRight).
    depth: a u16 or f32 plane, or None (monocular / stereo constructors: all -1)."""
    kps = np.asarray(kps)
    xy = np.stack([kps["x"], kps["y"]], 1).astype(F32)
    un = undistort_keypoints(xy, K, dist)
    out = kps.copy()
    out["x"], out["y"] = un[:, 0], un[:, 1]
    if depth is None:
        return out, np.full(len(kps), -1, F32), np.full(len(kps), -1, F32)
    dep, ur = stereo_from_rgbd(xy, un, depth_to_float(depth, scale), bf)
    return out, dep, ur
