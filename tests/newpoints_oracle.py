"""numpy restatement of csrc/orbfe_newpoints.h and of the loops of csrc/orbfe_newpoints.hip: the body of LocalMapping::
CreateNewMapPoints' match loop (src/LocalMapping.cc:446-611), KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:724-754), the
neighbour loop with its slot state (serial, as the reference runs it, and by rounds, as the device runs it) and the round planner.

UNPINNED: LocalMapping.cc and KeyFrame.cc are not among the compiled reference sources, so nothing compiled pins this file (like
tests/f12_oracle.py).  The cv::Mat expressions are restated as OpenCV 3.2 evaluates them, under these rules; every float operation
is one np.float32 operation, every double operation a Python float operation, nothing fused.

  N1  KeyFrame::invfx = 1.0f / fx (float division, src/KeyFrame.cc constructor copies Frame::invfx, src/Frame.cc).
  N2  xn = ((x - cx) * invfx, (y - cy) * invfy, 1.0f): float, left to right (Mat_<float> << takes the float expressions).
  N3  Rwc * xn (Rwc = Rcw.t() is an evaluated matrix): cv::gemm, no flags, 3x3 . 3x1, inner length 3 -> the inline float block
      (core/src/matmul.cpp, the `len <= 4` shortcut): s = a0 * b0 + a1 * b1 + a2 * b2 in float, stored (float)(s * alpha + 0 *
      beta) in double.
  N4  Mat::dot on CV_32F (core/src/matmul.cpp dotProd_32f): a double sum of (double)a * b from zero, left to right
      (initializer_oracle I5).
  N5  cv::norm (L2, CV_32F; core/src/stat.cpp normL2_32f): sqrt of the double sum of (double)v * v.  cosParallaxRays =
      (float)(dot / (norm1 * norm2)), all double.
  N6  z1 = Rcw1.row(2).dot(x3Dt) + tcw1.at<float>(2): double + float -> double, stored to float.  x1, y1, z2, x2, y2 alike.
  N7  cos(2 * atan2(mb / 2, depth)): the arguments are floats and <cmath>'s overloads are the float ones; the reference gets
      the host libm's cosf / atan2f.  By the project's rule (DESIGN "Canonical trig") the library evaluates a = (float)c_atan2(
      (double)(mb / 2), (double)depth), c = (float)c_cos((double)(2 * a)) with sim3_oracle's canonical functions.  `else if
      (bStereo2)`: keyframe 2's value only when keyframe 1's keypoint is monocular; otherwise cosParallaxRays + 1 (float).
      std::min(a, b) = b < a ? b : a.
  N8  The linear triangulation: rows `a * row2 - row0` are addWeighted (core/src/arithm.cpp): v1 * a + v2 * (-1.0f) + 0.0f in
      float (initializer_oracle I7), cv::SVD::compute on CV_32F = JacobiSVDImpl_<float> (I1, I2), vt.row(3); `== 0` on its last
      entry; rowRange(0, 3) / w is convertTo with the scale (float)(1. / w): v * a + 0.0f (I6).
  N9  KeyFrame::UnprojectStereo reads the RAW keypoint mvKeys[i]: x = (u - cx) * z * invfx (float, left to right), Twc(0..2,
      0..2) * x3Dc + Twc(0..2, 3) = gemm(A, B, 1, C, 1) through the inline block: the float sum of three products, then
      (float)(s + c) in double = the float sum (a double holds the sum of two floats to within the double rounding that is
      innocuous for p = 24): track_oracle's trk_unproject.  mvDepth <= 0 returns an empty Mat, on which the reference's next line
      (Mat::dot of unequal sizes) throws: THIS LIBRARY's verdict is DEPTH1 / DEPTH2.
  N10 invz = 1.0 / z: a double division stored to float (I8).  u = fx * x * invz + cx: float, left to right.  u_r = u - mbf * invz
      with keyframe 1's mbf for BOTH keyframes (sic).
  N11 (errX * errX + errY * errY [+ errX_r * errX_r]) is a float sum, promoted for the strict `>` against the double 5.991 *
      sigma2 / 7.8 * sigma2 (sigma2 a float, promoted).
  N12 normal = x3D - Ow in float (MatExpr subtraction of CV_32F), dist = (float)cv::norm(normal) (N5).
  N13 ratioDist = dist2 / dist1, ratioOctave = mvScaleFactors[o1] / mvScaleFactors[o2], ratioFactor = 1.5f * mfScaleFactor, the
      gate ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor: all float.
  N14 ComputeSceneMedianDepth: z = Rcw2.dot(x3Dw) + zcw is N4 + N6 on row 2 of Tcw; std::sort, vDepths[(size - 1) / q].  No
      MapPoint at all is undefined behaviour in the reference; THIS LIBRARY's value is -1.0f.
"""
import ctypes
import ctypes.util
import math

import numpy as np

import f12_oracle as FO
import initializer_oracle as IO
import sim3_oracle as SO

f32 = np.float32
LOW_PARALLAX, W_ZERO, DEPTH1, DEPTH2, ERR1, ERR2, DIST_ZERO, SCALE, OK, IGNORED = range(10)
VERDICTS = ("LOW_PARALLAX", "W_ZERO", "DEPTH1", "DEPTH2", "ERR1", "ERR2", "DIST_ZERO", "SCALE", "OK", "IGNORED")
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


# ---- the two trig modes (N7) --------------------------------------------------------------------------------------------------------
def _canonical(mb, depth):
    a = f32(SO.c_atan2(float(f32(mb / f32(2))), float(depth)))
    return f32(SO.c_cos(float(f32(f32(2) * a))))


_libm = None


def _host(mb, depth):
    """cosf(2 * atan2f(mb / 2, depth)) with this machine's libm"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.cosf.restype = _libm.atan2f.restype = ctypes.c_float
        _libm.cosf.argtypes = [ctypes.c_float]
        _libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
    a = f32(_libm.atan2f(float(f32(mb / f32(2))), float(depth)))
    return f32(_libm.cosf(float(f32(f32(2) * a))))


TRIG = dict(canonical=_canonical, host=_host)


# ---- one match ----------------------------------------------------------------------------------------------------------------------
def key(ux, uy, octave, depth=-1.0, uright=-1.0, rx=None, ry=None):
    return dict(ux=f32(ux), uy=f32(uy), rx=f32(ux if rx is None else rx), ry=f32(uy if ry is None else ry), depth=f32(depth),
                uright=f32(uright), octave=int(octave))


def np_ray(T, x, y):
    return [FO.geo_gemm_store(f32(f32(f32(T[i] * x) + f32(T[4 + i] * y)) + f32(T[8 + i] * f32(1)))) for i in range(3)]


def np_dot3(a, b):
    s = 0.0
    for k in range(3):
        s += float(a[k]) * float(b[k])
    return s


def np_cam_coord(T, r, x):
    return f32(np_dot3(T[4 * r:4 * r + 3], x) + float(T[4 * r + 3]))


def np_unproject(T, Ow, cam, invfx, invfy, u, v, z):
    x = f32(f32(f32(u - cam["cx"]) * z) * invfx)
    y = f32(f32(f32(v - cam["cy"]) * z) * invfy)
    return np.array([f32(f32(f32(f32(T[k] * x) + f32(T[4 + k] * y)) + f32(T[8 + k] * z)) + Ow[k]) for k in range(3)], f32)


def np_dist(x, Ow):
    n = [f32(x[k] - Ow[k]) for k in range(3)]
    return f32(math.sqrt(np_dot3(n, n)))


def cos_parallax_rays(T1, T2, cam, k1, k2):
    invfx, invfy = f32(f32(1) / cam["fx"]), f32(f32(1) / cam["fy"])
    xn1 = (f32(f32(k1["ux"] - cam["cx"]) * invfx), f32(f32(k1["uy"] - cam["cy"]) * invfy))
    xn2 = (f32(f32(k2["ux"] - cam["cx"]) * invfx), f32(f32(k2["uy"] - cam["cy"]) * invfy))
    r1, r2 = np_ray(T1, *xn1), np_ray(T2, *xn2)
    return f32(np_dot3(r1, r2) / (math.sqrt(np_dot3(r1, r1)) * math.sqrt(np_dot3(r2, r2)))), xn1, xn2


def camera(fx, fy, cx, cy, bf):
    return dict(fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), bf=f32(bf))


def triangulate_match(T1, O1, T2, O2, cam, mb, k1, k2, scale_factors, level_sigma2, scale_factor, trig="canonical", trace=None):
    """-> (verdict, x3D float32 [3]).  T row-major 3x4 as 12 floats, O [3]; cam = camera(); k = key().  `trace`, a list, receives
    (name, lhs, rhs) of every comparison the body makes, for the margin check of the cases."""
    T1, T2 = np.asarray(T1, f32).reshape(12), np.asarray(T2, f32).reshape(12)
    O1, O2 = np.asarray(O1, f32).reshape(3), np.asarray(O2, f32).reshape(3)
    mb, sf, s2 = f32(mb), np.asarray(scale_factors, f32), np.asarray(level_sigma2, f32)
    cosf = TRIG[trig]
    tr = (lambda *a: trace.append(a)) if trace is not None else (lambda *a: None)
    zero = np.zeros(3, f32)
    with np.errstate(**_ERR):
        st1, st2 = bool(k1["uright"] >= 0), bool(k2["uright"] >= 0)
        invfx, invfy = f32(f32(1) / cam["fx"]), f32(f32(1) / cam["fy"])
        cosRays, xn1, xn2 = cos_parallax_rays(T1, T2, cam, k1, k2)
        cs = f32(cosRays + f32(1))
        cs1 = cs2 = cs
        if st1:
            cs1 = cosf(mb, k1["depth"])
        elif st2:
            cs2 = cosf(mb, k2["depth"])
        cs = cs2 if cs2 < cs1 else cs1
        tr("rays<stereo", cosRays, cs)
        tr("rays>0", cosRays, f32(0))
        if not (st1 or st2):
            tr("rays<0.9998", float(cosRays), 0.9998)
        if cosRays < cs and cosRays > 0 and (st1 or st2 or float(cosRays) < 0.9998):
            xy = np.array([[xn1[0], xn1[1], xn2[0], xn2[1]]], f32)
            A = np.zeros((1, 4, 4), f32)
            for r, (c, P, row) in enumerate(((0, T1, 0), (1, T1, 1), (2, T2, 0), (3, T2, 1))):
                P = P.reshape(3, 4)
                A[:, r, :] = xy[:, c, None] * P[None, 2, :] + P[None, row, :] * f32(-1.0) + f32(0)
            _, _, vt = IO.svd_f(A)
            v = vt[0, 3, :]
            if v[3] == 0:
                return W_ZERO, zero
            a = f32(1.0 / float(v[3]))
            x = np.array([f32(f32(v[k] * a) + f32(0)) for k in range(3)], f32)
        elif st1 and cs1 < cs2:
            tr("stereo1<stereo2", cs1, cs2)
            if not k1["depth"] > 0:
                return DEPTH1, zero
            x = np_unproject(T1, O1, cam, invfx, invfy, k1["rx"], k1["ry"], k1["depth"])
        elif st2 and cs2 < cs1:
            tr("stereo2<stereo1", cs2, cs1)
            if not k2["depth"] > 0:
                return DEPTH2, zero
            x = np_unproject(T2, O2, cam, invfx, invfy, k2["rx"], k2["ry"], k2["depth"])
        else:
            return LOW_PARALLAX, zero
        z1 = np_cam_coord(T1, 2, x)
        tr("z1>0", z1, f32(0))
        if z1 <= 0:
            return DEPTH1, x
        z2 = np_cam_coord(T2, 2, x)
        tr("z2>0", z2, f32(0))
        if z2 <= 0:
            return DEPTH2, x
        for T, z, k, st, name, verdict in ((T1, z1, k1, st1, "err1", ERR1), (T2, z2, k2, st2, "err2", ERR2)):
            xc, yc = np_cam_coord(T, 0, x), np_cam_coord(T, 1, x)
            invz = f32(1.0 / float(z))
            u = f32(f32(f32(cam["fx"] * xc) * invz) + cam["cx"])
            v = f32(f32(f32(cam["fy"] * yc) * invz) + cam["cy"])
            ex, ey = f32(u - k["ux"]), f32(v - k["uy"])
            e = f32(f32(ex * ex) + f32(ey * ey))
            th = 5.991 * float(s2[k["octave"]])
            if st:
                er = f32(f32(u - f32(cam["bf"] * invz)) - k["uright"])
                e = f32(e + f32(er * er))
                th = 7.8 * float(s2[k["octave"]])
            tr(name, float(e), th)
            if float(e) > th:
                return verdict, x
        d1, d2 = np_dist(x, O1), np_dist(x, O2)
        if d1 == 0 or d2 == 0:
            return DIST_ZERO, x
        rd, ro, rf = f32(d2 / d1), f32(sf[k1["octave"]] / sf[k2["octave"]]), f32(f32(1.5) * f32(scale_factor))
        tr("scale_lo", f32(rd * rf), ro)
        tr("scale_hi", rd, f32(ro * rf))
        if f32(rd * rf) < ro or rd > f32(ro * rf):
            return SCALE, x
        return OK, x


def near_threshold(trace, rel=1e-4):
    """the comparisons of a trace whose two sides lie within rel of each other (relative to the threshold; absolute against 0)"""
    out = []
    for name, a, b in trace:
        a, b = float(a), float(b)
        if math.isfinite(a) and math.isfinite(b) and abs(a - b) <= rel * (abs(b) if b != 0 else 1.0):
            out.append(name)
    return out


# ---- ComputeSceneMedianDepth (N14) ----------------------------------------------------------------------------------------------------
def scene_median_depth(Tcw, has_mp, xyz, n, q):
    T = np.asarray(Tcw, f32).reshape(12)
    z = sorted(float(np_cam_coord(T, 2, xyz[i])) for i in range(int(n)) if has_mp[i])
    return f32(z[(len(z) - 1) // q]) if z else f32(-1.0)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def plan_rounds(kf1, kf2):
    """-> (round_of [P], order [P], round_off [nrounds + 1])"""
    last, round_of = {}, []
    for a, b in zip(kf1, kf2):
        r = max(last.get(int(a), -1), last.get(int(b), -1)) + 1
        last[int(a)] = last[int(b)] = r
        round_of.append(r)
    nr = max(round_of, default=-1) + 1
    order = sorted(range(len(round_of)), key=lambda i: (round_of[i], i))
    off = [0] * (nr + 1)
    for r in round_of:
        off[r + 1] += 1
    return np.array(round_of, np.int32), np.array(order, np.int32), np.cumsum(off).astype(np.int32)


# ---- the neighbour loop -----------------------------------------------------------------------------------------------------------------
def new_state(frames, cap):
    """(has_mp [B][cap] uint8, mp_xyz [B][cap][3], mp_id [B][cap]) from the frames' has_mp / mp_xyz"""
    B = len(frames)
    has, xyz, ids = np.zeros((B, cap), np.uint8), np.zeros((B, cap, 3), f32), np.full((B, cap), -1, np.int32)
    for b, f in enumerate(frames):
        n = len(f["has_mp"])
        has[b, :n] = f["has_mp"]
        if "mp_xyz" in f:
            xyz[b, :n] = f["mp_xyz"]
    return has, xyz, ids


def frame_key(f, i):
    raw = f.get("xy_raw", f["xy"])
    return key(f["xy"][i, 0], f["xy"][i, 1], f["octave"][i], f["depth"][i] if "depth" in f else -1.0, f["uRight"][i], raw[i, 0], raw[i, 1])


def one_pair(frames, i1, i2, has_mp, mp_xyz, cam, mb, mono, search, sf, s2, scale_factor, trig="canonical"):
    """one pass of the reference's loop body for neighbour i2 of keyframe i1 on the given slot state (read only) -> dict(skip,
    pairs [k][2], verdict [k], new_idx [m][2], new_xyz [m][3])"""
    f1, f2 = frames[i1], frames[i2]
    median = scene_median_depth(f2["Tcw"], has_mp[i2], mp_xyz[i2], len(f2["desc"]), 2) if mono else f32(0)
    skip = FO.f12_baseline_skip(f1["Ow"], f2["Ow"], mono, mb, median)
    out = dict(skip=skip, pairs=np.zeros((0, 2), np.int32), verdict=np.zeros(0, np.uint8), new_idx=np.zeros((0, 2), np.int32),
               new_xyz=np.zeros((0, 3), f32), median=median)
    if skip:
        return out
    k1 = dict(f1, has_mp=has_mp[i1, :len(f1["desc"])].copy())
    k2 = dict(f2, has_mp=has_mp[i2, :len(f2["desc"])].copy())
    pairs = search(k1, k2, cam)
    res = [triangulate_match(f1["Tcw"], f1["Ow"], f2["Tcw"], f2["Ow"], cam, mb, frame_key(f1, a), frame_key(f2, b), sf, s2, scale_factor, trig)
           for a, b in pairs]
    ok = [j for j, r in enumerate(res) if r[0] == OK]
    out.update(pairs=np.asarray(pairs, np.int32).reshape(-1, 2), verdict=np.array([r[0] for r in res], np.uint8),
               new_idx=np.asarray(pairs, np.int32).reshape(-1, 2)[ok], new_xyz=np.array([res[j][1] for j in ok], f32).reshape(-1, 3))
    return out


def _apply(out, pos, i1, i2, state, cap, id_base=0):
    has, xyz, ids = state
    for k, ((a, b), x) in enumerate(zip(out["new_idx"], out["new_xyz"])):
        for f, i in ((i1, a), (i2, b)):
            pid = id_base + pos * cap + k
            if pid > ids[f, i]:
                ids[f, i], has[f, i], xyz[f, i] = pid, 1, x


def serial_loop(frames, pairs, state, cap, pos=None, id_base=0, **kw):
    """the reference's loop: search -> triangulate -> fill slots, neighbour by neighbour in the given order.  pos[i] = the position
    that numbers pair i's points (default i); id_base is added to every id.  -> [one_pair dict]; `state` is updated in place."""
    outs = []
    for i, (i1, i2) in enumerate(pairs):
        o = one_pair(frames, i1, i2, state[0], state[1], **kw)
        # AddMapPoint overwrites: the later point stays.  Later = larger position here, which is the creation order whenever
        # pos ascends along the loop for the pairs that share a keyframe (plan_rounds keeps their order)
        _apply(o, i if pos is None else int(pos[i]), i1, i2, state, cap, id_base)
        outs.append(o)
    return outs


def round_loop(frames, pairs, round_off, state, cap, id_base=0, **kw):
    """the device's loop: every pair of a round reads the state at the start of the round; then the round's claims, the maximum id
    per slot.  `pairs` in round order; id_base is added to every id."""
    outs = []
    for r in range(len(round_off) - 1):
        frozen = (state[0].copy(), state[1].copy())
        rs = [(p, one_pair(frames, pairs[p][0], pairs[p][1], frozen[0], frozen[1], **kw)) for p in range(round_off[r], round_off[r + 1])]
        for p, o in rs:
            _apply(o, p, pairs[p][0], pairs[p][1], state, cap, id_base)
            outs.append(o)
    return outs
