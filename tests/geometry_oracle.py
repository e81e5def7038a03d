"""DynaSLAM::Geometry (perfect/src/Geometry.cc) restated in numpy, stage by stage, with every tap the library offers: the key-frame
ring (:532-550), GetRefFrames (:83-127), ExtractDynPoints (:136-471), RegionGrowing (:604-700), DepthRegionGrowing (:475-518) and
GeometricModelCorrection (:50-69).  Written from reading the fork's source and OpenCV 3.2's; UNPINNED: no OpenCV exists on any
machine of this project, so nothing here was compared with a compiled reference.  Imported by tests only.

float32 where the C++ uses float, float64 where it uses double, one operation at a time, no FMA.  The function names follow
csrc/orbfe_geometry_dev.h, which the kernels run.

OpenCV 3.2 behaviour restated here, with the file it was read from:
 O1  `A.inv() * B` with a plain B is MatOp_Invert::matmul -> MatOp_Solve: cv::solve(A, B, DECOMP_LU), and for a 4x4 CV_32F that is
     hal::LU32f = LUImpl<float> with partial pivoting over all columns, eps = FLT_EPSILON * 10 (modules/core/src/matop.cpp,
     lapack.cpp, hal_internal / matrix_decomp).  `K.inv() * X.t()`: e2 is a transpose, so MatOp::matmul evaluates the inverse
     (cv::invert's 3x3 case: determinant and cofactors in double, lapack.cpp) and issues gemm(.., GEMM_2_T) (matop.cpp).
 O2  cv::gemm (modules/core/src/matmul.cpp): with flags == 0 and an inner dimension len of 2..4 equal to the result's width or
     height there is a float-arithmetic block: `t = a0*b0 + a1*b1 + ..` in float, stored as (float)(t*alpha + c*beta).  For len 4 it
     serves (a) a result 4 columns wide and (b) a result 4 rows high (`len <= 16 && a != d`, always true); for len 3, a result 3
     wide or, 3 high, at most 16 columns wide.  Everything else goes to GEMMSingleMul_32f, which accumulates in double: the A * Bt
     branch (GEMM_2_T, or a one-column continuous B) keeps four partial sums s0..s3 over k in steps of 4 and adds s0 += s1 + s2 + s3;
     the plain branches add over k in order.  So in ExtractDynPoints: `mTcw * vAllMPw` (4x4 by 4xM) is float for every M;
     `K * aux` (3x3 by 3x4) is float and exact; `(K * aux) * vMPCurrentFrame` (3x4 by 4xh) is float only for h == 4, the A * Bt
     branch for h == 1 taken from a one-column matrix, and double sums in k order otherwise.
 O3  Mat::dot (dotProd_, matmul.cpp) and cv::norm (normL2_, stat.cpp) on float data accumulate in double; normL2Sqr takes the
     difference in the data's type first.
 O4  cv::meanStdDev (stat.cpp, sqsum_<float, double, double>): s += v, sq += (double)v * v over the rows in order; then
     mean = s * (1 / n), stddev = sqrt(max(sq * (1 / n) - mean * mean, 0)).
 O5  cv::minMaxLoc keeps the FIRST minimum (minMaxIdx_, stat.cpp: `<`).
 O6  `Mat /= s` is convertTo(.., 1. / s) (mat.inl.hpp): v * (1 / s) + 0; `0.7 * a + 0.3 * b` is addWeighted: a*0.7 + b*0.3 + 0.
 O7  getStructuringElement(MORPH_ELLIPSE) (modules/imgproc/src/morph.cpp): dx = cvRound(c * sqrt((r*r - dy*dy) * inv_r2)).
 O8  Mat::at<double> on a CV_32F matrix reads the 8 bytes at row * step + col * 8 (mat.inl.hpp): no conversion, no check in release.
"""
import math
import struct

import numpy as np

F = np.float32
D = np.float64
DB_SIZE, REF_FRAMES, INITIAL_MAP = 20, 5, 5
DMAX = 20
WIN = 2 * DMAX + 1
RAD = 15
NEIGH = ((-1, 0), (1, 0), (0, -1), (0, 1))
COUNT_NAMES = ("read", "depth", "parallax", "depth7", "in_frame", "found", "gate", "dyn")


# ---- the canonical acos (fdlibm e_acos.c), what geo_acos of csrc/orbfe_geometry_dev.h runs ------------------------------------------
def _words(x):
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    return u >> 32, u & 0xffffffff


def _clear_lo(x):
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    return struct.unpack("<d", struct.pack("<Q", u & 0xffffffff00000000))[0]


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(D(a) / D(b))


PI, PIO2_HI, PIO2_LO = 3.14159265358979311600e+00, 1.57079632679489655800e+00, 6.12323399573676603587e-17
PS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
      7.91534994289814532176e-04, 3.47933107596021167570e-05)
QS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)


def _pq(z):
    p = z * (PS[0] + z * (PS[1] + z * (PS[2] + z * (PS[3] + z * (PS[4] + z * PS[5])))))
    q = 1.0 + z * (QS[0] + z * (QS[1] + z * (QS[2] + z * QS[3])))
    return p, q


def geo_acos(x):
    x = float(x)
    hx, lx = _words(x)
    ix = hx & 0x7fffffff
    if ix >= 0x3ff00000:
        if ((ix - 0x3ff00000) | lx) == 0:
            return PI + 2.0 * PIO2_LO if hx >> 31 else 0.0
        return math.nan
    if ix < 0x3fe00000:
        if ix <= 0x3c600000:
            return PIO2_HI + PIO2_LO
        p, q = _pq(x * x)
        r = p / q
        return PIO2_HI - (x - (PIO2_LO - r * x))
    if hx >> 31:
        z = (1.0 + x) * 0.5
        p, q = _pq(z)
        s = math.sqrt(z)
        r = p / q
        w = r * s - PIO2_LO
        return PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _clear_lo(s)
    c = (z - df * df) / (s + df)
    p, q = _pq(z)
    r = p / q
    w = r * s + c
    return 2.0 * (df + w)


# ---- per-point arithmetic -------------------------------------------------------------------------------------------------------------
def geo_gemm_store(t):
    return F(D(t) * 1.0 + D(F(0)) * 0.0)


def geo_inv3(S):
    S = [D(v) for v in np.asarray(S, F).reshape(9)]
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0:
        return np.zeros(9, F)
    d = D(1.) / d
    return np.array([(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
                     (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
                     (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d], D).astype(F)


def geo_make_K(fx, fy, cx, cy):
    return np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], F)


class LU4:
    """geo_lu4_factor: LUImpl<float> on a copy of the 4x4 pose, the row operations recorded for geo_lu4_solve (O1)"""

    def __init__(self, T):
        A = np.array(T, F).reshape(4, 4).copy()
        self.alpha = np.zeros((4, 4), F)
        self.piv = [0, 1, 2, 3]
        self.ok = True
        eps = F(np.finfo(F).eps) * F(10)
        for i in range(4):
            k = i
            for j in range(i + 1, 4):
                if abs(A[j, i]) > abs(A[k, i]):
                    k = j
            self.piv[i] = k
            if abs(A[k, i]) < eps:
                self.ok = False
                break
            if k != i:
                A[[i, k], i:] = A[[k, i], i:]
            with np.errstate(all="ignore"):
                d = F(-1) / A[i, i]
                for j in range(i + 1, 4):
                    alpha = A[j, i] * d
                    self.alpha[j, i] = alpha
                    for q in range(i + 1, 4):
                        A[j, q] = A[j, q] + alpha * A[i, q]
            A[i, i] = -d
        self.A = A

    def solve(self, b):
        b = [F(v) for v in b]
        if not self.ok:
            return [F(0)] * 4
        with np.errstate(all="ignore"):
            for i in range(4):
                k = self.piv[i]
                if k != i:
                    b[i], b[k] = b[k], b[i]
                for j in range(i + 1, 4):
                    b[j] = b[j] + self.alpha[j, i] * b[i]
            for i in range(3, -1, -1):
                s = b[i]
                for k in range(i + 1, 4):
                    s = s - self.A[i, k] * b[k]
                b[i] = s * self.A[i, i]
        return b


def geo_backproject(Kinv, ux, uy, d):
    p = (F(ux), F(uy), F(1))
    b = []
    for i in range(3):
        s0 = D(0)
        for k in range(3):
            s0 = s0 + D(Kinv[i * 3 + k]) * D(p[k])
        s0 = s0 + ((D(0) + D(0)) + D(0))
        b.append(F(s0 * D(1)))
    with np.errstate(all="ignore"):
        b.append(F(D(1) / D(F(d))))
    return b


def parallax_angle(vmpw, invd, tref, tcur):
    """:214-227, the angle in degrees (NaN when the ratio is)"""
    with np.errstate(all="ignore"):
        a, c = [], []
        for k in range(3):
            mp = F(vmpw[k]) / F(invd)
            a.append(mp - F(tref[k]))
            c.append(mp - F(tcur[k]))
        dot = na = nc = D(0)
        for k in range(3):
            dot = dot + D(a[k]) * D(c[k])
        for k in range(3):
            na = na + D(a[k]) * D(a[k])
        for k in range(3):
            nc = nc + D(c[k]) * D(c[k])
        na, nc = np.sqrt(na), np.sqrt(nc)
        ratio = float(dot / (na * nc))
    return geo_acos(ratio) * 180 / math.pi


def geo_parallax_ok(vmpw, invd, tref, tcur):
    return parallax_angle(vmpw, invd, tref, tcur) < 30.0


def geo_to_current(T, v):
    T = np.asarray(T, F).reshape(16)
    with np.errstate(all="ignore"):
        o = [geo_gemm_store(T[i * 4] * v[0] + T[i * 4 + 1] * v[1] + T[i * 4 + 2] * v[2] + T[i * 4 + 3] * v[3]) for i in range(4)]
        o[0] = o[0] / o[3]
        o[1] = o[1] / o[3]
        o[2] = o[2] / o[3]
        o[3] = o[3] / o[3]
    return o


PROJ_DOUBLE, PROJ_FLOAT4, PROJ_SINGLE = 0, 1, 2


def geo_proj_mode(n_depth7, n_parallax):
    return PROJ_FLOAT4 if n_depth7 == 4 else PROJ_SINGLE if (n_depth7 == 1 and n_parallax == 1) else PROJ_DOUBLE


def geo_project(K, X, mode):
    m = []
    with np.errstate(all="ignore"):
        for i in range(3):
            a = (F(K[i * 3]), F(K[i * 3 + 1]), F(K[i * 3 + 2]), F(0))
            if mode == PROJ_FLOAT4:
                m.append(geo_gemm_store(a[0] * X[0] + a[1] * X[1] + a[2] * X[2] + a[3] * X[3]))
            elif mode == PROJ_SINGLE:
                s = [D(0) + D(a[k]) * D(X[k]) for k in range(4)]
                m.append(F((s[0] + (s[1] + s[2] + s[3])) * D(1)))
            else:
                s0 = D(0)
                for k in range(4):
                    s0 = s0 + D(a[k]) * D(X[k])
                m.append(F(s0 * D(1)))
        return np.ceil(m[0] / m[2]), np.ceil(m[1] / m[2])


def geo_in_frame(x, y, w, h):
    return bool(x > F(DMAX + 1) and x < F(w - DMAX - 1) and y > F(DMAX + 1) and y < F(h - DMAX - 1))


def ellipse_half_widths(r):
    """O7 for a (2r+1) x (2r+1) ellipse anchored at its centre: row i covers columns r - dx .. r + dx"""
    inv_r2 = 1. / (float(r) * r) if r else 0.
    return [int(np.rint(r * math.sqrt((r * r - (i - r) * (i - r)) * inv_r2))) for i in range(2 * r + 1)]


# ---- 1: the ring -----------------------------------------------------------------------------------------------------------------------
class DataBase:
    def __init__(self):
        self.ini = self.fin = self.num = 0
        self.slots = [None] * DB_SIZE

    def is_full(self):
        return self.ini == (self.fin + 1) % DB_SIZE

    def insert(self, frame):
        if not self.is_full():
            self.slots[self.fin] = frame
            self.fin = (self.fin + 1) % DB_SIZE
            self.num += 1
        else:
            self.slots[self.ini] = frame
            self.fin = self.ini
            self.ini = (self.ini + 1) % DB_SIZE


# ---- 2: GetRefFrames -----------------------------------------------------------------------------------------------------------------
def pose_as_double(T, i, j):
    """O8: `R.at<double>(i, j)` of the pose's 3x3 block (row step 16 bytes)"""
    raw = np.ascontiguousarray(T, F).tobytes()
    return struct.unpack_from("<d", raw, i * 16 + j * 8)[0]


def rotm2euler(T, punned=True):
    """:553-573.  punned=False reads the rotation as it was meant, for tests that show the difference."""
    R = (lambda i, j: pose_as_double(T, i, j)) if punned else (lambda i, j: float(np.asarray(T, F).reshape(4, 4)[i, j]))
    with np.errstate(all="ignore"):
        sy = F(np.sqrt(D(R(0, 0)) * D(R(0, 0)) + D(R(1, 0)) * D(R(1, 0))))
    if not float(sy) < 1e-6:
        x = F(math.atan2(R(2, 1), R(2, 2)))
        y = F(math.atan2(-R(2, 0), float(sy)))
        z = F(math.atan2(R(1, 0), R(0, 0)))
    else:
        x = F(math.atan2(-R(1, 2), R(1, 1)))
        y = F(math.atan2(-R(2, 0), float(sy)))
        z = F(0)
    return [float(x), float(y), float(z)]


def ref_scores(cur_T, db_T):
    cur = np.asarray(cur_T, F).reshape(16)
    e1 = rotm2euler(cur)
    vdist, vrot = [], []
    for T in db_T:
        T = np.asarray(T, F).reshape(16)
        e2 = rotm2euler(T)
        sr = st = 0.0
        for k in range(3):
            v = e2[k] - e1[k]
            sr = sr + v * v
        for k in range(3):
            v = float(T[k * 4 + 3] - cur[k * 4 + 3])
            st = st + v * v
        vrot.append(math.sqrt(sr))
        vdist.append(math.sqrt(st))
    sd, sr = _div(1., max(vdist)), _div(1., max(vrot))
    return [(d * sd + 0.) * 0.7 + (r * sr + 0.) * 0.3 + 0. for d, r in zip(vdist, vrot)]


def select_ref_frames(cur_T, db_T):
    score = ref_scores(cur_T, db_T)
    assert len(set(score)) == len(score), "equal scores: cv::sortIdx is not stable, outside the contract"
    return sorted(range(len(score)), key=lambda i: -score[i])[:min(REF_FRAMES, len(score))]


# ---- 3: ExtractDynPoints -----------------------------------------------------------------------------------------------------------
def extract_dyn_points(refs, cur_T, cur_depth, fx, fy, cx, cy):
    """refs: the reference frames in GetRefFrames' order, each a dict(Tcw, depth, keys [n][2], keys_un [n][2]).
    Returns (dyn int32 [m][3] of (x, y, label), counts dict by COUNT_NAMES, stages dict of intermediate lists)."""
    cur_T = np.asarray(cur_T, F).reshape(16)
    cur_depth = np.asarray(cur_depth, F)
    h, w = cur_depth.shape
    K = geo_make_K(fx, fy, cx, cy)
    Kinv = geo_inv3(K)
    tcur = (cur_T[3], cur_T[7], cur_T[11])
    cnt = dict.fromkeys(COUNT_NAMES, 0)
    pts = []   # (vMPw, label) of the parallax survivors
    angles = []
    for label, ref in enumerate(refs):
        T = np.asarray(ref["Tcw"], F).reshape(16)
        lu = LU4(T)
        tref = (T[3], T[7], T[11])
        dep = np.asarray(ref["depth"], F)
        rh, rw = dep.shape
        for kp, un in zip(np.asarray(ref["keys"], F).reshape(-1, 2), np.asarray(ref["keys_un"], F).reshape(-1, 2)):
            cnt["read"] += 1
            d = F(0)
            if kp[0] > F(-1) and kp[0] < F(rw) and kp[1] > F(-1) and kp[1] < F(rh):
                d = dep[int(kp[1]), int(kp[0])]
            if not (d > 0 and d < 6):
                continue
            cnt["depth"] += 1
            b = geo_backproject(Kinv, un[0], un[1], d)
            invd = b[3]
            v = lu.solve(b)
            ang = parallax_angle(v, invd, tref, tcur)
            angles.append(ang)
            if not ang < 30.0:
                continue
            cnt["parallax"] += 1
            pts.append((v, label))
    cur = []
    for v, label in pts:
        o = geo_to_current(cur_T, v)
        if o[2] < 7:
            cur.append((o, label))
    cnt["depth7"] = len(cur)
    mode = geo_proj_mode(len(cur), len(pts))
    dyn, proj_px = [], []
    for o, label in cur:
        x, y = geo_project(K, o, mode)
        if not geo_in_frame(x, y, w, h):
            continue
        xi, yi = int(x), int(y)
        if not cur_depth[yi, xi] > 0:
            continue
        cnt["in_frame"] += 1
        proj = o[2]
        proj_px.append((xi, yi, float(proj)))
        # the 41x41 window in scan order: x offset outer, y offset inner
        win = cur_depth[yi - DMAX:yi + DMAX + 1, xi - DMAX:xi + DMAX + 1]
        scan = win.T.reshape(-1)
        ok = (scan > 0) & (scan < proj)
        if not ok.any():
            continue
        cnt["found"] += 1
        diff = (proj - scan[ok]).astype(F)
        best = diff[int(np.argmin(diff))]   # O5: the first minimum
        if not best > F(0.6):
            continue
        cnt["gate"] += 1
        rows = win.reshape(-1).astype(D)   # O4: row order
        s = np.cumsum(rows)[-1]
        sq = np.cumsum(rows * rows)[-1]
        scale = D(1.) / D(WIN * WIN)
        s = s * scale
        sd = np.sqrt(max(sq * scale - s * s, D(0.)))
        if not sd * sd < D(F(0.001)):
            continue
        dyn.append((xi, yi, label))
    cnt["dyn"] = len(dyn)
    return np.array(dyn, np.int32).reshape(-1, 3), cnt, dict(angles=angles, projected=proj_px, mode=mode)


# ---- 4: RegionGrowing ----------------------------------------------------------------------------------------------------------------
def region_growing(im, x, y, maxdist=F(0.20), trace=None):
    """:604-700: J (uint8, region and frontier) of the seed (x, y).  trace, a list, receives (index, x, y, pixdist) per step."""
    im = np.asarray(im, F)
    h, w = im.shape
    J = np.zeros((h, w), np.int8)
    reg_mean = im[y, x]
    reg_size = 1
    neg_pos = -1
    lx = np.zeros(w * h + 8, np.int32)
    ly = np.zeros(w * h + 8, np.int32)
    ld = np.zeros(w * h + 8, F)
    pixdist = 0.0
    while pixdist < float(maxdist) and reg_size < w * h:
        for dx, dy in NEIGH:
            xn, yn = x + dx, y + dy
            if xn >= 0 and yn >= 0 and xn < w and yn < h and J[yn, xn] == 0:
                neg_pos += 1
                lx[neg_pos], ly[neg_pos], ld[neg_pos] = xn, yn, im[yn, xn]
                J[yn, xn] = 1
        if neg_pos >= 1:   # the candidates are the entries below neg_pos: the last one is never one
            dist = np.abs(ld[:neg_pos] - reg_mean)
            index = int(np.argmin(dist))
            pixdist = float(dist[index])
            J[y, x] = -1
            reg_size += 1
            reg_mean = (reg_mean * F(reg_size) + ld[index]) / F(reg_size + 1)
            x, y = int(lx[index]), int(ly[index])
            if trace is not None:
                trace.append((index, x, y, pixdist))
            lx[index], ly[index], ld[index] = lx[neg_pos], ly[neg_pos], ld[neg_pos]
            neg_pos -= 1
        else:
            pixdist = float(maxdist)
    return np.abs(J).astype(np.uint8)


# ---- 5: DepthRegionGrowing -----------------------------------------------------------------------------------------------------------
def dilate_ellipse(u, r=RAD):
    """cv::dilate with the (2r+1)^2 MORPH_ELLIPSE, zeros outside the image"""
    h, w = u.shape
    pad = np.zeros((h + 2 * r, w + 2 * r + 1), np.int64)
    pad[r:r + h, r + 1:r + 1 + w] = u != 0
    pre = np.cumsum(pad, axis=1)
    out = np.zeros((h, w), bool)
    for i, hw in enumerate(ellipse_half_widths(r)):
        rows = pre[i:i + h]
        out |= rows[:, r + hw + 1:r + hw + 1 + w] != rows[:, r - hw:r - hw + w]
    return out.astype(np.uint8)


def depth_region_growing(seeds, depth):
    """seeds: (x, y) in order.  Returns (mask, accepted flags, union before the dilation, regions of the accepted seeds by index)."""
    depth = np.asarray(depth, F)
    union = np.zeros(depth.shape, np.uint8)
    accepted = np.zeros(len(seeds), np.uint8)
    regions = {}
    for i, (x, y) in enumerate(seeds):
        x, y = int(x), int(y)
        if union[y, x] != 1 and depth[y, x] > 0:
            J = region_growing(depth, x, y)
            union |= J
            accepted[i] = 1
            regions[i] = J
    dil = dilate_ellipse(union) if len(seeds) else union
    return (1 - dil).astype(np.uint8), accepted, union, regions


# ---- 6: GeometricModelCorrection -------------------------------------------------------------------------------------------------------
class Geometry:
    def __init__(self):
        self.db = DataBase()
        self.taps = None

    def update_db(self, Tcw, depth, keys, keys_un):
        self.db.insert(dict(Tcw=np.array(Tcw, F).reshape(16), depth=np.array(depth, F), keys=np.array(keys, F).reshape(-1, 2),
                            keys_un=np.array(keys_un, F).reshape(-1, 2)))

    def correct(self, depth, Tcw, fx, fy, cx, cy):
        """(mask, computed); self.taps = dict(refs, dyn, counts, accepted, union, regions)"""
        depth = np.asarray(depth, F)
        self.taps = None
        if Tcw is None or self.db.num < INITIAL_MAP:
            return np.ones(depth.shape, np.uint8), 0
        frames = self.db.slots[:self.db.num]
        refs = select_ref_frames(Tcw, [f["Tcw"] for f in frames])
        dyn, counts, stages = extract_dyn_points([frames[i] for i in refs], Tcw, depth, fx, fy, cx, cy)
        mask, accepted, union, regions = depth_region_growing([(x, y) for x, y, _ in dyn], depth)
        self.taps = dict(refs=refs, dyn=dyn, counts=counts, accepted=accepted, union=union, regions=regions, stages=stages)
        return mask, 1
