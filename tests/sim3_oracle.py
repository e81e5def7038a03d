"""CPU oracle of the reference's Sim3Solver (src/Sim3Solver.cc; Horn 1987 on three point pairs inside a RANSAC loop), stage by
stage: constructor quantities, triple from draws, N matrix, float Jacobi, rotation, scale / t / T12 / T21, per-point errors
and the `iterate` loop with its state.

float32 where the C++ uses float, float64 where it uses double, one operation at a time, no FMA.  Two modes: "canonical"
(atan2 / sin / cos are the fixed fp64 operation sequences below: fdlibm's polynomials and Cody-Waite reduction, what the
kernel of csrc/orbfe_sim3.hip runs) and "libm" (math.atan2 / sin / cos of the host).

UNPINNED.  OpenCV is not available to this project, so the OpenCV 3.2 behaviour below rests on knowledge of its sources:

  S1  cv::reduce(P, C, 1, CV_REDUCE_SUM) of a CV_32F matrix sums in float through reduceC_: a0 = s[0], a1 = s[1], the tail
      adds s[2] to a0, then a0 + a1: (s0 + s2) + s1.  `C / P.cols` is a MatExpr with alpha = 1. / cols, assigned through
      convertTo: v * (float)alpha + 0.0f (cvtScale_ with float work type).  Every other `scalar * Mat` is evaluated the same
      way: one float product per element, plus 0.0f.
  S2  Small matrix products (M = Pr2 * Pr1^T, P3 = R * Pr2, sR * O2, sRinv * t, Rcw * X + tcw) accumulate left to right in
      float, (a0*b0 + a1*b1) + a2*b2, then + t: the one convention csrc/orbfe_hostgeom.hip documents.  Expressions are
      evaluated as written, left to right: t = O1 - ((s*R) * O2), tinv = -(sRinv * t).  (OpenCV folds some of them into a
      single gemm with a double alpha; that is not followed.)
  S3  The ten N entries are declared double; they are evaluated in double from the float M entries, left to right, and
      stored to float by the Mat_<float> initialiser.
  S4  cv::eigen of a CV_32F matrix is JacobiImpl_<float>: FLT_EPSILON, lapack.cpp's hypot template in float, at most
      n*n*30 rotations, selection sort to descending eigenvalues with the eigenvector rows swapped along.
  S5  cv::norm(vec) of 1x3 CV_32F sums the squares serially in double (normL2Sqr_<float, double>, tail loop), then sqrt.
  S6  vec = 2*ang*vec/norm(vec): `2*ang*vec` is a MatExpr with alpha = 2*ang; `/ norm` multiplies alpha by 1./norm; the
      assignment is convertTo: vec[i] * (float)((2*ang) * (1./norm)) + 0.0f.  norm == 0 gives 0 * inf (or 2*pi * inf, then
      inf * 0): NaN in every component.
  S7  cv::Rodrigues, vector branch of 3.2's cvRodrigues2: r in double, theta = sqrt(rx*rx + ry*ry + rz*rz); theta <
      DBL_EPSILON gives the identity; else c, s, c1 = 1 - c, r *= 1/theta, R = (c*I + c1*r*r^T) + s*[r]x per element (Matx
      arithmetic), converted to float.  A NaN theta takes the else branch and gives an all-NaN R.
  S8  Mat::dot of two continuous 3x3 CV_32F matrices is dotProd_<float> over 9 elements: double accumulation unrolled by
      four (r += a0*b0 + a1*b1 + a2*b2 + a3*b3), then a serial tail.  cv::pow(P3, 2) is a float multiply.  dist.dot(dist)
      of a 2x1 is the serial tail: (double)d0*d0 + (double)d1*d1.
  S9  DUtils::Random::RandomInt(min, max) is not in the tree; written from knowledge: d = max - min + 1,
      (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min.  The draws are an input here: raw values r in
      [0, 2^31 - 1] (bit 31 of a draw is ignored), index = (int)(((double)r / 2147483648.0) * size).
  S10 Fewer than 3 correspondences with min_inliers <= N (undefined in the reference: RandomInt(0, -1)): no model,
      bNoMore.
"""
import math
import struct

import numpy as np

F = np.float32
DBL_EPSILON = 2.220446049250313e-16
FLT_EPSILON = F(np.finfo(np.float32).eps)
ZERO = F(0)

# ---- the break switch (tests/test_sim3_edge_cases.py) -------------------------------------------------------------------------
# One rule at a time is broken to show that a case table would notice.  Empty: the oracle proper, bit for bit.
SIM3_RULES = {
    "tie_gt": "a count equal to the best does not replace it (> for >=)",
    "return_ge": "a count equal to min_inliers returns (>= for >)",
    "clamp_le": "the loop runs while iterations <= max_its",
    "fix_scale_ignored": "the scale is 1 whatever fix_scale says",
    "max_errors_no_trunc": "the thresholds are 9.210 * sigma2 without the integer truncation",
    "no_identity_arm": "Rodrigues without its theta < DBL_EPSILON arm",
}
SIM3_BREAK = frozenset()


# ---- canonical fp64 atan2 / sin / cos ------------------------------------------------------------------------------------------
def _hi(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def _from_hi(hi):
    return struct.unpack("<d", struct.pack("<Q", (hi & 0xffffffff) << 32))[0]


def _div(a, b):
    """IEEE a / b for Python floats"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
      9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
      4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)
PI = 3.1415926535897931160e+00
PI_LO = 1.2246467991473531772e-16
PIO2_HI = 1.57079632679489655800e+00


def c_atan_pos(x):
    """fdlibm's atan for a finite x >= 0"""
    if x >= 7.378697629483821e19:   # 2^66
        return ATANHI[3] + ATANLO[3]
    if x < 0.4375:
        if x < 1.862645149230957e-09:   # 2^-29
            return x
        idx = -1
    elif x < 1.1875:
        if x < 0.6875:
            idx = 0
            x = (2.0 * x - 1.0) / (2.0 + x)
        else:
            idx = 1
            x = (x - 1.0) / (x + 1.0)
    elif x < 2.4375:
        idx = 2
        x = (x - 1.5) / (1.0 + 1.5 * x)
    else:
        idx = 3
        x = -1.0 / x
    z = x * x
    w = z * z
    s1 = z * (AT[0] + w * (AT[2] + w * (AT[4] + w * (AT[6] + w * (AT[8] + w * AT[10])))))
    s2 = w * (AT[1] + w * (AT[3] + w * (AT[5] + w * (AT[7] + w * AT[9]))))
    if idx < 0:
        return x - x * (s1 + s2)
    z = ATANHI[idx] - ((x * (s1 + s2) - ATANLO[idx]) - x)
    return z


def c_atan2(y, x):
    """canonical atan2: fdlibm's __ieee754_atan2 for finite arguments; NaN when either is NaN or infinite"""
    y = float(y)
    x = float(x)
    if not (math.isfinite(x) and math.isfinite(y)):
        return math.nan
    xneg = math.copysign(1.0, x) < 0
    yneg = math.copysign(1.0, y) < 0
    if y == 0:
        if not xneg:
            return y
        return -PI if yneg else PI
    if x == 0:
        return -PIO2_HI if yneg else PIO2_HI
    ix = _hi(x) & 0x7fffffff
    iy = _hi(y) & 0x7fffffff
    k = (iy - ix) >> 20
    if k > 60:
        z = PIO2_HI + 0.5 * PI_LO
    elif xneg and k < -60:
        z = 0.0
    else:
        z = c_atan_pos(abs(y / x))
    if not xneg:
        return -z if yneg else z
    if not yneg:
        return PI - (z - PI_LO)
    return (z - PI_LO) - PI


INVPIO2 = 6.36619772367581382433e-01
PIO2_1 = 1.57079632673412561417e+00
PIO2_1T = 6.07710050650619224932e-11
PIO2_2 = 6.07710050630396597660e-11
PIO2_2T = 2.02226624879595063154e-21
PIO2_3 = 2.02226624871116645580e-21
PIO2_3T = 8.47842766036889956997e-32
TRIG_MAX = 823549.0   # the Cody-Waite range of fdlibm's medium path; past it the canonical functions are NaN by definition
S1, S2, S3, S4, S5, S6 = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
                          2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
C1, C2, C3, C4, C5, C6 = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
                          -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)


def c_rem_pio2(x):
    """x >= 0 finite, x <= TRIG_MAX: (n, y0, y1) with x = n*pi/2 + y0 + y1.  x <= pi/4 (by high word): n = 0, y0 = x.  Else
    the Cody-Waite steps of fdlibm's medium path, always (fdlibm's shortcuts for n = 1 are left out)."""
    ix = _hi(x) & 0x7fffffff
    if ix <= 0x3fe921fb:
        return 0, x, 0.0
    n = int(x * INVPIO2 + 0.5)
    fn = float(n)
    r = x - fn * PIO2_1
    w = fn * PIO2_1T
    j = ix >> 20
    y0 = r - w
    i = j - ((_hi(y0) >> 20) & 0x7ff)
    if i > 16:
        t = r
        w = fn * PIO2_2
        r = t - w
        w = fn * PIO2_2T - ((t - r) - w)
        y0 = r - w
        i = j - ((_hi(y0) >> 20) & 0x7ff)
        if i > 49:
            t = r
            w = fn * PIO2_3
            r = t - w
            w = fn * PIO2_3T - ((t - r) - w)
            y0 = r - w
    y1 = (r - y0) - w
    return n, y0, y1


def c_ksin(x, y, iy):
    """fdlibm's __kernel_sin"""
    ix = _hi(x) & 0x7fffffff
    if ix < 0x3e400000:
        return x
    z = x * x
    v = z * x
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    if iy == 0:
        return x + v * (S1 + z * r)
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def c_kcos(x, y):
    """fdlibm's __kernel_cos"""
    ix = _hi(x) & 0x7fffffff
    if ix < 0x3e400000:
        return 1.0
    z = x * x
    r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    if ix < 0x3fd33333:
        return 1.0 - (0.5 * z - (z * r - x * y))
    qx = 0.28125 if ix > 0x3fe90000 else _from_hi(ix - 0x00200000)
    hz = 0.5 * z - qx
    a = 1.0 - qx
    return a - (hz - (z * r - x * y))


def c_sin(x):
    x = float(x)
    if not math.isfinite(x) or abs(x) > TRIG_MAX:
        return math.nan
    neg = math.copysign(1.0, x) < 0
    n, y0, y1 = c_rem_pio2(abs(x))
    if n == 0:
        v = c_ksin(y0, 0.0, 0)
    else:
        q = n & 3
        v = c_ksin(y0, y1, 1) if q == 0 else c_kcos(y0, y1) if q == 1 else -c_ksin(y0, y1, 1) if q == 2 else -c_kcos(y0, y1)
    return -v if neg else v


def c_cos(x):
    x = float(x)
    if not math.isfinite(x) or abs(x) > TRIG_MAX:
        return math.nan
    n, y0, y1 = c_rem_pio2(abs(x))
    if n == 0:
        return c_kcos(y0, 0.0)
    q = n & 3
    return c_kcos(y0, y1) if q == 0 else -c_ksin(y0, y1, 1) if q == 1 else -c_kcos(y0, y1) if q == 2 else c_ksin(y0, y1, 1)


def trig(mode):
    if mode == "canonical":
        return c_atan2, c_sin, c_cos
    if mode == "libm":
        return math.atan2, math.sin, math.cos
    raise ValueError(mode)


# ---- constructor quantities ----------------------------------------------------------------------------------------------------
def affine(R, t, X):
    """R (3x3) * X[i] + t for every row of X [n, 3], float, left to right (S2)"""
    R = np.asarray(R, F).reshape(3, 3)
    t = np.asarray(t, F).reshape(3)
    X = np.asarray(X, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1]) + R[k, 2] * X[:, 2]) + t[k] for k in range(3)], 1)


def camera_points(Xw, Rcw, tcw):
    """mvX3Dc: Rcw * Xw + tcw (:80, :83)"""
    return affine(Rcw, tcw, Xw)


def max_errors(sigma2):
    """mvnMaxError: (size_t)(9.210 * (double)sigma2), as the float it becomes in `err < maxError` (:71-72, :359)"""
    s = np.asarray(sigma2, F).reshape(-1).astype(np.float64)
    if "max_errors_no_trunc" in SIM3_BREAK:
        return (9.210 * s).astype(F)
    return np.floor(9.210 * s).astype(np.uint64).astype(F)


def to_image(Xc, K):
    """FromCameraToImage / the tail of Project: K = (fx, fy, cx, cy)"""
    fx, fy, cx, cy = (F(v) for v in K)
    Xc = np.asarray(Xc, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        invz = F(1) / Xc[:, 2]
        x = Xc[:, 0] * invz
        y = Xc[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1)


def ransac_iterations(probability, min_inliers, max_its, n):
    """SetRansacParameters' clamp (:99-123), with the host's libm"""
    if n <= 0:
        return 1
    eps = F(min_inliers) / F(n)
    if min_inliers == n:
        its = 1
    else:
        e3 = math.pow(float(eps), 3)
        den = math.log(1 - e3) if e3 < 1 else -math.inf
        v = _div(math.log(1 - probability), den)
        # ceil() of a double converted to int: out of range (inf / NaN) is INT_MIN on x86-64
        its = int(math.ceil(v)) if math.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31
    return max(1, min(its, max_its))


# ---- draws -> triple -----------------------------------------------------------------------------------------------------------
def index_from_draw(r, size):
    return int((float(int(r) & 0x7fffffff) / 2147483648.0) * size)


def triple_from_draws(d3, n):
    avail = list(range(n))
    out = []
    for r in d3:
        k = index_from_draw(r, len(avail))
        out.append(avail[k])
        avail[k] = avail[-1]
        avail.pop()
    return out


# ---- ComputeSim3 ---------------------------------------------------------------------------------------------------------------
def centroid(P):
    """P: 3x3 float32, one point per column -> (Pr, C) (S1)"""
    with np.errstate(all="ignore"):
        C = ((P[:, 0] + P[:, 2]) + P[:, 1]) * F(1.0 / 3.0) + ZERO
        return P - C[:, None], C


def n_matrix(P1, P2):
    """-> (N float32 4x4, Pr1, Pr2, O1, O2, M)"""
    P1 = np.asarray(P1, F).reshape(3, 3)
    P2 = np.asarray(P2, F).reshape(3, 3)
    Pr1, O1 = centroid(P1)
    Pr2, O2 = centroid(P2)
    M = np.zeros((3, 3), F)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                M[i, j] = (Pr2[i, 0] * Pr1[j, 0] + Pr2[i, 1] * Pr1[j, 1]) + Pr2[i, 2] * Pr1[j, 2]
    m = M.astype(np.float64)
    N11 = m[0, 0] + m[1, 1] + m[2, 2]
    N12 = m[1, 2] - m[2, 1]
    N13 = m[2, 0] - m[0, 2]
    N14 = m[0, 1] - m[1, 0]
    N22 = m[0, 0] - m[1, 1] - m[2, 2]
    N23 = m[0, 1] + m[1, 0]
    N24 = m[2, 0] + m[0, 2]
    N33 = -m[0, 0] + m[1, 1] - m[2, 2]
    N34 = m[1, 2] + m[2, 1]
    N44 = -m[0, 0] - m[1, 1] + m[2, 2]
    with np.errstate(all="ignore"):
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], np.float64).astype(F)
    return N, Pr1, Pr2, O1, O2, M


def hypot_f32(a, b):
    a = abs(a)
    b = abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(F(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F(1) + a * a)
    return ZERO


def jacobi_f32(A_in):
    """eigen() of a symmetric n x n CV_32F matrix (S4): (W descending float32 [n], V rows = eigenvectors float32 [n, n])"""
    A0 = np.asarray(A_in, F)
    n = A0.shape[0]
    A = [F(v) for v in A0.ravel()]
    V = [ZERO] * (n * n)
    for i in range(n):
        V[i * n + i] = F(1)
    W = [ZERO] * n
    indR = [0] * n
    indC = [0] * n

    def row_max(k):
        m = k + 1
        mv = abs(A[n * k + m])
        for i in range(k + 2, n):
            val = abs(A[n * k + i])
            if mv < val:
                mv, m = val, i
        indR[k] = m

    def col_max(k):
        m = 0
        mv = abs(A[k])
        for i in range(1, k):
            val = abs(A[n * i + k])
            if mv < val:
                mv, m = val, i
        indC[k] = m

    with np.errstate(all="ignore"):
        for k in range(n):
            W[k] = A[(n + 1) * k]
            if k < n - 1:
                row_max(k)
            if k > 0:
                col_max(k)
        for _ in range(n * n * 30 if n > 1 else 0):
            k = 0
            mv = abs(A[indR[0]])
            for i in range(1, n - 1):
                val = abs(A[n * i + indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[n * indC[i] + i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[n * k + l]
            if abs(p) <= FLT_EPSILON:
                break
            y = (W[l] - W[k]) * F(0.5)
            t = abs(y) + hypot_f32(p, y)
            s = hypot_f32(p, t)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[n * k + l] = ZERO
            W[k] = W[k] - t
            W[l] = W[l] + t

            def rot(M, i0, i1):
                a0, b0 = M[i0], M[i1]
                M[i0] = a0 * c - b0 * s
                M[i1] = a0 * s + b0 * c

            for i in range(k):
                rot(A, n * i + k, n * i + l)
            for i in range(k + 1, l):
                rot(A, n * k + i, n * i + l)
            for i in range(l + 1, n):
                rot(A, n * k + i, n * l + i)
            for i in range(n):
                rot(V, n * k + i, n * l + i)
            for idx in (k, l):
                if idx < n - 1:
                    row_max(idx)
                if idx > 0:
                    col_max(idx)
        for k in range(n - 1):
            m = k
            for i in range(k + 1, n):
                if W[m] < W[i]:
                    m = i
            if k != m:
                W[m], W[k] = W[k], W[m]
                for i in range(n):
                    V[n * m + i], V[n * k + i] = V[n * k + i], V[n * m + i]
    return np.array(W, F), np.array(V, F).reshape(n, n)


def rotation_from_n(N, mode="canonical", trace=None):
    """eigen -> quaternion -> angle-axis -> cv::Rodrigues (S4-S7): R float32 3x3.  trace["identity"]: the theta < DBL_EPSILON arm"""
    atan2, sin, cos = trig(mode)
    _, V = jacobi_f32(N)
    vec = V[0, 1:4].copy()
    v = [float(q) for q in vec]
    nrm = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    ang = atan2(nrm, float(V[0, 0]))
    alpha = (2.0 * ang) * _div(1.0, nrm)
    with np.errstate(all="ignore"):
        vec = vec * F(alpha) + ZERO
    rx, ry, rz = (float(q) for q in vec)
    theta = math.sqrt(rx * rx + ry * ry + rz * rz)
    if trace is not None:
        trace["identity"] = bool(theta < DBL_EPSILON)
    if theta < DBL_EPSILON and "no_identity_arm" not in SIM3_BREAK:
        return np.eye(3, dtype=F)
    c = cos(theta)
    s = sin(theta)
    c1 = 1.0 - c
    it = _div(1.0, theta)
    r = (rx * it, ry * it, rz * it)
    eye = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    rxm = ((0.0, -r[2], r[1]), (r[2], 0.0, -r[0]), (-r[1], r[0], 0.0))
    R = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            R[i, j] = (c * eye[i][j] + c1 * (r[i] * r[j])) + s * rxm[i][j]
    with np.errstate(all="ignore"):
        return R.astype(F)


def mat3(A, B):
    """3x3 * 3xk in float, left to right (S2)"""
    with np.errstate(all="ignore"):
        return np.stack([(A[i, 0] * B[0] + A[i, 1] * B[1]) + A[i, 2] * B[2] for i in range(3)], 0)


def compute_sim3(P1, P2, fix_scale, mode="canonical"):
    """ComputeSim3 (:221-340): dict of R [3, 3], s, t [3], T12 [4, 4], T21 [4, 4] (float32) and N; the trace: identity (Rodrigues
    took its theta < DBL_EPSILON arm) and finite (every entry of T12 and T21 is)"""
    N, Pr1, Pr2, O1, O2, _ = n_matrix(P1, P2)
    tr = {}
    R = rotation_from_n(N, mode, tr)
    if "fix_scale_ignored" in SIM3_BREAK:
        fix_scale = True
    P3 = mat3(R, Pr2)
    if not fix_scale:
        a = [float(q) for q in Pr1.ravel()]
        b = [float(q) for q in P3.ravel()]
        nom = 0.0
        for i in (0, 4):
            nom += ((a[i] * b[i] + a[i + 1] * b[i + 1]) + a[i + 2] * b[i + 2]) + a[i + 3] * b[i + 3]
        nom += a[8] * b[8]
        with np.errstate(all="ignore"):
            sq = P3 * P3
        den = 0.0
        for q in sq.ravel():
            den += float(q)
        with np.errstate(all="ignore"):
            s = F(_div(nom, den))
    else:
        s = F(1)
    with np.errstate(all="ignore"):
        sR = R * s + ZERO
        t = O1 - mat3(sR, O2)
        T12 = np.eye(4, dtype=F)
        T12[:3, :3] = sR
        T12[:3, 3] = t
        sRinv = R.T * F(_div(1.0, float(s))) + ZERO
        tinv = -mat3(sRinv, t)
        T21 = np.eye(4, dtype=F)
        T21[:3, :3] = sRinv
        T21[:3, 3] = tinv
    return dict(R=R, s=s, t=t, T12=T12, T21=T21, N=N, identity=tr["identity"], finite=bool(np.isfinite(T12).all() and np.isfinite(T21).all()))


# ---- CheckInliers --------------------------------------------------------------------------------------------------------------
def errors(X1, X2, p1, p2, T12, T21, K1, K2):
    """err1 / err2 (float32 [n]) of CheckInliers (:343-367)"""
    q21 = to_image(affine(T12[:3, :3], T12[:3, 3], X2), K1)
    q12 = to_image(affine(T21[:3, :3], T21[:3, 3], X1), K2)
    with np.errstate(all="ignore"):
        d1 = (p1 - q21).astype(np.float64)
        d2 = (q12 - p2).astype(np.float64)
        e1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(F)
        e2 = (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(F)
    return e1, e2


# ---- the solver ----------------------------------------------------------------------------------------------------------------
class Solver:
    """Sim3Solver on the flattened inputs: X1 / X2 [n, 3] camera-frame points, sigma2_1 / sigma2_2 [n], K = (fx, fy, cx, cy).
    State across iterate calls: iterations, best_inliers, best (R, t, s, T12), best_mask."""

    def __init__(self, X1, X2, sigma2_1, sigma2_2, K1, K2, fix_scale=True, mode="canonical"):
        self.X1 = np.ascontiguousarray(X1, F).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2, F).reshape(-1, 3)
        self.n = len(self.X1)
        self.K1 = tuple(F(v) for v in K1)
        self.K2 = tuple(F(v) for v in K2)
        self.thr1 = max_errors(sigma2_1)
        self.thr2 = max_errors(sigma2_2)
        self.p1 = to_image(self.X1, self.K1)
        self.p2 = to_image(self.X2, self.K2)
        self.fix_scale = bool(fix_scale)
        self.mode = mode
        self.iterations = 0
        self.best_inliers = 0
        self.best = None
        self.best_mask = np.zeros(self.n, np.uint8)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_its=300):
        self.min_inliers = int(min_inliers)
        self.max_its = ransac_iterations(probability, min_inliers, max_its, self.n)
        self.iterations = 0

    def iterate(self, n_iterations, draws):
        """draws: at least 3 * n_iterations raw values.  -> dict(found, no_more, n_inliers, T12 (or None), mask uint8 [n],
        iterations_run, log); log[i] = dict(triple, T12, T21, R, s, t, count, err1, err2) of the i-th iteration run."""
        out = dict(found=False, no_more=False, n_inliers=0, T12=None, mask=np.zeros(self.n, np.uint8), iterations_run=0, log=[])
        if self.n < self.min_inliers or self.n < 3:
            out["no_more"] = True
            return out
        assert SIM3_BREAK <= set(SIM3_RULES)
        cur = 0
        while (self.iterations <= self.max_its if "clamp_le" in SIM3_BREAK else self.iterations < self.max_its) and cur < n_iterations:
            tri = triple_from_draws(draws[3 * cur:3 * cur + 3], self.n)
            cur += 1
            self.iterations += 1
            m = compute_sim3(self.X1[tri].T, self.X2[tri].T, self.fix_scale, self.mode)
            e1, e2 = errors(self.X1, self.X2, self.p1, self.p2, m["T12"], m["T21"], self.K1, self.K2)
            with np.errstate(all="ignore"):
                inl = (e1 < self.thr1) & (e2 < self.thr2)
            cnt = int(inl.sum())
            out["log"].append(dict(triple=tri, count=cnt, err1=e1, err2=e2, **{k: m[k] for k in ("T12", "T21", "R", "s", "t", "identity", "finite")}))
            out["iterations_run"] = cur
            if cnt > self.best_inliers if "tie_gt" in SIM3_BREAK else cnt >= self.best_inliers:
                self.best_mask = inl.astype(np.uint8)
                self.best_inliers = cnt
                self.best = m
                if cnt >= self.min_inliers if "return_ge" in SIM3_BREAK else cnt > self.min_inliers:
                    out.update(found=True, n_inliers=cnt, T12=m["T12"], mask=self.best_mask.copy())
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
        return out

    def find(self, draws):
        return self.iterate(self.max_its, draws)
