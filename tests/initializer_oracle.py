"""numpy restatement of the reference's monocular Initializer (src/Initializer.cc: Initialize and everything it calls), operation
for operation, for csrc/orbfe_initializer.hip to be checked against bit for bit.  Unpinned: OpenCV is not available, so the
OpenCV 3.2 routines the file resolves to are restated from knowledge, under the numbered assumptions below.  float where the
C++ is float, double where it is double, one rounding per operation, sums in the C++ order, no fused multiply-add.  The draws
are an input: iterations x 8 raw rand() values (pnp_oracle.py P5).

The linear algebra is vectorised over a leading batch axis (one hypothesis, or one match, per entry); an entry the C++ would
have skipped keeps its values (np.where), so every entry sees the operation sequence of its own scalar run.

  I1  cv::SVD::compute / cv::SVDecomp on CV_32F run JacobiSVDImpl_<float> (core/src/lapack.cpp): pnp_oracle.py P1 with these
      differences: minval = FLT_MIN, eps = FLT_EPSILON * 2 (a float); W, p, a, b, beta, gamma, delta and every row sum of
      squares are doubles fed by (double)t * t; c and s are floats, cast from the double expressions (the other one is then
      p / (gamma * (double)s * 2), cast); the rotations t0 = c * Ai + s * Aj, t1 = -s * Ai + c * Aj are float; w goes out as
      (float)W[i].  The refill: val0 = (float)(1. / m); sd (a double) += the FLOAT product At[i][k] * At[j][k]; t =
      (float)(At[i][k] - sd * At[j][k]); asum (a float) += |t|; asum = asum > eps * 100 ? 1 / asum : 0 (float); the final
      scale is s = (float)(sd > minval ? 1 / sd : 0.).
  I2  The wrapper (_SVDcompute): for rows >= cols the matrix is transposed into At (cols rows of length rows), n = cols; for
      rows < cols (ComputeF21's 8 x 9) it is copied untransposed, n = rows, and what comes back as vt is At.  With FULL_UV At
      has n1 = max(rows, cols) rows; the rows from n on start at zero and the refill loop of I1 runs over all n1 rows with sd
      = 0 for i >= n.  So vt.row(8) of the 8 x 9 system is the RNG(0x12345678) refill row after its two Gram-Schmidt sweeps.
      For 16 x 9 the seven extra rows are columns of u, which ComputeH21 never reads: `full=False` skips them (vt is the same).
      u(r, c) = At[c][r] when transposed in.
  I3  A product of two matrices, C = A * B, with no transposed operand and 2 <= inner length <= 4 takes gemm's inline path:
      float, s = a0 * b0 + a1 * b1 + a2 * b2 (left to right), out = (float)(s * alpha) with alpha a double (the scalar a
      MatExpr folded in, else 1); with an added matrix (R * p + t) out = (float)(s * alpha + c * beta) in double.  With a
      transposed operand (K.t() * F, u * W.t(), -R.t() * t) it takes GEMMSingleMul<float, double>: a double sum from 0.0 in
      k order of (double)a * (double)b, out = (float)(sum * alpha).  -R.t() folds alpha = -1 into that product.
  I4  Mat::inv() of a 3 x 3 CV_32F: d = det3 in double; d == 0 gives all zeros; else d = 1. / d and every entry is
      (float)((double)a * b - (double)c * d') * d) of the adjugate.  cv::determinant of a 3 x 3 CV_32F is the same det3, a
      double: m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20).
  I5  cv::norm (L2, CV_32F) = sqrt of a double sum of (double)v * v in order; Mat::dot (CV_32F) a double sum of (double)a * b.
  I6  Mat / double, Mat * double, Mat *= double, -Mat on CV_32F are convertTo with a scale: out = v * (float)alpha + 0.0f in
      float, alpha = 1. / s for a division (so -0 comes out as +0).
  I7  `a * row - row2` (Triangulate) is addWeighted in float: v1 * a + v2 * (-1.0f) + 0.0f, left to right.
  I8  sqrt / fabs / acos on a float resolve to the float overloads; `1.0 / x` with a float x is a double division stored to float.
  I9  The parallax test.  parallax = (float)((double)(acosf(c) * 180.0f) / CV_PI) only meets `> 1.0f` (ReconstructF) and
      `>= 1.0f` (ReconstructH).  Both are the same cut on the float cosine: true iff -1 <= c <= PARALLAX_CUT, the largest float
      whose parallax is above 1 (no float gives exactly 1); derive_parallax_cut() finds it with the host's acosf.
  I10 THE LIBRARY'S DECISIONS where the reference is undefined (left out of the parity cases): fewer than 8 matches is an
      argument error; when no iteration of either model has a positive score (SH = SF = 0, RH = NaN, ReconstructF on an empty
      cv::Mat) the answer is ok = 0 with status NO_MODEL; NaN cosines reaching std::sort are unspecified.  A failed Initialize
      leaves R21, t21, P3D and triangulated at zeros.
"""
import ctypes
import ctypes.util

import numpy as np

from pnp_oracle import _RNG, cv_hypot, index_from_draw, seqsum

F32 = np.float32
F64 = np.float64
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_EPSILON = float(np.finfo(np.float32).eps)
CV_PI = 3.1415926535897932384626433832795
PARALLAX_CUT_BITS = 0x3f7ff604   # 0.99984765: see I9 and derive_parallax_cut()
PARALLAX_CUT = np.array([PARALLAX_CUT_BITS], np.uint32).view(np.float32)[0]
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
STATUS_OK, STATUS_FEW, STATUS_INDEX, STATUS_NO_MODEL = 0, 1, 2, 3
MODEL_NONE, MODEL_H, MODEL_F = 0, 1, 2
# where CheckRT dropped a match
RT_OUTLIER, RT_NONFINITE, RT_DEPTH1, RT_DEPTH2, RT_ERROR1, RT_ERROR2, RT_FAR, RT_GOOD = range(8)


# ---- the parallax cut (I9) ------------------------------------------------------------------------------------------------------
def host_acosf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.acosf.restype = ctypes.c_float
    m.acosf.argtypes = [ctypes.c_float]
    return m.acosf


def parallax_of(c, acosf):
    """the reference's expression on one float cosine, with the host's acosf"""
    with np.errstate(**_ERR):
        return F32(F64(F32(acosf(float(c))) * F32(180)) / F64(CV_PI))


def floats_between(lo, hi):
    """every float from lo to hi, both positive, ends included"""
    a, b = F32(lo).view(np.uint32), F32(hi).view(np.uint32)
    return np.arange(int(a), int(b) + 1, dtype=np.uint32).view(np.float32)


def derive_parallax_cut(lo=0.999):
    """-> (largest float with parallax > 1, largest float with parallax >= 1) over [lo, 1]"""
    acosf = host_acosf()
    c = floats_between(lo, 1.0)
    P = np.array([parallax_of(x, acosf) for x in c], np.float32)
    return c[np.nonzero(P > F32(1))[0].max()], c[np.nonzero(P >= F32(1))[0].max()]


def parallax_cut(c):
    c = F32(c)
    return bool(c <= PARALLAX_CUT and c >= F32(-1))


# ---- float Jacobi SVD (I1, I2) ----------------------------------------------------------------------------------------------------
def _refill_f(At, W, m, n, n1):
    """the tail of JacobiSVDImpl_<float> for one matrix (scalar code): At [n1, m] float32, W [n] doubles"""
    eps = F32(FLT_EPSILON * 2)
    rng = _RNG(0x12345678)
    with np.errstate(**_ERR):
        for i in range(n1):
            sd = F64(W[i]) if i < n else F64(0)
            ii = 0
            while ii < 100 and sd <= FLT_MIN:
                val0 = F32(F64(1.0) / F64(m))
                for k in range(m):
                    At[i, k] = val0 if (rng.next() & 256) != 0 else -val0
                for _ in range(2):
                    for j in range(i):
                        sd = F64(0)
                        for k in range(m):
                            sd = sd + F64(F32(At[i, k] * At[j, k]))
                        asum = F32(0)
                        for k in range(m):
                            t = F32(F64(At[i, k]) - sd * F64(At[j, k]))
                            At[i, k] = t
                            asum = F32(asum + abs(t))
                        asum = F32(F32(1) / asum) if asum > F32(eps * F32(100)) else F32(0)
                        for k in range(m):
                            At[i, k] = F32(At[i, k] * asum)
                sd = F64(0)
                for k in range(m):
                    sd = sd + F64(At[i, k]) * F64(At[i, k])
                sd = np.sqrt(sd)
                ii += 1
            s = F32(1 / sd) if sd > FLT_MIN else F32(0)
            for k in range(m):
                At[i, k] = F32(At[i, k] * s)


def jacobi_svd_f(At, n, n1=None):
    """JacobiSVDImpl_<float> (I1) on At [B, >= n, m]: the first n rows take part in the Jacobi sweeps, n1 rows in the refill / scale
    loop (rows from n on must be given; they are overwritten).  -> (w float32 [B, n], At float32 [B, n1, m], Vt float32 [B, n, n])"""
    At = np.array(At, dtype=np.float32, copy=True)
    B, rows, m = At.shape
    n1 = n if n1 is None else n1
    assert rows >= n1 >= n
    eps = F64(F32(FLT_EPSILON * 2))
    with np.errstate(**_ERR):
        A64 = At[:, :n, :].astype(F64)
        W = seqsum(A64 * A64)
        Vt = np.broadcast_to(np.eye(n, dtype=np.float32), (B, n, n)).copy()
        for _ in range(max(m, 30)):
            changed = np.zeros(B, bool)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[:, i, :].copy(), At[:, j, :].copy()
                    a, b = W[:, i], W[:, j]
                    p = seqsum(Ai.astype(F64) * Aj.astype(F64))
                    act = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not act.any():
                        continue
                    p = p * 2
                    beta = a - b
                    gamma = cv_hypot(p, beta)
                    s_n = np.sqrt(((gamma - beta) * 0.5) / gamma).astype(F32)
                    c_n = (p / (gamma * s_n.astype(F64) * 2)).astype(F32)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2)).astype(F32)
                    s_p = (p / (gamma * c_p.astype(F64) * 2)).astype(F32)
                    neg = beta < 0
                    c = np.where(neg, c_n, c_p)[:, None]
                    s = np.where(neg, s_n, s_p)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = (-s) * Ai + c * Aj
                    am = act[:, None]
                    At[:, i, :] = np.where(am, t0, Ai)
                    At[:, j, :] = np.where(am, t1, Aj)
                    t064, t164 = t0.astype(F64), t1.astype(F64)
                    W[:, i] = np.where(act, seqsum(t064 * t064), a)
                    W[:, j] = np.where(act, seqsum(t164 * t164), b)
                    Vi, Vj = Vt[:, i, :].copy(), Vt[:, j, :].copy()
                    Vt[:, i, :] = np.where(am, c * Vi + s * Vj, Vi)
                    Vt[:, j, :] = np.where(am, (-s) * Vi + c * Vj, Vj)
                    changed |= act
            if not changed.any():
                break
        A64 = At[:, :n, :].astype(F64)
        W = np.sqrt(seqsum(A64 * A64))
        for q in range(B):
            for i in range(n - 1):
                j = i
                for k in range(i + 1, n):
                    if W[q, j] < W[q, k]:
                        j = k
                if i != j:
                    W[q, [i, j]] = W[q, [j, i]]
                    At[q, [i, j]] = At[q, [j, i]]
                    Vt[q, [i, j]] = Vt[q, [j, i]]
        w = W.astype(F32)
        out = At[:, :n1, :].copy()
        plain = np.all(W > FLT_MIN, axis=1) if n1 == n else np.zeros(B, bool)
        s = np.where(W > FLT_MIN, 1 / W, 0.0).astype(F32)
        if n1 == n:
            out = out * s[:, :, None]
        for q in np.nonzero(~plain)[0]:
            rowsq = At[q, :n1, :].copy()
            _refill_f(rowsq, W[q], m, n, n1)
            out[q] = rowsq
    return w, out, Vt


def svd_f(A, full=True):
    """cv::SVD::compute(A, w, u, vt, FULL_UV) on A float32 [B, rows, cols] (I2) -> (w [B, min], u [B, rows, rows or min], vt [B,
    cols or min, cols]).  full=False leaves out the refill rows of u for rows > cols (vt does not depend on them)."""
    A = np.asarray(A, np.float32)
    B, rows, cols = A.shape
    if rows >= cols:
        n, m = cols, rows
        n1 = rows if full else cols
        At = np.zeros((B, n1, m), np.float32)
        At[:, :n, :] = np.swapaxes(A, 1, 2)
        w, Ut, Vt = jacobi_svd_f(At, n, n1)
        return w, np.swapaxes(Ut, 1, 2).copy(), Vt
    n, m = rows, cols
    At = np.zeros((B, m, m), np.float32)
    At[:, :n, :] = A
    w, Ut, Vt = jacobi_svd_f(At, n, m)
    return w, np.swapaxes(Vt, 1, 2).copy(), Ut


# ---- small matrix pieces (I3 - I7) --------------------------------------------------------------------------------------------------
def mm(A, B, alpha=1.0):
    """gemm's inline path (I3): A [..., r, k] * B [..., k, c], float"""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    with np.errstate(**_ERR):
        s = A[..., :, 0, None] * B[..., None, 0, :]
        for k in range(1, A.shape[-1]):
            s = s + A[..., :, k, None] * B[..., None, k, :]
        return (s.astype(F64) * F64(alpha)).astype(F32)


def mm_add(A, B, Cm):
    """A * B + C through the inline path (I3): the sum joins C in double"""
    with np.errstate(**_ERR):
        s = mm(A, B)
        return (s.astype(F64) * F64(1.0) + np.asarray(Cm, np.float32).astype(F64) * F64(1.0)).astype(F32)


def mm_t(A, B, alpha=1.0, ta=False, tb=False):
    """GEMMSingleMul<float, double> (I3): a transposed operand, double sums in k order"""
    A = np.asarray(A, np.float32).astype(F64)
    B = np.asarray(B, np.float32).astype(F64)
    if ta:
        A = np.swapaxes(A, -1, -2)
    if tb:
        B = np.swapaxes(B, -1, -2)
    with np.errstate(**_ERR):
        s = seqsum(A[..., :, :, None] * B[..., None, :, :], axis=-2)
        return (s * F64(alpha)).astype(F32)


def det3(M):
    m = np.asarray(M, np.float32).astype(F64)
    with np.errstate(**_ERR):
        return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
                - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
                + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv3(M):
    """Mat::inv() of 3 x 3 CV_32F (I4), batched"""
    S = np.asarray(M, np.float32).astype(F64)
    with np.errstate(**_ERR):
        d = det3(M)
        ok = d != 0
        di = 1.0 / d
        def e(a, b, c, dd):
            return (S[..., a // 3, a % 3] * S[..., b // 3, b % 3] - S[..., c // 3, c % 3] * S[..., dd // 3, dd % 3]) * di
        t = np.stack([e(4, 8, 5, 7), e(2, 7, 1, 8), e(1, 5, 2, 4),
                      e(5, 6, 3, 8), e(0, 8, 2, 6), e(2, 3, 0, 5),
                      e(3, 7, 4, 6), e(1, 6, 0, 7), e(0, 4, 1, 3)], -1)
        t = np.where(np.asarray(ok)[..., None], t, 0.0)
    return t.astype(F32).reshape(S.shape)


def norm2(v):
    v = np.asarray(v, np.float32).astype(F64)
    with np.errstate(**_ERR):
        return np.sqrt(seqsum(v * v))


def scale(M, alpha):
    """convertTo with a scale (I6)"""
    with np.errstate(**_ERR):
        return np.asarray(M, np.float32) * F32(alpha) + F32(0)


def divide(M, s):
    with np.errstate(**_ERR):
        return scale(M, F64(1.0) / F64(s))


def recip(x):
    """1.0 / x stored to float (I8)"""
    with np.errstate(**_ERR):
        return (F64(1.0) / np.asarray(x, np.float32).astype(F64)).astype(F32)


# ---- Initialize's own pieces ------------------------------------------------------------------------------------------------------
def sets_from_draws(draws, iterations, N):
    """mvSets: the swap-with-back / pop-back selections with the list, eight per iteration"""
    d = np.asarray(draws).reshape(-1)
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            p = index_from_draw(d[8 * it + j], len(avail))
            sets[it, j] = avail[p]
            avail[p] = avail[-1]
            avail.pop()
    return sets


def set_without_list(d, N):
    """the same eight selections as the device makes them, without the N-long list: only the positions that took the back element
    differ from their index, and a later write to a position hides an earlier one"""
    pos, val, out = [], [], []
    for k in range(8):
        size = N - k
        p = index_from_draw(d[k], size)
        pick, back = p, size - 1
        for e in range(k):
            if pos[e] == p:
                pick = val[e]
            if pos[e] == size - 1:
                back = val[e]
        out.append(pick)
        pos.append(p)
        val.append(back)
    return out


def seqsum_f(x):
    """float sum in order from 0.0f"""
    x = np.asarray(x, np.float32).reshape(-1)
    if len(x) == 0:
        return F32(0)
    with np.errstate(**_ERR):
        return np.add.accumulate(x, dtype=np.float32)[-1]


def normalize(keys):
    """Normalize over ALL keys -> (points [n, 2], T [3, 3])"""
    k = np.asarray(keys, np.float32).reshape(-1, 2)
    N = len(k)
    with np.errstate(**_ERR):
        meanX = seqsum_f(k[:, 0]) / F32(N)
        meanY = seqsum_f(k[:, 1]) / F32(N)
        px = k[:, 0] - meanX
        py = k[:, 1] - meanY
        devX = seqsum_f(np.abs(px)) / F32(N)
        devY = seqsum_f(np.abs(py)) / F32(N)
        sX = F32(F64(1.0) / F64(devX))
        sY = F32(F64(1.0) / F64(devY))
        pts = np.stack([px * sX, py * sY], 1)
        T = np.eye(3, dtype=np.float32)
        T[0, 0] = sX
        T[1, 1] = sY
        T[0, 2] = (-meanX) * sX
        T[1, 2] = (-meanY) * sY
    return pts, T


def compute_h21(p1, p2):
    """ComputeH21 on p1, p2 float32 [B, 8, 2] -> Hn [B, 3, 3]"""
    B = len(p1)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.zeros((B, 16, 9), np.float32)
    with np.errstate(**_ERR):
        A[:, 0::2, 3] = -u1
        A[:, 0::2, 4] = -v1
        A[:, 0::2, 5] = -1
        A[:, 0::2, 6] = v2 * u1
        A[:, 0::2, 7] = v2 * v1
        A[:, 0::2, 8] = v2
        A[:, 1::2, 0] = u1
        A[:, 1::2, 1] = v1
        A[:, 1::2, 2] = 1
        A[:, 1::2, 6] = (-u2) * u1
        A[:, 1::2, 7] = (-u2) * v1
        A[:, 1::2, 8] = -u2
    _, _, vt = svd_f(A, full=False)
    return vt[:, 8, :].reshape(B, 3, 3).copy()


def compute_f21(p1, p2):
    """ComputeF21 on p1, p2 float32 [B, 8, 2] -> Fn [B, 3, 3]"""
    B = len(p1)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.zeros((B, 8, 9), np.float32)
    with np.errstate(**_ERR):
        A[:, :, 0] = u2 * u1
        A[:, :, 1] = u2 * v1
        A[:, :, 2] = u2
        A[:, :, 3] = v2 * u1
        A[:, :, 4] = v2 * v1
        A[:, :, 5] = v2
        A[:, :, 6] = u1
        A[:, :, 7] = v1
        A[:, :, 8] = 1
    _, _, vt = svd_f(A)
    Fpre = vt[:, 8, :].reshape(B, 3, 3)
    w, u, vt = svd_f(Fpre)
    D = np.zeros((B, 3, 3), np.float32)
    D[:, 0, 0] = w[:, 0]
    D[:, 1, 1] = w[:, 1]
    return mm(mm(u, D), vt)


TH_H = F32(5.991)
TH_F = F32(3.841)
TH_SCORE = F32(5.991)


def inv_sigma_square(sigma):
    s = F32(sigma)
    with np.errstate(**_ERR):
        return F32(F64(1.0) / F64(F32(s * s)))


def chi_homography(H21, H12, xy, sigma):
    """CheckHomography's chiSquare1, chiSquare2 for H21, H12 [B, 3, 3] over xy [N, 4] -> [B, N] each"""
    h = H21.reshape(-1, 9)[:, :, None]
    g = H12.reshape(-1, 9)[:, :, None]
    u1, v1, u2, v2 = (xy[None, :, k] for k in range(4))
    inv = inv_sigma_square(sigma)
    with np.errstate(**_ERR):
        w2 = recip(g[:, 6] * u2 + g[:, 7] * v2 + g[:, 8])
        u2in1 = (g[:, 0] * u2 + g[:, 1] * v2 + g[:, 2]) * w2
        v2in1 = (g[:, 3] * u2 + g[:, 4] * v2 + g[:, 5]) * w2
        chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv
        w1 = recip(h[:, 6] * u1 + h[:, 7] * v1 + h[:, 8])
        u1in2 = (h[:, 0] * u1 + h[:, 1] * v1 + h[:, 2]) * w1
        v1in2 = (h[:, 3] * u1 + h[:, 4] * v1 + h[:, 5]) * w1
        chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv
    return chi1, chi2


def chi_fundamental(F21, xy, sigma):
    f = F21.reshape(-1, 9)[:, :, None]
    u1, v1, u2, v2 = (xy[None, :, k] for k in range(4))
    inv = inv_sigma_square(sigma)
    with np.errstate(**_ERR):
        a2 = f[:, 0] * u1 + f[:, 1] * v1 + f[:, 2]
        b2 = f[:, 3] * u1 + f[:, 4] * v1 + f[:, 5]
        c2 = f[:, 6] * u1 + f[:, 7] * v1 + f[:, 8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1 = f[:, 0] * u2 + f[:, 3] * v2 + f[:, 6]
        b1 = f[:, 1] * u2 + f[:, 4] * v2 + f[:, 7]
        c1 = f[:, 2] * u2 + f[:, 5] * v2 + f[:, 8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
    return chi1, chi2


def score_of(chi1, chi2, th, th_score):
    """score += th_score - chi in match order, chi1 then chi2 of each match -> (score [B], inliers bool [B, N])"""
    with np.errstate(**_ERR):
        out1, out2 = chi1 > th, chi2 > th
        terms = np.stack([np.where(out1, F32(0), th_score - chi1), np.where(out2, F32(0), th_score - chi2)], -1)
        terms = terms.reshape(len(chi1), -1).astype(np.float32)
        if terms.shape[1] == 0:
            return np.zeros(len(chi1), np.float32), ~(out1 | out2)
        return np.add.accumulate(terms, axis=1, dtype=np.float32)[:, -1], ~(out1 | out2)


def pick(scores):
    """the acceptance rule: strict >, from 0 -> (winning iteration or -1, score)"""
    best, score = -1, F32(0)
    for it, s in enumerate(scores):
        if s > score:
            best, score = it, F32(s)
    return best, score


def triangulate(xy, P1, P2):
    """Triangulate over xy [N, 4] -> (x3D [N, 3], A [N, 4, 4])"""
    N = len(xy)
    A = np.zeros((N, 4, 4), np.float32)
    with np.errstate(**_ERR):
        for r, (c, P, row) in enumerate(((0, P1, 0), (1, P1, 1), (2, P2, 0), (3, P2, 1))):
            A[:, r, :] = xy[:, c, None] * P[None, 2, :] + P[None, row, :] * F32(-1.0) + F32(0)
        _, _, vt = svd_f(A)
        x = vt[:, 3, :]
        a = (F64(1.0) / x[:, 3].astype(F64)).astype(F32)
        return x[:, :3] * a[:, None] + F32(0), A


def check_rt(R, t, xy, inl, K, th2):
    """CheckRT over the matches xy [N, 4] with the inlier flags -> dict(nGood, stage [N], p3d [N, 3], cos [N], sel: the selected
    cosine (0 if nGood == 0), n_cos)"""
    K = np.asarray(K, np.float32).reshape(3, 3)
    R = np.asarray(R, np.float32).reshape(3, 3)
    t = np.asarray(t, np.float32).reshape(3, 1)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    N = len(xy)
    stage = np.full(N, RT_OUTLIER, np.int32)
    p3d = np.zeros((N, 3), np.float32)
    cosv = np.zeros(N, np.float32)
    idx = np.nonzero(inl)[0]
    out = dict(nGood=0, stage=stage, p3d=p3d, cos=cosv, sel=F32(0), n_cos=0)
    if len(idx) == 0:
        return out
    P1 = np.zeros((3, 4), np.float32)
    P1[:, :3] = K
    P2 = mm(K, np.concatenate([R, t], 1))
    O2 = mm_t(R, t, alpha=-1.0, ta=True).reshape(3)
    q = xy[idx]
    with np.errstate(**_ERR):
        x, _ = triangulate(q, P1, P2)
        fin = np.isfinite(x).all(1)
        n1 = x - F32(0)
        d1 = norm2(n1).astype(F32)
        n2 = x - O2[None, :]
        d2 = norm2(n2).astype(F32)
        dot = seqsum(n1.astype(F64) * n2.astype(F64))
        cosp = (dot / (d1 * d2).astype(F64)).astype(F32)
        far = ~(cosp.astype(F64) < 0.99998)
        x2 = mm_add(R[None], x[:, :, None], t[None])[:, :, 0]
        invZ1 = recip(x[:, 2])
        im1x = fx * x[:, 0] * invZ1 + cx
        im1y = fy * x[:, 1] * invZ1 + cy
        e1 = (im1x - q[:, 0]) * (im1x - q[:, 0]) + (im1y - q[:, 1]) * (im1y - q[:, 1])
        invZ2 = recip(x2[:, 2])
        im2x = fx * x2[:, 0] * invZ2 + cx
        im2y = fy * x2[:, 1] * invZ2 + cy
        e2 = (im2x - q[:, 2]) * (im2x - q[:, 2]) + (im2y - q[:, 3]) * (im2y - q[:, 3])
        st = np.full(len(idx), RT_GOOD, np.int32)
        st[far] = RT_FAR
        st[e2 > F32(th2)] = RT_ERROR2
        st[e1 > F32(th2)] = RT_ERROR1
        st[(x2[:, 2] <= 0) & ~far] = RT_DEPTH2
        st[(x[:, 2] <= 0) & ~far] = RT_DEPTH1
        st[~fin] = RT_NONFINITE
    stage[idx] = st
    p3d[idx] = x
    cosv[idx] = np.where(fin, cosp, F32(0))   # CheckRT leaves before it computes one
    passed = cosp[st >= RT_FAR]
    nGood = int((st == RT_GOOD).sum())
    out.update(nGood=nGood, n_cos=len(passed))
    if nGood > 0:
        srt = np.sort(passed)
        out["sel"] = srt[min(50, len(srt) - 1)]
    return out


def decompose_e(E):
    w, u, vt = svd_f(E[None])
    u, vt = u[0], vt[0]
    t = u[:, 2].copy()
    t = divide(t, norm2(t))
    W = np.zeros((3, 3), np.float32)
    W[0, 1] = -1
    W[1, 0] = 1
    W[2, 2] = 1
    R1 = mm(mm(u, W), vt)
    if det3(R1) < 0:
        R1 = scale(R1, -1.0)
    R2 = mm(mm_t(u, W, tb=True), vt)
    if det3(R2) < 0:
        R2 = scale(R2, -1.0)
    return R1, R2, t


def hypotheses_f(F21, K):
    K = np.asarray(K, np.float32).reshape(3, 3)
    E = mm(mm_t(K, F21, ta=True), K)
    R1, R2, t = decompose_e(E)
    t1, t2 = t, scale(t, -1.0)
    return [(R1, t1), (R2, t1), (R1, t2), (R2, t2)]


def hypotheses_h(H21, K):
    """-> the eight (R, t), or [] at the d1/d2, d2/d3 early-out"""
    K = np.asarray(K, np.float32).reshape(3, 3)
    A = mm(mm(inv3(K), H21), K)
    w, U, Vt = svd_f(A[None])
    w, U, Vt = w[0], U[0], Vt[0]
    with np.errstate(**_ERR):
        s = F32(det3(U) * det3(Vt))
        d1, d2, d3 = w
        if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001:
            return []
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_st, -aux_st, -aux_st, aux_st]
        out = []
        for i in range(4):
            Rp = np.eye(3, dtype=np.float32)
            Rp[0, 0] = ctheta
            Rp[0, 2] = -stheta[i]
            Rp[2, 0] = stheta[i]
            Rp[2, 2] = ctheta
            R = mm(mm(U, Rp, alpha=F64(s)), Vt)
            tp = scale(np.array([x1[i], 0, -x3[i]], np.float32), F64(F32(d1 - d3)))
            t = mm(U, tp.reshape(3, 1)).reshape(3)
            out.append((R, divide(t, norm2(t))))
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        for i in range(4):
            Rp = np.eye(3, dtype=np.float32)
            Rp[0, 0] = cphi
            Rp[0, 2] = sphi[i]
            Rp[1, 1] = -1
            Rp[2, 0] = sphi[i]
            Rp[2, 2] = -cphi
            R = mm(mm(U, Rp, alpha=F64(s)), Vt)
            tp = scale(np.array([x1[i], 0, x3[i]], np.float32), F64(F32(d1 + d3)))
            t = mm(U, tp.reshape(3, 1)).reshape(3)
            out.append((R, divide(t, norm2(t))))
    return out


def initialize(keys1, keys2, matches12, K, sigma=1.0, iterations=200, draws=None, tap_iteration=0, tap_hypothesis=0):
    """Initializer::Initialize.  keys float32 [n, 2], matches12 int32 [n1] (-1 = none), K float32 [3, 3], draws iterations x 8.
    -> dict: the result fields of orbfe_initializer_result, P3D [n1, 3], triangulated uint8 [n1], and the taps."""
    k1 = np.asarray(keys1, np.float32).reshape(-1, 2)
    k2 = np.asarray(keys2, np.float32).reshape(-1, 2)
    m12 = np.asarray(matches12, np.int32).reshape(-1)
    K = np.asarray(K, np.float32).reshape(3, 3)
    n1 = len(k1)
    first = np.nonzero(m12 >= 0)[0]
    second = m12[first]
    N = len(first)
    if N < 8:
        raise ValueError("fewer than 8 matches: undefined in the reference (I10)")
    xy = np.concatenate([k1[first], k2[second]], 1)
    sets = sets_from_draws(draws, iterations, N)
    pn1, T1 = normalize(k1)
    pn2, T2 = normalize(k2)
    p1 = pn1[first[sets]]
    p2 = pn2[second[sets]]
    Hn = compute_h21(p1, p2)
    Fn = compute_f21(p1, p2)
    H21i = mm(mm(inv3(T2)[None], Hn), T1[None])
    H12i = inv3(H21i)
    F21i = mm(mm(T2.T.copy()[None], Fn), T1[None])
    hc1, hc2 = chi_homography(H21i, H12i, xy, sigma)
    fc1, fc2 = chi_fundamental(F21i, xy, sigma)
    sH, inlH = score_of(hc1, hc2, TH_H, TH_H)
    sF, inlF = score_of(fc1, fc2, TH_F, TH_SCORE)
    itH, SH = pick(sH)
    itF, SF = pick(sF)
    r = dict(ok=0, status=STATUS_OK, model=MODEL_NONE, n_matches=N, SH=SH, SF=SF, iterH=itH, iterF=itF,
             H21=H21i[itH] if itH >= 0 else np.zeros((3, 3), np.float32), F21=F21i[itF] if itF >= 0 else np.zeros((3, 3), np.float32),
             R21=np.zeros((3, 3), np.float32), t21=np.zeros(3, np.float32), n_hyp=0, nGood=np.zeros(8, np.int32), best=-1,
             second=0, n_inliers=0, n_cos=np.zeros(8, np.int32), sel_cos=np.zeros(8, np.float32), parallax_ok=0, parallax_cos=F32(0),
             P3D=np.zeros((n1, 3), np.float32), triangulated=np.zeros(n1, np.uint8),
             tap=dict(sets=sets, Hn=Hn, Fn=Fn, H21i=H21i, F21i=F21i, scoreH=sH, scoreF=sF,
                      chi=np.stack([hc1[tap_iteration], hc2[tap_iteration], fc1[tap_iteration], fc2[tap_iteration]], 1)
                      if tap_iteration < iterations else None, rt=None),
             idx1=first, idx2=second)
    with np.errstate(**_ERR):
        RH = SH / (SH + SF)
    use_h = bool(F64(RH) > 0.40)
    if (use_h and itH < 0) or (not use_h and itF < 0):
        r["status"] = STATUS_NO_MODEL
        return r
    r["model"] = MODEL_H if use_h else MODEL_F
    inl = inlH[itH] if use_h else inlF[itF]
    Nin = int(inl.sum())
    r["n_inliers"] = Nin
    th2 = F32(F64(4.0) * F64(F32(F32(sigma) * F32(sigma))))
    hyps = hypotheses_h(r["H21"], K) if use_h else hypotheses_f(r["F21"], K)
    r["n_hyp"] = len(hyps)
    if not hyps:
        return r
    rts = [check_rt(R, t, xy, inl, K, th2) for R, t in hyps]
    good = [c["nGood"] for c in rts]
    r["nGood"][:len(good)] = good
    r["n_cos"][:len(good)] = [c["n_cos"] for c in rts]
    r["sel_cos"][:len(good)] = [c["sel"] for c in rts]
    if tap_hypothesis < len(hyps):
        c = rts[tap_hypothesis]
        r["tap"]["rt"] = np.concatenate([c["p3d"], c["cos"][:, None], c["stage"].astype(np.float32)[:, None]], 1)
    if use_h:
        bestGood, secondBest, best = 0, 0, -1
        for i, g in enumerate(good):
            if g > bestGood:
                secondBest, bestGood, best = bestGood, g, i
            elif g > secondBest:
                secondBest = g
        r["best"], r["second"] = best, secondBest
    else:
        maxGood = max(good)
        nMinGood = max(int(0.9 * Nin), 50)
        nsimilar = sum(1 for g in good if g > 0.7 * maxGood)
        best = good.index(maxGood)   # the if / else-if ladder: the first hypothesis that reaches maxGood
        r["best"], r["second"] = best, nsimilar
    # the selected cosine and the cut's verdict are reported for the best hypothesis whether or not the ladder gets that far
    if best >= 0 and good[best] > 0:
        r["parallax_cos"] = rts[best]["sel"]
        r["parallax_ok"] = int(parallax_cut(rts[best]["sel"]))
    if use_h:
        ok = best >= 0 and secondBest < 0.75 * bestGood and r["parallax_ok"] and bestGood > 50 and bestGood > 0.9 * Nin
    else:
        ok = not (maxGood < nMinGood or nsimilar > 1) and bool(r["parallax_ok"])
    if ok:
        c = rts[best]
        r["ok"] = 1
        r["R21"], r["t21"] = hyps[best][0], hyps[best][1].reshape(3)
        keep = c["stage"] >= RT_FAR
        r["P3D"][first[keep]] = c["p3d"][keep]
        r["triangulated"][first[c["stage"] == RT_GOOD]] = 1
    return r
