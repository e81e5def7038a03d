"""CPU oracle of cv::findHomography(points_current, points_last, RANSAC, 3) as the fork's Tracking::TrackHomo calls it
(perfect/src/Tracking.cc:1331-1399), and of method 0 (least squares over all points).

It restates OpenCV 3.2's generic C++ path (modules/calib3d/src/fundam.cpp, ptsetreg.cpp, levmarq.cpp, core/src/lapack.cpp,
matmul.cpp, stat.cpp) in Python / numpy: float32 where the C++ uses float, float64 where it uses double, one operation at a
time, no FMA.  Sums keep the C++ order (numpy's add.accumulate is a serial left-to-right sum).
  * the input: Point2f pairs, src = points_current, dst = points_last (dst ~ H * src); threshold <= 0 becomes 3;
  * method 0 or n == 4: runKernel on all points, mask all ones;
  * RANSAC (RANSACPointSetRegistrator::run, modelPoints 4, maxIters 2000, confidence 0.995 by default): RNG((uint64)-1),
    getSubset(maxAttempts 10000) with checkPartialSubsets false and checkSubset = haveCollinearPoints on both sets; runKernel
    (centroid / mean absolute deviation normalisation, LtL upper triangle, completeSymm, eigen = JacobiImpl_, V[8]
    de-normalised by two 3x3 gemm products, convertTo(1./H22)); findInliers with computeError in float; acceptance
    goodCount > max(maxGoodCount, 3); RANSACUpdateNumIters;
  * refit and refine when the result is true and n > 4: inliers compressed in index order, runKernel again (RANSAC only; a
    failed refit keeps the RANSAC model), then LMSolverImpl (maxIters 10, epsx = epsf = FLT_EPSILON) on H[0:8] with
    HomographyRefineCallback.  The output mask is the RANSAC mask.

UNPINNED.  OpenCV is not available to this project, so this oracle has never been compared with a real OpenCV build.  The
points below rest on knowledge of the OpenCV 3.2 sources and could not be confirmed here:

  H1  3.2's HomographyEstimatorCallback::checkSubset is haveCollinearPoints on both point sets only.  The four-triangle
      orientation test of later releases is left out.  With checkPartialSubsets = false haveCollinearPoints(ms, 4) tests
      only the last point against the lines through pairs of the first three (the first three are never tested alone);
      its dx / dy are float differences widened to double.
  H2  getSubset's checkPartialSubsets is false for the homography registrator (createRANSACPointSetRegistrator's
      default), so a subset is redrawn whole when checkSubset rejects it, and every attempt counts toward the 10000.
  H3  The `hypot` that JacobiImpl_ calls is the static template of core/src/lapack.cpp, found first by unqualified lookup
      inside namespace cv: a = |a|, b = |b|; a > b: a*sqrt(1 + (b/a)^2); b > 0: b*sqrt(1 + (a/b)^2); else 0.  It uses only
      IEEE + - * / sqrt, so no C library version enters.  The C library does enter RANSACUpdateNumIters (log, pow); this
      oracle calls Python's math.log / math.pow, i.e. the host's libm (glibc 2.35 where it was written).
  H4  SVBkSb (solve and invert with DECOMP_EIG) skips singular values with |w| <= (sum of w, in order) * 2*DBL_EPSILON.
  H5  The reduction orders: norm(NORM_L2SQR) of a double vector is normL2Sqr_ unrolled by four, s += v0*v0 + v1*v1 +
      v2*v2 + v3*v3, then a serial tail; Mat::dot is dotProd_ unrolled by four the same way (no IPP for dotProd_64f);
      mulTransposed(J, A, true) for an 8-column J is MulTransposedR, each entry a serial sum over the rows;
      gemm(J, r, GEMM_1_T) and gemm(A, d, -1, v, 2) are GEMMSingleMul's serial per-entry sums (s*alpha, s*alpha + c*beta);
      the 3x3 products of runKernel are gemm's small-matrix path, (a0*b0 + a1*b1) + a2*b2; the centroid, spread and LtL
      sums of runKernel are serial in point order.
  H6  n < 4 (where OpenCV 3.2 would assert or fail inside the registrator): the library returns "no model": ok = 0, H all
      zeros, mask all zeros.  A false result (no subset, no model with more than 3 inliers, a failed method-0 fit) also
      gives an all-zero mask; 3.2 leaves the mask unwritten then.
  H7  convertTo(_model, CV_64F, 1./H22) copies without scaling when |1./H22 - 1| < DBL_EPSILON and otherwise computes
      v*scale + 0.0 per entry (cvtScale_ with shift 0), so H22 is H22*(1./H22), which need not be exactly 1.
  H8  Eigen decomposition goes through JacobiImpl_ (no Lapack / IPP hook in a default 3.2 build): pivot search by indR /
      indC, stop at |p| <= DBL_EPSILON or after n*n*30 rotations, then a selection sort to descending eigenvalues.
"""
import math

import numpy as np

RANSAC = 8
DBL_EPSILON = 2.220446049250313e-16
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MIN = 2.2250738585072014e-308
MASK64 = (1 << 64) - 1
RNG_COEFF = 4164903690


def f32(v):
    return float(np.float32(v))


# ---- cv::RNG ------------------------------------------------------------------------------------------------------------------
class RNG:
    def __init__(self, state=MASK64):
        self.state = state if state else 0xffffffff

    def next(self):
        s = self.state
        self.state = ((s & 0xffffffff) * RNG_COEFF + (s >> 32)) & MASK64
        return self.state & 0xffffffff

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def rng_stream(n, state=MASK64):
    r = RNG(state)
    return np.array([r.next() for _ in range(n)], np.uint32)


# ---- subsets ------------------------------------------------------------------------------------------------------------------
def have_collinear_points(pts, count):
    """pts: list of (x, y) float32 values as Python floats; haveCollinearPoints(ms, count) (H1)"""
    i = count - 1
    for j in range(i):
        dx1 = f32(pts[j][0] - pts[i][0])
        dy1 = f32(pts[j][1] - pts[i][1])
        for k in range(j):
            dx2 = f32(pts[k][0] - pts[i][0])
            dy2 = f32(pts[k][1] - pts[i][1])
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (((abs(dx1) + abs(dy1)) + abs(dx2)) + abs(dy2)):
                return True
    return False


def get_subset(src, dst, rng, max_attempts=10000, trace=None):
    """getSubset with modelPoints 4 and checkPartialSubsets false (H2): the four indices, or None.  src / dst: lists of
    (x, y) Python floats holding float32 values.  trace["collinear"] counts the subsets checkSubset rejected."""
    count = len(src)
    idx = [0, 0, 0, 0]
    it = 0
    i = 0
    while it < max_attempts:
        i = 0
        while i < 4 and it < max_attempts:
            while True:
                v = idx[i] = rng.uniform(0, count)
                if all(v != idx[j] for j in range(i)):
                    break
            i += 1
        if i == 4 and (have_collinear_points([src[t] for t in idx], 4) or have_collinear_points([dst[t] for t in idx], 4)):
            it += 1
            if trace is not None:
                trace["collinear"] = trace.get("collinear", 0) + 1
            continue
        break
    return list(idx) if (i == 4 and it < max_attempts) else None


# ---- JacobiImpl_ --------------------------------------------------------------------------------------------------------------
def cv_hypot(a, b):
    """lapack.cpp's hypot template (H3)"""
    a = abs(a)
    b = abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1 + a * a)
    return 0.0


def jacobi(A_in):
    """eigen() of a symmetric n x n double matrix through JacobiImpl_ (H8): (W descending [n], V rows = eigenvectors [n][n])."""
    A = [float(v) for v in np.asarray(A_in, np.float64).ravel()]
    n = int(round(math.sqrt(len(A))))
    V = [0.0] * (n * n)
    for i in range(n):
        V[i * n + i] = 1.0
    W = [0.0] * n
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

    for k in range(n):
        W[k] = A[(n + 1) * k]
        if k < n - 1:
            row_max(k)
        if k > 0:
            col_max(k)
    if n > 1:
        for _ in range(n * n * 30):
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
            if abs(p) <= DBL_EPSILON:
                break
            y = (W[l] - W[k]) * 0.5
            t = abs(y) + cv_hypot(p, y)
            s = cv_hypot(p, t)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[n * k + l] = 0.0
            W[k] -= t
            W[l] += t

            def rot(i0, i1, M):
                a0, b0 = M[i0], M[i1]
                M[i0] = a0 * c - b0 * s
                M[i1] = a0 * s + b0 * c

            for i in range(k):
                rot(n * i + k, n * i + l, A)
            for i in range(k + 1, l):
                rot(n * k + i, n * i + l, A)
            for i in range(l + 1, n):
                rot(n * k + i, n * l + i, A)
            for i in range(n):
                rot(n * k + i, n * l + i, V)
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
    return np.array(W), np.array(V).reshape(n, n)


# ---- HomographyEstimatorCallback ----------------------------------------------------------------------------------------------
def _serial_sum(terms):
    """0 + t0 + t1 + ... left to right (a C accumulator that starts at +0.0)"""
    return float(np.add.accumulate(np.concatenate([[0.0], np.asarray(terms, np.float64)]))[-1])


def _gemm3(a, b):
    return [(a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def run_kernel(src, dst, with_ltl=False):
    """runKernel(src = M, dst = m): the 9 doubles of H (row-major), or None when a spread is below DBL_EPSILON.
    src / dst: float32 arrays [n, 2]."""
    M = np.asarray(src, np.float32).astype(np.float64)
    m = np.asarray(dst, np.float32).astype(np.float64)
    count = float(len(M))
    cmx, cmy = _serial_sum(m[:, 0]) / count, _serial_sum(m[:, 1]) / count
    cMx, cMy = _serial_sum(M[:, 0]) / count, _serial_sum(M[:, 1]) / count
    smx, smy = _serial_sum(np.abs(m[:, 0] - cmx)), _serial_sum(np.abs(m[:, 1] - cmy))
    sMx, sMy = _serial_sum(np.abs(M[:, 0] - cMx)), _serial_sum(np.abs(M[:, 1] - cMy))
    if abs(smx) < DBL_EPSILON or abs(smy) < DBL_EPSILON or abs(sMx) < DBL_EPSILON or abs(sMy) < DBL_EPSILON:
        return (None, None) if with_ltl else None
    smx, smy, sMx, sMy = count / smx, count / smy, count / sMx, count / sMy
    inv_hnorm = [1. / smx, 0., cmx, 0., 1. / smy, cmy, 0., 0., 1.]
    hnorm2 = [sMx, 0., -cMx * sMx, 0., sMy, -cMy * sMy, 0., 0., 1.]
    x = (m[:, 0] - cmx) * smx
    y = (m[:, 1] - cmy) * smy
    X = (M[:, 0] - cMx) * sMx
    Y = (M[:, 1] - cMy) * sMy
    one, zero = np.ones_like(X), np.zeros_like(X)
    Lx = [X, Y, one, zero, zero, zero, -x * X, -x * Y, -x]
    Ly = [zero, zero, zero, X, Y, one, -y * X, -y * Y, -y]
    LtL = np.zeros((9, 9))
    for j in range(9):
        for k in range(j, 9):
            LtL[j, k] = _serial_sum(Lx[j] * Lx[k] + Ly[j] * Ly[k])
            LtL[k, j] = LtL[j, k]
    _, V = jacobi(LtL)
    H0 = [float(v) for v in V[8]]
    Ht = _gemm3(inv_hnorm, H0)
    H0 = _gemm3(Ht, hnorm2)
    scale = 1. / H0[8]
    H = H0 if abs(scale - 1) < DBL_EPSILON else [v * scale + 0.0 for v in H0]   # H7
    H = np.array(H, np.float64)
    return (H, LtL) if with_ltl else H


def compute_error(src, dst, H):
    """computeError in float: err[i] float32"""
    Hf = np.asarray(H, np.float64)[:8].astype(np.float32)
    Mx, My = np.asarray(src, np.float32)[:, 0], np.asarray(src, np.float32)[:, 1]
    mx, my = np.asarray(dst, np.float32)[:, 0], np.asarray(dst, np.float32)[:, 1]
    with np.errstate(all="ignore"):
        ww = np.float32(1) / (Hf[6] * Mx + Hf[7] * My + np.float32(1))
        dx = (Hf[0] * Mx + Hf[1] * My + Hf[2]) * ww - mx
        dy = (Hf[3] * Mx + Hf[4] * My + Hf[5]) * ww - my
        return (dx * dx + dy * dy).astype(np.float32)


def find_inliers(src, dst, H, threshold):
    t = np.float32(threshold * threshold)
    return compute_error(src, dst, H) <= t


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters"""
    p = max(p, 0.)
    p = min(p, 1.)
    ep = max(ep, 0.)
    ep = min(ep, 1.)
    num = max(1. - p, DBL_MIN)
    denom = 1. - math.pow(1. - ep, model_points)
    if denom < DBL_MIN:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


# ---- the stages -------------------------------------------------------------------------------------------------------------
def _pairs(src, dst):
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    assert src.shape == dst.shape
    return src, dst


def ransac(src, dst, threshold=3.0, max_iters=2000, confidence=0.995, trace=None):
    """RANSACPointSetRegistrator::run for n >= 5: dict(ok, H [9] (zeros when not ok), mask bool [n], iters (the loop counter at
    exit), niters (the final bound)).  A `trace` dict receives accepts (the loop counter and the new niters at each
    acceptance), collinear (subsets checkSubset rejected) and fit_failed (4-point fits runKernel refused)."""
    src, dst = _pairs(src, dst)
    if trace is not None:
        trace.update(accepts=[], collinear=0, fit_failed=0)
    count = len(src)
    if threshold <= 0:
        threshold = 3.0
    sl = [(float(a), float(b)) for a, b in src]
    dl = [(float(a), float(b)) for a, b in dst]
    rng = RNG()
    niters = max(max_iters, 1)
    max_good = 0
    best = None
    it = 0
    failed = False
    while it < niters:
        idx = get_subset(sl, dl, rng, trace=trace)
        if idx is None:
            if it == 0:
                failed = True
            break
        H = run_kernel(src[idx], dst[idx])
        if H is not None:
            good = int(np.count_nonzero(find_inliers(src, dst, H, threshold)))
            if good > max(max_good, 3):
                best = H
                max_good = good
                niters = update_num_iters(confidence, float(count - good) / count, 4, niters)
                if trace is not None:
                    trace["accepts"].append((it, niters))
        elif trace is not None:
            trace["fit_failed"] += 1
        it += 1
    if failed or max_good <= 0:
        return dict(ok=False, H=np.zeros(9), mask=np.zeros(count, bool), iters=it, niters=niters)
    return dict(ok=True, H=best, mask=find_inliers(src, dst, best, threshold), iters=it, niters=niters)


def refit(src, dst, mask, H):
    """findHomography's runKernel over the inliers (index order); a failed fit keeps H.  Returns (H, refit_ok)."""
    src, dst = _pairs(src, dst)
    mask = np.asarray(mask, bool)
    Hr = run_kernel(src[mask], dst[mask])
    return (np.asarray(H, np.float64).copy(), False) if Hr is None else (Hr, True)


# LMSolverImpl pieces (H5)
def norm_l2sqr(v):
    v = np.asarray(v, np.float64)
    n4 = len(v) // 4 * 4
    q = v[:n4].reshape(-1, 4)
    terms = list(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]) + list(v[n4:] * v[n4:])
    return _serial_sum(terms)


def dot(a, b):
    """Mat::dot: dotProd_ unrolled by four"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n4 = len(a) // 4 * 4
    qa, qb = a[:n4].reshape(-1, 4), b[:n4].reshape(-1, 4)
    terms = list(((qa[:, 0] * qb[:, 0] + qa[:, 1] * qb[:, 1]) + qa[:, 2] * qb[:, 2]) + qa[:, 3] * qb[:, 3]) + list(a[n4:] * b[n4:])
    return _serial_sum(terms)


def norm_inf(v):
    s = 0.0
    for x in np.abs(np.asarray(v, np.float64)):
        s = x if s < x else s
    return float(s)


def refine_compute(src, dst, h, need_j=True):
    """HomographyRefineCallback::compute: r [2n] (x, y interleaved), J [2n, 8]"""
    M = np.asarray(src, np.float32).astype(np.float64)
    m = np.asarray(dst, np.float32).astype(np.float64)
    Mx, My = M[:, 0], M[:, 1]
    with np.errstate(all="ignore"):
        ww = h[6] * Mx + h[7] * My + 1.
        ww = np.where(np.abs(ww) > DBL_EPSILON, 1. / ww, 0.)
        xi = (h[0] * Mx + h[1] * My + h[2]) * ww
        yi = (h[3] * Mx + h[4] * My + h[5]) * ww
    n = len(M)
    r = np.empty(2 * n)
    r[0::2] = xi - m[:, 0]
    r[1::2] = yi - m[:, 1]
    if not need_j:
        return r, None
    J = np.zeros((2 * n, 8))
    J[0::2, 0] = Mx * ww
    J[0::2, 1] = My * ww
    J[0::2, 2] = ww
    J[0::2, 6] = -Mx * ww * xi
    J[0::2, 7] = -My * ww * xi
    J[1::2, 3] = Mx * ww
    J[1::2, 4] = My * ww
    J[1::2, 5] = ww
    J[1::2, 6] = -Mx * ww * yi
    J[1::2, 7] = -My * ww * yi
    return r, J


def _jtj(J):
    A = np.zeros((8, 8))
    for i in range(8):
        for j in range(i, 8):
            A[i, j] = A[j, i] = _serial_sum(J[:, i] * J[:, j])
    return A


def _jtr(J, r):
    return np.array([_serial_sum(J[:, i] * r) for i in range(8)])


def solve_eig(Ap, v):
    """solve(Ap, v, d, DECOMP_EIG): Jacobi, then SVBkSb with nb = 1 (H4)"""
    W, U = jacobi(Ap)
    thr = _serial_sum(W) * (DBL_EPSILON * 2)
    x = np.zeros(8)
    for i in range(8):
        wi = W[i]
        if abs(wi) <= thr:
            continue
        wi = 1 / wi
        s = _serial_sum(U[i] * v)
        s *= wi
        x = x + s * U[i]
    return x


def invert_eig_diag(A):
    """diag(invert(A, DECOMP_EIG)): eigen, transpose, SVD::backSubst with no right-hand side (H4)"""
    W, Vt = jacobi(A)
    thr = _serial_sum(W) * (DBL_EPSILON * 2)
    X = np.zeros((8, 8))
    for i in range(8):
        wi = W[i]
        if abs(wi) <= thr:
            continue
        wi = 1 / wi
        buf = Vt[i] * wi
        for rr in range(8):
            X[rr] = X[rr] + Vt[i][rr] * buf
    return np.diag(X).copy()


# The LM rules a test may break one at a time, to show that a case table can tell them apart (tests/test_homography_edge_cases.py).
# Empty = OpenCV's behaviour; nothing but a test sets it.
#   lc_stale            lc keeps its old value when the lambda == 0 inversion re-inflates lambda
#   nu_unclamped_10     nu is not clamped at 10
#   nu_not_halved       the inversion leaves out nu *= 0.5
#   lambda_always_zero  R > 0.75 zeroes lambda even when lambda / 2 >= lc
#   iters_9             9 iterations at most instead of 10
#   mid_as_low          0.25 <= R <= 0.75 takes the R < 0.25 branch
#   no_r_exit           the loop does not leave on ||r||inf < FLT_EPSILON
LM_RULES = ("lc_stale", "nu_unclamped_10", "nu_not_halved", "lambda_always_zero", "iters_9", "mid_as_low", "no_r_exit")
LM_BREAK = frozenset()


def refine(src, dst, mask, H, max_iters=10, trace=None):
    """createLMSolver(HomographyRefineCallback(inliers), 10)->run(H[0:8]): the refined 9 doubles (H22 kept).  A `trace` dict
    receives lm: one dict per iteration with band ("high": R > 0.75, "low": R < 0.25, "mid"), lam ("zeroed" / "kept" on the
    high band, else None), inverted (the lambda == 0 re-inflation ran), nu ("clamp2" / "clamp10" / "between" on the low band,
    else None) and accepted (Sd < S); lm_exit ("iters", "d" or "r": the first test of the loop condition that failed) and
    lm_iters."""
    assert LM_BREAK <= set(LM_RULES)
    if "iters_9" in LM_BREAK:
        max_iters -= 1
    src, dst = _pairs(src, dst)
    mask = np.asarray(mask, bool)
    s, d_ = src[mask], dst[mask]
    x = np.asarray(H, np.float64)[:8].copy()
    r, J = refine_compute(s, d_, x)
    S = norm_l2sqr(r)
    A = _jtj(J)
    v = _jtr(J, r)
    D = np.diag(A).copy()
    Rlo, Rhi = 0.25, 0.75
    lam, lc = 1.0, 0.75
    it = 0
    steps = []
    while True:
        Ap = A.copy()
        for i in range(8):
            Ap[i, i] += lam * D[i]
        d = solve_eig(Ap, v)
        xd = x - d
        rd, _ = refine_compute(s, d_, xd, need_j=False)
        Sd = norm_l2sqr(rd)
        temp_d = np.array([_serial_sum(A[i] * d) * -1 + v[i] * 2 for i in range(8)])
        dS = dot(d, temp_d)
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1)
        step = dict(band="high" if R > Rhi else "low" if R < Rlo else "mid", lam=None, inverted=False, nu=None)
        if R > Rhi:
            lam *= 0.5
            if lam < lc or "lambda_always_zero" in LM_BREAK:
                lam = 0.0
            step["lam"] = "zeroed" if lam == 0 else "kept"
        elif R < Rlo or "mid_as_low" in LM_BREAK:
            t = dot(d, v)
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1) + 2
            step["nu"] = "clamp2" if nu <= 2. else "clamp10" if nu >= 10. else "between"
            nu = 2. if nu < 2. else nu
            if "nu_unclamped_10" not in LM_BREAK:
                nu = 10. if 10. < nu else nu
            if lam == 0:
                dg = invert_eig_diag(A)
                maxval = DBL_EPSILON
                for i in range(8):
                    a = abs(dg[i])
                    maxval = a if maxval < a else maxval
                lam = 1. / maxval
                if "lc_stale" not in LM_BREAK:
                    lc = lam
                if "nu_not_halved" not in LM_BREAK:
                    nu *= 0.5
                step["inverted"] = True
            lam *= nu
        step["accepted"] = bool(Sd < S)
        steps.append(step)
        if Sd < S:
            S = Sd
            x = xd
            r, J = refine_compute(s, d_, x)
            A = _jtj(J)
            v = _jtr(J, r)
        it += 1
        if not it < max_iters:
            why = "iters"
        elif not norm_inf(d) >= FLT_EPSILON:
            why = "d"
        elif not (norm_inf(r) >= FLT_EPSILON or "no_r_exit" in LM_BREAK):
            why = "r"
        else:
            continue
        break
    if trace is not None:
        trace.update(lm=steps, lm_exit=why, lm_iters=it)
    out = np.asarray(H, np.float64).copy()
    out[:8] = x
    return out


def find_homography(src, dst, method=RANSAC, threshold=3.0, max_iters=2000, confidence=0.995, taps=False):
    """(H [3, 3] float64 or None, mask uint8 [n]); with taps=True also a dict of the stage results, whose "trace" holds what
    ransac() and refine() record (empty for a stage that did not run)."""
    src, dst = _pairs(src, dst)
    n = len(src)
    if method not in (0, RANSAC):
        raise ValueError("method must be 0 or RANSAC")
    if threshold <= 0:
        threshold = 3.0
    tr = {}
    t = dict(ransac_ok=False, ransac_H=np.zeros(9), iters=0, niters=0, refit_H=np.zeros(9), refit_ok=False, trace=tr)
    if n < 4:   # H6
        return (None, np.zeros(n, np.uint8), t) if taps else (None, np.zeros(n, np.uint8))
    if method == 0 or n == 4:
        mask = np.ones(n, bool)
        H = run_kernel(src, dst)
        ok = H is not None
    else:
        rr = ransac(src, dst, threshold, max_iters, confidence, trace=tr)
        t.update(ransac_ok=rr["ok"], ransac_H=rr["H"], iters=rr["iters"], niters=rr["niters"])
        mask, ok, H = rr["mask"], rr["ok"], rr["H"]
        if ok and n > 4:
            H, t["refit_ok"] = refit(src, dst, mask, H)
            t["refit_H"] = H.copy()
    if ok and n > 4:
        H = refine(src, dst, mask, H, trace=tr)
    if not ok:
        mask = np.zeros(n, bool)
    out = (H.reshape(3, 3) if ok else None, mask.astype(np.uint8))
    return out + (t,) if taps else out
