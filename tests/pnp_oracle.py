"""numpy restatement of the reference's PnPsolver (src/PnPsolver.cc: EPnP inside the RANSAC loop of `iterate`), operation for
operation, for csrc/orbfe_pnp.hip to be checked against bit for bit.  Unpinned: OpenCV is not available, so the OpenCV 3.2
routines the file resolves to are restated from knowledge, under the numbered assumptions below.  Everything is IEEE double
(or float where the C++ uses float) with one rounding per operation, sums in the C++ order, no fused multiply-add.

The linear algebra is vectorised over a leading batch axis B (one hypothesis per entry); a lane that the C++ would have
skipped keeps its values (np.where), so every entry sees the operation sequence of its own scalar run.

  P1  cvSVD / cvInvert(CV_SVD) / cvSolve(CV_SVD) on CV_64F run JacobiSVDImpl_<double> (core/src/lapack.cpp): a one-sided
      Jacobi on the rows of At (= A transposed, n rows of length m), minval = DBL_MIN, eps = DBL_EPSILON * 10, max_iter =
      max(m, 30); W[i] starts as the row's sum of squares; a pair is skipped when |p| <= eps * sqrt(a * b); else p *= 2, beta
      = a - b, gamma = hypot(p, beta) with lapack.cpp's own hypot template (a * sqrt(1 + (b/a)^2), no libm: H3 of
      homography_oracle.py); beta < 0: s = sqrt(((gamma - beta) * 0.5) / gamma), c = p / (gamma * s * 2); else c =
      sqrt((gamma + beta) / (gamma * 2)), s = p / (gamma * c * 2); rows rotate as t0 = c * Ai + s * Aj, t1 = -s * Ai + c * Aj
      and W[i], W[j] become the new sums of squares; Vt rotates alike.  A sweep without a rotation ends the loop.  Then W[i] =
      sqrt(sum of squares), a selection sort, descending, strict <, swapping the rows of At and Vt; then for every i < n: a row
      with W[i] <= minval is refilled from RNG(0x12345678) (state = (uint32)state * 4164903690 + (state >> 32); value +-1/m by
      bit 8), orthogonalised twice against the rows before it with the L1 renormalisation (asum > eps * 100 ? 1 / asum : 0),
      up to 100 tries; every row is multiplied by 1 / W[i] (0 if not > minval).  NaN compares false everywhere, as in C++.
  P2  cv::SVD::compute transposes A into At for m >= n (all uses here), so the rows of At afterwards are the left singular
      vectors: cvSVD(A, W, U, 0, MODIFY_A | U_T) returns them as the rows of U (= U transposed); cvSVD(A, W, U, V, MODIFY_A)
      returns U and V untransposed, i.e. abt_u[3 * i + k] = At[k][i], abt_v[3 * j + k] = Vt[k][j].
  P3  SVBkSb (H4 of homography_oracle.py): threshold = (sum of w in order) * (DBL_EPSILON * 2); a singular value with |w| <=
      threshold is skipped; solve (nb = 1): s = sum_j u_i[j] * b[j], s *= 1 / w, x[j] = x[j] + s * vt_i[j]; invert (no right-hand
      side, nb = m): buffer[j] = U[j][i] * (1 / w), x[r][j] = x[r][j] + Vt[i][r] * buffer[j].
  P4  cvMulTransposed(A, dst, 1) runs MulTransposedR: dst[i][j], j >= i, is the sum over the rows k, in order from 0.0, of
      A[k][i] * A[k][j], times scale 1.0; the lower triangle is copied from the upper.
  P5  DUtils::Random::RandomInt(min, max) = min + (int)(((double)rand() / (RAND_MAX + 1.0)) * (max - min + 1)), RAND_MAX =
      2^31 - 1 (S-numbered likewise in sim3_oracle.py).
  P6  qr_solve's singular branch returns without writing X.  In the reference the first Gauss-Newton step then adds an
      uninitialised stack array.  THE LIBRARY'S DECISION, shared by this oracle: x starts at zeros before the five steps, and
      a singular step leaves it at the previous step's values, as the C++ would.
  P7  qr_solve's pivot scan reads rows k, k .. nr - 2 (its pointer starts on the diagonal and trails the index by one); kept.
  P8  CheckInliers: Xc / Yc are double sums stored to float; `1 / (double sum)` is a double division (int over double) stored
      to float; ue = uc + fu * Xc * invZc in double; distX = (float)(P2D.x - ue); error2 = distX * distX + distY * distY in
      float; the test is error2 < sigma2 * th2, float, strict.
  P9  iterate(n) on a solver: the loop runs while mnIterations < mRansacMaxIts OR nCurrentIterations < n.
  P10 SetRansacParameters computes log / pow / ceil in the host's libm; pow(epsilon, 3) although the set is 4; the int
      conversion of an out-of-range or NaN double gives INT_MIN (x86-64).
"""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")

# ---- the break switch (tests/test_pnp_edge_cases.py) --------------------------------------------------------------------------
# One rule at a time is broken to show that a case table would notice.  Empty: the oracle proper, bit for bit.
EPNP_RULES = {   # the EPnP arithmetic: these take a scope
    "betas1_sign": "_betas_1 with b4[0] < 0 leaves betas 1..3 un-negated",
    "betas23_b0": "_betas_23 with b[0] < 0 tests b[2] as the other arm does (> 0)",
    "betas23_b2": "_betas_23 takes sqrt(|b[2]|) whatever the sign of b[2]",
    "betas23_b1": "_betas_23 never negates beta 0 on b[1] < 0",
    "solve_for_sign": "the camera points are never negated",
    "det_neg": "the third row of R is never negated",
    "choose_2": "N = 2 is never chosen",
    "choose_3": "N = 3 is never chosen",
}
SCAN_RULES = {   # the acceptance scan of iterate
    "best_tie_replaces": "a count equal to the best replaces it",
    "refine_current_mask": "Refine runs over the current iteration's mask",
    "refine_return_ge": "Refine returns on rcnt >= min_inliers",
    "loop_and": "the loop runs while iterations < max_its AND cur < n_iterations",
}
EPNP_BREAK = frozenset()
EPNP_BREAK_SCOPE = "all"   # "all": every compute_pose; "refine": only calls over more than four points (the cooperative path)


def _broken(rule, n):
    return rule in EPNP_BREAK and (EPNP_BREAK_SCOPE == "all" or n > 4)


# ---- draws (P5) ---------------------------------------------------------------------------------------------------------------
def index_from_draw(r, size):
    return int((float(int(r) & 0x7fffffff) / 2147483648.0) * size)


def quad_from_draws(d, n):
    """the four swap-with-back / pop-back selections out of a fresh 0 .. n-1, with the list"""
    avail = list(range(n))
    out = []
    for k in range(4):
        p = index_from_draw(d[k], len(avail))
        out.append(avail[p])
        avail[p] = avail[-1]
        avail.pop()
    return out


# ---- SetRansacParameters (P10) --------------------------------------------------------------------------------------------------
def _to_int(v):
    if v != v or v <= -2147483649.0 or v >= 2147483648.0:
        return -2147483648
    return int(v)


def ransac_params(probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4, n=0):
    """-> (mRansacMinInliers, mRansacEpsilon (float32), mRansacMaxIts)"""
    eps = np.float32(epsilon)
    n_min = _to_int(float(np.float32(n) * eps))   # int * float -> float
    if n_min < min_inliers:
        n_min = min_inliers
    if n_min < min_set:
        n_min = min_set
    with np.errstate(**_ERR):
        ratio = np.float32(n_min) / np.float32(n)
    if eps < ratio:
        eps = ratio
    if n_min == n:
        its = 1
    else:
        def _log(x):
            return math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan)
        with np.errstate(**_ERR):
            v = np.float64(_log(1 - probability)) / np.float64(_log(1 - math.pow(float(eps), 3)))
        its = _to_int(float(np.ceil(v)))
    its = max(1, min(its, max_its))
    return int(n_min), np.float32(eps), int(its)


# ---- sequential sums ------------------------------------------------------------------------------------------------------------
def seqsum(terms, axis=-1):
    """0.0 + t0 + t1 + ... strictly in order along `axis`"""
    t = np.moveaxis(np.asarray(terms, np.float64), axis, -1)
    z = np.zeros(t.shape[:-1] + (1,))
    return np.add.accumulate(np.concatenate([z, t], -1), axis=-1)[..., -1]


def cv_hypot(a, b):
    a = np.abs(a)
    b = np.abs(b)
    with np.errstate(**_ERR):
        big = a > b
        r1 = a * np.sqrt(1 + (b / a) * (b / a))
        r2 = b * np.sqrt(1 + (a / b) * (a / b))
    return np.where(big, r1, np.where(b > 0, r2, 0.0))


class _RNG:
    def __init__(self, state):
        self.state = state or 0xffffffff

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & 0xffffffffffffffff
        return self.state & 0xffffffff


def _refill(At, W, m, n):
    """the tail of JacobiSVDImpl_ for one matrix: random refill of null rows and the 1 / W scaling (scalar code)"""
    eps = DBL_EPSILON * 10
    rng = _RNG(0x12345678)
    with np.errstate(**_ERR):
        for i in range(n):
            sd = W[i]
            ii = 0
            while ii < 100 and sd <= DBL_MIN:
                val0 = np.float64(1.0) / np.float64(m)
                for k in range(m):
                    At[i, k] = val0 if (rng.next() & 256) != 0 else -val0
                for _ in range(2):
                    for j in range(i):
                        sd = np.float64(0)
                        for k in range(m):
                            sd = sd + At[i, k] * At[j, k]
                        asum = np.float64(0)
                        for k in range(m):
                            t = At[i, k] - sd * At[j, k]
                            At[i, k] = t
                            asum = asum + abs(t)
                        asum = 1 / asum if asum > eps * 100 else np.float64(0)
                        for k in range(m):
                            At[i, k] = At[i, k] * asum
                sd = np.float64(0)
                for k in range(m):
                    sd = sd + At[i, k] * At[i, k]
                sd = np.sqrt(sd)
                ii += 1
            s = 1 / sd if sd > DBL_MIN else np.float64(0)
            for k in range(m):
                At[i, k] = At[i, k] * s


def jacobi_svd(At):
    """JacobiSVDImpl_<double> (P1) on At [B, n, m] (the transposed matrices).  -> (W [B, n], Ut [B, n, m], Vt [B, n, n])"""
    At = np.array(At, dtype=np.float64, copy=True)
    B, n, m = At.shape
    eps = DBL_EPSILON * 10
    with np.errstate(**_ERR):
        W = seqsum(At * At)
        Vt = np.broadcast_to(np.eye(n), (B, n, n)).copy()
        for _ in range(max(m, 30)):
            changed = np.zeros(B, bool)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[:, i, :].copy(), At[:, j, :].copy()
                    a, b = W[:, i], W[:, j]
                    p = seqsum(Ai * Aj)
                    act = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not act.any():
                        continue
                    p = p * 2
                    beta = a - b
                    gamma = cv_hypot(p, beta)
                    s_n = np.sqrt(((gamma - beta) * 0.5) / gamma)
                    c_n = p / (gamma * s_n * 2)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2))
                    s_p = p / (gamma * c_p * 2)
                    neg = beta < 0
                    c = np.where(neg, c_n, c_p)[:, None]
                    s = np.where(neg, s_n, s_p)[:, None]
                    t0 = c * Ai + s * Aj
                    t1 = (-s) * Ai + c * Aj
                    am = act[:, None]
                    At[:, i, :] = np.where(am, t0, Ai)
                    At[:, j, :] = np.where(am, t1, Aj)
                    W[:, i] = np.where(act, seqsum(t0 * t0), a)
                    W[:, j] = np.where(act, seqsum(t1 * t1), b)
                    Vi, Vj = Vt[:, i, :].copy(), Vt[:, j, :].copy()
                    Vt[:, i, :] = np.where(am, c * Vi + s * Vj, Vi)
                    Vt[:, j, :] = np.where(am, (-s) * Vi + c * Vj, Vj)
                    changed |= act
            if not changed.any():
                break
        W = np.sqrt(seqsum(At * At))
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
        plain = np.all(W > DBL_MIN, axis=1)
        s = np.where(W > DBL_MIN, 1 / W, 0.0)
        At_scaled = At * s[:, :, None]
        for q in np.nonzero(~plain)[0]:
            _refill(At[q], W[q], m, n)
            At_scaled[q] = At[q]
    return W, At_scaled, Vt


def svd(A):
    """cv::SVD::compute on A [B, m, n], m >= n (P2) -> (w [B, n], Ut [B, n, m], Vt [B, n, n])"""
    A = np.asarray(A, np.float64)
    return jacobi_svd(np.swapaxes(A, 1, 2))


def _threshold(w):
    return seqsum(w) * (DBL_EPSILON * 2)


def sv_solve(A, b):
    """cvSolve(A, b, x, CV_SVD) (P3): A [B, m, n], b [B, m] -> x [B, n]"""
    w, Ut, Vt = svd(A)
    B, n = w.shape
    x = np.zeros((B, n))
    thr = _threshold(w)
    with np.errstate(**_ERR):
        for i in range(n):
            wi = w[:, i]
            skip = np.abs(wi) <= thr
            s = seqsum(Ut[:, i, :] * b) * (1 / wi)
            x = np.where(skip[:, None], x, x + s[:, None] * Vt[:, i, :])
    return x


def sv_invert(A):
    """cvInvert(A, Ainv, CV_SVD) on square A [B, n, n] (P3)"""
    w, Ut, Vt = svd(A)
    B, n = w.shape
    x = np.zeros((B, n, n))
    thr = _threshold(w)
    with np.errstate(**_ERR):
        for i in range(n):
            wi = w[:, i]
            skip = np.abs(wi) <= thr
            buf = Ut[:, i, :] * (1 / wi)[:, None]            # buffer[j] = U[j][i] * wi
            upd = x + Vt[:, i, :, None] * buf[:, None, :]      # x[r][j] + Vt[i][r] * buffer[j]
            x = np.where(skip[:, None, None], x, upd)
    return x


def mul_transposed(A):
    """cvMulTransposed(A, dst, 1) (P4): A [B, rows, cols] -> [B, cols, cols]"""
    A = np.asarray(A, np.float64)
    with np.errstate(**_ERR):
        return seqsum(A[:, :, :, None] * A[:, :, None, :], axis=1)   # symmetric by commutativity of the products


def qr_solve(A, b, x, kept=None):
    """qr_solve (P6, P7) on A [B, nr, nc], b [B, nr]; x [B, nc] is overwritten where the matrix is not found singular.  `kept`
    (bool [B], in / out) is set where x was left as it was"""
    A = np.array(A, np.float64, copy=True)
    b = np.array(b, np.float64, copy=True)
    x = np.array(x, np.float64, copy=True)
    B, nr, nc = A.shape
    A1 = np.zeros((B, nc))
    A2 = np.zeros((B, nc))
    alive = np.ones(B, bool)
    with np.errstate(**_ERR):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            alive = alive & ~(eta == 0)
            inv_eta = 1.0 / eta
            col = A[:, k:, k] * inv_eta[:, None]
            sigma = np.sqrt(seqsum(col * col))
            sigma = np.where(col[:, 0] < 0, -sigma, sigma)
            col[:, 0] = col[:, 0] + sigma
            A[:, k:, k] = col
            A1[:, k] = sigma * col[:, 0]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                tau = seqsum(col * A[:, k:, j]) / A1[:, k]
                A[:, k:, j] = A[:, k:, j] - tau[:, None] * col
        for j in range(nc):
            tau = seqsum(A[:, j:, j] * b[:, j:]) / A1[:, j]
            b[:, j:] = b[:, j:] - tau[:, None] * A[:, j:, j]
        X = np.zeros((B, nc))
        X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            X[:, i] = (b[:, i] - seqsum(A[:, i, i + 1:] * X[:, i + 1:])) / A2[:, i]
    if kept is not None:
        kept |= ~alive
    return np.where(alive[:, None], X, x)


# ---- EPnP -----------------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _dist2(a, b):
    d = a - b
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def compute_pose(pws, us, K, detail=False, trace=None):
    """compute_pose on pws [B, n, 3], us [B, n, 2] (double), K = (fu, fv, uc, vc) -> (R [B, 3, 3], t [B, 3], err [B], N [B]); with
    detail also the three reprojection errors [B, 3].  A `trace` dict receives, per item: betas1_neg bool [B]; betas23_arm {2, 3:
    int [B]} = 4 * (b[0] < 0) + 2 * (b[2] < 0) + (b[1] < 0); flip and det_neg {1, 2, 3: bool [B]}; qr_kept {1, 2, 3: bool [B]} (a
    Gauss-Newton step left x as it was); N [B]; n."""
    pws = np.asarray(pws, np.float64)
    us = np.asarray(us, np.float64)
    fu, fv, uc, vc = (np.float64(v) for v in K)
    B, n, _ = pws.shape
    nd = np.float64(n)
    with np.errstate(**_ERR):
        # choose_control_points
        cws = np.zeros((B, 4, 3))
        cws[:, 0] = seqsum(pws, axis=1) / nd
        pw0 = pws - cws[:, None, 0]
        dc, uct, _ = svd(mul_transposed(pw0))
        for i in range(1, 4):
            k = np.sqrt(dc[:, i - 1] / nd)
            cws[:, i] = cws[:, 0] + k[:, None] * uct[:, i - 1]
        # compute_barycentric_coordinates
        cc = np.swapaxes(cws[:, 1:] - cws[:, None, 0], 1, 2)   # cc[i][j - 1] = cws[j][i] - cws[0][i]
        ci = sv_invert(cc)
        d = pws - cws[:, None, 0]
        alphas = np.zeros((B, n, 4))
        for j in range(3):
            alphas[:, :, 1 + j] = ci[:, None, j, 0] * d[:, :, 0] + ci[:, None, j, 1] * d[:, :, 1] + ci[:, None, j, 2] * d[:, :, 2]
        alphas[:, :, 0] = 1.0 - alphas[:, :, 1] - alphas[:, :, 2] - alphas[:, :, 3]
        # fill_M, MtM, its SVD
        M = np.zeros((B, 2 * n, 12))
        for i in range(4):
            M[:, 0::2, 3 * i] = alphas[:, :, i] * fu
            M[:, 0::2, 3 * i + 2] = alphas[:, :, i] * (uc - us[:, :, 0])
            M[:, 1::2, 3 * i + 1] = alphas[:, :, i] * fv
            M[:, 1::2, 3 * i + 2] = alphas[:, :, i] * (vc - us[:, :, 1])
        _, ut, _ = svd(mul_transposed(M))
        # compute_L_6x10, compute_rho
        v = [ut[:, 11 - i].reshape(B, 4, 3) for i in range(4)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = [[v[i][:, a] - v[i][:, b] for (a, b) in pairs] for i in range(4)]
        L = np.zeros((B, 6, 10))
        for i in range(6):
            L[:, i, 0] = _dot3(dv[0][i], dv[0][i])
            L[:, i, 1] = 2.0 * _dot3(dv[0][i], dv[1][i])
            L[:, i, 2] = _dot3(dv[1][i], dv[1][i])
            L[:, i, 3] = 2.0 * _dot3(dv[0][i], dv[2][i])
            L[:, i, 4] = 2.0 * _dot3(dv[1][i], dv[2][i])
            L[:, i, 5] = _dot3(dv[2][i], dv[2][i])
            L[:, i, 6] = 2.0 * _dot3(dv[0][i], dv[3][i])
            L[:, i, 7] = 2.0 * _dot3(dv[1][i], dv[3][i])
            L[:, i, 8] = 2.0 * _dot3(dv[2][i], dv[3][i])
            L[:, i, 9] = _dot3(dv[3][i], dv[3][i])
        rho = np.stack([_dist2(cws[:, a], cws[:, b]) for (a, b) in pairs], 1)
        tr = dict(n=n, betas23_arm={}, flip={}, det_neg={}, qr_kept={})
        betas = [None, _betas_1(L, rho, n, tr), _betas_2(L, rho, n, tr), _betas_3(L, rho, n, tr)]
        Rs, ts, errs = [None], [None], [None]
        for k in (1, 2, 3):
            tr["qr_kept"][k] = np.zeros(B, bool)
            betas[k] = gauss_newton(L, rho, betas[k], tr["qr_kept"][k])
            R, t = _compute_R_and_t(ut, betas[k], alphas, pws, tr, k)
            Rs.append(R)
            ts.append(t)
            errs.append(reprojection_error(R, t, pws, us, K))
        N = np.ones(B, np.int64)
        if not _broken("choose_2", n):
            N = np.where(errs[2] < errs[1], 2, N)
        eN = np.where(N == 2, errs[2], errs[1])
        if not _broken("choose_3", n):
            N = np.where(errs[3] < eN, 3, N)
        tr["N"] = N
        if trace is not None:
            trace.update(tr)
        R = np.where((N == 1)[:, None, None], Rs[1], np.where((N == 2)[:, None, None], Rs[2], Rs[3]))
        t = np.where((N == 1)[:, None], ts[1], np.where((N == 2)[:, None], ts[2], ts[3]))
        err = np.where(N == 1, errs[1], np.where(N == 2, errs[2], errs[3]))
    if detail:
        return R, t, err, N, np.stack(errs[1:], 1)
    return R, t, err, N


def _betas_1(L, rho, n=4, tr=None):
    b4 = sv_solve(L[:, :, [0, 1, 3, 6]], rho)
    neg = b4[:, 0] < 0
    if tr is not None:
        tr["betas1_neg"] = neg
    b0 = np.sqrt(np.where(neg, -b4[:, 0], b4[:, 0]))
    out = np.zeros_like(b4)
    out[:, 0] = b0
    neg_rest = neg & (not _broken("betas1_sign", n))
    for k in (1, 2, 3):
        out[:, k] = np.where(neg_rest, -b4[:, k], b4[:, k]) / b0
    return out


def _betas_23(b, third, n=4, tr=None):
    neg = b[:, 0] < 0
    if tr is not None:
        tr["betas23_arm"][3 if third else 2] = 4 * neg.astype(np.int64) + 2 * (b[:, 2] < 0) + (b[:, 1] < 0)
    b0 = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
    pos_rule = np.where(b[:, 2] > 0, np.sqrt(b[:, 2]), 0.0)
    neg_rule = pos_rule if _broken("betas23_b0", n) else np.where(b[:, 2] < 0, np.sqrt(-b[:, 2]), 0.0)
    b1 = np.where(neg, neg_rule, pos_rule)
    if _broken("betas23_b2", n):
        b1 = np.sqrt(np.abs(b[:, 2]))
    if not _broken("betas23_b1", n):
        b0 = np.where(b[:, 1] < 0, -b0, b0)
    out = np.zeros((len(b), 4))
    out[:, 0] = b0
    out[:, 1] = b1
    if third:
        out[:, 2] = b[:, 3] / b0
    return out


def _betas_2(L, rho, n=4, tr=None):
    return _betas_23(sv_solve(L[:, :, [0, 1, 2]], rho), False, n, tr)


def _betas_3(L, rho, n=4, tr=None):
    return _betas_23(sv_solve(L[:, :, [0, 1, 2, 3, 4]], rho), True, n, tr)


def gauss_newton(L, rho, betas, kept=None):
    betas = np.array(betas, np.float64, copy=True)
    B = len(betas)
    x = np.zeros((B, 4))   # P6
    for _ in range(5):
        b0, b1, b2, b3 = (betas[:, k, None] for k in range(4))
        A = np.zeros((B, 6, 4))
        A[:, :, 0] = (2 * L[:, :, 0] * b0 + L[:, :, 1] * b1 + L[:, :, 3] * b2 + L[:, :, 6] * b3)
        A[:, :, 1] = (L[:, :, 1] * b0 + 2 * L[:, :, 2] * b1 + L[:, :, 4] * b2 + L[:, :, 7] * b3)
        A[:, :, 2] = (L[:, :, 3] * b0 + L[:, :, 4] * b1 + 2 * L[:, :, 5] * b2 + L[:, :, 8] * b3)
        A[:, :, 3] = (L[:, :, 6] * b0 + L[:, :, 7] * b1 + L[:, :, 8] * b2 + 2 * L[:, :, 9] * b3)
        b = rho - (L[:, :, 0] * b0 * b0 + L[:, :, 1] * b0 * b1 + L[:, :, 2] * b1 * b1 + L[:, :, 3] * b0 * b2 + L[:, :, 4] * b1 * b2 +
                   L[:, :, 5] * b2 * b2 + L[:, :, 6] * b0 * b3 + L[:, :, 7] * b1 * b3 + L[:, :, 8] * b2 * b3 + L[:, :, 9] * b3 * b3)
        x = qr_solve(A, b, x, kept)
        betas = betas + x
    return betas


def _compute_R_and_t(ut, betas, alphas, pws, tr=None, k=0):
    B, n, _ = pws.shape
    nd = np.float64(n)
    ccs = np.zeros((B, 4, 3))
    for i in range(4):
        ccs = ccs + betas[:, i, None, None] * ut[:, 11 - i].reshape(B, 4, 3)
    pcs = (alphas[:, :, 0, None] * ccs[:, None, 0] + alphas[:, :, 1, None] * ccs[:, None, 1] + alphas[:, :, 2, None] * ccs[:, None, 2] +
           alphas[:, :, 3, None] * ccs[:, None, 3])
    flip = pcs[:, 0, 2] < 0.0   # solve_for_sign
    if tr is not None:
        tr["flip"][k] = flip
    if not _broken("solve_for_sign", n):
        pcs = np.where(flip[:, None, None], -pcs, pcs)
    # estimate_R_and_t
    pc0 = seqsum(pcs, axis=1) / nd
    pw0 = seqsum(pws, axis=1) / nd
    dpc = pcs - pc0[:, None]
    dpw = pws - pw0[:, None]
    abt = seqsum(dpc[:, :, :, None] * dpw[:, :, None, :], axis=1)
    _, Ut, Vt = svd(abt)
    U = np.swapaxes(Ut, 1, 2)
    V = np.swapaxes(Vt, 1, 2)
    R = np.zeros((B, 3, 3))
    for i in range(3):
        for j in range(3):
            R[:, i, j] = _dot3(U[:, i], V[:, j])
    det = (R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] -
           R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1])
    if tr is not None:
        tr["det_neg"][k] = det < 0
    if not _broken("det_neg", n):
        R[:, 2] = np.where((det < 0)[:, None], -R[:, 2], R[:, 2])
    t = np.stack([pc0[:, k] - _dot3(R[:, k], pw0) for k in range(3)], 1)
    return R, t


def reprojection_error(R, t, pws, us, K):
    fu, fv, uc, vc = (np.float64(v) for v in K)
    n = pws.shape[1]
    Xc = _dot3(R[:, None, 0], pws) + t[:, None, 0]
    Yc = _dot3(R[:, None, 1], pws) + t[:, None, 1]
    inv = 1.0 / (_dot3(R[:, None, 2], pws) + t[:, None, 2])
    ue = uc + fu * Xc * inv
    ve = vc + fv * Yc * inv
    du = us[:, :, 0] - ue
    dv = us[:, :, 1] - ve
    return seqsum(np.sqrt(du * du + dv * dv)) / np.float64(n)


# ---- CheckInliers (P8) ----------------------------------------------------------------------------------------------------------
def check_inliers(R, t, P3Dw, P2D, max_error, K):
    """R [3, 3], t [3] double; P3Dw [N, 3], P2D [N, 2], max_error [N] float32 -> (mask bool [N], error2 float32 [N])"""
    fu, fv, uc, vc = (np.float64(v) for v in K)
    P = np.asarray(P3Dw, np.float32).astype(np.float64)
    p2 = np.asarray(P2D, np.float32)
    with np.errstate(**_ERR):
        row = [R[k, 0] * P[:, 0] + R[k, 1] * P[:, 1] + R[k, 2] * P[:, 2] + t[k] for k in range(3)]
        Xc = row[0].astype(np.float32)
        Yc = row[1].astype(np.float32)
        invZ = (1.0 / row[2]).astype(np.float32)
        ue = uc + fu * Xc.astype(np.float64) * invZ.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZ.astype(np.float64)
        dx = (p2[:, 0].astype(np.float64) - ue).astype(np.float32)
        dy = (p2[:, 1].astype(np.float64) - ve).astype(np.float32)
        e2 = dx * dx + dy * dy
        return e2 < np.asarray(max_error, np.float32), e2


def tcw_from(R, t):
    T = np.eye(4, dtype=np.float32)
    with np.errstate(**_ERR):
        T[:3, :3] = np.asarray(R, np.float64).astype(np.float32)
        T[:3, 3] = np.asarray(t, np.float64).astype(np.float32)
    return T


class PnPSolver:
    """The reference's class on flattened inputs: P3Dw [N, 3], P2D [N, 2], sigma2 [N] (float32), K = (fu, fv, uc, vc)."""

    def __init__(self, P3Dw, P2D, sigma2, K):
        self.P3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        self.P2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.K = tuple(float(np.float32(v)) for v in K)
        self.N = len(self.P3Dw)
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_Tcw = np.zeros((4, 4), np.float32)
        self.refine_log = []   # one trace of compute_pose per refine(), with m, the inliers it ran over
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4, th2=5.991):
        self.min_inliers, self.epsilon, self.max_its = ransac_params(probability, min_inliers, max_its, min_set, epsilon, self.N)
        self.max_error = self.sigma2 * np.float32(th2)

    def _pose(self, idx, trace=None):
        pws = self.P3Dw[idx].astype(np.float64)[None]
        us = self.P2D[idx].astype(np.float64)[None]
        return compute_pose(pws, us, self.K, detail=True, trace=trace)

    def refine(self, over=None):
        idx = np.nonzero(self.best_mask if over is None else over)[0]
        tr = dict(m=len(idx))
        R, t, _, _, _ = self._pose(idx, tr)
        self.refine_log.append(tr)
        mask, _ = check_inliers(R[0], t[0], self.P3Dw, self.P2D, self.max_error, self.K)
        cnt = int(mask.sum())
        ok = cnt >= self.min_inliers if "refine_return_ge" in EPNP_BREAK else cnt > self.min_inliers
        return ok, mask, cnt, tcw_from(R[0], t[0])

    def iterate(self, n_iterations, draws, taps=None):
        """-> dict(Tcw float32 [4, 4] or None, no_more, mask bool [N], n_inliers, iterations_run).  `draws`: four raw values per
        iteration; max(n_iterations, max_its - iterations) iterations can run (P9)."""
        out = dict(Tcw=None, no_more=False, mask=np.zeros(self.N, bool), n_inliers=0, iterations_run=0)
        if self.N < self.min_inliers or self.N < 4:
            out["no_more"] = True
            return out
        draws = np.asarray(draws).reshape(-1)
        total = max(int(n_iterations), self.max_its - self.iterations, 0)
        # every hypothesis of the call at once (one is a function of its own draws only); the scan below walks them in order
        quads = np.array([quad_from_draws(draws[4 * k:4 * k + 4], self.N) for k in range(total)], np.int64).reshape(total, 4)
        if total:
            R, t, _, Nc, _ = compute_pose(self.P3Dw[quads].astype(np.float64), self.P2D[quads].astype(np.float64), self.K, detail=True)
        assert EPNP_BREAK <= set(EPNP_RULES) | set(SCAN_RULES) and EPNP_BREAK_SCOPE in ("all", "refine")
        cur = 0
        while ((self.iterations < self.max_its and cur < n_iterations) if "loop_and" in EPNP_BREAK else
               (self.iterations < self.max_its or cur < n_iterations)):
            k = cur
            cur += 1
            self.iterations += 1
            out["iterations_run"] = cur
            mask, e2 = check_inliers(R[k], t[k], self.P3Dw, self.P2D, self.max_error, self.K)
            cnt = int(mask.sum())
            rec = dict(quad=quads[k].copy(), N=int(Nc[k]), R=R[k].copy(), t=t[k].copy(), n_inliers=cnt, refined=False, refine_inliers=0,
                       error2=e2, mask=mask)
            if taps is not None:
                taps.append(rec)
            if cnt >= self.min_inliers:
                if cnt > self.best_inliers or ("best_tie_replaces" in EPNP_BREAK and cnt == self.best_inliers):
                    self.best_mask = mask.copy()
                    self.best_inliers = cnt
                    self.best_Tcw = tcw_from(R[k], t[k])
                ok, rmask, rcnt, rT = self.refine(mask if "refine_current_mask" in EPNP_BREAK else None)
                rec["refined"] = True
                rec["refine"] = self.refine_log[-1]
                rec["refine_inliers"] = rcnt
                if ok:
                    out.update(Tcw=rT, mask=rmask, n_inliers=rcnt)
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
            if self.best_inliers >= self.min_inliers:
                out.update(Tcw=self.best_Tcw.copy(), mask=self.best_mask.copy(), n_inliers=self.best_inliers)
        return out

    def find(self, draws):
        return self.iterate(self.max_its, draws)


def construct(keys_pt, keys_octave, level_sigma2, mappoint_index, mappoint_pos):
    """The constructor's gather: for every keypoint with a map point (index >= 0: neither NULL nor bad), in keypoint order, its
    undistorted position, the sigma^2 of its octave, the map point's position and the keypoint's index.
    -> (P2D [N, 2], sigma2 [N], P3Dw [N, 3], mvKeyPointIndices [N])"""
    P2D, sg, P3, kp = [], [], [], []
    for i, m in enumerate(mappoint_index):
        if m >= 0:
            P2D.append(keys_pt[i])
            sg.append(level_sigma2[keys_octave[i]])
            P3.append(mappoint_pos[m])
            kp.append(i)
    return (np.array(P2D, np.float32).reshape(-1, 2), np.array(sg, np.float32), np.array(P3, np.float32).reshape(-1, 3),
            np.array(kp, np.int32))
