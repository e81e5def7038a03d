"""CPU oracle of FlowSLAM::Flow::ComputeMask(GrayImg, Homo, mask, th) (perfect/src/Flow.cc:73-80): cv::warpPerspective(GrayImg,
dest, Homo, GrayImg.size()) with its defaults (INTER_LINEAR, BORDER_CONSTANT, border value 0, no WARP_INVERSE_MAP), then the
plain ComputeMask of tests/flow_oracle.py on the warped frame.

It restates OpenCV 3.2's generic C++ path for a CV_8UC1 frame in numpy (modules/imgproc/src/imgwarp.cpp, core/src/lapack.cpp):
  * the matrix: Homo converted to a 3x3 double matrix (a CV_32F one widened exactly), inverted by invert(DECOMP_LU), which for
    n = 3 is the closed form d = det3(M), d = 1./d, t[k] = (cofactor difference) * d; a singular M leaves all zeros;
  * WarpPerspectiveInvoker: the frame in blocks of bh0 = min(16, h) rows and bw0 = min(1024 / bh0, w) columns; per row of a
    block X0 = M0*xb + M1*y + M2 (and Y0, W0) at the block's first column xb, then per pixel x1 = x - xb:
    W = W0 + M6*x1, W = W ? 32/W : 0, fX = max(INT_MIN, min(INT_MAX, (X0 + M0*x1)*W)), X = cvRound(fX), source cell
    saturate_cast<short>(X >> 5), sub-pixel index (Y & 31)*32 + (X & 31).  float64, one operation at a time, no FMA;
  * remapBilinear<FixedPtCast<int, uchar, 15>, RemapVec_8u, short> with the table of initInterTab2D(INTER_LINEAR, true):
    (v0*w0 + v1*w1 + v2*w2 + v3*w3 + 16384) >> 15 when all four neighbours are inside, 0 when the sample is wholly outside,
    otherwise the neighbours outside the frame count as the border value 0.

The block split matters: M0*xb + M0*x1 is not M0*x in floating point, so the column blocks change bits.

The table.  For INTER_LINEAR every float weight (1 - i/32)(1 - j/32)... is exact, and 32768 times it is an integer, but the
(0, 0) entry's 32768 saturates to 32767 as a short.  Its sum is then 32767 and the sum fix runs: with ksize = 2 it searches
entries [3..6] of the 2x2 block (ksize/2 = 1 is its start), which are entry 0's last weight and three zeros of the next, not
yet written entry, so it adds the missing 1 to w3: entry 0 is (32767, 0, 0, 1).  For a u8 output that gives the same value
as (32768, 0, 0, 0) for every v0, v3 (the remainder (v3 - v0 + 16384) stays inside [0, 32768)), so a kernel may use the closed
form (32-ty)(32-tx)*32, (32-ty)*tx*32, ty*(32-tx)*32, ty*tx*32; tests/test_warp_oracle.py checks both facts.

UNPINNED.  OpenCV is not available to this project, so this oracle has never been compared with a real OpenCV build.  The
points below rest on knowledge of the OpenCV 3.2 sources and could not be confirmed here:

  W1  The SSE4.1 coordinate loop of WarpPerspectiveInvoker gives the same bits as the scalar one: the same operations
      (M6*x1 + W0 is W0 + M6*x1, addition commutes), the same division and clamps, and _mm_cvtpd_epi32 rounds to nearest
      even as cvRound does.  The one difference, a NaN product (0 * inf when |W| < 32 / DBL_MAX), gives INT_MAX in the
      scalar std::min / std::max and INT_MIN in _mm_min_pd / _mm_max_pd / cvtpd; no finite homography reaches it in
      practice, and this oracle (and the library) take the scalar form.
  W2  RemapVec_8u (the SSE2 loop over runs of inlier pixels) gives the same bits as the scalar loop: the same integer
      weights from the short table, the same + 16384 >> 15.
  W3  The IPP branch of 3.2's warpPerspective is disabled (IPP_DISABLE_BLOCK), and no HAL or OpenVX hook replaces the
      generic path (none is built by default).
  W4  invert's n = 3 formulas and their operation order, for CV_64F: det3 as
      m00*(m11*m22 - m12*m21) - m01*(m10*m22 - m12*m20) + m02*(m10*m21 - m11*m20), then t[k] as listed in invert3().
  W5  A singular M (det3 == 0) leaves an all-zero inverse (dst = Scalar(0)), so every destination pixel maps to source (0, 0)
      with zero sub-pixel offset and the warped frame is src[0][0] everywhere.
  W6  initInterTab2D's sum fix for INTER_LINEAR (described above), and that the short table is the one remap uses for u8.
"""
import numpy as np


F32, F64 = np.float32, np.float64
INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS          # 32
INTER_REMAP_COEF_SCALE = 1 << 15          # 32768
INT_MIN, INT_MAX = -2147483648, 2147483647
BLOCK_SZ = 32


# ---- the matrix -------------------------------------------------------------------------------------------------------------
def as_matrix(H):
    """Homo as warpPerspective takes it: 3x3, CV_32F or CV_64F, converted to double (exact for float32)."""
    H = np.asarray(H)
    assert H.shape == (3, 3) and H.dtype in (np.float32, np.float64), "warpPerspective: M0 must be a 3x3 CV_32F / CV_64F matrix"
    return [[float(H[r, c]) for c in range(3)] for r in range(3)]


def invert3(M):
    """cv::invert(M, M, DECOMP_LU) for a 3x3 double matrix (lapack.cpp, n == 3): Python floats are IEEE doubles, one operation
    at a time.  Returns 9 floats, row-major; all zeros when det3 == 0 (W4, W5)."""
    m = M
    d = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) + \
        m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])
    if d == 0.0:
        return [0.0] * 9
    d = 1.0 / d
    return [(m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d,
            (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d,
            (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d,
            (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d,
            (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d,
            (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d,
            (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d,
            (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d,
            (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d]


# ---- the coordinates --------------------------------------------------------------------------------------------------------
def block_size(w, h):
    """WarpPerspectiveInvoker's block: (bw0, bh0).  Only the column split changes bits (rows enter as the integer y + y1)."""
    bh0 = min(BLOCK_SZ // 2, h)
    bw0 = min(BLOCK_SZ * BLOCK_SZ // bh0, w)
    bh0 = min(BLOCK_SZ * BLOCK_SZ // bw0, h)
    return bw0, bh0


def _std_min(a, b):
    return np.where(b < a, b, a)


def _std_max(a, b):
    return np.where(a < b, b, a)


def coordinates(Minv, w, h, split=True):
    """The invoker's per-pixel results for the inverse matrix Minv (9 floats): (sx, sy) int16-saturated source cells and the
    sub-pixel index alpha, each int64 [h, w]; plus the raw fixed-point X, Y and W (for the coverage tests).  split=False
    computes every pixel as one block starting at column 0 (what a kernel that ignores the split would get)."""
    M = [F64(v) for v in Minv]
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    bw0 = block_size(w, h)[0] if split else w
    xb = (x // bw0) * bw0
    x1 = x - xb
    xbf, yf, x1f = xb.astype(F64), y.astype(F64), x1.astype(F64)
    X0 = M[0] * xbf + M[1] * yf + M[2]
    Y0 = M[3] * xbf + M[4] * yf + M[5]
    W0 = M[6] * xbf + M[7] * yf + M[8]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = W0 + M[6] * x1f
        W = np.where(W != 0, F64(INTER_TAB_SIZE) / np.where(W != 0, W, 1.0), F64(0))
        tX = (X0 + M[0] * x1f) * W
        tY = (Y0 + M[3] * x1f) * W
    fX = _std_max(F64(INT_MIN), _std_min(F64(INT_MAX), tX))
    fY = _std_max(F64(INT_MIN), _std_min(F64(INT_MAX), tY))
    X = np.rint(fX).astype(np.int64)      # saturate_cast<int>(double) = cvRound: nearest, ties to even
    Y = np.rint(fY).astype(np.int64)
    sx = np.clip(X >> INTER_BITS, -32768, 32767)
    sy = np.clip(Y >> INTER_BITS, -32768, 32767)
    alpha = (Y & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (X & (INTER_TAB_SIZE - 1))
    return sx, sy, alpha, X, Y, np.broadcast_to(W0 + M[6] * x1f, (h, w))


# ---- the table --------------------------------------------------------------------------------------------------------------
def _saturate_short(v):
    r = int(np.rint(v))
    return max(-32768, min(32767, r))


def inter_tab_linear():
    """initInterTab2D(INTER_LINEAR, fixpt=true): int16 [1024, 4] (entry ty*32 + tx: w00, w01, w10, w11), restated with its
    float products, the short saturation and the sum fix that reads past the 2x2 block (W6)."""
    scale = F32(1.0 / INTER_TAB_SIZE)
    tab1 = np.zeros((INTER_TAB_SIZE, 2), F32)
    for i in range(INTER_TAB_SIZE):            # initInterTab1D -> interpolateLinear(i * scale)
        x = F32(i) * scale
        tab1[i] = (F32(1.0) - x, x)
    ksize = 2
    itab = np.zeros(INTER_TAB_SIZE * INTER_TAB_SIZE * 4 + 8, np.int64)   # the static table, zero before it is filled
    for i in range(INTER_TAB_SIZE):
        for j in range(INTER_TAB_SIZE):
            base = (i * INTER_TAB_SIZE + j) * 4
            isum = 0
            for k1 in range(ksize):
                vy = tab1[i, k1]
                for k2 in range(ksize):
                    v = F32(vy * tab1[j, k2])
                    itab[base + k1 * ksize + k2] = _saturate_short(F32(v * F32(INTER_REMAP_COEF_SCALE)))
                    isum += int(itab[base + k1 * ksize + k2])
            if isum != INTER_REMAP_COEF_SCALE:
                diff = isum - INTER_REMAP_COEF_SCALE
                ksize2 = ksize // 2
                Mk1 = Mk2 = mk1 = mk2 = ksize2
                for k1 in range(ksize2, ksize2 + 2):
                    for k2 in range(ksize2, ksize2 + 2):
                        if itab[base + k1 * ksize + k2] < itab[base + mk1 * ksize + mk2]:
                            mk1, mk2 = k1, k2
                        elif itab[base + k1 * ksize + k2] > itab[base + Mk1 * ksize + Mk2]:
                            Mk1, Mk2 = k1, k2
                if diff < 0:
                    itab[base + Mk1 * ksize + Mk2] -= diff
                else:
                    itab[base + mk1 * ksize + mk2] -= diff
    return itab[:INTER_TAB_SIZE * INTER_TAB_SIZE * 4].reshape(-1, 4).astype(np.int16)


def closed_form_tab():
    """(32-ty)(32-tx)*32, (32-ty)*tx*32, ty*(32-tx)*32, ty*tx*32 for entry ty*32 + tx (int64: 32768 does not fit a short)"""
    a = np.arange(INTER_TAB_SIZE * INTER_TAB_SIZE)
    ty, tx = a // INTER_TAB_SIZE, a % INTER_TAB_SIZE
    return np.stack([(32 - ty) * (32 - tx) * 32, (32 - ty) * tx * 32, ty * (32 - tx) * 32, ty * tx * 32], 1).astype(np.int64)


_TAB = None


def tab():
    global _TAB
    if _TAB is None:
        _TAB = inter_tab_linear().astype(np.int64)
    return _TAB


# ---- the remap --------------------------------------------------------------------------------------------------------------
def border_case(sx, sy, w, h):
    """0: all four neighbours inside, 1: wholly outside (border value), 2: some neighbours outside"""
    inl = ((sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1))
    out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    return np.where(inl, 0, np.where(out, 1, 2))


def remap_bilinear(src, sx, sy, alpha):
    """remapBilinear for CV_8UC1, BORDER_CONSTANT 0: every pixel from its cell (sx, sy) and table entry alpha."""
    src = np.asarray(src, np.uint8)
    h, w = src.shape
    wt = tab()[alpha]
    case = border_case(sx, sy, w, h)

    def at(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)

    v0, v1, v2, v3 = at(sx, sy), at(sx + 1, sy), at(sx, sy + 1), at(sx + 1, sy + 1)
    val = (v0 * wt[..., 0] + v1 * wt[..., 1] + v2 * wt[..., 2] + v3 * wt[..., 3] + (1 << 14)) >> 15
    val = np.clip(val, 0, 255)   # FixedPtCast's saturate_cast<uchar> (never active: the weights are >= 0 and sum to 32768)
    return np.where(case == 1, 0, val).astype(np.uint8)


def warp(gray, H, split=True):
    """cv::warpPerspective(gray, dst, H, gray.size()) with the defaults"""
    gray = np.asarray(gray, np.uint8)
    assert gray.size > 0, "warpPerspective: empty frame"
    h, w = gray.shape
    sx, sy, alpha = coordinates(invert3(as_matrix(H)), w, h, split)[:3]
    return remap_bilinear(gray, sx, sy, alpha)


def compute_mask_homo(flow, gray, H, th):
    """Flow::ComputeMask(GrayImg, Homo, mask, th) on a flow_oracle.Flow: the warped frame goes through the plain ComputeMask, so
    the state becomes the warped frame's half-size image.  flow.taps['warp'] holds the warped frame."""
    dest = warp(gray, H)
    mask = flow.compute_mask(dest, th)
    flow.taps["warp"] = dest
    return mask

