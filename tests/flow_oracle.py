"""CPU oracle of FlowSLAM::Flow::ComputeMask (perfect/src/Flow.cc:15-52) and of the masked-Frame keypoint rule
(perfect/src/Frame.cc:360-377), in numpy.

It restates OpenCV 3.2's generic C++ code paths (IPP, OpenCL, HAL and the SSE loops off) of every function ComputeMask
calls: pyrDown (u8), calcOpticalFlowFarneback (modules/video/src/optflowgf.cpp, flags 0: the box-filter update),
pyrUp (float, two channels), getStructuringElement, erode and dilate.  float32 and float64 are used exactly where the
C++ uses float and double, one operation at a time, following C++'s usual arithmetic conversions: `float + float` stays
float even when the result goes into a double accumulator.  No fused multiply-add anywhere.

UNPINNED.  OpenCV is not available to this project, so the oracle has never been compared with a real OpenCV build.
Two independent checks keep it honest (tests/test_flow_oracle.py): the integer stages (pyrDown, erode, dilate) equal
scipy.ndimage bit for bit, and the restated Farneback recovers known translations and affine motions of textured frames.
The points below rest on knowledge of the OpenCV 3.2 sources and could not be confirmed here:

  U1  resize INTER_LINEAR at an exact 2x downscale takes the INTER_AREA fast path; its scalar loop sums
      ((a + b) + c) + d (then * 0.25f).  The SSE2 loop of 3.2 (ResizeAreaFastVec_SIMD_32f) sums (a + b) + (c + d) for
      four output pixels at a time; a build with SSE2 on would differ in the last bit of some level-1 pixels.
  U2  The row filter of GaussianBlur for 3 taps is SymmRowSmallFilter (S0*k0 + (S-1 + S1)*k1); for 9 and 19 taps it is
      the plain RowFilter, taps summed left to right.  The column filter is the symmetric form k0*S0 + sum k_i*(S_i + S_-i)
      for every size (SymmColumnSmallFilter for 3 taps gives the same bits: float + and * commute).
  U3  pyrUp's vertical sum is (row0 + row1*6) + row2; its SSE loop (PyrUpVec_32f) may associate differently.
  U4  G.inv(DECOMP_CHOLESKY) in FarnebackPrepareGaussian is hal::Cholesky64f (CholImpl): L stores 1/sqrt of the
      diagonal, then forward and back substitution on the identity.
  U5  `flow *= 1./pyr_scale` is convertTo(flow, -1, 2.0): float x*2.0f + 0.0f.
  U6  cv::resize returns a plain copy when the size does not change (level 0 of the pyramid).
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA = 0.5, 3, 15, 3, 5, 1.2
MIN_SIZE = 32
ELLIPSE_HALF = (0, 4, 6, 7, 8, 9, 9, 10, 10, 10, 10, 10, 10, 10, 9, 9, 8, 7, 6, 4, 0)


def _refl101(i, n):
    """borderInterpolate(i, n, BORDER_REFLECT_101) for |overhang| < n."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def cv_round(v):
    """cvRound: round half to even (lrint in the default rounding mode)."""
    return int(round(v))


# --------------------------------------------------------------------------------------------------------------------
def pyr_down_u8(img):
    """cv::pyrDown(src, dst, Size(w/2, h/2)) on CV_8U (pyrDown_<FixPtCast<uchar, 8>>): the 5x5 [1 4 6 4 1]^2 kernel at
    even positions, BORDER_REFLECT_101, (sum + 128) >> 8.  Exact integer work."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    dh, dw = h // 2, w // 2
    k = np.array([1, 4, 6, 4, 1], np.int64)
    xs = _refl101(2 * np.arange(dw)[:, None] + np.arange(-2, 3)[None, :], w)
    ys = _refl101(2 * np.arange(dh)[:, None] + np.arange(-2, 3)[None, :], h)
    src = img.astype(np.int64)
    rows = sum(k[j] * src[:, xs[:, j]] for j in range(5))
    out = sum(k[i] * rows[ys[:, i], :] for i in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def level_plan(w, h, pyr_scale=PYR_SCALE, levels=LEVELS):
    """The level loop of calcOpticalFlowFarneback: levels are cut where a side would fall under min_size = 32.
    Returns [(width, height, sigma, ksize)] from the coarsest level to level 0."""
    scale = 1.0
    k = 0
    while k < levels:
        scale *= pyr_scale
        if w * scale < MIN_SIZE or h * scale < MIN_SIZE:
            break
        k += 1
    plan = []
    for lv in range(k, -1, -1):
        scale = 1.0
        for _ in range(lv):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        ksize = max(cv_round(sigma * 5) | 1, 3)
        plan.append((cv_round(w * scale), cv_round(h * scale), sigma, ksize))
    return plan


def gaussian_kernel(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_32F): the fixed tables for odd n <= 7 at sigma <= 0, otherwise exp; taps in
    float, their sum in double, normalised as (float)(cf[i]*sum)."""
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    fixed = small[n] if (n % 2 == 1 and n <= 7 and sigma <= 0) else None
    sigma_x = sigma if sigma > 0 else ((n - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (sigma_x * sigma_x)
    cf, s = [], 0.0
    for i in range(n):
        x = i - (n - 1) * 0.5
        t = float(F32(fixed[i])) if fixed else math.exp(scale2x * x * x)
        cf.append(F32(t))
        s += float(cf[i])
    s = 1.0 / s
    return np.array([F32(float(c) * s) for c in cf], F32)


def gaussian_blur_f32(img, ksize, sigma):
    """cv::GaussianBlur on CV_32F with BORDER_REFLECT_101 (sepFilter2D): the row filter (U2), then the symmetric column
    filter k0*S0 + sum_i k_i*(S_i + S_-i), all in float."""
    k = gaussian_kernel(ksize, sigma)
    r = ksize // 2
    h, w = img.shape
    src = np.asarray(img, F32)
    xs = _refl101(np.arange(w)[:, None] + np.arange(-r, r + 1)[None, :], w)
    if ksize == 3:
        t = src[:, xs[:, 1]] * k[1] + (src[:, xs[:, 0]] + src[:, xs[:, 2]]) * k[2]
    else:
        t = src[:, xs[:, 0]] * k[0]
        for j in range(1, ksize):
            t = t + src[:, xs[:, j]] * k[j]
    ys = _refl101(np.arange(h)[:, None] + np.arange(-r, r + 1)[None, :], h)
    out = t[ys[:, r], :] * k[r]
    for i in range(1, r + 1):
        out = out + k[r + i] * (t[ys[:, r + i], :] + t[ys[:, r - i], :])
    return out.astype(F32)


def _linear_taps(dsize, ssize):
    """The x (or y) table of cv::resize INTER_LINEAR: fx = (float)((d + 0.5)*scale - 0.5), sx = cvFloor(fx),
    fx -= sx; on the x axis sx < 0 clamps to (0, fx = 0) and sx >= ssize-1 to (ssize-1, fx = 0).  Also returns
    xmax, the first d whose right tap is outside (from there on the row is S[sx]*1)."""
    scale = 1.0 / (float(dsize) / float(ssize))
    d = np.arange(dsize, dtype=F64)
    f = ((d + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    return s, f


def resize_linear(src, dw, dh):
    """cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) on CV_32F with 1 or 2 channels, generic path.
    Same size: a copy (U6).  Exact 2x downscale: the INTER_AREA fast path ((a+b)+c)+d, * 0.25f (U1).  Otherwise
    HResizeLinear (S[sx]*a0 + S[sx+1]*a1; past xmax S[sx]*1) and VResizeLinear (S0*b0 + S1*b1, rows clipped), float."""
    src = np.asarray(src, F32)
    squeeze = src.ndim == 2
    if squeeze:
        src = src[:, :, None]
    sh, sw = src.shape[:2]
    if (sw, sh) == (dw, dh):
        out = src.copy()
    elif sw == 2 * dw and sh == 2 * dh:
        a, b = src[0::2, 0::2], src[0::2, 1::2]
        c, d = src[1::2, 0::2], src[1::2, 1::2]
        out = (F32(0) + (((a + b) + c) + d)) * F32(0.25)
    else:
        sx, fx = _linear_taps(dw, sw)
        xmax = dw
        hit = np.nonzero(sx + 1 >= sw)[0]
        if len(hit):
            xmax = int(hit[0])
        left = sx < 0
        fx = np.where(left, F32(0), fx).astype(F32)
        sx = np.where(left, 0, sx)
        right = sx >= sw - 1
        fx = np.where(right, F32(0), fx).astype(F32)
        sx = np.where(right, sw - 1, sx)
        a0, a1 = (F32(1) - fx).astype(F32), fx
        sx1 = np.minimum(sx + 1, sw - 1)
        hr = src[:, sx, :] * a0[None, :, None] + src[:, sx1, :] * a1[None, :, None]
        hr[:, xmax:, :] = src[:, sx[xmax:], :] * F32(1)
        sy, fy = _linear_taps(dh, sh)
        b0, b1 = (F32(1) - fy).astype(F32), fy
        r0 = hr[np.clip(sy, 0, sh - 1)]
        r1 = hr[np.clip(sy + 1, 0, sh - 1)]
        out = r0 * b0[:, None, None] + r1 * b1[:, None, None]
    out = out.astype(F32)
    return out[:, :, 0] if squeeze else out


# --------------------------------------------------------------------------------------------------------------------
def _cholesky_inverse(G):
    """G.inv(DECOMP_CHOLESKY) = hal::Cholesky64f(A, n, identity) (U4), restated loop for loop."""
    m = 6
    L = [list(map(float, row)) for row in G]
    b = [[1.0 if i == j else 0.0 for j in range(m)] for i in range(m)]
    for i in range(m):
        for j in range(i):
            s = L[i][j]
            for k in range(j):
                s -= L[i][k] * L[j][k]
            L[i][j] = s * L[j][j]
        s = L[i][i]
        for k in range(i):
            t = L[i][k]
            s -= t * t
        assert s >= np.finfo(F64).eps
        L[i][i] = 1.0 / math.sqrt(s)
    for i in range(m):
        for j in range(m):
            s = b[i][j]
            for k in range(i):
                s -= L[i][k] * b[k][j]
            b[i][j] = s * L[i][i]
    for i in range(m - 1, -1, -1):
        for j in range(m):
            s = b[i][j]
            for k in range(m - 1, i, -1):
                s -= L[k][i] * b[k][j]
            b[i][j] = s * L[i][i]
    return b


def prepare_gaussian(n=POLY_N, sigma=POLY_SIGMA):
    """FarnebackPrepareGaussian: g, xg, xxg (float, index -n..n) and ig11, ig03, ig33, ig55 from the Cholesky inverse of
    the 6x6 double matrix G.  Returns (g, xg, xxg, (ig11, ig03, ig33, ig55)) with the arrays indexed 0..2n."""
    if sigma < np.finfo(F32).eps:
        sigma = n * 0.3
    g = {}
    s = 0.0
    for x in range(-n, n + 1):
        g[x] = F32(math.exp(-x * x / (2 * sigma * sigma)))
        s += float(g[x])
    s = 1.0 / s
    xg, xxg = {}, {}
    for x in range(-n, n + 1):
        g[x] = F32(float(g[x]) * s)
        xg[x] = F32(x) * g[x]
        xxg[x] = F32(x * x) * g[x]
    G = [[0.0] * 6 for _ in range(6)]
    for y in range(-n, n + 1):
        for x in range(-n, n + 1):
            gg = g[y] * g[x]
            G[0][0] += float(gg)
            G[1][1] += float(gg * F32(x) * F32(x))
            G[3][3] += float(gg * F32(x) * F32(x) * F32(x) * F32(x))
            G[5][5] += float(gg * F32(x) * F32(x) * F32(y) * F32(y))
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1]
    G[4][4] = G[3][3]
    G[3][4] = G[4][3] = G[5][5]
    inv = _cholesky_inverse(G)
    arr = lambda d: np.array([d[x] for x in range(-n, n + 1)], F32)  # noqa: E731
    return arr(g), arr(xg), arr(xxg), (inv[1][1], inv[0][3], inv[3][3], inv[5][5])


def poly_exp(img, n=POLY_N, sigma=POLY_SIGMA):
    """FarnebackPolyExp: the vertical pass in float (rows clamped), the horizontal pass into double sums b1..b6 with the
    pixel row replicated at both ends.  Returns R [h, w, 5] float32 in OpenCV's channel order
    (b3*ig11, b2*ig11, b1*ig03 + b5*ig33, b1*ig03 + b4*ig33, b6*ig55)."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = prepare_gaussian(n, sigma)
    src = np.asarray(img, F32)
    h, w = src.shape
    r0 = src * g[n]
    r1 = np.zeros_like(src)
    r2 = np.zeros_like(src)
    for k in range(1, n + 1):
        s0 = src[np.maximum(np.arange(h) - k, 0)]
        s1 = src[np.minimum(np.arange(h) + k, h - 1)]
        p = s0 + s1
        r0 = r0 + g[n + k] * p
        r1 = r1 + xg[n + k] * (s1 - s0)
        r2 = r2 + xxg[n + k] * p
    xi = lambda k: np.clip(np.arange(w) + k, 0, w - 1)  # noqa: E731
    b1 = (r0 * g[n]).astype(F64)
    b2 = np.zeros((h, w), F64)
    b3 = (r1 * g[n]).astype(F64)
    b4 = np.zeros((h, w), F64)
    b5 = (r2 * g[n]).astype(F64)
    b6 = np.zeros((h, w), F64)
    for k in range(1, n + 1):
        p, m_ = xi(k), xi(-k)
        tg = (r0[:, p] + r0[:, m_]).astype(F64)
        g0 = F64(g[n + k])
        b1 = b1 + tg * g0
        b4 = b4 + tg * F64(xxg[n + k])
        b2 = b2 + ((r0[:, p] - r0[:, m_]) * xg[n + k]).astype(F64)
        b3 = b3 + ((r1[:, p] + r1[:, m_]) * g[n + k]).astype(F64)
        b6 = b6 + ((r1[:, p] - r1[:, m_]) * xg[n + k]).astype(F64)
        b5 = b5 + ((r2[:, p] + r2[:, m_]) * g[n + k]).astype(F64)
    R = np.empty((h, w, 5), F32)
    R[:, :, 1] = (b2 * ig11).astype(F32)
    R[:, :, 0] = (b3 * ig11).astype(F32)
    R[:, :, 3] = (b1 * ig03 + b4 * ig33).astype(F32)
    R[:, :, 2] = (b1 * ig03 + b5 * ig33).astype(F32)
    R[:, :, 4] = (b6 * ig55).astype(F32)
    return R


_BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], F32)


def update_matrices(R0, R1, flow):
    """FarnebackUpdateMatrices over all rows: R1 fetched bilinearly at (x + dx, y + dy) when (unsigned)x1 < w-1 and
    (unsigned)y1 < h-1, the 5-entry border weight table on the 5-pixel frame.  Returns M [h, w, 5] float32."""
    h, w = flow.shape[:2]
    dx, dy = flow[:, :, 0], flow[:, :, 1]
    X = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    Y = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    fx = X + dx
    fy = Y + dy
    with np.errstate(invalid="ignore"):
        x1 = np.floor(fx)
        y1 = np.floor(fy)
        inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    x1i = np.where(inside, x1, 0).astype(np.int64)
    y1i = np.where(inside, y1, 0).astype(np.int64)
    fx = (fx - x1i.astype(F32)).astype(F32)
    fy = (fy - y1i.astype(F32)).astype(F32)
    one = F32(1)
    a00, a01 = (one - fx) * (one - fy), fx * (one - fy)
    a10, a11 = (one - fx) * fy, fx * fy
    p00, p01, p10, p11 = R1[y1i, x1i], R1[y1i, x1i + 1], R1[y1i + 1, x1i], R1[y1i + 1, x1i + 1]
    r = [((a00 * p00[:, :, c] + a01 * p01[:, :, c]) + a10 * p10[:, :, c]) + a11 * p11[:, :, c] for c in range(5)]
    r2, r3, r4, r5, r6 = r
    half, quarter = F32(0.5), F32(0.25)
    r4 = np.where(inside, (R0[:, :, 2] + r4) * half, R0[:, :, 2])
    r5 = np.where(inside, (R0[:, :, 3] + r5) * half, R0[:, :, 3])
    r6 = np.where(inside, (R0[:, :, 4] + r6) * quarter, R0[:, :, 4] * half)
    r2 = np.where(inside, r2, F32(0))
    r3 = np.where(inside, r3, F32(0))
    r2 = (R0[:, :, 0] - r2) * half
    r3 = (R0[:, :, 1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)
    xs, ys = np.arange(w), np.arange(h)
    u32 = lambda v: np.asarray(v).astype(np.int64) & 0xFFFFFFFF  # noqa: E731
    xb = u32(xs - 5) >= u32(w - 10)
    yb = u32(ys - 5) >= u32(h - 10)
    bx0 = np.where(xs < 5, _BORDER[np.minimum(xs, 4)], one)
    bx1 = np.where(xs >= w - 5, _BORDER[np.clip(w - xs - 1, 0, 4)], one)
    by0 = np.where(ys < 5, _BORDER[np.minimum(ys, 4)], one)
    by1 = np.where(ys >= h - 5, _BORDER[np.clip(h - ys - 1, 0, 4)], one)
    scale = ((bx0[None, :] * bx1[None, :]) * by0[:, None]) * by1[:, None]
    sel = xb[None, :] | yb[:, None]
    r2, r3, r4, r5, r6 = [np.where(sel, v * scale, v).astype(F32) for v in (r2, r3, r4, r5, r6)]
    M = np.empty((h, w, 5), F32)
    M[:, :, 0] = r4 * r4 + r6 * r6
    M[:, :, 1] = (r4 + r5) * r6
    M[:, :, 2] = r5 * r5 + r6 * r6
    M[:, :, 3] = r4 * r2 + r6 * r3
    M[:, :, 4] = r6 * r2 + r5 * r3
    return M


def update_flow_blur(M, block=WINSIZE):
    """FarnebackUpdateFlow_Blur's blur and solve: the column sums vsum (double) are updated row by row, each row's sums
    run across the columns, borders replicated, the first row / column entering (m+2) times.
      idet = 1/(g11*g22 - g12^2 + 1e-3);  flow = ((g11*h2 - g12*h1)*idet, (g22*h1 - g12*h2)*idet), cast to float.
    The reference refreshes M from the new flow lazily, block_size rows behind the row it solves, inside this loop.
    Row y of M depends only on row y of the flow, and the rows refreshed after solving row y are < y - block_size + 1,
    while every later row y' > y reads (adds or subtracts) only rows >= y' - m - 1 >= y - m > y - block_size: a refreshed
    row is never read again in the same pass, and the last solved row refreshes all the rest.  So the lazy refresh equals
    "blur with the old M, then recompute M from the whole new flow" (farneback() does exactly that)."""
    h, w = M.shape[:2]
    m = block // 2
    Mf = M.reshape(h, w * 5)
    vsum = (Mf[0] * F32(m + 2)).astype(F64)
    for y in range(1, m):
        vsum = vsum + Mf[min(y, h - 1)].astype(F64)
    V = np.empty((h, w * 5), F64)
    for y in range(h):
        vsum = vsum + (Mf[min(y + m, h - 1)] - Mf[max(y - m - 1, 0)]).astype(F64)
        V[y] = vsum
    V = V.reshape(h, w, 5)
    P = np.concatenate([np.repeat(V[:, :1], m + 1, 1), V, np.repeat(V[:, -1:], m + 1, 1)], 1)  # pixel x at P[:, x + m + 1]
    g = P[:, m + 1] * F64(m + 2)
    for x in range(1, m):
        g = g + P[:, x + m + 1]
    scale = 1.0 / (block * block)
    flow = np.empty((h, w, 2), F32)
    for x in range(w):
        g = g + (P[:, x + 2 * m + 1] - P[:, x])
        gs = g * scale
        g11, g12, g22, h1, h2 = (gs[:, c] for c in range(5))
        idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
        flow[:, x, 0] = ((g11 * h2 - g12 * h1) * idet).astype(F32)
        flow[:, x, 1] = ((g22 * h1 - g12 * h2) * idet).astype(F32)
    return flow


def farneback(prev, nxt, taps=None):
    """calcOpticalFlowFarneback(prev, next, flow, 0.5, 3, 15, 3, 5, 1.2, 0) on two u8 images.  For every level, coarsest
    first: the WHOLE image is blurred with sigma = (1/scale - 1)/2, resized to the level, expanded (PolyExp); the flow is
    the previous level's, resized (INTER_LINEAR) and scaled by 1/pyr_scale, or zeros; then M, and 3 box-filter updates
    with M refreshed after each but the last.  taps (a dict) receives 'flow_levels' (coarsest first)."""
    h, w = prev.shape
    plan = level_plan(w, h)
    flow = None
    levels = []
    for (lw, lh, sigma, ksize) in plan:
        Rs = []
        for img in (prev, nxt):
            I = resize_linear(gaussian_blur_f32(img.astype(F32), ksize, sigma), lw, lh)
            Rs.append(poly_exp(I))
        if flow is None:
            flow = np.zeros((lh, lw, 2), F32)
        else:
            flow = (resize_linear(flow, lw, lh) * F32(2.0) + F32(0.0)).astype(F32)
        M = update_matrices(Rs[0], Rs[1], flow)
        for it in range(ITERATIONS):
            flow = update_flow_blur(M)
            if it < ITERATIONS - 1:
                M = update_matrices(Rs[0], Rs[1], flow)
        levels.append(flow)
    if taps is not None:
        taps["flow_levels"] = levels
    return flow


def pyr_up_f32(src):
    """cv::pyrUp(src, dst, Size(2w, 2h)) on CV_32FC2 (pyrUp_<FltCast<float, 6>>): per row, left edge
    t0 = s0*6 + s1*2, interior t0 = (s[x-1] + s[x]*6) + s[x+1], right edge t0 = s[w-2] + s[w-1]*7, t1 = s[w-1]*8,
    odd outputs t1 = (s[x] + s[x+1])*4; rows -1 -> 1 and h -> h-1; dst0 = (row0 + row1*6) + row2,
    dst1 = (row1 + row2)*4, both * (1/64)."""
    src = np.asarray(src, F32)
    h, w = src.shape[:2]
    s = src
    t = np.empty((h, 2 * w, 2), F32)
    six, four, seven, eight = F32(6), F32(4), F32(7), F32(8)
    t[:, 0] = s[:, 0] * six + s[:, 1] * F32(2)
    t[:, 1] = (s[:, 0] + s[:, 1]) * four
    t[:, 2:2 * w - 2:2] = (s[:, :-2] + s[:, 1:-1] * six) + s[:, 2:]
    t[:, 3:2 * w - 2:2] = (s[:, 1:-1] + s[:, 2:]) * four
    t[:, 2 * w - 2] = s[:, w - 2] + s[:, w - 1] * seven
    t[:, 2 * w - 1] = s[:, w - 1] * eight
    ym = np.r_[1, np.arange(h - 1)]
    yp = np.r_[np.arange(1, h), h - 1]
    row0, row1, row2 = t[ym], t, t[yp]
    out = np.empty((2 * h, 2 * w, 2), F32)
    sc = F32(1.0 / 64)
    out[0::2] = ((row0 + row1 * six) + row2) * sc
    out[1::2] = ((row1 + row2) * four) * sc
    return out


def ellipse21():
    """getStructuringElement(MORPH_ELLIPSE, Size(21, 21), Point(10, 10)): row dy spans c +- cvRound(c*sqrt((r^2-dy^2)/r^2))."""
    r = c = 10
    inv_r2 = 1.0 / (r * r)
    el = np.zeros((21, 21), np.uint8)
    for i in range(21):
        dy = i - r
        dx = cv_round(c * math.sqrt((r * r - dy * dy) * inv_r2))
        el[i, max(c - dx, 0):min(c + dx + 1, 21)] = 1
    return el


def _morph(mask, op):
    """cv::erode / cv::dilate with the 21x21 ellipse, anchor (10, 10), default border: outside the image is the
    type's maximum for erode (counts as 1) and its minimum for dilate (0).  Row by row of the ellipse: a min / max over
    the row's span, then over the 21 rows."""
    h, w = mask.shape
    border = 255 if op == "erode" else 0
    red = np.minimum if op == "erode" else np.maximum
    p = np.full((h + 20, w + 20), border, np.uint8)
    p[10:10 + h, 10:10 + w] = mask
    spans = {}
    for hw in sorted(set(ELLIPSE_HALF)):
        acc = p[:, 10 - hw:10 - hw + w]
        for d in range(-hw + 1, hw + 1):
            acc = red(acc, p[:, 10 + d:10 + d + w])
        spans[hw] = acc
    out = None
    for i, hw in enumerate(ELLIPSE_HALF):
        v = spans[hw][i:i + h]
        out = v if out is None else red(out, v)
    return out.astype(np.uint8)


def erode(mask):
    return _morph(mask, "erode")


def dilate(mask):
    return _morph(mask, "dilate")


class Flow:
    """FlowSLAM::Flow: ComputeMask(GrayImg, mask, th), with the previous half-size frame as state.  taps (after a call):
    'half', 'flow_levels', 'flow', 'flow2', 'mask_pre', 'mask'."""

    def __init__(self):
        self.last = None
        self.taps = {}

    def reset(self):
        self.last = None

    def compute_mask(self, gray, th):
        gray = np.asarray(gray, np.uint8)
        h, w = gray.shape
        th = F32(th)
        if th < 40.0:
            th = F32(40.0)
        mask = np.ones((h, w), np.uint8)
        cur = pyr_down_u8(gray)
        self.taps = {"half": cur}
        if self.last is not None:
            assert self.last.shape == cur.shape, "cv::calcOpticalFlowFarneback: size mismatch"
            flow = farneback(self.last, cur, self.taps)
            flow2 = pyr_up_f32(flow)
            fh, fw = flow2.shape[:2]
            t = flow2[:, :, 0] * flow2[:, :, 0] + flow2[:, :, 1] * flow2[:, :, 1]
            with np.errstate(invalid="ignore"):
                sub = mask[:fh, :fw]
                sub[~(t < th)] = 0
            self.taps.update(flow=flow, flow2=flow2, mask_pre=mask.copy())
            mask = dilate(erode(erode(mask)))
        self.taps["mask"] = mask
        self.last = cur
        return mask


def mask_rule(mask, kps, desc):
    """perfect/src/Frame.cc:360-377: when sum(mask) > rows*cols*0.65, keep the keypoints with mask[int(y)][int(x)] == 1
    (descriptors follow, order kept); otherwise keep all.  The reference reads the mask unchecked, so outside the plane it
    has no defined result; the project's rule: a keypoint is in the plane iff x > -1 and x < w and y > -1 and y < h, decided in
    float before the truncation (a NaN is out), and a keypoint outside the plane is dropped."""
    h, w = mask.shape
    if float(mask.astype(np.float64).sum()) > h * w * 0.65:
        x, y = kps["x"].astype(F32), kps["y"].astype(F32)
        with np.errstate(invalid="ignore"):
            inside = (x > F32(-1)) & (x < F32(w)) & (y > F32(-1)) & (y < F32(h))
        xi = np.where(inside, x, F32(0)).astype(np.int32)   # C's (int): towards zero
        yi = np.where(inside, y, F32(0)).astype(np.int32)
        keep = inside & (mask[yi, xi] == 1)
        return kps[keep], desc[keep]
    return kps, desc
