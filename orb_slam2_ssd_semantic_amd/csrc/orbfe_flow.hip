// orbfe_flow.hip -- FlowSLAM::Flow::ComputeMask (perfect/src/Flow.cc:15-52) and the masked-Frame keypoint rule
// (perfect/src/Frame.cc:360-377) on the GPU.  Every kernel restates one stage of tests/flow_oracle.py (OpenCV 3.2's
// generic C++ paths) operation for operation, float where the C++ uses float, double where it uses double, no FMA
// (-ffp-contract=off), so the outputs are bit-exact against it.  Layout and reuse: DESIGN.md "Optical-flow mask".
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <new>

#include "orbfe_common.h"
#include "orbfe_host.h"

namespace {

constexpr int FL_MAX_LEVELS = 4;   // levels = 3 -> at most 4 pyramid levels
constexpr int FL_MAX_TAPS = 19;    // GaussianBlur ksize at level 3 (sigma 3.5)
constexpr int FL_CHUNK = 64;       // pairs per internal pass (bounds the scratch: about 11 MB per 640x480 pair)
constexpr int FL_POLY_N = 5;
constexpr int FL_WIN = 15;         // winsize
constexpr int FL_ITERS = 3;
constexpr int FL_MIN_SIDE = 16;

struct FlowLevel {
    int w, h, ksize;
    double sigma;
    float taps[FL_MAX_TAPS];
    size_t roff;   // offset (floats) of this level inside a slot's PolyExp block
    size_t foff;   // offset (floats) of this level inside a pair's flow block
};

struct FlowPlan {
    int n;                          // levels; lv[0] = finest (the half-size image), lv[n-1] = coarsest
    FlowLevel lv[FL_MAX_LEVELS];
    size_t rtotal, ftotal;          // floats per slot (PolyExp) / per pair (flows)
};

struct PolyConst {
    float g[2 * FL_POLY_N + 1], xg[2 * FL_POLY_N + 1], xxg[2 * FL_POLY_N + 1];
    double ig11, ig03, ig33, ig55;
};

struct BlurTaps { float k[FL_MAX_TAPS]; };

// ---- host constants: the oracle's operation order, libm exp / sqrt ------------------------------------------------------
static int cv_round(double v) { return (int)lrint(v); }

// cv::getGaussianKernel(n, sigma, CV_32F)
static void gaussian_kernel(int n, double sigma, float *out)
{
    static const float small_tab[4][7] = {{1.f},
                                          {0.25f, 0.5f, 0.25f},
                                          {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                          {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    const float *fixed = (n % 2 == 1 && n <= 7 && sigma <= 0) ? small_tab[n >> 1] : nullptr;
    double sigma_x = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    double scale2x = -0.5 / (sigma_x * sigma_x);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        double x = i - (n - 1) * 0.5;
        double t = fixed ? (double)fixed[i] : exp(scale2x * x * x);
        out[i] = (float)t;
        sum += out[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) out[i] = (float)(out[i] * sum);
}

// the level loop of calcOpticalFlowFarneback on a w2 x h2 image (pyr_scale 0.5, levels 3, min_size 32)
static void make_plan(int w2, int h2, FlowPlan &p)
{
    const double pyr_scale = 0.5;
    const int levels = 3, min_size = 32;
    double scale = 1;
    int k;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (w2 * scale < min_size || h2 * scale < min_size) break;
    }
    p.n = k + 1;
    size_t ro = 0, fo = 0;
    for (int l = 0; l < p.n; l++) {
        scale = 1;
        for (int i = 0; i < l; i++) scale *= pyr_scale;
        FlowLevel &L = p.lv[l];
        L.sigma = (1. / scale - 1) * 0.5;
        L.ksize = std::max(cv_round(L.sigma * 5) | 1, 3);
        L.w = cv_round(w2 * scale);
        L.h = cv_round(h2 * scale);
        memset(L.taps, 0, sizeof(L.taps));
        gaussian_kernel(L.ksize, L.sigma, L.taps);
        L.roff = ro;
        L.foff = fo;
        ro += (size_t)L.w * L.h * 5;
        fo += (size_t)L.w * L.h * 2;
    }
    p.rtotal = ro;
    p.ftotal = fo;
}

// hal::Cholesky64f(A, 6, identity): G.inv(DECOMP_CHOLESKY)
static bool cholesky_inverse6(double A[6][6], double b[6][6])
{
    const int m = 6;
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) b[i][j] = i == j ? 1. : 0.;
    double s;
    for (int i = 0; i < m; i++) {
        int j;
        for (j = 0; j < i; j++) {
            s = A[i][j];
            for (int k = 0; k < j; k++) s -= A[i][k] * A[j][k];
            A[i][j] = s * A[j][j];
        }
        s = A[i][i];
        for (int k = 0; k < j; k++) {
            double t = A[i][k];
            s -= t * t;
        }
        if (s < 2.220446049250313e-16) return false;
        A[i][i] = 1. / sqrt(s);
    }
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) {
            s = b[i][j];
            for (int k = 0; k < i; k++) s -= A[i][k] * b[k][j];
            b[i][j] = s * A[i][i];
        }
    for (int i = m - 1; i >= 0; i--)
        for (int j = 0; j < m; j++) {
            s = b[i][j];
            for (int k = m - 1; k > i; k--) s -= A[k][i] * b[k][j];
            b[i][j] = s * A[i][i];
        }
    return true;
}

// FarnebackPrepareGaussian(5, 1.2)
static void prepare_gaussian(PolyConst &c)
{
    const int n = FL_POLY_N;
    double sigma = 1.2;
    float *g = c.g + n, *xg = c.xg + n, *xxg = c.xxg + n;
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)exp(-x * x / (2 * sigma * sigma));
        s += g[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        xg[x] = (float)(x * g[x]);
        xxg[x] = (float)(x * x * g[x]);
    }
    double G[6][6] = {};
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += g[y] * g[x];
            G[1][1] += g[y] * g[x] * x * x;
            G[3][3] += g[y] * g[x] * x * x * x * x;
            G[5][5] += g[y] * g[x] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    double inv[6][6];
    cholesky_inverse6(G, inv);
    c.ig11 = inv[1][1];
    c.ig03 = inv[0][3];
    c.ig33 = inv[3][3];
    c.ig55 = inv[5][5];
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int refl101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// pyrDown (u8): the 5x5 [1 4 6 4 1]^2 sum, BORDER_REFLECT_101, (s + 128) >> 8, at half-size pixel (x, y) of frame s
__device__ __forceinline__ uint8_t pyrdown_at(const uint8_t *s, int stride, int w, int h, int x, int y)
{
    const int k[5] = {1, 4, 6, 4, 1};
    int acc = 0;
    for (int a = 0; a < 5; a++) {
        const uint8_t *row = s + (size_t)refl101(2 * y + a - 2, h) * stride;
        int r = 0;
        for (int b = 0; b < 5; b++) r += k[b] * row[refl101(2 * x + b - 2, w)];
        acc += k[a] * r;
    }
    return (uint8_t)((acc + 128) >> 8);
}

// Frame b of the call -> slot b + slot0.
__global__ void k_flow_pyrdown(const uint8_t *src, int stride, size_t fstride, int w, int h, uint8_t *half, int w2, int h2,
                               int slot0)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w2 * h2) return;
    half[(size_t)(slot0 + blockIdx.y) * w2 * h2 + i] = pyrdown_at(src + blockIdx.y * fstride, stride, w, h, i % w2, i / w2);
}

// ---- warpPerspective(src, dst, H, src.size()), INTER_LINEAR, BORDER_CONSTANT 0 (modules/imgproc/src/imgwarp.cpp) ----------
// std::min / std::max as <algorithm> defines them (a NaN argument in second place loses)
__device__ __forceinline__ double std_min(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double std_max(double a, double b) { return (a < b) ? b : a; }

// One thread per frame: warped[b] = (use == NULL || use[b] != 0); inv[b] = invert(H[b]) (DECOMP_LU, n = 3: the closed form of
// lapack.cpp, det3 in its macro order, d = 1./d, each cofactor difference times d; all zeros when det3 == 0).
__global__ void k_flow_homo_prep(const double *H, const int32_t *use, int n, double *inv, int32_t *warped)
{
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    warped[b] = use ? (use[b] != 0) : 1;
    const double *m = H + (size_t)b * 9;
    double *t = inv + (size_t)b * 9;
#define Md(r, c) m[(r) * 3 + (c)]
    double d = Md(0, 0) * (Md(1, 1) * Md(2, 2) - Md(1, 2) * Md(2, 1)) - Md(0, 1) * (Md(1, 0) * Md(2, 2) - Md(1, 2) * Md(2, 0)) +
               Md(0, 2) * (Md(1, 0) * Md(2, 1) - Md(1, 1) * Md(2, 0));
    if (d != 0.) {
        d = 1. / d;
        double r[9];
        r[0] = (Md(1, 1) * Md(2, 2) - Md(1, 2) * Md(2, 1)) * d;
        r[1] = (Md(0, 2) * Md(2, 1) - Md(0, 1) * Md(2, 2)) * d;
        r[2] = (Md(0, 1) * Md(1, 2) - Md(0, 2) * Md(1, 1)) * d;
        r[3] = (Md(1, 2) * Md(2, 0) - Md(1, 0) * Md(2, 2)) * d;
        r[4] = (Md(0, 0) * Md(2, 2) - Md(0, 2) * Md(2, 0)) * d;
        r[5] = (Md(0, 2) * Md(1, 0) - Md(0, 0) * Md(1, 2)) * d;
        r[6] = (Md(1, 0) * Md(2, 1) - Md(1, 1) * Md(2, 0)) * d;
        r[7] = (Md(0, 1) * Md(2, 0) - Md(0, 0) * Md(2, 1)) * d;
        r[8] = (Md(0, 0) * Md(1, 1) - Md(0, 1) * Md(1, 0)) * d;
        for (int k = 0; k < 9; k++) t[k] = r[k];
    } else {
        for (int k = 0; k < 9; k++) t[k] = 0.;
    }
#undef Md
}

// One thread per destination pixel of the warped frames: WarpPerspectiveInvoker's coordinates (blocks of bw0 = min(64, w)
// columns; the block start xb enters X0 / Y0 / W0, the offset x1 = x - xb is added per pixel: the split changes bits), then
// remapBilinear<FixedPtCast<int, uchar, 15>> with the INTER_LINEAR table (32 x 32 sub-pixel steps, weights in 1/32768).
// Frames with warped[b] == 0 are skipped (pyrDown reads the caller's frame for them).
__global__ void k_flow_warp(const uint8_t *src, int stride, size_t fstride, int w, int h, const double *inv, const int32_t *warped,
                            uint8_t *dst)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int b = blockIdx.y;
    if (i >= w * h || !warped[b]) return;
    int x = i % w, y = i / w;
    const double *M = inv + (size_t)b * 9;
    const int bw0 = min(64, w);
    int xb = x - x % bw0, x1 = x - xb;
    double X0 = M[0] * xb + M[1] * y + M[2];
    double Y0 = M[3] * xb + M[4] * y + M[5];
    double W0 = M[6] * xb + M[7] * y + M[8];
    double W = W0 + M[6] * x1;
    W = W != 0. ? 32.0 / W : 0.;
    double fX = std_max((double)INT_MIN, std_min((double)INT_MAX, (X0 + M[0] * x1) * W));
    double fY = std_max((double)INT_MIN, std_min((double)INT_MAX, (Y0 + M[3] * x1) * W));
    int X = (int)rint(fX), Y = (int)rint(fY);   // cvRound: nearest, ties to even
    int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
    int tx = X & 31, ty = Y & 31;
    const uint8_t *S = src + (size_t)b * fstride;
    int out;
    if ((unsigned)sx < (unsigned)(w - 1) && (unsigned)sy < (unsigned)(h - 1)) {
        const uint8_t *p = S + (size_t)sy * stride + sx;
        int v0 = p[0], v1 = p[1], v2 = p[stride], v3 = p[stride + 1];
        out = (v0 * ((32 - ty) * (32 - tx) * 32) + v1 * ((32 - ty) * tx * 32) + v2 * (ty * (32 - tx) * 32) + v3 * (ty * tx * 32) +
               16384) >> 15;
    } else if (sx >= w || sx + 1 < 0 || sy >= h || sy + 1 < 0) {
        out = 0;
    } else {
        bool x0in = sx >= 0, x1in = sx + 1 < w, y0in = sy >= 0, y1in = sy + 1 < h;
        int v0 = x0in && y0in ? S[(size_t)sy * stride + sx] : 0;
        int v1 = x1in && y0in ? S[(size_t)sy * stride + sx + 1] : 0;
        int v2 = x0in && y1in ? S[(size_t)(sy + 1) * stride + sx] : 0;
        int v3 = x1in && y1in ? S[(size_t)(sy + 1) * stride + sx + 1] : 0;
        out = (v0 * ((32 - ty) * (32 - tx) * 32) + v1 * ((32 - ty) * tx * 32) + v2 * (ty * (32 - tx) * 32) + v3 * (ty * tx * 32) +
               16384) >> 15;
    }
    dst[(size_t)b * w * h + i] = (uint8_t)out;
}

// pyrDown of the homography path: frame b reads its warped plane (w x h, packed) when warped[b], the caller's frame otherwise
__global__ void k_flow_pyrdown_sel(const uint8_t *src, int stride, size_t fstride, const uint8_t *wsrc, const int32_t *warped, int w,
                                   int h, uint8_t *half, int w2, int h2, int slot0)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w2 * h2) return;
    int b = blockIdx.y;
    uint8_t v = warped[b] ? pyrdown_at(wsrc + (size_t)b * w * h, w, w, h, i % w2, i / w2)
                          : pyrdown_at(src + (size_t)b * fstride, stride, w, h, i % w2, i / w2);
    half[(size_t)(slot0 + b) * w2 * h2 + i] = v;
}

// GaussianBlur row filter on the u8 half-size image converted to float (SymmRowSmallFilter for 3 taps, RowFilter otherwise)
__global__ void k_flow_blur_row(const uint8_t *half, int w, int h, int slot0, BlurTaps kt, int ksize, float *T)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    int x = i % w, y = i / w;
    size_t so = (size_t)(slot0 + blockIdx.y) * w * h;
    const uint8_t *row = half + so + (size_t)y * w;
    int r = ksize / 2;
    float t;
    if (ksize == 3) {
        t = (float)row[x] * kt.k[1] + ((float)row[refl101(x - 1, w)] + (float)row[refl101(x + 1, w)]) * kt.k[2];
    } else {
        t = (float)row[refl101(x - r, w)] * kt.k[0];
        for (int j = 1; j < ksize; j++) t = t + (float)row[refl101(x - r + j, w)] * kt.k[j];
    }
    T[so + i] = t;
}

// GaussianBlur column filter: k0*S0 + sum k_i*(S_i + S_-i)
__global__ void k_flow_blur_col(const float *T, int w, int h, int slot0, BlurTaps kt, int ksize, float *B)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    int x = i % w, y = i / w;
    size_t so = (size_t)(slot0 + blockIdx.y) * w * h;
    const float *t = T + so + x;
    int r = ksize / 2;
    float s = t[(size_t)y * w] * kt.k[r];
    for (int k = 1; k <= r; k++) s = s + kt.k[r + k] * (t[(size_t)refl101(y + k, h) * w] + t[(size_t)refl101(y - k, h) * w]);
    B[so + i] = s;
}

// cv::resize INTER_LINEAR, float, CN channels, one output element.  mode 0: same size (copy), 1: exact 2x downscale
// (INTER_AREA fast path), 2: generic HResizeLinear + VResizeLinear.
template <int CN>
__device__ __forceinline__ float resize_at(const float *S, int sw, int sh, int dx, int dy, int c, int mode, double scx, double scy)
{
    if (mode == 0) return S[((size_t)dy * sw + dx) * CN + c];
    if (mode == 1) {
        const float *p = S + ((size_t)(2 * dy) * sw + 2 * dx) * CN + c;
        const float *q = p + (size_t)sw * CN;
        float a = p[0], b = p[CN], cc = q[0], d = q[CN];
        return (0.f + (((a + b) + cc) + d)) * 0.25f;
    }
    float fx = (float)((dx + 0.5) * scx - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    bool past = sx + 1 >= sw;       // dx >= xmax (sx is monotone in dx)
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; }
    float fy = (float)((dy + 0.5) * scy - 0.5);
    int sy = (int)floorf(fy);
    fy -= (float)sy;
    int y0 = min(max(sy, 0), sh - 1), y1 = min(max(sy + 1, 0), sh - 1);
    const float *r0 = S + (size_t)y0 * sw * CN + c, *r1 = S + (size_t)y1 * sw * CN + c;
    float h0, h1;
    if (past) {
        h0 = r0[sx * CN] * 1.f;
        h1 = r1[sx * CN] * 1.f;
    } else {
        float a0 = 1.f - fx, a1 = fx;
        h0 = r0[sx * CN] * a0 + r0[(sx + 1) * CN] * a1;
        h1 = r1[sx * CN] * a0 + r1[(sx + 1) * CN] * a1;
    }
    return h0 * (1.f - fy) + h1 * fy;
}

__global__ void k_flow_resize_img(const float *B, int sw, int sh, float *I, int dw, int dh, int slot0, int mode, double scx, double scy)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh) return;
    int s = slot0 + blockIdx.y;
    I[(size_t)s * dw * dh + i] = resize_at<1>(B + (size_t)s * sw * sh, sw, sh, i % dw, i / dw, 0, mode, scx, scy);
}

// the previous level's flow resized to this level, * (1/pyr_scale) as convertTo(.., 2.0): x*2 + 0
__global__ void k_flow_resize_flow(const float *F, size_t fstride, int sw, int sh, float *D, int dw, int dh, int mode, double scx,
                                   double scy)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dw * dh * 2) return;
    int c = i & 1, p = i >> 1;
    const float *src = F + (size_t)blockIdx.y * fstride;
    float v = resize_at<2>(src, sw, sh, p % dw, p / dw, c, mode, scx, scy);
    D[(size_t)blockIdx.y * fstride + i] = v * 2.f + 0.f;
}

__global__ void k_flow_zero(float *D, size_t fstride, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) D[(size_t)blockIdx.y * fstride + i] = 0.f;
}

// FarnebackPolyExp: one row segment of 256 pixels per block; the vertical part of the 266 columns it needs (clamped, i.e.
// the replicated border of the horizontal pass) goes through LDS.
constexpr int PE_T = 256;
__global__ __launch_bounds__(PE_T) void k_flow_polyexp(const float *I, int w, int h, int slot0, size_t rstride, size_t roff,
                                                       PolyConst pc, float *R)
{
    __shared__ float row[(PE_T + 2 * FL_POLY_N) * 3];
    const int n = FL_POLY_N;
    int y = blockIdx.y, x0 = blockIdx.x * PE_T;
    int s = slot0 + blockIdx.z;
    const float *src = I + (size_t)s * w * h;
    const float *g = pc.g + n, *xg = pc.xg + n, *xxg = pc.xxg + n;
    for (int t = threadIdx.x; t < PE_T + 2 * n; t += PE_T) {
        int x = min(max(x0 - n + t, 0), w - 1);
        float r0 = src[(size_t)y * w + x] * g[0], r1 = 0.f, r2 = 0.f;
        for (int k = 1; k <= n; k++) {
            float s0 = src[(size_t)max(y - k, 0) * w + x], s1 = src[(size_t)min(y + k, h - 1) * w + x];
            float p = s0 + s1;
            r0 = r0 + g[k] * p;
            r1 = r1 + xg[k] * (s1 - s0);
            r2 = r2 + xxg[k] * p;
        }
        row[t * 3] = r0;
        row[t * 3 + 1] = r1;
        row[t * 3 + 2] = r2;
    }
    __syncthreads();
    int x = x0 + threadIdx.x;
    if (x >= w) return;
    const float *c = row + (threadIdx.x + n) * 3;
    double b1 = c[0] * g[0], b2 = 0, b3 = c[1] * g[0], b4 = 0, b5 = c[2] * g[0], b6 = 0;
    for (int k = 1; k <= n; k++) {
        const float *P = c + k * 3, *Q = c - k * 3;
        double tg = P[0] + Q[0];
        float g0 = g[k];
        b1 += tg * g0;
        b4 += tg * xxg[k];
        b2 += (P[0] - Q[0]) * xg[k];
        b3 += (P[1] + Q[1]) * g0;
        b6 += (P[1] - Q[1]) * xg[k];
        b5 += (P[2] + Q[2]) * g0;
    }
    float *d = R + (size_t)s * rstride + roff + ((size_t)y * w + x) * 5;
    d[1] = (float)(b2 * pc.ig11);
    d[0] = (float)(b3 * pc.ig11);
    d[3] = (float)(b1 * pc.ig03 + b4 * pc.ig33);
    d[2] = (float)(b1 * pc.ig03 + b5 * pc.ig33);
    d[4] = (float)(b6 * pc.ig55);
}

// FarnebackUpdateMatrices, all rows.  Pair p: R0 = slot pslot0 + p - 1... given as slot (p0 + p) and R1 = slot (p0 + p + 1).
__global__ void k_flow_update_matrices(const float *R, size_t rstride, size_t roff, int p0, const float *F, size_t fstride, int w,
                                       int h, float *M)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    int x = i % w, y = i / w;
    int p = blockIdx.y;
    const float *R0 = R + (size_t)(p0 + p) * rstride + roff;
    const float *R1 = R + (size_t)(p0 + p + 1) * rstride + roff;
    const float *flow = F + (size_t)p * fstride;
    const float border[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    float dx = flow[i * 2], dy = flow[i * 2 + 1];
    float fx = (float)x + dx, fy = (float)y + dy;
    int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
    float r2, r3, r4, r5, r6;
    fx -= (float)x1;
    fy -= (float)y1;
    const float *r0 = R0 + (size_t)i * 5;
    if ((unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1)) {
        const float *ptr = R1 + ((size_t)y1 * w + x1) * 5;
        const float *ptr2 = ptr + (size_t)w * 5;
        float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        r2 = a00 * ptr[0] + a01 * ptr[5] + a10 * ptr2[0] + a11 * ptr2[5];
        r3 = a00 * ptr[1] + a01 * ptr[6] + a10 * ptr2[1] + a11 * ptr2[6];
        r4 = a00 * ptr[2] + a01 * ptr[7] + a10 * ptr2[2] + a11 * ptr2[7];
        r5 = a00 * ptr[3] + a01 * ptr[8] + a10 * ptr2[3] + a11 * ptr2[8];
        r6 = a00 * ptr[4] + a01 * ptr[9] + a10 * ptr2[4] + a11 * ptr2[9];
        r4 = (r0[2] + r4) * 0.5f;
        r5 = (r0[3] + r5) * 0.5f;
        r6 = (r0[4] + r6) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = r0[2];
        r5 = r0[3];
        r6 = r0[4] * 0.5f;
    }
    r2 = (r0[0] - r2) * 0.5f;
    r3 = (r0[1] - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
        float scale = (x < 5 ? border[x] : 1.f) * (x >= w - 5 ? border[w - x - 1] : 1.f) * (y < 5 ? border[y] : 1.f) *
                      (y >= h - 5 ? border[h - y - 1] : 1.f);
        r2 *= scale;
        r3 *= scale;
        r4 *= scale;
        r5 *= scale;
        r6 *= scale;
    }
    float *m = M + (size_t)p * w * h * 5 + (size_t)i * 5;
    m[0] = r4 * r4 + r6 * r6;
    m[1] = (r4 + r5) * r6;
    m[2] = r5 * r5 + r6 * r6;
    m[3] = r4 * r2 + r6 * r3;
    m[4] = r6 * r2 + r5 * r3;
}

// FarnebackUpdateFlow_Blur, vertical part: one lane per (column, channel) of a pair walks down the rows in the reference's
// order and leaves every row's vsum in V (double).
__global__ void k_flow_vsum(const float *M, int w, int h, double *V)
{
    int xc = blockIdx.x * blockDim.x + threadIdx.x;
    int W5 = w * 5;
    if (xc >= W5) return;
    const int m = FL_WIN / 2;
    const float *Mp = M + (size_t)blockIdx.y * W5 * h + xc;
    double *Vp = V + (size_t)blockIdx.y * W5 * h + xc;
    double vsum = Mp[0] * (float)(m + 2);
    for (int y = 1; y < m; y++) vsum += Mp[(size_t)min(y, h - 1) * W5];
    for (int y = 0; y < h; y++) {
        vsum += Mp[(size_t)min(y + m, h - 1) * W5] - Mp[(size_t)max(y - m - 1, 0) * W5];
        Vp[(size_t)y * W5] = vsum;
    }
}

// horizontal part and the solve: one lane per row of a pair walks across the columns (replicated vsum borders)
__global__ void k_flow_hsolve(const double *V, int w, int h, float *F, size_t fstride)
{
    int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= h) return;
    const int m = FL_WIN / 2;
    const double scale = 1. / (FL_WIN * FL_WIN);
    const double *v = V + (size_t)blockIdx.y * w * h * 5 + (size_t)y * w * 5;
    float *flow = F + (size_t)blockIdx.y * fstride + (size_t)y * w * 2;
    double g[5];
    for (int c = 0; c < 5; c++) g[c] = v[c] * (m + 2);
    for (int x = 1; x < m; x++) {
        int xx = min(x, w - 1);
        for (int c = 0; c < 5; c++) g[c] += v[xx * 5 + c];
    }
    for (int x = 0; x < w; x++) {
        int xa = min(x + m, w - 1), xs = max(x - m - 1, 0);
        for (int c = 0; c < 5; c++) g[c] += v[xa * 5 + c] - v[xs * 5 + c];
        double g11 = g[0] * scale, g12 = g[1] * scale, g22 = g[2] * scale, h1 = g[3] * scale, h2 = g[4] * scale;
        double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        flow[x * 2] = (float)((g11 * h2 - g12 * h1) * idet);
        flow[x * 2 + 1] = (float)((g22 * h1 - g12 * h2) * idet);
    }
}

// pyrUp (float, 2 channels) of the finest flow evaluated at each output pixel, then the threshold: mask = 0 where
// !(fx*fx + fy*fy < th); pixels outside the pyrUp'ed flow (odd w or h) stay 1.  Frame slots without a pair get all ones.
__global__ void k_flow_pyrup_threshold(const float *F, size_t fstride, int fw, int fh, int w, int h, float th, float *F2,
                                       uint8_t *mask, int pair0)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= w * h) return;
    int X = i % w, Y = i / w;
    int b = blockIdx.y;   // frame of the chunk
    uint8_t *mk = mask + (size_t)b * w * h;
    int p = b - pair0;
    if (p < 0 || X >= 2 * fw || Y >= 2 * fh) { mk[i] = 1; return; }
    const float *s = F + (size_t)p * fstride;
    int y = Y >> 1, x = X >> 1;
    int ry[3] = {y == 0 ? 1 : y - 1, y, min(y + 1, fh - 1)};
    float out[2];
    for (int c = 0; c < 2; c++) {
        float t[3];
        for (int k = 0; k < 3; k++) {
            const float *r = s + (size_t)ry[k] * fw * 2 + c;
            float v;
            if (!(X & 1)) {
                if (x == 0) v = r[0] * 6.f + r[2] * 2.f;
                else if (x == fw - 1) v = r[(fw - 2) * 2] + r[(fw - 1) * 2] * 7.f;
                else v = (r[(x - 1) * 2] + r[x * 2] * 6.f) + r[(x + 1) * 2];
            } else {
                if (x == fw - 1) v = r[x * 2] * 8.f;
                else v = (r[x * 2] + r[(x + 1) * 2]) * 4.f;
            }
            t[k] = v;
        }
        float o = (Y & 1) ? (t[1] + t[2]) * 4.f : (t[0] + t[1] * 6.f) + t[2];
        out[c] = o * (1.f / 64);
    }
    float *f2 = F2 + (size_t)p * (2 * fw) * (2 * fh) * 2 + ((size_t)Y * 2 * fw + X) * 2;
    f2[0] = out[0];
    f2[1] = out[1];
    float tep2 = out[0] * out[0] + out[1] * out[1];
    mk[i] = (tep2 < th) ? 1 : 0;
}

// erode (OP 0) / dilate (OP 1) of a 0/1 mask with the 21x21 ellipse.  Tile 64 x 16; the 36 x 84 input window in LDS (outside
// the image: 1 for erode, 0 for dilate); per window row and column a 7-bit code holds the AND / OR over the 7 distinct row
// spans (half-widths 0 4 6 7 8 9 10); each output ANDs / ORs one bit of 21 codes.  Exact.
__constant__ int8_t c_ell_idx[21] = {0, 1, 2, 3, 4, 5, 5, 6, 6, 6, 6, 6, 6, 6, 5, 5, 4, 3, 2, 1, 0};
constexpr int MO_TW = 64, MO_TH = 16;
template <int OP>
__global__ __launch_bounds__(256) void k_flow_morph(const uint8_t *src, int sstride, size_t sfs, uint8_t *dst, int dstride,
                                                    size_t dfs, uint8_t *dst2, int w, int h, int32_t *ones, int pair0)
{
    __shared__ uint8_t win[MO_TH + 20][MO_TW + 20];
    __shared__ uint8_t code[MO_TH + 20][MO_TW];
    __shared__ int cnt;
    int b = blockIdx.z;
    const uint8_t *s = src + (size_t)b * sfs;
    int x0 = blockIdx.x * MO_TW, y0 = blockIdx.y * MO_TH;
    const uint8_t outside = OP == 0 ? 1 : 0;
    if (threadIdx.x == 0) cnt = 0;
    for (int t = threadIdx.x; t < (MO_TH + 20) * (MO_TW + 20); t += 256) {
        int r = t / (MO_TW + 20), c = t % (MO_TW + 20);
        int yy = y0 + r - 10, xx = x0 + c - 10;
        win[r][c] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? (s[(size_t)yy * sstride + xx] != 0) : outside;
    }
    __syncthreads();
    const int hw[7] = {0, 4, 6, 7, 8, 9, 10};
    for (int t = threadIdx.x; t < (MO_TH + 20) * MO_TW; t += 256) {
        int r = t / MO_TW, c = t % MO_TW + 10;
        int acc = win[r][c];
        int code_v = 0, d = 0;
        for (int k = 0; k < 7; k++) {
            for (; d < hw[k]; d++) {
                int a = win[r][c - d - 1], bb = win[r][c + d + 1];
                acc = OP == 0 ? (acc & a & bb) : (acc | a | bb);
            }
            code_v |= acc << k;
        }
        code[r][c - 10] = (uint8_t)code_v;
    }
    __syncthreads();
    int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
    int mine = 0;
    for (int ty = ty0; ty < MO_TH; ty += 4) {
        int x = x0 + tx, y = y0 + ty;
        if (x >= w || y >= h) continue;
        int acc = OP == 0 ? 1 : 0;
        for (int dy = 0; dy < 21; dy++) {
            int bit = (code[ty + dy][tx] >> c_ell_idx[dy]) & 1;
            acc = OP == 0 ? (acc & bit) : (acc | bit);
        }
        dst[(size_t)b * dfs + (size_t)y * dstride + x] = (uint8_t)acc;
        if (dst2) dst2[(size_t)b * w * h + (size_t)y * w + x] = (uint8_t)acc;
        mine += acc;
    }
    if (ones) {
        atomicAdd(&cnt, mine);
        __syncthreads();
        if (threadIdx.x == 0 && cnt) atomicAdd(&ones[b], cnt);
    }
}

// frames of the chunk that had no previous frame: all ones (w*h of them)
__global__ void k_flow_fill_ones(uint8_t *dst, int dstride, size_t dfs, uint8_t *dst2, int w, int h, int32_t *ones)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int b = blockIdx.y;
    if (i == 0 && ones) ones[b] = w * h;
    if (i >= w * h) return;
    int x = i % w, y = i / w;
    dst[(size_t)b * dfs + (size_t)y * dstride + x] = 1;
    dst2[(size_t)b * w * h + i] = 1;
}

// perfect/src/Frame.cc:360-377 in place: one block per frame, stable compaction chunk by chunk (every destination slot is at
// or before its source, and a chunk is read completely before any of it is written), then the freed slots are zeroed.
constexpr int MK_T = 256;
__global__ __launch_bounds__(MK_T) void k_mask_keypoints(const uint8_t *mask, int w, int h, int mstride, size_t mfs,
                                                         const int32_t *ones, orbfe_keypoint *kps, uint8_t *desc, int32_t *nn,
                                                         int cap)
{
    __shared__ int scan[MK_T];
    __shared__ int base;
    int b = blockIdx.x;
    int n = min(nn[b], cap);
    if ((double)ones[b] <= (double)w * h * 0.65) return;   // sum(mask) > rows*cols*0.65 (double) filters
    const uint8_t *mk = mask + (size_t)b * mfs;
    orbfe_keypoint *K = kps + (size_t)b * cap;
    uint4 *D = (uint4 *)(desc + (size_t)b * cap * 32);
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += MK_T) {
        int i = c0 + threadIdx.x;
        orbfe_keypoint k = {};
        uint4 d0 = {}, d1 = {};
        int keep = 0;
        if (i < n) {
            k = K[i];
            d0 = D[i * 2];
            d1 = D[i * 2 + 1];
            // the range is decided in float, as grid_cell_of does: the reference reads the plane unchecked, and the device's
            // conversion gives 0 for a NaN (column / row 0 of the mask); (int) truncates towards zero, so (-1, 0) is column 0
            if (k.x > -1.f && k.x < (float)w && k.y > -1.f && k.y < (float)h)
                keep = mk[(size_t)(int)k.y * mstride + (int)k.x] == 1;
        }
        scan[threadIdx.x] = keep;
        __syncthreads();
        for (int off = 1; off < MK_T; off <<= 1) {
            int v = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        int pos = base + scan[threadIdx.x] - keep;
        if (keep) {
            K[pos] = k;
            D[pos * 2] = d0;
            D[pos * 2 + 1] = d1;
        }
        __syncthreads();
        if (threadIdx.x == MK_T - 1) base += scan[MK_T - 1];
        __syncthreads();
    }
    int m = base;
    for (int i = m + threadIdx.x; i < n; i += MK_T) {
        K[i] = orbfe_keypoint{};
        D[i * 2] = uint4{};
        D[i * 2 + 1] = uint4{};
    }
    if (threadIdx.x == 0) nn[b] = m;
}

inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

struct orbfe_flow {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;
    int maxw = 0, maxh = 0, maxb = 0, chunk = 0;
    PolyConst pc;
    FlowPlan maxplan;
    // state: FlowSLAM::Flow::mImGrayLast
    uint8_t *d_last = nullptr;
    bool have_last = false;
    int last_w2 = 0, last_h2 = 0;
    // scratch for one chunk (chunk + 1 frame slots, chunk pairs)
    uint8_t *d_half = nullptr, *d_gray = nullptr, *d_mask_host = nullptr, *d_m0 = nullptr, *d_m1 = nullptr, *d_mfinal = nullptr;
    float *d_T = nullptr, *d_B = nullptr, *d_I = nullptr, *d_R = nullptr, *d_FL = nullptr, *d_M = nullptr, *d_F2 = nullptr;
    double *d_V = nullptr;
    int32_t *d_ones = nullptr;
    // the homography path: one chunk of warped full-size frames, their inverse matrices and warped flags, the host call's H
    uint8_t *d_warp = nullptr;
    double *d_hinv = nullptr, *d_homo1 = nullptr;
    int32_t *d_warped = nullptr;
    // what the taps read: the last chunk of the last call
    int tap_valid = 0, tap_n = 0, tap_first = 0, tap_pair0 = 0, tap_w = 0, tap_h = 0, tap_homo = 0;
    FlowPlan tap_plan;
};

static void flow_free(orbfe_flow *f)
{
    orb_free_all(f->stream, {f->d_last, f->d_half, f->d_gray, f->d_mask_host, f->d_m0, f->d_m1, f->d_mfinal, f->d_T, f->d_B, f->d_I, f->d_R,
                             f->d_FL, f->d_M, f->d_F2, f->d_V, f->d_ones, f->d_warp, f->d_hinv, f->d_homo1, f->d_warped});
}

extern "C" orbfe_status orbfe_flow_plan(int32_t w, int32_t h, int32_t *nlevels, int32_t *lw, int32_t *lh, int32_t *ksize, float *taps)
{
    if (w < FL_MIN_SIDE || h < FL_MIN_SIDE || !nlevels) return ORBFE_ERR_ARG;
    FlowPlan p;
    make_plan(w / 2, h / 2, p);
    *nlevels = p.n;
    for (int l = 0; l < p.n; l++) {
        if (lw) lw[l] = p.lv[l].w;
        if (lh) lh[l] = p.lv[l].h;
        if (ksize) ksize[l] = p.lv[l].ksize;
        if (taps) memcpy(taps + l * FL_MAX_TAPS, p.lv[l].taps, sizeof(p.lv[l].taps));
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_flow_poly_constants(float *g, double *ig)
{
    if (!g || !ig) return ORBFE_ERR_ARG;
    PolyConst c;
    prepare_gaussian(c);
    memcpy(g, c.g, sizeof(c.g));
    memcpy(g + 11, c.xg, sizeof(c.xg));
    memcpy(g + 22, c.xxg, sizeof(c.xxg));
    ig[0] = c.ig11;
    ig[1] = c.ig03;
    ig[2] = c.ig33;
    ig[3] = c.ig55;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_flow_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_batch, orbfe_flow **out)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    if (max_width < FL_MIN_SIDE || max_height < FL_MIN_SIDE || max_batch < 1 || (int64_t)max_width * max_height > (1 << 26))
        return ORBFE_ERR_ARG;
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    orbfe_flow *f = new (std::nothrow) orbfe_flow();
    if (!f) return ORBFE_ERR_NOMEM;
    DeviceGuard dg(device);
    f->device = device;
    f->maxw = max_width;
    f->maxh = max_height;
    f->maxb = max_batch;
    f->chunk = std::min(max_batch, FL_CHUNK);
    prepare_gaussian(f->pc);
    int w2 = max_width / 2, h2 = max_height / 2;
    make_plan(w2, h2, f->maxplan);
    size_t hw2 = (size_t)w2 * h2, hw = (size_t)max_width * max_height, slots = f->chunk + 1, pairs = f->chunk;
    size_t f2 = (size_t)(2 * w2) * (2 * h2) * 2;
    auto blk = [](auto **p, size_t bytes) { return OrbAlloc{(void **)p, bytes}; };
    const bool ok = orb_alloc_all(
        &f->stream,
        {blk(&f->d_last, hw2), blk(&f->d_half, slots * hw2), blk(&f->d_gray, hw), blk(&f->d_mask_host, hw), blk(&f->d_m0, pairs * hw),
         blk(&f->d_m1, pairs * hw), blk(&f->d_mfinal, pairs * hw), blk(&f->d_T, slots * hw2 * sizeof(float)),
         blk(&f->d_B, slots * hw2 * sizeof(float)), blk(&f->d_I, slots * hw2 * sizeof(float)),
         blk(&f->d_R, slots * f->maxplan.rtotal * sizeof(float)), blk(&f->d_FL, pairs * f->maxplan.ftotal * sizeof(float)),
         blk(&f->d_M, pairs * hw2 * 5 * sizeof(float)), blk(&f->d_V, pairs * hw2 * 5 * sizeof(double)),
         blk(&f->d_F2, pairs * f2 * sizeof(float)), blk(&f->d_ones, pairs * sizeof(int32_t)), blk(&f->d_warp, pairs * hw),
         blk(&f->d_hinv, pairs * 9 * sizeof(double)), blk(&f->d_homo1, 9 * sizeof(double)), blk(&f->d_warped, pairs * sizeof(int32_t))});
    if (!ok) {
        (void)hipGetLastError();
        orbfe_set_error("orbfe_flow_create: device allocation failed");
        flow_free(f);
        delete f;
        return ORBFE_ERR_NOMEM;
    }
    f->last_stream = f->stream;
    *out = f;
    return ORBFE_OK;
}

extern "C" void orbfe_flow_destroy(orbfe_flow *f)
{
    if (!f) return;
    DeviceGuard dg(f->device);
    (void)hipStreamSynchronize(f->last_stream);
    (void)hipStreamSynchronize(f->stream);
    flow_free(f);
    delete f;
}

extern "C" orbfe_status orbfe_flow_reset(orbfe_flow *f)
{
    if (!f) return ORBFE_ERR_ARG;
    f->have_last = false;
    return ORBFE_OK;
}

extern "C" void *orbfe_flow_get_stream(orbfe_flow *f) { return f ? (void *)f->stream : nullptr; }

// One chunk: frames [0, n) of d_gray; slot 0 holds the previous frame's half-size image when have_prev.  With d_homo
// ([n][9], device) the frames with a nonzero d_use entry (all when d_use is NULL) are warped first and pyrDown reads the warped
// planes; without it the launches are those of the plain ComputeMask.
static orbfe_status flow_chunk(orbfe_flow *f, const uint8_t *d_gray, int n, int w, int h, int stride, size_t fstride, float th,
                               uint8_t *d_mask, int mstride, size_t mfs, int32_t *d_ones, bool have_prev, const double *d_homo,
                               const int32_t *d_use, hipStream_t st)
{
    const int w2 = w / 2, h2 = h / 2;
    const size_t hw2 = (size_t)w2 * h2;
    FlowPlan P;
    make_plan(w2, h2, P);
    if (P.rtotal > f->maxplan.rtotal || P.ftotal > f->maxplan.ftotal) {
        orbfe_set_error("flow plan exceeds the handle's scratch");
        return ORBFE_ERR_SIZE;
    }
    const int T = 256;
    if (have_prev) ORBFE_HIP(hipMemcpyAsync(f->d_half, f->d_last, hw2, hipMemcpyDeviceToDevice, st));
    if (d_homo) {
        k_flow_homo_prep<<<nblk(n, 64), 64, 0, st>>>(d_homo, d_use, n, f->d_hinv, f->d_warped);
        k_flow_warp<<<dim3(nblk((size_t)w * h, T), n), T, 0, st>>>(d_gray, stride, fstride, w, h, f->d_hinv, f->d_warped, f->d_warp);
        k_flow_pyrdown_sel<<<dim3(nblk(hw2, T), n), T, 0, st>>>(d_gray, stride, fstride, f->d_warp, f->d_warped, w, h, f->d_half, w2,
                                                                 h2, 1);
    } else {
        k_flow_pyrdown<<<dim3(nblk(hw2, T), n), T, 0, st>>>(d_gray, stride, fstride, w, h, f->d_half, w2, h2, 1);
    }
    const int s0 = have_prev ? 0 : 1;            // first slot with an image
    const int nslots = n + 1 - s0;
    const int pair0 = have_prev ? 0 : 1;         // first frame of the chunk with a pair (frame b pairs slots b, b + 1)
    const int npairs = n - pair0;
    if (npairs > 0) {
        // PolyExp of every slot at every level (each frame's once: R1 of one pair, R0 of the next)
        for (int l = P.n - 1; l >= 0; l--) {
            const FlowLevel &L = P.lv[l];
            BlurTaps kt;
            memcpy(kt.k, L.taps, sizeof(kt.k));
            k_flow_blur_row<<<dim3(nblk(hw2, T), nslots), T, 0, st>>>(f->d_half, w2, h2, s0, kt, L.ksize, f->d_T);
            k_flow_blur_col<<<dim3(nblk(hw2, T), nslots), T, 0, st>>>(f->d_T, w2, h2, s0, kt, L.ksize, f->d_B);
            const float *lev = f->d_B;
            if (L.w != w2 || L.h != h2) {
                int mode = (w2 == 2 * L.w && h2 == 2 * L.h) ? 1 : 2;
                double scx = 1. / ((double)L.w / w2), scy = 1. / ((double)L.h / h2);
                k_flow_resize_img<<<dim3(nblk((size_t)L.w * L.h, T), nslots), T, 0, st>>>(f->d_B, w2, h2, f->d_I, L.w, L.h, s0, mode,
                                                                                          scx, scy);
                lev = f->d_I;
            }
            k_flow_polyexp<<<dim3(nblk(L.w, PE_T), L.h, nslots), PE_T, 0, st>>>(lev, L.w, L.h, s0, P.rtotal, L.roff, f->pc, f->d_R);
        }
        // the flow, coarsest level first
        for (int l = P.n - 1; l >= 0; l--) {
            const FlowLevel &L = P.lv[l];
            size_t npx = (size_t)L.w * L.h;
            float *F = f->d_FL + L.foff;
            if (l == P.n - 1) {
                k_flow_zero<<<dim3(nblk(npx * 2, T), npairs), T, 0, st>>>(F, P.ftotal, (int)(npx * 2));
            } else {
                const FlowLevel &C = P.lv[l + 1];
                int mode = (C.w == 2 * L.w && C.h == 2 * L.h) ? 1 : 2;
                double scx = 1. / ((double)L.w / C.w), scy = 1. / ((double)L.h / C.h);
                k_flow_resize_flow<<<dim3(nblk(npx * 2, T), npairs), T, 0, st>>>(f->d_FL + C.foff, P.ftotal, C.w, C.h, F, L.w, L.h,
                                                                                 mode, scx, scy);
            }
            k_flow_update_matrices<<<dim3(nblk(npx, T), npairs), T, 0, st>>>(f->d_R, P.rtotal, L.roff, s0, F, P.ftotal, L.w, L.h,
                                                                              f->d_M);
            for (int it = 0; it < FL_ITERS; it++) {
                k_flow_vsum<<<dim3(nblk(npx * 5 / L.h, 64), npairs), 64, 0, st>>>(f->d_M, L.w, L.h, f->d_V);
                k_flow_hsolve<<<dim3(nblk(L.h, 64), npairs), 64, 0, st>>>(f->d_V, L.w, L.h, F, P.ftotal);
                if (it < FL_ITERS - 1)
                    k_flow_update_matrices<<<dim3(nblk(npx, T), npairs), T, 0, st>>>(f->d_R, P.rtotal, L.roff, s0, F, P.ftotal, L.w,
                                                                                      L.h, f->d_M);
            }
        }
    }
    const size_t hw = (size_t)w * h;
    if (d_ones) ORBFE_HIP(hipMemsetAsync(d_ones, 0, n * sizeof(int32_t), st));
    if (pair0 > 0) k_flow_fill_ones<<<dim3(nblk(hw, T), pair0), T, 0, st>>>(d_mask, mstride, mfs, f->d_mfinal, w, h, d_ones);
    if (npairs > 0) {
        // pyrUp + threshold into m0 (frames b >= pair0), erode m0 -> m1, erode m1 -> m0, dilate m0 -> caller (and mfinal)
        k_flow_pyrup_threshold<<<dim3(nblk(hw, T), n), T, 0, st>>>(f->d_FL + P.lv[0].foff, P.ftotal, w2, h2, w, h, th, f->d_F2,
                                                                   f->d_m0, pair0);
        dim3 mg(nblk(w, MO_TW), nblk(h, MO_TH), npairs);
        uint8_t *m0 = f->d_m0 + (size_t)pair0 * hw, *m1 = f->d_m1 + (size_t)pair0 * hw;
        k_flow_morph<0><<<mg, 256, 0, st>>>(m0, w, hw, m1, w, hw, nullptr, w, h, nullptr, 0);
        k_flow_morph<0><<<mg, 256, 0, st>>>(m1, w, hw, f->d_mfinal + (size_t)pair0 * hw, w, hw, nullptr, w, h, nullptr, 0);
        k_flow_morph<1><<<mg, 256, 0, st>>>(f->d_mfinal + (size_t)pair0 * hw, w, hw, d_mask + (size_t)pair0 * mfs, mstride, mfs,
                                            m1, w, h, d_ones ? d_ones + pair0 : nullptr, 0);
    }
    ORBFE_HIP(hipGetLastError());
    // the new state: the chunk's last half-size image
    ORBFE_HIP(hipMemcpyAsync(f->d_last, f->d_half + (size_t)n * hw2, hw2, hipMemcpyDeviceToDevice, st));
    f->tap_valid = 1;
    f->tap_n = n;
    f->tap_pair0 = pair0;
    f->tap_w = w;
    f->tap_h = h;
    f->tap_homo = d_homo != nullptr;
    f->tap_plan = P;
    return ORBFE_OK;
}

static orbfe_status flow_check(orbfe_flow *f, int w, int h, int stride)
{
    if (w < FL_MIN_SIDE || h < FL_MIN_SIDE || w > f->maxw || h > f->maxh || stride < w) {
        orbfe_set_error("frame %dx%d (stride %d) outside [%d, %d] x [%d, %d]", w, h, stride, FL_MIN_SIDE, f->maxw, FL_MIN_SIDE, f->maxh);
        return ORBFE_ERR_SIZE;
    }
    if (f->have_last && (w / 2 != f->last_w2 || h / 2 != f->last_h2)) {
        orbfe_set_error("half-size frame %dx%d differs from the previous frame's %dx%d", w / 2, h / 2, f->last_w2, f->last_h2);
        return ORBFE_ERR_SIZE;
    }
    return ORBFE_OK;
}

static orbfe_status flow_run(orbfe_flow *f, const uint8_t *d_gray, int n, int w, int h, int stride, size_t fstride, float th,
                             uint8_t *d_mask, int mstride, size_t mfs, int32_t *d_ones, const double *d_homo, const int32_t *d_use,
                             hipStream_t st)
{
    if (th < 40.0) th = 40.0f;   // if (BInaryThreshold < 40.0) BInaryThreshold = 40.0
    // the mask of a frame lives in d_mask; the pre-morphology / erosion scratch is one chunk of w*h planes
    f->last_stream = st;
    for (int c0 = 0; c0 < n; c0 += f->chunk) {
        int m = std::min(f->chunk, n - c0);
        orbfe_status s = flow_chunk(f, d_gray + (size_t)c0 * fstride, m, w, h, stride, fstride, th, d_mask + (size_t)c0 * mfs, mstride,
                                    mfs, d_ones ? d_ones + c0 : nullptr, f->have_last, d_homo ? d_homo + (size_t)c0 * 9 : nullptr,
                                    d_use ? d_use + c0 : nullptr, st);
        if (s != ORBFE_OK) return s;
        f->have_last = true;
        f->last_w2 = w / 2;
        f->last_h2 = h / 2;
        f->tap_first = c0;
    }
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_flow_compute_masks_device(orbfe_flow *f, const uint8_t *d_gray, int32_t nframes, int32_t w, int32_t h,
                                                        int32_t stride, size_t frame_stride, float threshold, uint8_t *d_mask,
                                                        int32_t mask_stride, size_t mask_frame_stride, int32_t *d_mask_ones,
                                                        void *stream)
{
    if (!f || !d_gray || !d_mask || nframes < 1) return ORBFE_ERR_ARG;
    if (nframes > f->maxb) {
        orbfe_set_error("%d frames exceed max_batch %d", nframes, f->maxb);
        return ORBFE_ERR_SIZE;
    }
    orbfe_status s = flow_check(f, w, h, stride);
    if (s != ORBFE_OK) return s;
    if (mask_stride < w || (nframes > 1 && (frame_stride < (size_t)stride * h || mask_frame_stride < (size_t)mask_stride * h)))
        return ORBFE_ERR_ARG;
    DeviceGuard dg(f->device);
    return flow_run(f, d_gray, nframes, w, h, stride, frame_stride, threshold, d_mask, mask_stride, mask_frame_stride, d_mask_ones,
                    nullptr, nullptr, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_flow_compute_masks_homo_device(orbfe_flow *f, const uint8_t *d_gray, int32_t nframes, int32_t w,
                                                             int32_t h, int32_t stride, size_t frame_stride, const double *d_homo,
                                                             const int32_t *d_use_homo, float threshold, uint8_t *d_mask,
                                                             int32_t mask_stride, size_t mask_frame_stride, int32_t *d_mask_ones,
                                                             void *stream)
{
    if (!f || !d_gray || !d_mask || !d_homo || nframes < 1) return ORBFE_ERR_ARG;
    if (nframes > f->maxb) {
        orbfe_set_error("%d frames exceed max_batch %d", nframes, f->maxb);
        return ORBFE_ERR_SIZE;
    }
    orbfe_status s = flow_check(f, w, h, stride);
    if (s != ORBFE_OK) return s;
    if (mask_stride < w || (nframes > 1 && (frame_stride < (size_t)stride * h || mask_frame_stride < (size_t)mask_stride * h)))
        return ORBFE_ERR_ARG;
    DeviceGuard dg(f->device);
    return flow_run(f, d_gray, nframes, w, h, stride, frame_stride, threshold, d_mask, mask_stride, mask_frame_stride, d_mask_ones,
                    d_homo, d_use_homo, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_flow_compute_mask(orbfe_flow *f, const uint8_t *gray, int32_t w, int32_t h, int32_t stride, float threshold,
                                                uint8_t *mask, int32_t mask_stride)
{
    if (!f || !gray || !mask || mask_stride < w) return ORBFE_ERR_ARG;
    orbfe_status s = flow_check(f, w, h, stride);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(f->device);
    hipStream_t st = f->stream;
    ORBFE_HIP(hipMemcpy2DAsync(f->d_gray, w, gray, stride, w, h, hipMemcpyHostToDevice, st));
    s = flow_run(f, f->d_gray, 1, w, h, w, (size_t)w * h, threshold, f->d_mask_host, w, (size_t)w * h, nullptr, nullptr, nullptr, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(hipMemcpy2DAsync(mask, mask_stride, f->d_mask_host, w, w, h, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_flow_compute_mask_homo(orbfe_flow *f, const uint8_t *gray, int32_t w, int32_t h, int32_t stride,
                                                     const double *homo, float threshold, uint8_t *mask, int32_t mask_stride)
{
    if (!f || !gray || !homo || !mask || mask_stride < w) return ORBFE_ERR_ARG;
    orbfe_status s = flow_check(f, w, h, stride);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(f->device);
    hipStream_t st = f->stream;
    ORBFE_HIP(hipMemcpy2DAsync(f->d_gray, w, gray, stride, w, h, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(f->d_homo1, homo, 9 * sizeof(double), hipMemcpyHostToDevice, st));
    s = flow_run(f, f->d_gray, 1, w, h, w, (size_t)w * h, threshold, f->d_mask_host, w, (size_t)w * h, nullptr, f->d_homo1, nullptr, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(hipMemcpy2DAsync(mask, mask_stride, f->d_mask_host, w, w, h, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_mask_keypoints_device(const uint8_t *d_mask, int32_t w, int32_t h, int32_t mask_stride,
                                                    size_t mask_frame_stride, const int32_t *d_mask_ones, int32_t nframes,
                                                    orbfe_keypoint *d_kps, uint8_t *d_desc, int32_t *d_n, int32_t cap, void *stream)
{
    if (!d_mask || !d_mask_ones || !d_kps || !d_desc || !d_n || nframes < 1 || cap < 1 || w < 1 || h < 1 || mask_stride < w ||
        (nframes > 1 && mask_frame_stride < (size_t)mask_stride * h))
        return ORBFE_ERR_ARG;
    int32_t device = -1;   // the caller's current device: the buffers are theirs
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    k_mask_keypoints<<<nframes, MK_T, 0, (hipStream_t)stream>>>(d_mask, w, h, mask_stride, mask_frame_stride, d_mask_ones, d_kps, d_desc,
                                                                d_n, cap);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_flow_tap(orbfe_flow *f, int32_t frame, int32_t stage, int32_t level, void *dst, size_t cap, int32_t *w,
                                       int32_t *h)
{
    if (!f || !dst) return ORBFE_ERR_ARG;
    if (!f->tap_valid) return ORBFE_ERR_STATE;
    int b = frame - f->tap_first;
    if (b < 0 || b >= f->tap_n) return ORBFE_ERR_ARG;
    const FlowPlan &P = f->tap_plan;
    int W = f->tap_w, H = f->tap_h, w2 = W / 2, h2 = H / 2;
    int p = b - f->tap_pair0;
    if ((stage == ORBFE_FLOW_TAP_FLOW || stage == ORBFE_FLOW_TAP_FLOW2 || stage == ORBFE_FLOW_TAP_PRE) && p < 0) return ORBFE_ERR_STATE;
    if ((stage == ORBFE_FLOW_TAP_FLOW || stage == ORBFE_FLOW_TAP_POLY) && (level < 0 || level >= P.n)) return ORBFE_ERR_ARG;
    const void *src;
    size_t bytes;
    int ow, oh;
    switch (stage) {
    case ORBFE_FLOW_TAP_HALF:
        ow = w2, oh = h2, bytes = (size_t)ow * oh, src = f->d_half + (size_t)(b + 1) * w2 * h2;
        break;
    case ORBFE_FLOW_TAP_FLOW:
        ow = P.lv[level].w, oh = P.lv[level].h, bytes = (size_t)ow * oh * 8, src = f->d_FL + (size_t)p * P.ftotal + P.lv[level].foff;
        break;
    case ORBFE_FLOW_TAP_FLOW2:
        ow = 2 * w2, oh = 2 * h2, bytes = (size_t)ow * oh * 8, src = f->d_F2 + (size_t)p * ow * oh * 2;
        break;
    case ORBFE_FLOW_TAP_PRE:
        ow = W, oh = H, bytes = (size_t)W * H, src = f->d_m0 + (size_t)b * W * H;
        break;
    case ORBFE_FLOW_TAP_MASK:
        // frames with a pair: the dilate's second output (m1); frames without: mfinal (all ones)
        ow = W, oh = H, bytes = (size_t)W * H, src = (p < 0 ? f->d_mfinal : f->d_m1) + (size_t)b * W * H;
        break;
    case ORBFE_FLOW_TAP_POLY:
        if (p < 0 && b == 0) return ORBFE_ERR_STATE;
        ow = P.lv[level].w, oh = P.lv[level].h, bytes = (size_t)ow * oh * 20, src = f->d_R + (size_t)(b + 1) * P.rtotal + P.lv[level].roff;
        break;
    case ORBFE_FLOW_TAP_WARP:
        if (!f->tap_homo) return ORBFE_ERR_STATE;
        ow = W, oh = H, bytes = (size_t)W * H, src = f->d_warp + (size_t)b * W * H;
        break;
    default:
        return ORBFE_ERR_ARG;
    }
    if (cap < bytes) return ORBFE_ERR_CAP;
    DeviceGuard dg(f->device);
    ORBFE_HIP(hipStreamSynchronize(f->last_stream));
    if (stage == ORBFE_FLOW_TAP_WARP) {
        int32_t warped = 0;
        ORBFE_HIP(hipMemcpy(&warped, f->d_warped + b, sizeof(warped), hipMemcpyDeviceToHost));
        if (!warped) return ORBFE_ERR_STATE;
    }
    ORBFE_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    if (w) *w = ow;
    if (h) *h = oh;
    return ORBFE_OK;
}
