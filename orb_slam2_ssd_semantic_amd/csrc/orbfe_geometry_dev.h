// orbfe_geometry_dev.h -- the per-point arithmetic of DynaSLAM::Geometry::ExtractDynPoints (perfect/src/Geometry.cc:136-471) as
// OpenCV 3.2 evaluates it, one __host__ __device__ function per step, so that the kernels of csrc/orbfe_geometry.hip and the host
// helpers run the same code.  float where the C++ uses float, double where it uses double, one operation at a time (the library
// is built with -ffp-contract=off).  tests/geometry_oracle.py restates every function here under the same name.
#pragma once

#include "orbfe_cvmat_dev.h"   // GEO_HD, geo_gemm_store, geo_inv3: shared with orbfe_f12.h

GEO_HD uint32_t geo_hi(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return (uint32_t)(u >> 32);
}
GEO_HD uint32_t geo_lo(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return (uint32_t)u;
}
GEO_HD double geo_clear_lo(double x)
{
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    u &= 0xffffffff00000000ull;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// The canonical acos: fdlibm's __ieee754_acos (e_acos.c) as a fixed fp64 operation sequence; sqrt and the divisions are IEEE.
GEO_HD double geo_acos(double x)
{
    const double pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
                 pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05,
                 qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
                 qS4 = 7.70381505559019352791e-02;
    const uint32_t hx = geo_hi(x), ix = hx & 0x7fffffffu;
    if (ix >= 0x3ff00000u) {
        if (((ix - 0x3ff00000u) | geo_lo(x)) == 0) return (hx >> 31) ? pi + 2.0 * pio2_lo : 0.0;
        return (x - x) / (x - x);   // |x| > 1, an infinity or a NaN: NaN
    }
    if (ix < 0x3fe00000u) {   // |x| < 0.5
        if (ix <= 0x3c600000u) return pio2_hi + pio2_lo;
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        return pio2_hi - (x - (pio2_lo - r * x));
    }
    if (hx >> 31) {   // x < -0.5
        const double z = (1.0 + x) * 0.5;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double s = sqrt(z);
        const double r = p / q;
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;   // x > 0.5
    const double s = sqrt(z);
    const double df = geo_clear_lo(s);
    const double c = (z - df * df) / (s + df);
    const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const double r = p / q;
    const double w = r * s + c;
    return 2.0 * (df + w);
}

// K = eye(3) with fx, fy, cx, cy (Geometry.cc:141-145)
GEO_HD void geo_make_K(float fx, float fy, float cx, float cy, float *K)
{
    K[0] = fx, K[1] = 0.f, K[2] = cx, K[3] = 0.f, K[4] = fy, K[5] = cy, K[6] = 0.f, K[7] = 0.f, K[8] = 1.f;
}

// cv::solve(A, B, DECOMP_LU) for a 4x4 CV_32F A (hal::LU32f = LUImpl<float>, modules/core/src/lapack.cpp / hal_internal): the
// elimination of A does not depend on B, so it is done once (geo_lu4_factor) and replayed on every column (geo_lu4_solve).
struct GeoLU4 {
    float A[16];      // A after the elimination: the upper triangle, reciprocal pivots on the diagonal
    float alpha[16];  // alpha[j * 4 + i]: the multiplier of row i added to row j in step i
    int32_t piv[4];   // the row swapped with row i in step i
    int32_t ok;       // 0: a pivot below FLT_EPSILON * 10, solve answers false and the result is set to zero
};

GEO_HD void geo_lu4_factor(const float *T, GeoLU4 *lu)
{
    float *A = lu->A;
    for (int k = 0; k < 16; k++) A[k] = T[k], lu->alpha[k] = 0.f;
    lu->ok = 1;
    const float eps = 1.1920928955078125e-07f * 10;
    for (int i = 0; i < 4; i++) {
        int k = i;
        for (int j = i + 1; j < 4; j++)
            if (fabsf(A[j * 4 + i]) > fabsf(A[k * 4 + i])) k = j;
        lu->piv[i] = k;
        if (fabsf(A[k * 4 + i]) < eps) {
            lu->ok = 0;
            for (int q = i; q < 4; q++) lu->piv[q] = q;
            return;
        }
        if (k != i)
            for (int j = i; j < 4; j++) {
                const float t = A[i * 4 + j];
                A[i * 4 + j] = A[k * 4 + j];
                A[k * 4 + j] = t;
            }
        const float d = -1 / A[i * 4 + i];
        for (int j = i + 1; j < 4; j++) {
            const float alpha = A[j * 4 + i] * d;
            lu->alpha[j * 4 + i] = alpha;
            for (int q = i + 1; q < 4; q++) A[j * 4 + q] += alpha * A[i * 4 + q];
        }
        A[i * 4 + i] = -d;
    }
}

GEO_HD void geo_lu4_solve(const GeoLU4 *lu, float *b)
{
    if (!lu->ok) {
        b[0] = b[1] = b[2] = b[3] = 0.f;
        return;
    }
    for (int i = 0; i < 4; i++) {
        const int k = lu->piv[i];
        if (k != i) {
            const float t = b[i];
            b[i] = b[k];
            b[k] = t;
        }
        for (int j = i + 1; j < 4; j++) b[j] += lu->alpha[j * 4 + i] * b[i];
    }
    for (int i = 3; i >= 0; i--) {
        float s = b[i];
        for (int k = i + 1; k < 4; k++) s -= lu->A[i * 4 + k] * b[k];
        b[i] = s * lu->A[i * 4 + i];
    }
}

// One column of K.inv() * matRefFrame.t() stacked on 1/d (:173-198): the product is a GEMM_2_T gemm, so GEMMSingleMul's A * Bt
// branch accumulates it in double (s0 over k, then s0 += s1 + s2 + s3 of three zeros); 1./d is a double division stored as float.
GEO_HD void geo_backproject(const float *Kinv, float ux, float uy, float d, float *b)
{
    const float p[3] = {ux, uy, 1.f};
    for (int i = 0; i < 3; i++) {
        double s0 = 0.;
        for (int k = 0; k < 3; k++) s0 += (double)Kinv[i * 3 + k] * (double)p[k];
        s0 += (0. + 0.) + 0.;
        b[i] = (float)(s0 * 1.0);
    }
    b[3] = (float)(1. / (double)d);
}

// :214-228: the angle between (mp - tRef) and (mp - tCur), the poses' translation columns, not the camera centres.  Mat::dot and
// cv::norm accumulate float data in double (modules/core/src/matmul.cpp dotProd_, stat.cpp normL2_); acos is geo_acos.  True iff
// angle < 30 (a NaN angle is false).
GEO_HD bool geo_parallax_ok(const float *vmpw, float invd, const float *tref, const float *tcur)
{
    float a[3], c[3];
    for (int k = 0; k < 3; k++) {
        const float mp = vmpw[k] / invd;
        a[k] = mp - tref[k];
        c[k] = mp - tcur[k];
    }
    double dot = 0., na = 0., nc = 0.;
    for (int k = 0; k < 3; k++) dot += (double)a[k] * (double)c[k];
    for (int k = 0; k < 3; k++) na += (double)a[k] * (double)a[k];
    for (int k = 0; k < 3; k++) nc += (double)c[k] * (double)c[k];
    na = sqrt(na);
    nc = sqrt(nc);
    const double angle = geo_acos(dot / (na * nc)) * 180 / 3.14159265358979323846;
    return angle < 30.0;
}

// :275-284: one column of currentFrame.mTcw * vAllMPw (gemm's float shortcut for a 4-long inner dimension: every column count
// takes it), then the division by the fourth row, rows 0, 1, 2 first and the fourth by itself last
GEO_HD void geo_to_current(const float *T, const float *v, float *o)
{
    for (int i = 0; i < 4; i++) {
        const float t = T[i * 4] * v[0] + T[i * 4 + 1] * v[1] + T[i * 4 + 2] * v[2] + T[i * 4 + 3] * v[3];
        o[i] = geo_gemm_store(t);
    }
    o[0] /= o[3];
    o[1] /= o[3];
    o[2] /= o[3];
    o[3] /= o[3];
}

// :339-351: one column of (K * aux) * vMPCurrentFrame and the ceil of its pixel.  K * aux = [K | 0] exactly.  gemm takes the float
// shortcut only when the result is 4 columns wide (mode 1); one column of a one-column matrix turns into the A * Bt branch with
// its four partial sums (mode 2); every other shape accumulates over k in double (mode 0).
enum { GEO_PROJ_DOUBLE = 0, GEO_PROJ_FLOAT4 = 1, GEO_PROJ_SINGLE = 2 };
GEO_HD int geo_proj_mode(int n_depth7, int n_parallax)
{
    return n_depth7 == 4 ? GEO_PROJ_FLOAT4 : (n_depth7 == 1 && n_parallax == 1) ? GEO_PROJ_SINGLE : GEO_PROJ_DOUBLE;
}
GEO_HD void geo_project(const float *K, const float *X, int mode, float *px, float *py)
{
    float m[3];
    for (int i = 0; i < 3; i++) {
        const float a[4] = {K[i * 3], K[i * 3 + 1], K[i * 3 + 2], 0.f};
        if (mode == GEO_PROJ_FLOAT4) {
            const float t = a[0] * X[0] + a[1] * X[1] + a[2] * X[2] + a[3] * X[3];
            m[i] = geo_gemm_store(t);
        } else if (mode == GEO_PROJ_SINGLE) {
            double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
            s0 += (double)a[0] * (double)X[0];
            s1 += (double)a[1] * (double)X[1];
            s2 += (double)a[2] * (double)X[2];
            s3 += (double)a[3] * (double)X[3];
            s0 += s1 + s2 + s3;
            m[i] = (float)(s0 * 1.0);
        } else {
            double s0 = 0.;
            for (int k = 0; k < 4; k++) s0 += (double)a[k] * (double)X[k];
            m[i] = (float)(s0 * 1.0);
        }
    }
    *px = ceilf(m[0] / m[2]);
    *py = ceilf(m[1] / m[2]);
}

// IsInFrame (:586-593) with mDmax = 20: strictly inside a 21-pixel border
GEO_HD bool geo_in_frame(float x, float y, int w, int h)
{
    return x > (float)(20 + 1) && x < (float)(w - 20 - 1) && y > (float)(20 + 1) && y < (float)(h - 20 - 1);
}

// getStructuringElement(MORPH_ELLIPSE, (2r+1, 2r+1)) (modules/imgproc/src/morph.cpp): the half-width of row i
GEO_HD int geo_ellipse_half_width(int r, int i)
{
    const double inv_r2 = r ? 1. / ((double)r * r) : 0;
    const int dy = i - r;
    return (int)rint(r * sqrt((r * r - dy * dy) * inv_r2));
}
