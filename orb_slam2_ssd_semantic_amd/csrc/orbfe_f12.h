// orbfe_f12.h -- what LocalMapping::CreateNewMapPoints computes per neighbour before it calls SearchForTriangulation
// (src/LocalMapping.cc:390-417): the baseline gate, ComputeF12 (:848-867) and the epipole (src/ORBmatcher.cc:833-843), one
// __host__ __device__ function each, so that k_tri_pairs (orbfe_tri_search.hip) and the host orbfe_compute_f12 run the same code.
// cv::Mat expressions are restated as OpenCV 3.2 evaluates them; tests/f12_oracle.py restates every function here under the same
// name.  The library is built with -ffp-contract=off: one operation at a time.
#pragma once

#include "orbfe_cvmat_dev.h"

// gemm's float shortcut (flags == 0, inner length 3) for one element: a float sum of three float products, left to right,
// stored as (float)(t * alpha + c * beta) in double
GEO_HD float f12_dot3(float a0, float b0, float a1, float b1, float a2, float b2) { return a0 * b0 + a1 * b1 + a2 * b2; }

// D = A * B for 3x3 row-major floats: a plain product of two evaluated matrices, the shortcut with len == d_size.width
GEO_HD void f12_mul33(const float *A, const float *B, float *D)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) D[i * 3 + j] = geo_gemm_store(f12_dot3(A[i * 3], B[j], A[i * 3 + 1], B[3 + j], A[i * 3 + 2], B[6 + j]));
}

// LocalMapping::ComputeF12 (:848-867) from two poses Tcw = row-major 3x4 (Rcw | tcw) and the pinhole K both keyframes share
GEO_HD void f12_compute(const float *T1, const float *T2, float fx, float fy, float cx, float cy, float *F12)
{
    // R12 = R1w * R2w.t(): the transpose travels as GEMM_2_T, so the general A * Bt loop runs -- double accumulation over k in s0,
    // then s0 += s1 + s2 + s3 of three zeros, stored as (float)(s0 * alpha)
    float R12[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s0 = 0.;
            for (int k = 0; k < 3; k++) s0 += (double)T1[i * 4 + k] * (double)T2[j * 4 + k];
            s0 += (0. + 0.) + 0.;
            R12[i * 3 + j] = (float)(s0 * 1.0);
        }
    // t12 = -R12 * t2w + t1w: ONE gemm(R12, t2w, alpha = -1, t1w, beta = 1), the shortcut with len == d_size.height
    float t12[3];
    for (int i = 0; i < 3; i++) {
        const float t = f12_dot3(R12[i * 3], T2[3], R12[i * 3 + 1], T2[7], R12[i * 3 + 2], T2[11]);
        t12[i] = (float)((double)t * -1.0 + (double)T1[i * 4 + 3] * 1.0);
    }
    // SkewSymmetricMatrix (:869-874)
    const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    // K1.t().inv() and K2.inv(): cv::invert's 3x3 case on the evaluated matrices
    // (open: OpenCV's MatOp_Invert::matmul turns inv(A) * B into solve(A, B, DECOMP_LU), a float LU with three right-hand sides,
    // so the first product may differ from a real build in its last bits; nothing compiled pins this function -- DESIGN.md 8n)
    const float K1t[9] = {fx, 0.f, 0.f, 0.f, fy, 0.f, cx, cy, 1.f}, K2[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    float K1ti[9], K2i[9], A[9], B[9];
    geo_inv3(K1t, K1ti);
    geo_inv3(K2, K2i);
    // ((K1.t().inv() * t12x) * R12) * K2.inv(): left to right, three shortcut products
    f12_mul33(K1ti, tx, A);
    f12_mul33(A, R12, B);
    f12_mul33(B, K2i, F12);
}

// The epipole of keyframe 1 in keyframe 2 (src/ORBmatcher.cc:833-843): C2 = R2w * Cw + t2w with the 3x3 . 3x1 product accumulated
// left to right in float from zero, then fx * C2x * invz + cx, every operation rounded separately
GEO_HD void f12_epipole(const float *T2, const float *Ow1, float fx, float fy, float cx, float cy, float *ex, float *ey)
{
    float C2[3];
    for (int y = 0; y < 3; y++) {
        float s = 0.f;
        for (int k = 0; k < 3; k++) s = s + T2[y * 4 + k] * Ow1[k];
        C2[y] = s + T2[y * 4 + 3];
    }
    const float invz = 1.0f / C2[2];
    *ex = fx * C2[0] * invz + cx;
    *ey = fy * C2[1] * invz + cy;
}

// The baseline gate (src/LocalMapping.cc:390-411): true = the neighbour is skipped.  cv::norm accumulates the float differences
// in double and its sqrt is stored as float.  Stereo / RGB-D: baseline < mb.  Monocular: the float ratio baseline / medianDepth
// against the double 0.01.
GEO_HD bool f12_baseline_skip(const float *Ow1, const float *Ow2, int mono, float mb, float median_depth2)
{
    double s = 0.;
    for (int k = 0; k < 3; k++) {
        const float v = Ow2[k] - Ow1[k];
        s += (double)v * (double)v;
    }
    const float baseline = (float)sqrt(s);
    if (!mono) return baseline < mb;
    const float ratio = baseline / median_depth2;
    return (double)ratio < 0.01;
}
