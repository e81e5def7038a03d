// orbfe_undistort.h -- cv::undistortPoints(src, dst, K, D, noArray(), P) of OpenCV 3.2 (cvUndistortPoints, imgproc/src/undistort.cpp)
// for one point, stated ONCE for the kernels of orbfe_frame.hip and the host bounds helper, so that the two cannot drift.
// Double arithmetic in the C++ evaluation order, nothing fused (the library is built with -ffp-contract=off), IEEE division.
// Restated in tests/undistort_oracle.py (points U1-U5 there).
#pragma once

#include <hip/hip_runtime.h>

#include "orbfe.h"

struct OrbUndistort {
    double ifx, ify, cx, cy;
    double k[14];    // zero-filled beyond the caller's ndist coefficients
    double RR[9];    // P * I (= P exactly; identity when P is absent)
    int iters;       // 5 with coefficients, 0 without (3.2 has no termination criterion)
};

// 0, 4, 5, 8, 12: the coefficient counts built here (14, the tilted model, is not)
__host__ __device__ inline bool orb_undistort_ndist_ok(int n) { return n == 0 || n == 4 || n == 5 || n == 8 || n == 12; }

// Frame.cc:752 / :786: mDistCoef.at<float>(0) == 0.0 -- no undistortion at all
__host__ __device__ inline bool orb_undistort_k1_zero(const orbfe_camera &c) { return c.ndist == 0 || c.dist[0] == 0.0f; }

// the per-call constants (cvConvert of K, D and P to double; ifx = 1./fx)
__host__ __device__ inline OrbUndistort orb_undistort_prepare(const orbfe_camera &c)
{
    OrbUndistort u;
    const double fx = (double)c.K[0], fy = (double)c.K[4];
    u.ifx = 1. / fx;
    u.ify = 1. / fy;
    u.cx = (double)c.K[2];
    u.cy = (double)c.K[5];
    for (int i = 0; i < 14; ++i) u.k[i] = 0.;
    for (int i = 0; i < c.ndist && i < 12; ++i) u.k[i] = (double)c.dist[i];
    u.iters = c.ndist > 0 ? 5 : 0;
    for (int i = 0; i < 9; ++i) u.RR[i] = c.has_P ? (double)c.P[i] : (i % 4 == 0 ? 1. : 0.);
    return u;
}

// one point: the body of cvUndistortPoints' loop.  The identity tilt step of 3.1+ (invMatTilt = I) changes no bit of a finite
// value and is left out.
__host__ __device__ inline void orb_undistort_point(const OrbUndistort &u, float xs, float ys, float *xo, float *yo)
{
    const double *k = u.k;
    double x = (double)xs, y = (double)ys;
    x = (x - u.cx) * u.ifx;
    y = (y - u.cy) * u.ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < u.iters; ++j) {
        double r2 = x * x + y * y;
        double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double *R = u.RR;
    double xx = R[0] * x + R[1] * y + R[2];
    double yy = R[3] * x + R[4] * y + R[5];
    double ww = 1. / (R[6] * x + R[7] * y + R[8]);
    *xo = (float)(xx * ww);
    *yo = (float)(yy * ww);
}
