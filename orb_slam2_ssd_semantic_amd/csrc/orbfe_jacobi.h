// orbfe_jacobi.h -- OpenCV 3.2's JacobiImpl_ (core/src/lapack.cpp; what cv::eigen runs on a symmetric matrix) as one device
// template on the scalar: double for the 8x8 / 9x9 systems of csrc/orbfe_homography.hip, float for the 4x4 quaternion matrix of
// csrc/orbfe_sim3.hip.  Every operation is the scalar's own (float: FLT_EPSILON, sqrtf), one at a time; the files that include
// this are compiled with -ffp-contract=off.  Restated by tests/homography_oracle.py (H3, H8) and tests/sim3_oracle.py (S4).
#pragma once
#include <float.h>
#include <math.h>

template <typename T> struct JacobiEps;
template <> struct JacobiEps<double> { static constexpr double value = DBL_EPSILON; };
template <> struct JacobiEps<float> { static constexpr float value = FLT_EPSILON; };

__device__ inline double cv_abs(double a) { return fabs(a); }
__device__ inline float cv_abs(float a) { return fabsf(a); }
__device__ inline double cv_sqrt(double a) { return sqrt(a); }
__device__ inline float cv_sqrt(float a) { return sqrtf(a); }

// lapack.cpp's hypot template (oracle H3)
template <typename T>
__device__ inline T cv_hypot(T a, T b)
{
    a = cv_abs(a);
    b = cv_abs(b);
    if (a > b) {
        b /= a;
        return a * cv_sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * cv_sqrt(1 + a * a);
    }
    return 0;
}

// JacobiImpl_ on an N x N symmetric matrix whose element e lives at A[e * st] (V likewise); W[k * st] eigenvalues, descending
template <int N, typename T>
__device__ void jacobi(T *A, T *W, T *V, int st)
{
    int indR[N], indC[N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) V[(i * N + j) * st] = i == j ? T(1) : T(0);
    auto row_max = [&](int k) {
        int m = k + 1;
        T mv = cv_abs(A[(N * k + m) * st]);
        for (int i = k + 2; i < N; i++) {
            T val = cv_abs(A[(N * k + i) * st]);
            if (mv < val) mv = val, m = i;
        }
        indR[k] = m;
    };
    auto col_max = [&](int k) {
        int m = 0;
        T mv = cv_abs(A[k * st]);
        for (int i = 1; i < k; i++) {
            T val = cv_abs(A[(N * i + k) * st]);
            if (mv < val) mv = val, m = i;
        }
        indC[k] = m;
    };
    for (int k = 0; k < N; k++) {
        W[k * st] = A[(N + 1) * k * st];
        if (k < N - 1) row_max(k);
        if (k > 0) col_max(k);
    }
    for (int iters = 0; iters < N * N * 30; iters++) {
        int k = 0;
        T mv = cv_abs(A[indR[0] * st]);
        for (int i = 1; i < N - 1; i++) {
            T val = cv_abs(A[(N * i + indR[i]) * st]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (int i = 1; i < N; i++) {
            T val = cv_abs(A[(N * indC[i] + i) * st]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        T p = A[(N * k + l) * st];
        if (cv_abs(p) <= JacobiEps<T>::value) break;
        T y = (W[l * st] - W[k * st]) * T(0.5);
        T t = cv_abs(y) + cv_hypot(p, y);
        T s = cv_hypot(p, t);
        T c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[(N * k + l) * st] = 0;
        W[k * st] -= t;
        W[l * st] += t;
        auto rot = [&](T *M, int i0, int i1) {
            T a0 = M[i0 * st], b0 = M[i1 * st];
            M[i0 * st] = a0 * c - b0 * s;
            M[i1 * st] = a0 * s + b0 * c;
        };
        for (int i = 0; i < k; i++) rot(A, N * i + k, N * i + l);
        for (int i = k + 1; i < l; i++) rot(A, N * k + i, N * i + l);
        for (int i = l + 1; i < N; i++) rot(A, N * k + i, N * l + i);
        for (int i = 0; i < N; i++) rot(V, N * k + i, N * l + i);
        for (int j = 0; j < 2; j++) {
            int idx = j == 0 ? k : l;
            if (idx < N - 1) row_max(idx);
            if (idx > 0) col_max(idx);
        }
    }
    for (int k = 0; k < N - 1; k++) {
        int m = k;
        for (int i = k + 1; i < N; i++)
            if (W[m * st] < W[i * st]) m = i;
        if (k != m) {
            T tw = W[m * st];
            W[m * st] = W[k * st];
            W[k * st] = tw;
            for (int i = 0; i < N; i++) {
                T tv = V[(N * m + i) * st];
                V[(N * m + i) * st] = V[(N * k + i) * st];
                V[(N * k + i) * st] = tv;
            }
        }
    }
}
