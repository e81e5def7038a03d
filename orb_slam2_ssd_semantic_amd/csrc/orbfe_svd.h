// orbfe_svd.h -- OpenCV 3.2's one-sided Jacobi SVD (JacobiSVDImpl_<double>, core/src/lapack.cpp) and SVBkSb, which is what
// cvSVD, cvInvert(.., CV_SVD) and cvSolve(.., CV_SVD) resolve to on small CV_64F matrices.  Plain C++ on doubles, one operation
// at a time, for host and device alike; the files that include this are compiled with -ffp-contract=off.  Restated by
// tests/pnp_oracle.py (P1-P3); sizes up to SVD_MAX columns.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ORBFE_HD __host__ __device__
#else
#define ORBFE_HD
#endif

constexpr int SVD_MAX = 12;

// lapack.cpp's hypot template (oracle H3 / P1): no libm
ORBFE_HD inline double svd_hypot(double a, double b)
{
    a = fabs(a);
    b = fabs(b);
    if (a > b) {
        b /= a;
        return a * sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sqrt(1 + a * a);
    }
    return 0;
}

// JacobiSVDImpl_ on At (n rows of length m: the matrix transposed, m >= n), Vt n x n, W n values, n1 = n.  Afterwards the rows of
// At are the left singular vectors, the rows of Vt the right ones, W descending.
ORBFE_HD inline void jacobi_svd(double *At, double *W, double *Vt, int m, int n)
{
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * m + k];
            sd += t * t;
        }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = svd_hypot(p, beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                double *Vi = Vt + i * n, *Vj = Vt + j * n;
                for (int k = 0; k < n; k++) {
                    const double t0 = c * Vi[k] + s * Vj[k];
                    const double t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const double t = At[i * m + k];
            sd += t * t;
        }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double t = W[i];
            W[i] = W[j];
            W[j] = t;
            for (int k = 0; k < m; k++) {
                t = At[i * m + k];
                At[i * m + k] = At[j * m + k];
                At[j * m + k] = t;
            }
            for (int k = 0; k < n; k++) {
                t = Vt[i * n + k];
                Vt[i * n + k] = Vt[j * n + k];
                Vt[j * n + k] = t;
            }
        }
    }
    uint64_t rng = 0x12345678;   // cv::RNG, one per call
    for (int i = 0; i < n; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            // a null singular value: a random vector, orthogonalised against the rows before it
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) {
                rng = (uint64_t)(uint32_t)rng * 4164903690U + (uint32_t)(rng >> 32);
                At[i * m + k] = ((uint32_t)rng & 256) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) {
                const double t = At[i * m + k];
                sd += t * t;
            }
            sd = sqrt(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// JacobiSVDImpl_<float> (tests/initializer_oracle.py I1, I2): the float instantiation with OpenCV's own constants (minval =
// FLT_MIN, eps = FLT_EPSILON * 2), float rotations, double accumulators, and the n1 >= n form: At has n1 rows of length m, the first
// n take part in the sweeps, the rows from n on (columns of a FULL_UV u, or ComputeF21's vt.row(8) of the 8 x 9 system, which goes
// in untransposed) come out of the RNG refill and the two Gram-Schmidt sweeps.  W: n doubles of workspace; the float singular
// values are (float)W[i].  PA / PV / PW are anything indexable (a pointer, or LdsLane below), so that a lane's matrices can live
// in LDS laid out [entry][lane].
template <class T, int S>
struct LdsLane {
    T *p;
    ORBFE_HD T &operator[](int i) const { return p[(size_t)i * S]; }
};

template <class PA, class PW, class PV>
ORBFE_HD inline void jacobi_svd_f(PA At, PW W, PV Vt, int m, int n, int n1)
{
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const float t = At[i * m + k];
            sd += (double)t * t;
        }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)At[i * m + k] * At[j * m + k];
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = svd_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const float ai = At[i * m + k], aj = At[j * m + k];
                    const float t0 = c * ai + s * aj;
                    const float t1 = -s * ai + c * aj;
                    At[i * m + k] = t0;
                    At[j * m + k] = t1;
                    a += (double)t0 * t0;
                    b += (double)t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                for (int k = 0; k < n; k++) {
                    const float vi = Vt[i * n + k], vj = Vt[j * n + k];
                    const float t0 = c * vi + s * vj;
                    const float t1 = -s * vi + c * vj;
                    Vt[i * n + k] = t0;
                    Vt[j * n + k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) {
            const float t = At[i * m + k];
            sd += (double)t * t;
        }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i];
            W[i] = W[j];
            W[j] = tw;
            for (int k = 0; k < m; k++) {
                const float t = At[i * m + k];
                At[i * m + k] = At[j * m + k];
                At[j * m + k] = t;
            }
            for (int k = 0; k < n; k++) {
                const float t = Vt[i * n + k];
                Vt[i * n + k] = Vt[j * n + k];
                Vt[j * n + k] = t;
            }
        }
    }
    uint64_t rng = 0x12345678;   // cv::RNG, one per call
    for (int i = 0; i < n1; i++) {
        double sd = i < n ? (double)W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / m);
            for (int k = 0; k < m; k++) {
                rng = (uint64_t)(uint32_t)rng * 4164903690U + (uint32_t)(rng >> 32);
                At[i * m + k] = ((uint32_t)rng & 256) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) {
                        const float pr = At[i * m + k] * At[j * m + k];   // a float product into the double sum
                        sd += pr;
                    }
                    float asum = 0;
                    for (int k = 0; k < m; k++) {
                        const float t = (float)(At[i * m + k] - sd * At[j * m + k]);
                        At[i * m + k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] = At[i * m + k] * asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) {
                const float t = At[i * m + k];
                sd += (double)t * t;
            }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; k++) At[i * m + k] = At[i * m + k] * s;
    }
}

// convertTo with a scale: v * (float)alpha + 0.0f
ORBFE_HD inline float cvt_scale(float v, float a) { return v * a + 0.0f; }

// Initializer::Triangulate (src/Initializer.cc) and the linear triangulation of LocalMapping::CreateNewMapPoints
// (src/LocalMapping.cc:498-513): P1, P2 3 x 4 row-major, (u, v) the two observations.  x3 = vt.row(3)(0..2) / vt.row(3)(3); the
// return value is vt.row(3)(3), which CreateNewMapPoints tests against 0 before it divides (x3 is not to be used then).
template <class PA, class PW, class PV>
ORBFE_HD inline float triangulate(float u1, float v1, float u2, float v2, const float *P1, const float *P2, PA At, PW W, PV Vt, float *x3)
{
    for (int c = 0; c < 4; c++) {   // At is A transposed; a * row - row2 is addWeighted: v1 * a + v2 * (-1) + 0
        At[c * 4 + 0] = u1 * P1[8 + c] + P1[c] * -1.0f + 0.0f;
        At[c * 4 + 1] = v1 * P1[8 + c] + P1[4 + c] * -1.0f + 0.0f;
        At[c * 4 + 2] = u2 * P2[8 + c] + P2[c] * -1.0f + 0.0f;
        At[c * 4 + 3] = v2 * P2[8 + c] + P2[4 + c] * -1.0f + 0.0f;
    }
    jacobi_svd_f(At, W, Vt, 4, 4, 4);
    const float w = Vt[15];
    const float a = (float)(1.0 / (double)w);
    for (int k = 0; k < 3; k++) x3[k] = cvt_scale(Vt[12 + k], a);
    return w;
}

// cv::SVD::compute on A (m x n row-major, m >= n): At takes the transpose
ORBFE_HD inline void svd_compute(const double *A, int m, int n, double *At, double *W, double *Vt)
{
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) At[i * m + k] = A[k * n + i];
    jacobi_svd(At, W, Vt, m, n);
}

ORBFE_HD inline double svbksb_threshold(const double *W, int n)
{
    double threshold = 0;
    for (int i = 0; i < n; i++) threshold += W[i];
    return threshold * (DBL_EPSILON * 2);
}

// SVBkSb with one right-hand side: x = V * inv(w) * Ut * b over the factors jacobi_svd left (m >= n)
ORBFE_HD inline void svbksb_solve(const double *Ut, const double *W, const double *Vt, int m, int n, const double *b, double *x)
{
    const double threshold = svbksb_threshold(W, n);
    for (int j = 0; j < n; j++) x[j] = 0;
    for (int i = 0; i < n; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; j++) s += Ut[i * m + j] * b[j];
        s *= wi;
        for (int j = 0; j < n; j++) x[j] = x[j] + s * Vt[i * n + j];
    }
}

// SVBkSb without a right-hand side on a square matrix: the pseudo-inverse, n x n row-major
ORBFE_HD inline void svbksb_invert(const double *Ut, const double *W, const double *Vt, int n, double *x)
{
    const double threshold = svbksb_threshold(W, n);
    double buffer[SVD_MAX];
    for (int j = 0; j < n * n; j++) x[j] = 0;
    for (int i = 0; i < n; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        for (int j = 0; j < n; j++) buffer[j] = Ut[i * n + j] * wi;
        for (int r = 0; r < n; r++) {
            const double s = Vt[i * n + r];
            for (int j = 0; j < n; j++) x[r * n + j] = x[r * n + j] + s * buffer[j];
        }
    }
}
