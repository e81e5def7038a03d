// orbfe_initializer.hip -- the reference's monocular Initializer (src/Initializer.cc: Initialize, FindHomography, FindFundamental,
// ComputeH21 / F21, CheckHomography / Fundamental, ReconstructH / F, DecomposeE, CheckRT, Triangulate, Normalize) on the GPU, one
// frame pair or a batch.  The arithmetic restates tests/initializer_oracle.py operation for operation (its assumptions I1 - I10):
// float where the C++ is float, double where it is double, no FMA (-ffp-contract=off), sums in the C++ order, nothing from libm
// but IEEE sqrt and division on the paths that decide.  So every result field, the points and every tap are bit-exact against
// the oracle.  Layout: DESIGN.md section 8j.
//   k_init_prepare      one workgroup per pair: ordered compaction of the matches into (index, u1 v1 u2 v2) records, the index
//                       checks, Normalize of both key sets (four serial float sums, one lane each), T1, T2, T2inv.
//   k_init_ransac       one lane per (model, iteration), one wave per workgroup, all lanes of a workgroup on the same model.  The
//                       lane replays its eight draws, fits its model with the float Jacobi SVD on matrices kept in LDS laid out
//                       [entry][lane], and walks ALL matches in index order adding to its own score (the float sum's order is the
//                       reference's; no cross-lane sums).  The matches are staged in LDS once per workgroup and read as broadcasts.
//   k_init_reconstruct  one workgroup per pair: the winners (maximum score, first on ties, positive only), RH, the winner's inlier
//                       mask recomputed, the 3 x 3 decompositions and the 8 or 4 (R, t) on lane 0, CheckRT one lane per
//                       (hypothesis, match) with Triangulate's 4 x 4 SVD in LDS, integer counts, an exact radix selection of
//                       vCosParallax[min(50, size - 1)] one wave per hypothesis, and the final ladder on lane 0.
// The handle, its taps and create / destroy are csrc/orbfe_ransac.h.
#include <float.h>
#include <math.h>

#include "orbfe_common.h"
#include "orbfe_ransac.h"
#include "orbfe_svd.h"

namespace {

constexpr int IN_W = 64;        // k_init_ransac workgroup: one wave
constexpr int IN_T = 256;       // k_init_prepare / k_init_reconstruct workgroup
constexpr int IN_STAGE = 256;   // matches staged in LDS per pass
constexpr int IN_MAXIT = ORBFE_INIT_MAX_ITERATIONS;
constexpr int IN_HYP = 10;      // floats of a hypothesis record: score, model [9]
// tests/initializer_oracle.py I9: parallax > 1 (and >= 1) degree iff -1 <= cos <= this, derived there with the host's acosf
constexpr uint32_t IN_PARALLAX_CUT_BITS = 0x3f7ff604u;   // 0.99984765

struct InPrep {
    float mean1[2], s1[2], mean2[2], s2[2];
    float T1[9], T2[9], T2inv[9], T2t[9];
    int32_t N, status, n1, n2, o1, o2;
};

// ---- small matrix pieces (oracle I3 - I7) ---------------------------------------------------------------------------------------------
// gemm's inline path: float sums left to right, (float)(s * alpha)
__device__ inline void mm3(const float *A, const float *B, float *out, double alpha = 1.0)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float s = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
            out[3 * i + j] = (float)((double)s * alpha);
        }
}

// GEMMSingleMul<float, double>: a transposed operand, double sums from 0.0 in k order
__device__ inline void mm3_t(const float *A, const float *B, float *out, double alpha, bool ta, bool tb)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += (double)(ta ? A[3 * k + i] : A[3 * i + k]) * (double)(tb ? B[3 * j + k] : B[3 * k + j]);
            out[3 * i + j] = (float)(s * alpha);
        }
}

__device__ inline double det3d(const float *m)
{
    return (double)m[0] * ((double)m[4] * m[8] - (double)m[5] * m[7]) - (double)m[1] * ((double)m[3] * m[8] - (double)m[5] * m[6]) +
           (double)m[2] * ((double)m[3] * m[7] - (double)m[4] * m[6]);
}

// Mat::inv() of a 3 x 3 CV_32F
__device__ inline void inv3f(const float *S, float *D)
{
    double d = det3d(S);
    if (d != 0.) {
        d = 1. / d;
        D[0] = (float)(((double)S[4] * S[8] - (double)S[5] * S[7]) * d);
        D[1] = (float)(((double)S[2] * S[7] - (double)S[1] * S[8]) * d);
        D[2] = (float)(((double)S[1] * S[5] - (double)S[2] * S[4]) * d);
        D[3] = (float)(((double)S[5] * S[6] - (double)S[3] * S[8]) * d);
        D[4] = (float)(((double)S[0] * S[8] - (double)S[2] * S[6]) * d);
        D[5] = (float)(((double)S[2] * S[3] - (double)S[0] * S[5]) * d);
        D[6] = (float)(((double)S[3] * S[7] - (double)S[4] * S[6]) * d);
        D[7] = (float)(((double)S[1] * S[6] - (double)S[0] * S[7]) * d);
        D[8] = (float)(((double)S[0] * S[4] - (double)S[1] * S[3]) * d);
    } else
        for (int k = 0; k < 9; k++) D[k] = 0.0f;
}

__device__ inline double norm3d(const float *v) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

__device__ inline bool parallax_cut(float c) { return c <= __uint_as_float(IN_PARALLAX_CUT_BITS) && c >= -1.0f; }

// the eight swap-with-back / pop-back selections out of a fresh 0 .. n-1 (n >= 8) without the list (as csrc/orbfe_pnp.hip's four)
template <class PS>
__device__ inline void set_from_draws(const int32_t *d, int n, PS set)
{
    int pos[8], val[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int size = n - k;
        const int p = index_from_draw(d[k], size);
        int pick = p, back = size - 1;
#pragma unroll
        for (int e = 0; e < k; e++) {   // in the order written: the last match stays
            if (pos[e] == p) pick = val[e];
            if (pos[e] == size - 1) back = val[e];
        }
        set[k] = pick;
        pos[k] = p;
        val[k] = back;
    }
}

// ComputeH21: pt(i, u1, v1, u2, v2) gives the i-th pair of normalised points
template <class PT, class PA, class PW, class PV>
__device__ inline void compute_h21(PT pt, PA At, PW W, PV Vt, float *Hn)
{
    for (int i = 0; i < 8; i++) {
        float u1, v1, u2, v2;
        pt(i, u1, v1, u2, v2);
        const int r0 = 2 * i, r1 = 2 * i + 1;   // At is A transposed: 9 rows of 16
        At[0 * 16 + r0] = 0.0f;
        At[1 * 16 + r0] = 0.0f;
        At[2 * 16 + r0] = 0.0f;
        At[3 * 16 + r0] = -u1;
        At[4 * 16 + r0] = -v1;
        At[5 * 16 + r0] = -1.0f;
        At[6 * 16 + r0] = v2 * u1;
        At[7 * 16 + r0] = v2 * v1;
        At[8 * 16 + r0] = v2;
        At[0 * 16 + r1] = u1;
        At[1 * 16 + r1] = v1;
        At[2 * 16 + r1] = 1.0f;
        At[3 * 16 + r1] = 0.0f;
        At[4 * 16 + r1] = 0.0f;
        At[5 * 16 + r1] = 0.0f;
        At[6 * 16 + r1] = -u2 * u1;
        At[7 * 16 + r1] = -u2 * v1;
        At[8 * 16 + r1] = -u2;
    }
    // FULL_UV's seven extra rows are columns of u, which ComputeH21 never reads: n1 = n (vt is the same)
    jacobi_svd_f(At, W, Vt, 16, 9, 9);
    for (int k = 0; k < 9; k++) Hn[k] = Vt[72 + k];
}

// SVD of a 3 x 3 (FULL_UV or not: square): u, w, vt as cv::SVD::compute returns them
template <class PA, class PW, class PV>
__device__ inline void svd3(const float *A, PA At, PW W, PV Vt, float *u, float *w, float *vt)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) At[c * 3 + r] = A[3 * r + c];
    jacobi_svd_f(At, W, Vt, 3, 3, 3);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            u[3 * r + c] = At[c * 3 + r];
            vt[3 * r + c] = Vt[3 * r + c];
        }
    for (int k = 0; k < 3; k++) w[k] = (float)W[k];
}

// ComputeF21: the 8 x 9 system goes in untransposed, vt.row(8) is the refill row
template <class PT, class PA, class PW, class PV>
__device__ inline void compute_f21(PT pt, PA At, PW W, PV Vt, float *Fn)
{
    for (int i = 0; i < 8; i++) {
        float u1, v1, u2, v2;
        pt(i, u1, v1, u2, v2);
        At[i * 9 + 0] = u2 * u1;
        At[i * 9 + 1] = u2 * v1;
        At[i * 9 + 2] = u2;
        At[i * 9 + 3] = v2 * u1;
        At[i * 9 + 4] = v2 * v1;
        At[i * 9 + 5] = v2;
        At[i * 9 + 6] = u1;
        At[i * 9 + 7] = v1;
        At[i * 9 + 8] = 1.0f;
    }
    for (int k = 0; k < 9; k++) At[72 + k] = 0.0f;
    jacobi_svd_f(At, W, Vt, 9, 8, 9);
    float Fpre[9], u[9], w[3], vt[9], D[9], uD[9];
    for (int k = 0; k < 9; k++) Fpre[k] = At[72 + k];
    svd3(Fpre, At, W, Vt, u, w, vt);
    for (int k = 0; k < 9; k++) D[k] = 0.0f;
    D[0] = w[0];
    D[4] = w[1];
    D[8] = 0.0f;   // w.at<float>(2) = 0
    mm3(u, D, uD);
    mm3(uD, vt, Fn);
}

// CheckHomography's chiSquare pair for one match
__device__ inline void chi_h(const float *h, const float *g, float inv_s2, float u1, float v1, float u2, float v2, float &c1, float &c2)
{
    const float w2in1inv = (float)(1.0 / (double)(g[6] * u2 + g[7] * v2 + g[8]));
    const float u2in1 = (g[0] * u2 + g[1] * v2 + g[2]) * w2in1inv;
    const float v2in1 = (g[3] * u2 + g[4] * v2 + g[5]) * w2in1inv;
    c1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    c2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2;
}

__device__ inline void chi_f(const float *f, float inv_s2, float u1, float v1, float u2, float v2, float &c1, float &c2)
{
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2l = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2l;
    c1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1l = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1l;
    c2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
}

constexpr float IN_TH_H = 5.991f, IN_TH_F = 3.841f;

__device__ inline float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// Triangulate and cvt_scale: csrc/orbfe_svd.h (shared with CreateNewMapPoints, csrc/orbfe_newpoints.h)

struct InHyp {
    float R[9], t[3], P2[12], O2[3];
};

// what CheckRT needs of a hypothesis beyond (R, t): P2 = K * [R | t], O2 = -R.t() * t
__device__ inline void hyp_finish(const float *K, InHyp &H)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            const float m0 = j < 3 ? H.R[j] : H.t[0], m1 = j < 3 ? H.R[3 + j] : H.t[1], m2 = j < 3 ? H.R[6 + j] : H.t[2];
            H.P2[4 * i + j] = K[3 * i] * m0 + K[3 * i + 1] * m1 + K[3 * i + 2] * m2;
        }
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)H.R[3 * k + i] * (double)H.t[k];
        H.O2[i] = (float)(s * -1.0);
    }
}

// CheckRT's body for one inlier match -> the stage at which it was dropped (ORBFE_INIT_RT_*); p and cosp are what the tap shows
template <class PA, class PW, class PV>
__device__ inline int check_rt_point(float u1, float v1, float u2, float v2, const float *K, const float *P1, const InHyp &H, float th2,
                                     PA At, PW W, PV Vt, float *p, float &cosp)
{
    triangulate(u1, v1, u2, v2, P1, H.P2, At, W, Vt, p);
    cosp = 0.0f;
    if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) return ORBFE_INIT_RT_NONFINITE;
    float n1[3], n2[3];
    for (int k = 0; k < 3; k++) {
        n1[k] = p[k] - 0.0f;
        n2[k] = p[k] - H.O2[k];
    }
    const float dist1 = (float)norm3d(n1), dist2 = (float)norm3d(n2);
    const double dot = (double)n1[0] * n2[0] + (double)n1[1] * n2[1] + (double)n1[2] * n2[2];
    cosp = (float)(dot / (double)(dist1 * dist2));
    const bool near = (double)cosp < 0.99998;
    if (p[2] <= 0 && near) return ORBFE_INIT_RT_DEPTH1;
    float p2[3];
    for (int i = 0; i < 3; i++) {
        const float s = H.R[3 * i] * p[0] + H.R[3 * i + 1] * p[1] + H.R[3 * i + 2] * p[2];
        p2[i] = (float)((double)s * 1.0 + (double)H.t[i] * 1.0);
    }
    if (p2[2] <= 0 && near) return ORBFE_INIT_RT_DEPTH2;
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const float invZ1 = (float)(1.0 / (double)p[2]);
    const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
    const float e1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (e1 > th2) return ORBFE_INIT_RT_ERROR1;
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
    const float e2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (e2 > th2) return ORBFE_INIT_RT_ERROR2;
    return near ? ORBFE_INIT_RT_GOOD : ORBFE_INIT_RT_FAR;
}

// DecomposeE and the four (R, t) of ReconstructF
template <class PA, class PW, class PV>
__device__ inline int hypotheses_f(const float *F21, const float *K, PA At, PW W, PV Vt, InHyp *hyp)
{
    float KtF[9], E[9], u[9], w[3], vt[9], t[3], t2[3], Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f}, uW[9], R1[9], R2[9];
    mm3_t(K, F21, KtF, 1.0, true, false);
    mm3(KtF, K, E);
    svd3(E, At, W, Vt, u, w, vt);
    for (int r = 0; r < 3; r++) t[r] = u[3 * r + 2];
    const float a = (float)(1.0 / norm3d(t));
    for (int r = 0; r < 3; r++) {
        t[r] = cvt_scale(t[r], a);
        t2[r] = cvt_scale(t[r], -1.0f);
    }
    mm3(u, Wm, uW);
    mm3(uW, vt, R1);
    if (det3d(R1) < 0)
        for (int k = 0; k < 9; k++) R1[k] = cvt_scale(R1[k], -1.0f);
    mm3_t(u, Wm, uW, 1.0, false, true);
    mm3(uW, vt, R2);
    if (det3d(R2) < 0)
        for (int k = 0; k < 9; k++) R2[k] = cvt_scale(R2[k], -1.0f);
    for (int h = 0; h < 4; h++) {
        for (int k = 0; k < 9; k++) hyp[h].R[k] = (h & 1) ? R2[k] : R1[k];
        for (int k = 0; k < 3; k++) hyp[h].t[k] = h < 2 ? t[k] : t2[k];
        hyp_finish(K, hyp[h]);
    }
    return 4;
}

// the eight (R, t) of ReconstructH, or 0 at the d1/d2, d2/d3 early-out
template <class PA, class PW, class PV>
__device__ inline int hypotheses_h(const float *H21, const float *K, PA At, PW W, PV Vt, InHyp *hyp)
{
    float invK[9], iH[9], A[9], U[9], w[3], VT[9];
    inv3f(K, invK);
    mm3(invK, H21, iH);
    mm3(iH, K, A);
    svd3(A, At, W, Vt, U, w, VT);
    const float s = (float)(det3d(U) * det3d(VT));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    for (int h = 0; h < 8; h++) {
        const int i = h & 3;
        const bool second = h >= 4;
        const float sgn = (i == 0 || i == 3) ? 1.0f : -1.0f;
        float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, URp[9], tp[3];
        if (!second) {
            const float st = sgn > 0 ? aux_stheta : -aux_stheta;
            Rp[0] = ctheta;
            Rp[2] = -st;
            Rp[6] = st;
            Rp[8] = ctheta;
        } else {
            const float sp = sgn > 0 ? aux_sphi : -aux_sphi;
            Rp[0] = cphi;
            Rp[2] = sp;
            Rp[4] = -1.0f;
            Rp[6] = sp;
            Rp[8] = -cphi;
        }
        mm3(U, Rp, URp, (double)s);
        mm3(URp, VT, hyp[h].R);
        const float k = second ? d1 + d3 : d1 - d3;   // tp *= d1 -+ d3
        tp[0] = cvt_scale(x1[i], k);
        tp[1] = cvt_scale(0.0f, k);
        tp[2] = cvt_scale(second ? x3[i] : -x3[i], k);
        float t[3];
        for (int r = 0; r < 3; r++) t[r] = U[3 * r] * tp[0] + U[3 * r + 1] * tp[1] + U[3 * r + 2] * tp[2];
        const float a = (float)(1.0 / norm3d(t));
        for (int r = 0; r < 3; r++) hyp[h].t[r] = cvt_scale(t[r], a);
        hyp_finish(K, hyp[h]);
    }
    return 8;
}

struct InArgs {
    const int32_t *off1, *off2;
    const float *keys1, *keys2;
    const int32_t *matches;
    const orbfe_initializer_pair *pairs;
    const int32_t *draws;
    orbfe_initializer_result *result;
    float *P3D;
    uint8_t *tri;
    // the handle's scratch
    InPrep *prep;
    int32_t *first;    // [max_points]: index into keys1 of the compacted match
    float4 *xy;        // [max_points]: u1 v1 u2 v2 of the compacted match
    float *hyp;        // [max_sets][2][IN_MAXIT][IN_HYP]
    float4 *rt;        // [max_points][8]: p3dC1, cosParallax per (match, hypothesis)
    uint8_t *rt_stage; // [max_points][8]
    uint8_t *mask;     // [max_points]: the winner's inliers
    int max_points;
    orbfe_initializer_iter *tap_iter;   // [tap_sets][ORBFE_INIT_TAP_ITERS]
    float *tap_err;                     // [tap_sets][max_points][ORBFE_INIT_ERR_FLOATS]
    int32_t *tap_info;                  // [tap_sets][2]: iterations, matches
    int tap_sets, tap_iteration, tap_hypothesis;
};

__device__ inline void result_clear(orbfe_initializer_result *r, int status, int n_matches)
{
    int32_t *w = (int32_t *)r;
    for (int k = 0; k < (int)(sizeof(*r) / 4); k++) w[k] = 0;
    r->status = status;
    r->n_matches = n_matches;
    r->iterH = r->iterF = r->best = -1;
}

// ---- prepare ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IN_T) void k_init_prepare(InArgs a)
{
    __shared__ int sWave[IN_T / 64], sBad;
    __shared__ float sSum[4], sDev[4];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o1 = a.off1[pair], n1 = a.off1[pair + 1] - o1, o2 = a.off2[pair], n2 = a.off2[pair + 1] - o2;
    const orbfe_initializer_pair P = a.pairs[pair];
    InPrep *pr = a.prep + pair;
    const bool tapped = pair < a.tap_sets;
    if (tapped && tid == 0) {
        a.tap_info[2 * pair] = 0;
        a.tap_info[2 * pair + 1] = 0;
    }
    if (o1 < 0 || n1 < 0 || o2 < 0 || n2 < 0 || (long long)o1 + n1 > a.max_points || P.iterations < 1 || P.iterations > IN_MAXIT ||
        P.draws_offset < 0) {   // nothing but the status is written
        if (tid == 0) {
            pr->status = ORBFE_INIT_BAD_SIZES;
            pr->N = 0;
        }
        return;
    }
    if (tid == 0) sBad = 0;
    __syncthreads();
    const int32_t *m12 = a.matches + o1;
    const float *k1 = a.keys1 + 2 * (size_t)o1, *k2 = a.keys2 + 2 * (size_t)o2;
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += IN_T) {   // mvMatches12: the matched keys in index order
        const int i = i0 + tid;
        int m = -1;
        if (i < n1) {
            m = m12[i];
            if (m >= n2) {
                sBad = 1;
                m = -1;
            }
        }
        const bool keep = m >= 0;
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1));
        if (lane == 0) sWave[wave] = __popcll(b);
        __syncthreads();
        int wbase = 0, total = 0;
        for (int w = 0; w < IN_T / 64; w++) {
            if (w < wave) wbase += sWave[w];
            total += sWave[w];
        }
        if (keep) {
            const int dst = o1 + base + wbase + before;
            a.first[dst] = i;
            a.xy[dst] = make_float4(k1[2 * (size_t)i], k1[2 * (size_t)i + 1], k2[2 * (size_t)m], k2[2 * (size_t)m + 1]);
        }
        base += total;
        __syncthreads();
    }
    // Normalize over ALL keys of a frame: four float sums in index order, one lane each; then the four absolute moments
    if (tid < 4) {
        const float *k = tid < 2 ? k1 : k2;
        const int n = tid < 2 ? n1 : n2, c = tid & 1;
        float s = 0;
        for (int i = 0; i < n; i++) s += k[2 * (size_t)i + c];
        sSum[tid] = s / n;
    }
    __syncthreads();
    if (tid < 4) {
        const float *k = tid < 2 ? k1 : k2;
        const int n = tid < 2 ? n1 : n2, c = tid & 1;
        const float mean = sSum[tid];
        float s = 0;
        for (int i = 0; i < n; i++) s += fabsf(k[2 * (size_t)i + c] - mean);
        s = s / n;
        sDev[tid] = (float)(1.0 / (double)s);
    }
    __syncthreads();
    if (tid == 0) {
        for (int c = 0; c < 2; c++) {
            pr->mean1[c] = sSum[c];
            pr->s1[c] = sDev[c];
            pr->mean2[c] = sSum[2 + c];
            pr->s2[c] = sDev[2 + c];
        }
        float T1[9] = {sDev[0], 0.0f, -sSum[0] * sDev[0], 0.0f, sDev[1], -sSum[1] * sDev[1], 0.0f, 0.0f, 1.0f};
        float T2[9] = {sDev[2], 0.0f, -sSum[2] * sDev[2], 0.0f, sDev[3], -sSum[3] * sDev[3], 0.0f, 0.0f, 1.0f};
        float T2inv[9];
        inv3f(T2, T2inv);
        for (int k = 0; k < 9; k++) {
            pr->T1[k] = T1[k];
            pr->T2[k] = T2[k];
            pr->T2inv[k] = T2inv[k];
            pr->T2t[k] = T2[3 * (k % 3) + k / 3];
        }
        pr->N = base;
        pr->n1 = n1;
        pr->n2 = n2;
        pr->o1 = o1;
        pr->o2 = o2;
        pr->status = sBad ? ORBFE_INIT_BAD_INDEX : base < 8 ? ORBFE_INIT_FEW_MATCHES : ORBFE_INIT_OK;
    }
}

// ---- RANSAC -------------------------------------------------------------------------------------------------------------------------
// blockIdx.x: pair; blockIdx.y: bit 0 the model (0 H, 1 F), the rest the chunk of 64 iterations
__global__ __launch_bounds__(IN_W) void k_init_ransac(InArgs a)
{
    __shared__ float sM[225 * IN_W];    // per lane At (9 x 16) and Vt (9 x 9), [entry][lane]
    __shared__ double sWd[9 * IN_W];
    __shared__ int sSet[8 * IN_W];
    __shared__ float4 sXY[IN_STAGE];
    const int pair = blockIdx.x, model = blockIdx.y & 1, lane = threadIdx.x;
    const int it = (blockIdx.y >> 1) * IN_W + lane;
    const InPrep *pr = a.prep + pair;
    if (pr->status != ORBFE_INIT_OK) return;
    const orbfe_initializer_pair P = a.pairs[pair];
    if ((int)(blockIdx.y >> 1) * IN_W >= P.iterations) return;   // uniform over the workgroup
    const bool active = it < P.iterations;
    const int N = pr->N, o1 = pr->o1;
    const float4 *xy = a.xy + o1;
    const bool tapped = pair < a.tap_sets;
    LdsLane<float, IN_W> At{sM + lane}, Vt{sM + 144 * IN_W + lane};
    LdsLane<double, IN_W> W{sWd + lane};
    LdsLane<int, IN_W> set{sSet + lane};
    float M[9], Minv[9], Mn[9];
    for (int k = 0; k < 9; k++) M[k] = Minv[k] = Mn[k] = 0.0f;
    if (active) {
        set_from_draws(a.draws + P.draws_offset + 8 * (size_t)it, N, set);
        const float m1x = pr->mean1[0], m1y = pr->mean1[1], s1x = pr->s1[0], s1y = pr->s1[1];
        const float m2x = pr->mean2[0], m2y = pr->mean2[1], s2x = pr->s2[0], s2y = pr->s2[1];
        auto pt = [&](int i, float &u1, float &v1, float &u2, float &v2) {
            const float4 q = xy[set[i]];
            u1 = (q.x - m1x) * s1x;
            v1 = (q.y - m1y) * s1y;
            u2 = (q.z - m2x) * s2x;
            v2 = (q.w - m2y) * s2y;
        };
        float tmp[9];
        if (model == 0) {
            compute_h21(pt, At, W, Vt, Mn);
            mm3(pr->T2inv, Mn, tmp);
            mm3(tmp, pr->T1, M);
            inv3f(M, Minv);
        } else {
            compute_f21(pt, At, W, Vt, Mn);
            mm3(pr->T2t, Mn, tmp);
            mm3(tmp, pr->T1, M);
        }
    }
    // the score: every lane walks all matches in index order; a staged match is read by all lanes at once (an LDS broadcast)
    const float inv_s2 = inv_sigma_square(P.sigma);
    const bool tap_chi = tapped && active && it == a.tap_iteration;
    float *tap_err = tap_chi ? a.tap_err + (size_t)pair * a.max_points * ORBFE_INIT_ERR_FLOATS + 2 * model : nullptr;
    float score = 0;
    for (int base = 0; base < N; base += IN_STAGE) {
        const int cnt = min(IN_STAGE, N - base);
        __syncthreads();
        for (int q = lane; q < cnt; q += IN_W) sXY[q] = xy[base + q];
        __syncthreads();
        if (active)
            for (int q = 0; q < cnt; q++) {
                const float4 m = sXY[q];
                float c1, c2;
                if (model == 0) {
                    chi_h(M, Minv, inv_s2, m.x, m.y, m.z, m.w, c1, c2);
                    if (!(c1 > IN_TH_H)) score += IN_TH_H - c1;
                    if (!(c2 > IN_TH_H)) score += IN_TH_H - c2;
                } else {
                    chi_f(M, inv_s2, m.x, m.y, m.z, m.w, c1, c2);
                    if (!(c1 > IN_TH_F)) score += IN_TH_H - c1;   // thScore = 5.991
                    if (!(c2 > IN_TH_F)) score += IN_TH_H - c2;
                }
                if (tap_chi) {
                    tap_err[(size_t)(base + q) * ORBFE_INIT_ERR_FLOATS] = c1;
                    tap_err[(size_t)(base + q) * ORBFE_INIT_ERR_FLOATS + 1] = c2;
                }
            }
    }
    if (!active) return;
    float *rec = a.hyp + (((size_t)pair * 2 + model) * IN_MAXIT + it) * IN_HYP;
    rec[0] = score;
    for (int k = 0; k < 9; k++) rec[1 + k] = M[k];
    if (tapped && it < ORBFE_INIT_TAP_ITERS) {
        orbfe_initializer_iter *ti = a.tap_iter + (size_t)pair * ORBFE_INIT_TAP_ITERS + it;
        if (model == 0) {
            for (int k = 0; k < 8; k++) ti->set[k] = set[k];
            for (int k = 0; k < 9; k++) {
                ti->Hn[k] = Mn[k];
                ti->H21i[k] = M[k];
            }
            ti->scoreH = score;
            ti->reserved[0] = ti->reserved[1] = 0;
        } else {
            for (int k = 0; k < 9; k++) {
                ti->Fn[k] = Mn[k];
                ti->F21i[k] = M[k];
            }
            ti->scoreF = score;
        }
    }
}

// ---- reconstruction -------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t order_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

__global__ __launch_bounds__(IN_T) void k_init_reconstruct(InArgs a)
{
    __shared__ float sM[32 * IN_T];   // per lane At and Vt of the 4 x 4 (and 3 x 3) SVDs, [entry][lane]
    __shared__ double sWd[4 * IN_T];
    __shared__ InHyp sHyp[8];
    __shared__ float sBestM[2][9], sBestS[2], sInv[9], sP1[12], sSel[8];
    __shared__ int sBestI[2], sModel, sNhyp, sInl, sGood[8], sCos[8], sBest, sOk;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const InPrep *pr = a.prep + pair;
    orbfe_initializer_result *res = a.result + pair;
    const int status = pr->status;
    if (status != ORBFE_INIT_OK) {   // nothing but the result is written
        if (tid == 0) result_clear(res, status, pr->N);
        return;
    }
    const orbfe_initializer_pair P = a.pairs[pair];
    const int N = pr->N, o1 = pr->o1, n1 = pr->n1;
    const float4 *xy = a.xy + o1;
    const int32_t *first = a.first + o1;
    uint8_t *mask = a.mask + o1;
    float4 *rt = a.rt + 8 * (size_t)o1;
    uint8_t *rt_stage = a.rt_stage + 8 * (size_t)o1;
    float *P3D = a.P3D + 3 * (size_t)o1;
    uint8_t *tri = a.tri + o1;
    const bool tapped = pair < a.tap_sets;
    LdsLane<float, IN_T> At{sM + tid}, Vt{sM + 16 * IN_T + tid};
    LdsLane<double, IN_T> W{sWd + tid};
    // vP3D / vbTriangulated of a failed Initialize: zeros
    for (int i = tid; i < n1; i += IN_T) {
        P3D[3 * (size_t)i] = P3D[3 * (size_t)i + 1] = P3D[3 * (size_t)i + 2] = 0.0f;
        tri[i] = 0;
    }
    // the winners: `if (currentScore > score)` from score = 0, in iteration order
    if (tid == 0 || tid == 64) {
        const int model = tid >> 6;
        const float *rec = a.hyp + ((size_t)pair * 2 + model) * IN_MAXIT * IN_HYP;
        float score = 0;
        int best = -1;
        for (int it = 0; it < P.iterations; it++) {
            const float s = rec[(size_t)it * IN_HYP];
            if (s > score) {
                score = s;
                best = it;
            }
        }
        sBestS[model] = score;
        sBestI[model] = best;
        for (int k = 0; k < 9; k++) sBestM[model][k] = best >= 0 ? rec[(size_t)best * IN_HYP + 1 + k] : 0.0f;
    }
    if (tid == 0) {
        sInl = 0;
        sNhyp = 0;
        for (int h = 0; h < 8; h++) {
            sGood[h] = sCos[h] = 0;
            sSel[h] = 0.0f;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float SH = sBestS[0], SF = sBestS[1];
        const float RH = SH / (SH + SF);
        const bool use_h = (double)RH > 0.40;
        sModel = (use_h ? sBestI[0] : sBestI[1]) < 0 ? 0 : use_h ? 1 : 2;
        if (sModel == 1) inv3f(sBestM[0], sInv);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) sP1[4 * i + j] = j < 3 ? P.K[3 * i + j] : 0.0f;
    }
    __syncthreads();
    const int model = sModel;
    if (model != 0) {
        // the winner's inliers, recomputed from its model
        const float inv_s2 = inv_sigma_square(P.sigma);
        for (int q0 = 0; q0 < N; q0 += IN_T) {
            const int q = q0 + tid;
            bool in = false;
            if (q < N) {
                const float4 m = xy[q];
                float c1, c2;
                if (model == 1) {
                    chi_h(sBestM[0], sInv, inv_s2, m.x, m.y, m.z, m.w, c1, c2);
                    in = !(c1 > IN_TH_H) && !(c2 > IN_TH_H);
                } else {
                    chi_f(sBestM[1], inv_s2, m.x, m.y, m.z, m.w, c1, c2);
                    in = !(c1 > IN_TH_F) && !(c2 > IN_TH_F);
                }
                mask[q] = in;
            }
            const unsigned long long b = __ballot(in);
            if (lane == 0 && b) atomicAdd(&sInl, __popcll(b));
        }
        if (tid == 0) sNhyp = model == 1 ? hypotheses_h(sBestM[0], P.K, At, W, Vt, sHyp) : hypotheses_f(sBestM[1], P.K, At, W, Vt, sHyp);
    }
    __syncthreads();
    const int nh = sNhyp;
    const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));
    const bool tap_rt = tapped && a.tap_hypothesis < nh;
    if (tapped && !tap_rt)   // that hypothesis does not exist: its part of the tap reads as zeros
        for (int q = tid; q < N; q += IN_T)
            for (int k = 4; k < ORBFE_INIT_ERR_FLOATS; k++) a.tap_err[((size_t)pair * a.max_points + q) * ORBFE_INIT_ERR_FLOATS + k] = 0.0f;
    // CheckRT: one lane per (hypothesis, match); the counts are integers
    for (int h = 0; h < nh; h++)
        for (int q0 = 0; q0 < N; q0 += IN_T) {
            const int q = q0 + tid;
            int stage = ORBFE_INIT_RT_OUTLIER;
            if (q < N) {
                float p[3] = {0.0f, 0.0f, 0.0f}, cosp = 0.0f;
                if (mask[q]) {
                    const float4 m = xy[q];
                    stage = check_rt_point(m.x, m.y, m.z, m.w, P.K, sP1, sHyp[h], th2, At, W, Vt, p, cosp);
                }
                rt[8 * (size_t)q + h] = make_float4(p[0], p[1], p[2], cosp);
                rt_stage[8 * (size_t)q + h] = (uint8_t)stage;
                if (tap_rt && h == a.tap_hypothesis) {
                    float *te = a.tap_err + ((size_t)pair * a.max_points + q) * ORBFE_INIT_ERR_FLOATS + 4;
                    te[0] = p[0];
                    te[1] = p[1];
                    te[2] = p[2];
                    te[3] = cosp;
                    te[4] = (float)stage;
                }
            }
            const unsigned long long bg = __ballot(stage == ORBFE_INIT_RT_GOOD), bc = __ballot(stage >= ORBFE_INIT_RT_FAR);
            if (lane == 0) {
                if (bg) atomicAdd(&sGood[h], __popcll(bg));
                if (bc) atomicAdd(&sCos[h], __popcll(bc));
            }
        }
    __syncthreads();
    // vCosParallax[min(50, size - 1)] after the sort: an exact selection by the bits of the float, most significant first, one wave
    // per hypothesis; the counts of a wave come from its ballots
    for (int h = wave; h < nh; h += IN_T / 64) {
        if (sGood[h] <= 0) continue;   // parallax = 0, nothing sorted
        int k = min(50, sCos[h] - 1);
        uint32_t prefix = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t high = bit == 31 ? 0u : ~0u << (bit + 1);
            int zeros = 0;
            for (int q0 = 0; q0 < N; q0 += 64) {
                const int q = q0 + lane;
                bool z = false;
                if (q < N && rt_stage[8 * (size_t)q + h] >= ORBFE_INIT_RT_FAR) {
                    const uint32_t key = order_key(rt[8 * (size_t)q + h].w);
                    z = (key & high) == prefix && !(key >> bit & 1u);
                }
                zeros += __popcll(__ballot(z));
            }
            if (k >= zeros) {
                k -= zeros;
                prefix |= 1u << bit;
            }
        }
        if (lane == 0) sSel[h] = __uint_as_float((prefix & 0x80000000u) ? prefix & 0x7fffffffu : ~prefix);
    }
    __syncthreads();
    if (tid == 0) {
        result_clear(res, model == 0 ? ORBFE_INIT_NO_MODEL : ORBFE_INIT_OK, N);
        res->model = model;
        res->SH = sBestS[0];
        res->SF = sBestS[1];
        res->iterH = sBestI[0];
        res->iterF = sBestI[1];
        for (int k = 0; k < 9; k++) {
            res->H21[k] = sBestM[0][k];
            res->F21[k] = sBestM[1][k];
        }
        res->n_hyp = nh;
        res->n_inliers = sInl;
        int best = -1, second = 0, ok = 0;
        if (nh > 0) {
            const int Nin = sInl;
            for (int h = 0; h < nh; h++) {
                res->nGood[h] = sGood[h];
                res->n_cos[h] = sCos[h];
                res->sel_cos[h] = sSel[h];
            }
            int bestGood = 0;
            if (model == 1) {
                for (int h = 0; h < 8; h++) {
                    const int g = sGood[h];
                    if (g > bestGood) {
                        second = bestGood;
                        bestGood = g;
                        best = h;
                    } else if (g > second)
                        second = g;
                }
            } else {
                for (int h = 0; h < 4; h++) bestGood = max(bestGood, sGood[h]);
                for (int h = 3; h >= 0; h--)
                    if (sGood[h] == bestGood) best = h;   // the if / else-if ladder: the first hypothesis with maxGood
                for (int h = 0; h < 4; h++)
                    if ((double)sGood[h] > 0.7 * (double)bestGood) second++;   // nsimilar
            }
            int pok = 0;
            if (best >= 0 && sGood[best] > 0) {
                res->parallax_cos = sSel[best];
                res->parallax = acosf(sSel[best]) * 180.0f / 3.14159265358979f;
                pok = parallax_cut(sSel[best]);
            }
            res->parallax_ok = pok;
            if (model == 1)
                ok = best >= 0 && (double)second < 0.75 * (double)bestGood && pok && bestGood > 50 && (double)bestGood > 0.9 * (double)Nin;
            else {
                const int nMinGood = max((int)(0.9 * (double)Nin), 50);
                ok = !(bestGood < nMinGood || second > 1) && pok;
            }
        }
        res->best = best;
        res->second = second;
        res->ok = ok;
        if (ok) {
            for (int k = 0; k < 9; k++) res->R21[k] = sHyp[best].R[k];
            for (int k = 0; k < 3; k++) res->t21[k] = sHyp[best].t[k];
        }
        sBest = best;
        sOk = ok;
        if (tapped) {
            a.tap_info[2 * pair] = P.iterations;
            a.tap_info[2 * pair + 1] = N;
        }
    }
    __syncthreads();
    if (sOk) {
        const int best = sBest;
        for (int q = tid; q < N; q += IN_T) {
            const int stage = rt_stage[8 * (size_t)q + best];
            if (stage >= ORBFE_INIT_RT_FAR) {
                const float4 p = rt[8 * (size_t)q + best];
                const int i = first[q];
                P3D[3 * (size_t)i] = p.x;
                P3D[3 * (size_t)i + 1] = p.y;
                P3D[3 * (size_t)i + 2] = p.z;
                tri[i] = stage == ORBFE_INIT_RT_GOOD;
            }
        }
    }
}

// ---- known-answer kernel ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void init_kat_sizes(int what, int *in, int *out)
{
    const int I[9] = {144, 72, 9, 16, 9, 32, 32, 28, 1}, O[9] = {9 + 256 + 81, 8 + 64 + 81, 21, 36, 9, 9, 9, 3, 1};
    *in = I[what];
    *out = O[what];
}

__global__ void k_init_kat(int what, int n, const float *in, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int id, od;
    init_kat_sizes(what, &id, &od);
    const float *x = in + (size_t)i * id;
    float *y = out + (size_t)i * od;
    float At[256], Vt[81];
    double W[9];
    auto pt = [&](int j, float &u1, float &v1, float &u2, float &v2) {
        u1 = x[2 * j];
        v1 = x[2 * j + 1];
        u2 = x[16 + 2 * j];
        v2 = x[16 + 2 * j + 1];
    };
    switch (what) {
    case ORBFE_INIT_KAT_SVD16X9:   // FULL_UV: u is 16 x 16, its last seven columns are refill rows
        for (int k = 0; k < 256; k++) At[k] = 0.0f;
        for (int r = 0; r < 16; r++)
            for (int c = 0; c < 9; c++) At[c * 16 + r] = x[r * 9 + c];
        jacobi_svd_f(At, W, Vt, 16, 9, 16);
        for (int k = 0; k < 9; k++) y[k] = (float)W[k];
        for (int r = 0; r < 16; r++)
            for (int c = 0; c < 16; c++) y[9 + r * 16 + c] = At[c * 16 + r];
        for (int k = 0; k < 81; k++) y[9 + 256 + k] = Vt[k];
        break;
    case ORBFE_INIT_KAT_SVD8X9:   // untransposed: u = Vt transposed, vt = At with the refill row 8
        for (int k = 0; k < 72; k++) At[k] = x[k];
        for (int k = 72; k < 81; k++) At[k] = 0.0f;
        jacobi_svd_f(At, W, Vt, 9, 8, 9);
        for (int k = 0; k < 8; k++) y[k] = (float)W[k];
        for (int r = 0; r < 8; r++)
            for (int c = 0; c < 8; c++) y[8 + r * 8 + c] = Vt[c * 8 + r];
        for (int k = 0; k < 81; k++) y[8 + 64 + k] = At[k];
        break;
    case ORBFE_INIT_KAT_SVD3:
    case ORBFE_INIT_KAT_SVD4: {
        const int n = what == ORBFE_INIT_KAT_SVD3 ? 3 : 4;
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) At[c * n + r] = x[r * n + c];
        jacobi_svd_f(At, W, Vt, n, n, n);
        for (int k = 0; k < n; k++) y[k] = (float)W[k];
        for (int r = 0; r < n; r++)
            for (int c = 0; c < n; c++) {
                y[n + r * n + c] = At[c * n + r];
                y[n + n * n + r * n + c] = Vt[r * n + c];
            }
        break;
    }
    case ORBFE_INIT_KAT_INV3:
        inv3f(x, y);
        break;
    case ORBFE_INIT_KAT_H21:
        compute_h21(pt, At, W, Vt, y);
        break;
    case ORBFE_INIT_KAT_F21:
        compute_f21(pt, At, W, Vt, y);
        break;
    case ORBFE_INIT_KAT_TRIANGULATE:
        triangulate(x[0], x[1], x[2], x[3], x + 4, x + 16, At, W, Vt, y);
        break;
    case ORBFE_INIT_KAT_PARALLAX:
        y[0] = parallax_cut(x[0]) ? 1.0f : 0.0f;
        break;
    }
}

}  // namespace

struct orbfe_initializer : RansacHandle {
    float *d_keys1 = nullptr, *d_P3D = nullptr, *d_hyp = nullptr;
    int32_t *d_match = nullptr, *d_first = nullptr, *d_off2 = nullptr;
    uint8_t *d_tri = nullptr, *d_rt_stage = nullptr;
    float4 *d_xy = nullptr, *d_rt = nullptr;
    InPrep *d_prep = nullptr;
    DevBuf keys2;
    int tap_hypothesis = 0;
    std::vector<OrbAlloc> blocks(size_t np)
    {
        const size_t ns = (size_t)max_sets;
        return {orb_blk(&d_keys1, np * 8), orb_blk(&d_P3D, np * 12), orb_blk(&d_hyp, ns * 2 * IN_MAXIT * IN_HYP * sizeof(float)),
                orb_blk(&d_match, np * 4), orb_blk(&d_first, np * 4), orb_blk(&d_off2, 2 * sizeof(int32_t)), orb_blk(&d_tri, np),
                orb_blk(&d_rt_stage, np * 8), orb_blk(&d_xy, np * sizeof(float4)), orb_blk(&d_rt, np * 8 * sizeof(float4)),
                orb_blk(&d_prep, ns * sizeof(InPrep))};
    }
};

// no state is carried between calls: the scaffold's state record is a placeholder
static const RansacSizes IN_SIZES = {sizeof(orbfe_initializer_pair), 16, sizeof(orbfe_initializer_result), sizeof(orbfe_initializer_iter),
                                     ORBFE_INIT_ERR_FLOATS, ORBFE_INIT_TAP_SETS, ORBFE_INIT_TAP_ITERS};

static void init_free(orbfe_initializer *h)
{
    h->keys2.release();
    ransac_free(h);
}

extern "C" orbfe_status orbfe_initializer_create(int32_t device, int32_t max_matches, int32_t max_pairs, orbfe_initializer **out)
{
    return ransac_create("orbfe_initializer_create", IN_SIZES, device, max_matches, max_pairs, out);
}

extern "C" void orbfe_initializer_destroy(orbfe_initializer *h) { orb_destroy(h, init_free); }

extern "C" void *orbfe_initializer_get_stream(orbfe_initializer *h) { return h ? (void *)h->stream : nullptr; }

// the three launches over npairs pairs; max_iterations bounds the pairs' iteration counts (the device form cannot read them)
static orbfe_status init_launch(orbfe_initializer *h, InArgs &a, int npairs, int max_iterations, hipStream_t st)
{
    a.prep = h->d_prep;
    a.first = h->d_first;
    a.xy = h->d_xy;
    a.hyp = h->d_hyp;
    a.rt = h->d_rt;
    a.rt_stage = h->d_rt_stage;
    a.mask = h->d_mask;
    a.tap_hypothesis = h->tap_hypothesis;
    ransac_bind_taps(h, a, npairs, st);
    if (npairs == 0) return ORBFE_OK;
    k_init_prepare<<<npairs, IN_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    k_init_ransac<<<dim3(npairs, 2 * ((max_iterations + IN_W - 1) / IN_W)), IN_W, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    k_init_reconstruct<<<npairs, IN_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_initializer_initialize(orbfe_initializer *h, const float *keys1_xy, int32_t n1, const float *keys2_xy,
                                                     int32_t n2, const int32_t *matches12, const float *K, float sigma, int32_t iterations,
                                                     const int32_t *draws, orbfe_initializer_result *result, float *P3D,
                                                     uint8_t *triangulated)
{
    if (!h || !keys1_xy || !keys2_xy || !matches12 || !K || !draws || !result || !P3D || !triangulated || n1 < 0 || n2 < 0) {
        orbfe_set_error("orbfe_initializer_initialize: a required pointer is NULL or a count is negative");
        return ORBFE_ERR_ARG;
    }
    if (n1 > h->max_points) {
        orbfe_set_error("%d keys exceed max_matches %d", n1, h->max_points);
        return ORBFE_ERR_ARG;
    }
    if (iterations < 1 || iterations > IN_MAXIT) {
        orbfe_set_error("%d iterations outside [1, %d]", iterations, IN_MAXIT);
        return ORBFE_ERR_ARG;
    }
    int N = 0;
    for (int i = 0; i < n1; i++) {
        if (matches12[i] >= n2) {
            orbfe_set_error("matches12[%d] = %d is past the %d keys of the second frame", i, matches12[i], n2);
            return ORBFE_ERR_ARG;
        }
        N += matches12[i] >= 0;
    }
    if (N < 8) {   // RandomInt(0, size - 1) on an emptied vector in the reference
        orbfe_set_error("%d matches: Initialize needs at least 8", N);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    hipStream_t st = h->stream;
    const size_t nd = 8 * (size_t)iterations;
    ORBFE_HIP(h->draws.ensure(nd * sizeof(int32_t)));
    ORBFE_HIP(h->keys2.ensure((n2 ? (size_t)n2 : 1) * 8));
    orbfe_initializer_pair pair = {};
    for (int k = 0; k < 9; k++) pair.K[k] = K[k];
    pair.sigma = sigma;
    pair.iterations = iterations;
    const int32_t off1[2] = {0, n1}, off2[2] = {0, n2};
    ORBFE_HIP(hipMemcpyAsync(h->d_off, off1, sizeof(off1), hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_off2, off2, sizeof(off2), hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_set, &pair, sizeof(pair), hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->draws.p, draws, nd * sizeof(int32_t), hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_keys1, keys1_xy, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
    if (n2) ORBFE_HIP(hipMemcpyAsync(h->keys2.p, keys2_xy, (size_t)n2 * 8, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(h->d_match, matches12, (size_t)n1 * 4, hipMemcpyHostToDevice, st));
    InArgs a = {};
    a.off1 = h->d_off;
    a.off2 = h->d_off2;
    a.keys1 = h->d_keys1;
    a.keys2 = h->keys2.as<float>();
    a.matches = h->d_match;
    a.pairs = (const orbfe_initializer_pair *)h->d_set;
    a.draws = h->draws.as<int32_t>();
    a.result = (orbfe_initializer_result *)h->d_result;
    a.P3D = h->d_P3D;
    a.tri = h->d_tri;
    const orbfe_status s = init_launch(h, a, 1, iterations, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(hipMemcpyAsync(result, h->d_result, sizeof(*result), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(P3D, h->d_P3D, (size_t)n1 * 12, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(triangulated, h->d_tri, (size_t)n1, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_initializer_initialize_device(orbfe_initializer *h, const int32_t *d_offsets1, const int32_t *d_offsets2,
                                                            const float *d_keys1_xy, const float *d_keys2_xy, const int32_t *d_matches12,
                                                            const orbfe_initializer_pair *d_pairs, const int32_t *d_draws, int32_t npairs,
                                                            orbfe_initializer_result *d_result, float *d_P3D, uint8_t *d_triangulated,
                                                            void *stream)
{
    if (!h || npairs < 0 ||
        (npairs > 0 && (!d_offsets1 || !d_offsets2 || !d_keys1_xy || !d_keys2_xy || !d_matches12 || !d_pairs || !d_draws || !d_result ||
                        !d_P3D || !d_triangulated))) {
        orbfe_set_error("orbfe_initializer_initialize_device: a required pointer is NULL or npairs < 0");
        return ORBFE_ERR_ARG;
    }
    if (npairs > h->max_sets) {
        orbfe_set_error("%d pairs exceed max_pairs %d", npairs, h->max_sets);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    InArgs a = {};
    a.off1 = d_offsets1;
    a.off2 = d_offsets2;
    a.keys1 = d_keys1_xy;
    a.keys2 = d_keys2_xy;
    a.matches = d_matches12;
    a.pairs = d_pairs;
    a.draws = d_draws;
    a.result = d_result;
    a.P3D = d_P3D;
    a.tri = d_triangulated;
    return init_launch(h, a, npairs, IN_MAXIT, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_initializer_set_tap_iteration(orbfe_initializer *h, int32_t iteration, int32_t hypothesis)
{
    if (!h || hypothesis < 0 || hypothesis > 7) return ORBFE_ERR_ARG;
    const orbfe_status s = ransac_set_tap_iteration(h, IN_SIZES, "orbfe_initializer_set_tap_iteration", iteration);
    if (s == ORBFE_OK) h->tap_hypothesis = hypothesis;
    return s;
}

extern "C" orbfe_status orbfe_initializer_tap(orbfe_initializer *h, int32_t pair, int32_t stage, void *dst, size_t cap, int32_t *count)
{
    if (!h || !dst || !count || stage < ORBFE_INIT_TAP_ITERATIONS || stage > ORBFE_INIT_TAP_MATCHES) return ORBFE_ERR_ARG;
    return ransac_tap(h, IN_SIZES, pair, stage == ORBFE_INIT_TAP_ITERATIONS, dst, cap, count);
}

extern "C" orbfe_status orbfe_initializer_kat(int32_t what, int32_t n, const float *in, float *out)
{
    if (n < 0 || !out || (!in && n > 0) || what < ORBFE_INIT_KAT_SVD16X9 || what > ORBFE_INIT_KAT_PARALLAX) return ORBFE_ERR_ARG;
    if (n == 0) return ORBFE_OK;
    int id = 0, od = 0;
    init_kat_sizes(what, &id, &od);
    return orb_kat_run("orbfe_initializer_kat", in, (size_t)n * id * sizeof(float), out, (size_t)n * od * sizeof(float), 0,
                       [&](void *d_in, void *d_out, void *) {
                           const unsigned T = 64, B = (unsigned)((n + T - 1) / T);
                           k_init_kat<<<B, T>>>(what, n, (const float *)d_in, (float *)d_out);
                       });
}
