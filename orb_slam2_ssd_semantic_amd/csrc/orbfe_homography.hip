// orbfe_homography.hip -- cv::findHomography(src, dst, RANSAC | 0, thr) as the fork's Tracking::TrackHomo calls it
// (perfect/src/Tracking.cc:1331-1399) on the GPU.  Every step restates tests/homography_oracle.py (OpenCV 3.2's fundam.cpp,
// ptsetreg.cpp, levmarq.cpp, lapack.cpp) operation for operation: float where the C++ uses float, double where it uses
// double, no FMA (-ffp-contract=off), sums in the C++ order, so H, the mask and every tap are bit-exact against it.
// Layout: DESIGN.md section 8c.
//   k_homo_ransac   one workgroup per point set.  Lane 0 draws the subsets of a chunk of HO_K iterations (the RNG never
//                   depends on a model), HO_K lanes fit one hypothesis each (runKernel, 9x9 Jacobi in LDS), the workgroup
//                   counts every hypothesis's inliers, then lane 0 scans the chunk in order with the serial acceptance
//                   rule and the niters update.  The best mask is recomputed from the best model.
//   k_homo_refine   one wave per set: the refit (one lane per centroid / spread sum and per LtL entry, each walking the
//                   inliers in order) and the Levenberg-Marquardt refinement (one lane per JtJ / Jtr entry and per norm).
#include <float.h>
#include <math.h>

#include "orbfe_common.h"
#include "orbfe_host.h"
#include "orbfe_jacobi.h"

namespace {

constexpr int HO_K = 32;        // hypotheses per chunk (one lane each; 2 x 81 doubles of LDS per hypothesis)
constexpr int HO_T = 256;       // k_homo_ransac workgroup
constexpr int HO_RT = 64;       // k_homo_refine workgroup (one wave)
constexpr int HO_ATTEMPTS = 10000;
constexpr int HO_LM_ITERS = 10;

enum { ST_NONE = 0, ST_RANSAC = 1, ST_FITALL = 2 };   // what k_homo_ransac left for k_homo_refine

// ---- primitives ----------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t rng_next(uint64_t &s)
{
    s = (uint64_t)(uint32_t)s * 4164903690u + (uint32_t)(s >> 32);
    return (uint32_t)s;
}

// cv_hypot and jacobi<N> (lapack.cpp's hypot template and JacobiImpl_, oracle H3 / H8): orbfe_jacobi.h

__device__ inline int update_num_iters(double p, double ep, int model_points, int max_iters)
{
    p = fmax(p, 0.);   // MAX / MIN of finite values
    p = fmin(p, 1.);
    ep = fmax(ep, 0.);
    ep = fmin(ep, 1.);
    double num = fmax(1. - p, DBL_MIN);
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// the end of runKernel: V8 de-normalised by the two 3x3 products, then convertTo(1./H22) (oracle H7)
__device__ inline void denormalise(const double *V8, const double inv[9], const double hn2[9], double *H, int hst)
{
    double T[9], H0[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            T[3 * i + j] = (inv[3 * i] * V8[j] + inv[3 * i + 1] * V8[3 + j]) + inv[3 * i + 2] * V8[6 + j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) H0[3 * i + j] = (T[3 * i] * hn2[j] + T[3 * i + 1] * hn2[3 + j]) + T[3 * i + 2] * hn2[6 + j];
    double scale = 1. / H0[8];
    bool copy = fabs(scale - 1) < DBL_EPSILON;
    for (int e = 0; e < 9; e++) H[e * hst] = copy ? H0[e] : H0[e] * scale + 0.0;
}

// one row pair of runKernel's L matrix
__device__ inline void l_rows(double x, double y, double X, double Y, double Lx[9], double Ly[9])
{
    Lx[0] = X; Lx[1] = Y; Lx[2] = 1; Lx[3] = 0; Lx[4] = 0; Lx[5] = 0; Lx[6] = -x * X; Lx[7] = -x * Y; Lx[8] = -x;
    Ly[0] = 0; Ly[1] = 0; Ly[2] = 0; Ly[3] = X; Ly[4] = Y; Ly[5] = 1; Ly[6] = -y * X; Ly[7] = -y * Y; Ly[8] = -y;
}

// runKernel on a 4-point subset, in one lane; A / V / W strided by st.  False when a spread is below DBL_EPSILON.
__device__ bool run_kernel4(const float2 *M, const float2 *m, double *A, double *V, double *W, int st, double *H, int hst)
{
    const int count = 4;
    double cmx = 0, cmy = 0, cMx = 0, cMy = 0, smx = 0, smy = 0, sMx = 0, sMy = 0;
    for (int i = 0; i < count; i++) {
        cmx += m[i].x; cmy += m[i].y;
        cMx += M[i].x; cMy += M[i].y;
    }
    cmx /= count; cmy /= count; cMx /= count; cMy /= count;
    for (int i = 0; i < count; i++) {
        smx += fabs(m[i].x - cmx);
        smy += fabs(m[i].y - cmy);
        sMx += fabs(M[i].x - cMx);
        sMy += fabs(M[i].y - cMy);
    }
    if (fabs(smx) < DBL_EPSILON || fabs(smy) < DBL_EPSILON || fabs(sMx) < DBL_EPSILON || fabs(sMy) < DBL_EPSILON) return false;
    smx = count / smx; smy = count / smy; sMx = count / sMx; sMy = count / sMy;
    for (int e = 0; e < 81; e++) A[e * st] = 0;
    for (int i = 0; i < count; i++) {
        double x = (m[i].x - cmx) * smx, y = (m[i].y - cmy) * smy;
        double X = (M[i].x - cMx) * sMx, Y = (M[i].y - cMy) * sMy;
        double Lx[9], Ly[9];
        l_rows(x, y, X, Y, Lx, Ly);
        for (int j = 0; j < 9; j++)
            for (int k = j; k < 9; k++) A[(9 * j + k) * st] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
    }
    for (int j = 0; j < 9; j++)
        for (int k = 0; k < j; k++) A[(9 * j + k) * st] = A[(9 * k + j) * st];
    jacobi<9>(A, W, V, st);
    const double inv[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
    const double hn2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
    double V8[9];
    for (int e = 0; e < 9; e++) V8[e] = V[(72 + e) * st];
    denormalise(V8, inv, hn2, H, hst);
    return true;
}

// haveCollinearPoints(ms, 4): the last point against the lines through pairs of the first three (oracle H1)
__device__ inline bool collinear4(const float2 *p)
{
    const int i = 3;
    for (int j = 0; j < i; j++) {
        double dx1 = p[j].x - p[i].x;   // float differences, widened
        double dy1 = p[j].y - p[i].y;
        for (int k = 0; k < j; k++) {
            double dx2 = p[k].x - p[i].x;
            double dy2 = p[k].y - p[i].y;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

// getSubset(maxAttempts 10000), checkPartialSubsets false: the four indices, or false
__device__ bool get_subset(const float2 *src, const float2 *dst, int count, uint64_t &rng, int idx[4])
{
    int iters = 0, i = 0;
    for (; iters < HO_ATTEMPTS; iters++) {
        for (i = 0; i < 4 && iters < HO_ATTEMPTS;) {
            int idx_i;
            for (;;) {
                idx_i = idx[i] = (int)(rng_next(rng) % (uint32_t)count);
                int j;
                for (j = 0; j < i; j++)
                    if (idx_i == idx[j]) break;
                if (j == i) break;
            }
            i++;
        }
        if (i == 4) {
            float2 a[4], b[4];
            for (int t = 0; t < 4; t++) a[t] = src[idx[t]], b[t] = dst[idx[t]];
            if (collinear4(a) || collinear4(b)) continue;
        }
        break;
    }
    return i == 4 && iters < HO_ATTEMPTS;
}

// computeError in float, compared with (float)(thr*thr)
__device__ inline bool inlier(const float *Hf, float2 M, float2 m, float t)
{
    float ww = 1.f / (Hf[6] * M.x + Hf[7] * M.y + 1.f);
    float dx = (Hf[0] * M.x + Hf[1] * M.y + Hf[2]) * ww - m.x;
    float dy = (Hf[3] * M.x + Hf[4] * M.y + Hf[5]) * ww - m.y;
    return (float)(dx * dx + dy * dy) <= t;
}

struct HoArgs {
    const int32_t *off;
    const float2 *src, *dst;
    int method, max_iters, max_pairs, min_pairs;
    float t;             // (float)(thr*thr)
    double confidence;
    uint8_t *mask;       // CSR, like the points
    double *H;           // [nsets][9]
    int32_t *ok;         // [nsets]
    int32_t *state;      // [nsets] ST_*
    double *tap_ransac;  // [nsets][9]
    double *tap_refit;   // [nsets][9]
    int32_t *tap_info;   // [nsets][4]: ransac result, iterations run, final niters, refit accepted
};

// ---- RANSAC -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HO_T) void k_homo_ransac(HoArgs a)
{
    __shared__ double sA[81 * HO_K], sV[81 * HO_K], sW[9 * HO_K];
    __shared__ double sH[HO_K][9], best[9];
    __shared__ float sHf[HO_K][8];
    __shared__ int sIdx[HO_K][4], sFit[HO_K], sCnt[HO_K];
    __shared__ int sDrawn, sDone, sResult, sIter, sNiters;
    const int set = blockIdx.x, tid = threadIdx.x;
    const int o = a.off[set], n = a.off[set + 1] - o;
    const float2 *src = a.src + o, *dst = a.dst + o;
    uint8_t *mask = a.mask + o;
    if (tid < 9) a.tap_ransac[set * 9 + tid] = 0;
    if (tid == 0) {
        a.tap_info[set * 4 + 0] = 0;
        a.tap_info[set * 4 + 1] = 0;
        a.tap_info[set * 4 + 2] = 0;
    }
    if (n < 4 || n > a.max_pairs) {   // oracle H6: no model
        if (tid == 0) a.state[set] = ST_NONE;
        if (n > 0 && n <= a.max_pairs)
            for (int i = tid; i < n; i += HO_T) mask[i] = 0;
        return;
    }
    if (a.method == 0 || n == 4) {
        for (int i = tid; i < n; i += HO_T) mask[i] = 1;
        if (tid == 0) a.state[set] = ST_FITALL;
        return;
    }
    uint64_t rng = ~(uint64_t)0;   // lane 0's RNG((uint64)-1)
    int maxGood = 0;               // lane 0's
    if (tid == 0) {
        sDone = 0;
        sResult = 0;
        sIter = 0;
        sNiters = a.max_iters > 1 ? a.max_iters : 1;
    }
    __syncthreads();
    for (int base = 0; !sDone; base += HO_K) {
        // lane 0: the subsets of iterations [base, base + HO_K) (none past the current niters, none after a failed draw)
        if (tid == 0) {
            int k = 0, lim = min(HO_K, sNiters - base);
            for (; k < lim; k++) {
                if (!get_subset(src, dst, n, rng, sIdx[k])) {
                    sIdx[k][0] = -1;
                    k++;
                    break;
                }
            }
            sDrawn = k;
        }
        __syncthreads();
        if (tid < HO_K) {
            int ok = 0;
            if (tid < sDrawn && sIdx[tid][0] >= 0) {
                float2 M[4], m[4];
                for (int t = 0; t < 4; t++) M[t] = src[sIdx[tid][t]], m[t] = dst[sIdx[tid][t]];
                ok = run_kernel4(M, m, sA + tid, sV + tid, sW + tid, HO_K, &sH[tid][0], 1);
                if (ok)
                    for (int e = 0; e < 8; e++) sHf[tid][e] = (float)sH[tid][e];
            }
            sFit[tid] = ok;
            sCnt[tid] = 0;
        }
        __syncthreads();
        // inlier counts: integer sums, any order
        for (int h = 0; h < sDrawn; h++) {
            if (!sFit[h]) continue;
            int c = 0;
            for (int i = tid; i < n; i += HO_T) c += inlier(sHf[h], src[i], dst[i], a.t);
            if (c) atomicAdd(&sCnt[h], c);
        }
        __syncthreads();
        // lane 0: the serial loop over the chunk
        if (tid == 0) {
            int it = base;
            for (int h = 0; h < sDrawn; h++, it++) {
                if (it >= sNiters) break;
                if (sIdx[h][0] < 0) {
                    if (it == 0) sResult = -1;
                    sDone = 1;
                    break;
                }
                if (!sFit[h]) continue;
                int good = sCnt[h];
                if (good > max(maxGood, 3)) {
                    for (int e = 0; e < 9; e++) best[e] = sH[h][e];
                    maxGood = good;
                    sNiters = update_num_iters(a.confidence, (double)(n - good) / n, 4, sNiters);
                }
            }
            sIter = it;
            if (it >= sNiters) sDone = 1;
            if (sDone && sResult == 0 && maxGood > 0) sResult = 1;
        }
        __syncthreads();
    }
    const bool ok = sResult == 1;
    if (ok) {
        float Hf[8];
        for (int e = 0; e < 8; e++) Hf[e] = (float)best[e];
        for (int i = tid; i < n; i += HO_T) mask[i] = inlier(Hf, src[i], dst[i], a.t);
    } else {
        for (int i = tid; i < n; i += HO_T) mask[i] = 0;
    }
    if (tid < 9 && ok) a.tap_ransac[set * 9 + tid] = best[tid];
    if (tid == 0) {
        a.state[set] = ok ? ST_RANSAC : ST_NONE;
        a.tap_info[set * 4 + 0] = ok;
        a.tap_info[set * 4 + 1] = sIter;
        a.tap_info[set * 4 + 2] = sNiters;
    }
}

// ---- refit + LM ----------------------------------------------------------------------------------------------------------
// HomographyRefineCallback::compute for one point: the two residuals and the two rows of J
__device__ inline void refine_point(const double *h, float2 Mp, float2 mp, double r[2], double J0[8], double J1[8])
{
    double Mx = Mp.x, My = Mp.y;
    double ww = h[6] * Mx + h[7] * My + 1.;
    ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
    double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
    double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
    r[0] = xi - mp.x;
    r[1] = yi - mp.y;
    if (J0) {
        J0[0] = Mx * ww; J0[1] = My * ww; J0[2] = ww; J0[3] = 0; J0[4] = 0; J0[5] = 0; J0[6] = -Mx * ww * xi; J0[7] = -My * ww * xi;
        J1[0] = 0; J1[1] = 0; J1[2] = 0; J1[3] = Mx * ww; J1[4] = My * ww; J1[5] = ww; J1[6] = -Mx * ww * yi; J1[7] = -My * ww * yi;
    }
}

// normL2Sqr_ of the residual vector (x, y interleaved), unrolled by four as OpenCV's, in one lane
__device__ double res_l2sqr(const double *h, const float2 *src, const float2 *dst, const uint8_t *mask, int n)
{
    double s = 0, q[4];
    int nq = 0;
    for (int i = 0; i < n; i++) {
        if (!mask[i]) continue;
        double r[2];
        refine_point(h, src[i], dst[i], r, nullptr, nullptr);
        q[nq++] = r[0];
        q[nq++] = r[1];
        if (nq == 4) {
            s += q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            nq = 0;
        }
    }
    for (int t = 0; t < nq; t++) s += q[t] * q[t];
    return s;
}

__device__ inline double dot8(const double *a, const double *b)
{
    double r = 0;
    for (int i = 0; i < 8; i += 4) r += a[i] * b[i] + a[i + 1] * b[i + 1] + a[i + 2] * b[i + 2] + a[i + 3] * b[i + 3];
    return r;
}

__global__ __launch_bounds__(HO_RT) void k_homo_refine(HoArgs a)
{
    __shared__ double sA[81], sV[81], sW[9];
    __shared__ double sum[8], H[9];
    __shared__ double x[8], xd[8], d[8], v[8], JA[64], Ap[64], D[8], sS, sSd, sRinf;
    __shared__ int sCount, sFlag, sCont;
    const int set = blockIdx.x, tid = threadIdx.x;
    const int o = a.off[set], n = a.off[set + 1] - o;
    const int state = a.state[set];
    const float2 *src = a.src + o, *dst = a.dst + o;
    const uint8_t *mask = a.mask + o;
    if (tid < 9) a.tap_refit[set * 9 + tid] = 0;
    if (state == ST_NONE) {
        if (tid < 9) a.H[set * 9 + tid] = 0;
        if (tid == 0) {
            a.ok[set] = 0;
            a.tap_info[set * 4 + 3] = 0;
        }
        return;
    }
    if (tid < 9 && state == ST_RANSAC) H[tid] = a.tap_ransac[set * 9 + tid];
    // ---- runKernel over the mask's points (the refit of RANSAC, or method 0 / n == 4 on all points)
    if (state == ST_FITALL || n > 4) {
        if (tid < 4) {   // centroids: cm.x, cm.y (dst), cM.x, cM.y (src)
            const float2 *p = tid < 2 ? dst : src;
            double s = 0;
            int c = 0;
            for (int i = 0; i < n; i++)
                if (mask[i]) s += (tid & 1) ? p[i].y : p[i].x, c++;
            sum[tid] = s / c;
            if (tid == 0) sCount = c;
        }
        __syncthreads();
        const int count = sCount;
        if (tid < 4) {   // spreads
            const float2 *p = tid < 2 ? dst : src;
            double cen = sum[tid], s = 0;
            for (int i = 0; i < n; i++)
                if (mask[i]) s += fabs(((tid & 1) ? p[i].y : p[i].x) - cen);
            sum[4 + tid] = s;
        }
        __syncthreads();
        const double cmx = sum[0], cmy = sum[1], cMx = sum[2], cMy = sum[3];
        const bool fit = !(fabs(sum[4]) < DBL_EPSILON || fabs(sum[5]) < DBL_EPSILON || fabs(sum[6]) < DBL_EPSILON ||
                           fabs(sum[7]) < DBL_EPSILON);
        if (fit) {
            const double smx = count / sum[4], smy = count / sum[5], sMx = count / sum[6], sMy = count / sum[7];
            if (tid < 45) {   // LtL entry (j, k), k >= j, over the inliers in order
                int j = 0, r = tid;
                while (r >= 9 - j) r -= 9 - j, j++;
                const int k = j + r;
                double s = 0;
                for (int i = 0; i < n; i++) {
                    if (!mask[i]) continue;
                    double xx = (dst[i].x - cmx) * smx, yy = (dst[i].y - cmy) * smy;
                    double X = (src[i].x - cMx) * sMx, Y = (src[i].y - cMy) * sMy;
                    double Lx[9], Ly[9];
                    l_rows(xx, yy, X, Y, Lx, Ly);
                    s += Lx[j] * Lx[k] + Ly[j] * Ly[k];
                }
                sA[9 * j + k] = s;
                sA[9 * k + j] = s;
            }
            __syncthreads();
            if (tid == 0) {
                jacobi<9>(sA, sW, sV, 1);
                const double inv[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
                const double hn2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
                denormalise(sV + 72, inv, hn2, H, 1);
            }
        }
        __syncthreads();
        if (tid == 0) {
            a.tap_info[set * 4 + 3] = state == ST_RANSAC && fit;
            sFlag = fit || state == ST_RANSAC;   // a failed method-0 fit is a false result; a failed refit keeps the model
        }
        if (tid < 9 && state == ST_RANSAC && fit) a.tap_refit[set * 9 + tid] = H[tid];
        __syncthreads();
        if (!sFlag) {
            if (tid < 9) a.H[set * 9 + tid] = 0;
            if (tid == 0) a.ok[set] = 0;
            for (int i = tid; i < n; i += HO_RT) a.mask[o + i] = 0;
            return;
        }
    } else if (tid == 0) {
        a.tap_info[set * 4 + 3] = 0;
    }
    // ---- LMSolverImpl::run on H[0:8] over the inliers (n > 4 only)
    if (n > 4) {
        if (tid < 8) x[tid] = H[tid];
        __syncthreads();
        // compute(x, r, J): JtJ (36 lanes), Jtr (8 lanes), ||r||^2 (one lane), ||r||_inf (one lane)
        auto jacobian_sums = [&](const double *h) {
            if (tid < 36) {
                int i = 0, r = tid;
                while (r >= 8 - i) r -= 8 - i, i++;
                const int j = i + r;
                double s = 0;
                for (int p = 0; p < n; p++) {
                    if (!mask[p]) continue;
                    double rr[2], J0[8], J1[8];
                    refine_point(h, src[p], dst[p], rr, J0, J1);
                    s += J0[i] * J0[j];
                    s += J1[i] * J1[j];
                }
                JA[8 * i + j] = s;
                JA[8 * j + i] = s;
            } else if (tid < 44) {
                const int i = tid - 36;
                double s = 0;
                for (int p = 0; p < n; p++) {
                    if (!mask[p]) continue;
                    double rr[2], J0[8], J1[8];
                    refine_point(h, src[p], dst[p], rr, J0, J1);
                    s += J0[i] * rr[0];
                    s += J1[i] * rr[1];
                }
                v[i] = s;
            } else if (tid == 44) {
                sS = res_l2sqr(h, src, dst, mask, n);
            } else if (tid == 45) {
                double s = 0;
                for (int p = 0; p < n; p++) {
                    if (!mask[p]) continue;
                    double rr[2];
                    refine_point(h, src[p], dst[p], rr, nullptr, nullptr);
                    for (int t = 0; t < 2; t++) {
                        double q = fabs(rr[t]);
                        s = s < q ? q : s;
                    }
                }
                sRinf = s;
            }
        };
        jacobian_sums(x);
        __syncthreads();
        if (tid < 8) D[tid] = JA[9 * tid];
        double lambda = 1, lc = 0.75;   // lane 0's
        int iter = 0;
        for (;;) {
            __syncthreads();
            if (tid == 0) {
                for (int e = 0; e < 64; e++) Ap[e] = JA[e];
                for (int i = 0; i < 8; i++) Ap[9 * i] += lambda * D[i];
                // solve(Ap, v, d, DECOMP_EIG): Jacobi, SVBkSb with nb = 1 (oracle H4)
                jacobi<8>(Ap, sW, sV, 1);
                double thr = 0;
                for (int i = 0; i < 8; i++) thr += sW[i];
                thr *= DBL_EPSILON * 2;
                for (int j = 0; j < 8; j++) d[j] = 0;
                for (int i = 0; i < 8; i++) {
                    double wi = sW[i];
                    if (fabs(wi) <= thr) continue;
                    wi = 1 / wi;
                    double s = 0;
                    for (int j = 0; j < 8; j++) s += sV[8 * i + j] * v[j];
                    s *= wi;
                    for (int j = 0; j < 8; j++) d[j] = d[j] + s * sV[8 * i + j];
                }
                for (int j = 0; j < 8; j++) xd[j] = x[j] - d[j];
                sSd = res_l2sqr(xd, src, dst, mask, n);
                double temp_d[8];
                for (int i = 0; i < 8; i++) {
                    double s = 0;
                    for (int k = 0; k < 8; k++) s += JA[8 * i + k] * d[k];
                    temp_d[i] = s * -1 + v[i] * 2;
                }
                const double S = sS, Sd = sSd;
                double dS = dot8(d, temp_d);
                double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
                if (R > 0.75) {
                    lambda *= 0.5;
                    if (lambda < lc) lambda = 0;
                } else if (R < 0.25) {
                    double t = dot8(d, v);
                    double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
                    nu = nu < 2. ? 2. : nu;
                    nu = 10. < nu ? 10. : nu;
                    if (lambda == 0) {
                        // invert(A, DECOMP_EIG): only the diagonal is read
                        for (int e = 0; e < 64; e++) Ap[e] = JA[e];
                        jacobi<8>(Ap, sW, sV, 1);
                        double thr2 = 0;
                        for (int i = 0; i < 8; i++) thr2 += sW[i];
                        thr2 *= DBL_EPSILON * 2;
                        double dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                        for (int i = 0; i < 8; i++) {
                            double wi = sW[i];
                            if (fabs(wi) <= thr2) continue;
                            wi = 1 / wi;
                            for (int r = 0; r < 8; r++) dg[r] = dg[r] + sV[8 * i + r] * (sV[8 * i + r] * wi);
                        }
                        double maxval = DBL_EPSILON;
                        for (int i = 0; i < 8; i++) {
                            double q = fabs(dg[i]);
                            maxval = maxval < q ? q : maxval;
                        }
                        lambda = lc = 1. / maxval;
                        nu *= 0.5;
                    }
                    lambda *= nu;
                }
                sFlag = Sd < S;
                if (sFlag) {
                    sS = Sd;
                    for (int j = 0; j < 8; j++) x[j] = xd[j];
                }
            }
            __syncthreads();
            if (sFlag) jacobian_sums(x);
            __syncthreads();
            if (tid == 0) {
                iter++;
                double dinf = 0;
                for (int j = 0; j < 8; j++) {
                    double q = fabs(d[j]);
                    dinf = dinf < q ? q : dinf;
                }
                sCont = iter < HO_LM_ITERS && dinf >= FLT_EPSILON && sRinf >= FLT_EPSILON;
            }
            __syncthreads();
            if (!sCont) break;
        }
        if (tid < 8) H[tid] = x[tid];
        __syncthreads();
    }
    if (tid < 9) a.H[set * 9 + tid] = H[tid];
    if (tid == 0) a.ok[set] = n > a.min_pairs;
}

// ---- known-answer kernels ------------------------------------------------------------------------------------------------
__global__ void k_homo_kat_rng(uint64_t state, int n, uint32_t *out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int i = 0; i < n; i++) out[i] = rng_next(state);
}

__global__ void k_homo_kat_hypot(int n, const double *in, double *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cv_hypot(in[2 * i], in[2 * i + 1]);
}

__global__ void k_homo_kat_iters(int n, const double *in, int32_t *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = update_num_iters(in[3 * i], in[3 * i + 1], 4, (int)in[3 * i + 2]);
}

template <int N>
__global__ void k_homo_kat_jacobi(int n, double *A, double *out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) jacobi<N>(A + (size_t)i * N * N, out + (size_t)i * (N + N * N), out + (size_t)i * (N + N * N) + N, 1);
}

}  // namespace

struct orbfe_homography {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;
    int max_pairs = 0, max_sets = 0;
    int tap_sets = 0;   // sets of the last call
    float2 *d_src = nullptr, *d_dst = nullptr;
    uint8_t *d_mask = nullptr;
    int32_t *d_off = nullptr, *d_ok = nullptr, *d_state = nullptr, *d_tap_info = nullptr;
    double *d_H = nullptr, *d_tap_ransac = nullptr, *d_tap_refit = nullptr;
};

static void homo_free(orbfe_homography *h)
{
    orb_free_all(h->stream, {h->d_src, h->d_dst, h->d_mask, h->d_off, h->d_ok, h->d_state, h->d_tap_info, h->d_H, h->d_tap_ransac, h->d_tap_refit});
}

extern "C" orbfe_status orbfe_homography_create(int32_t device, int32_t max_pairs, int32_t max_sets, orbfe_homography **out)
{
    orbfe_homography *h = nullptr;
    const orbfe_status s = orb_create_begin(&device, max_pairs, max_sets, out, &h);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(device);
    h->max_pairs = max_pairs;
    size_t np = (size_t)max_pairs, ns = (size_t)max_sets;
    const bool ok = orb_alloc_all(
        &h->stream, {orb_blk(&h->d_src, np * sizeof(float2)), orb_blk(&h->d_dst, np * sizeof(float2)), orb_blk(&h->d_mask, np),
                     orb_blk(&h->d_off, 2 * sizeof(int32_t)), orb_blk(&h->d_ok, sizeof(int32_t)), orb_blk(&h->d_H, 9 * sizeof(double)),
                     orb_blk(&h->d_state, ns * sizeof(int32_t)), orb_blk(&h->d_tap_info, ns * 4 * sizeof(int32_t)),
                     orb_blk(&h->d_tap_ransac, ns * 9 * sizeof(double)), orb_blk(&h->d_tap_refit, ns * 9 * sizeof(double))});
    return orb_create_finish(ok, "orbfe_homography_create", h, homo_free, out);
}

extern "C" void orbfe_homography_destroy(orbfe_homography *h) { orb_destroy(h, homo_free); }

extern "C" void *orbfe_homography_get_stream(orbfe_homography *h) { return h ? (void *)h->stream : nullptr; }

static orbfe_status homo_args(const orbfe_homography *h, int32_t method, double threshold, int32_t max_iters, double confidence,
                              HoArgs &a)
{
    if (method != 0 && method != ORBFE_HOMOGRAPHY_RANSAC) {
        orbfe_set_error("findHomography method %d: only 0 and RANSAC (8) are built", method);
        return ORBFE_ERR_ARG;
    }
    if (method == ORBFE_HOMOGRAPHY_RANSAC && !(confidence > 0 && confidence < 1)) {
        orbfe_set_error("RANSAC confidence %g outside (0, 1)", confidence);
        return ORBFE_ERR_ARG;
    }
    if (threshold <= 0) threshold = 3;
    a.method = method;
    a.max_iters = max_iters;
    a.max_pairs = h->max_pairs;
    a.t = (float)(threshold * threshold);
    a.confidence = confidence;
    a.state = h->d_state;
    a.tap_ransac = h->d_tap_ransac;
    a.tap_refit = h->d_tap_refit;
    a.tap_info = h->d_tap_info;
    return ORBFE_OK;
}

static orbfe_status homo_launch(orbfe_homography *h, const HoArgs &a, int nsets, hipStream_t st)
{
    h->last_stream = st;
    h->tap_sets = nsets;
    if (nsets == 0) return ORBFE_OK;
    k_homo_ransac<<<nsets, HO_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    k_homo_refine<<<nsets, HO_RT, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_find_homography(orbfe_homography *h, const float *src_xy, const float *dst_xy, int32_t n,
                                              int32_t method, double threshold, int32_t max_iters, double confidence, double *H,
                                              uint8_t *mask, int32_t *ok)
{
    if (!h || !H || !ok || n < 0 || (n > 0 && (!src_xy || !dst_xy))) return ORBFE_ERR_ARG;
    if (n > h->max_pairs) {
        orbfe_set_error("%d pairs exceed max_pairs %d", n, h->max_pairs);
        return ORBFE_ERR_ARG;
    }
    HoArgs a;
    orbfe_status s = homo_args(h, method, threshold, max_iters, confidence, a);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(h->device);
    hipStream_t st = h->stream;
    const int32_t off[2] = {0, n};
    ORBFE_HIP(hipMemcpyAsync(h->d_off, off, sizeof(off), hipMemcpyHostToDevice, st));
    if (n > 0) {
        ORBFE_HIP(hipMemcpyAsync(h->d_src, src_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
        ORBFE_HIP(hipMemcpyAsync(h->d_dst, dst_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    }
    a.off = h->d_off;
    a.src = h->d_src;
    a.dst = h->d_dst;
    a.mask = h->d_mask;
    a.H = h->d_H;
    a.ok = h->d_ok;
    a.min_pairs = -1;
    s = homo_launch(h, a, 1, st);
    if (s != ORBFE_OK) return s;
    ORBFE_HIP(hipMemcpyAsync(H, h->d_H, 9 * sizeof(double), hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(ok, h->d_ok, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (mask && n > 0) ORBFE_HIP(hipMemcpyAsync(mask, h->d_mask, (size_t)n, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_find_homographies_device(orbfe_homography *h, const int32_t *d_offsets, const float *d_src_xy,
                                                       const float *d_dst_xy, int32_t nsets, int32_t method, double threshold,
                                                       int32_t max_iters, double confidence, int32_t min_pairs, double *d_H,
                                                       int32_t *d_ok, uint8_t *d_mask, void *stream)
{
    if (!h || nsets < 0 || (nsets > 0 && (!d_offsets || !d_src_xy || !d_dst_xy || !d_H || !d_ok || !d_mask))) return ORBFE_ERR_ARG;
    if (nsets > h->max_sets) {
        orbfe_set_error("%d point sets exceed max_sets %d", nsets, h->max_sets);
        return ORBFE_ERR_ARG;
    }
    HoArgs a;
    orbfe_status s = homo_args(h, method, threshold, max_iters, confidence, a);
    if (s != ORBFE_OK) return s;
    DeviceGuard dg(h->device);
    a.off = d_offsets;
    a.src = (const float2 *)d_src_xy;
    a.dst = (const float2 *)d_dst_xy;
    a.mask = d_mask;
    a.H = d_H;
    a.ok = d_ok;
    a.min_pairs = min_pairs;
    return homo_launch(h, a, nsets, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_homography_tap(orbfe_homography *h, int32_t set, int32_t stage, void *dst, size_t cap)
{
    if (!h || !dst) return ORBFE_ERR_ARG;
    if (set < 0 || set >= h->tap_sets) return ORBFE_ERR_STATE;
    size_t need = stage == ORBFE_HOMO_TAP_INFO ? 4 * sizeof(int32_t) : 9 * sizeof(double);
    if (stage < ORBFE_HOMO_TAP_RANSAC || stage > ORBFE_HOMO_TAP_REFIT) return ORBFE_ERR_ARG;
    if (cap < need) return ORBFE_ERR_CAP;
    DeviceGuard dg(h->device);
    ORBFE_HIP(hipStreamSynchronize(h->last_stream));
    const void *srcp = stage == ORBFE_HOMO_TAP_RANSAC ? (const void *)(h->d_tap_ransac + (size_t)set * 9)
                     : stage == ORBFE_HOMO_TAP_INFO   ? (const void *)(h->d_tap_info + (size_t)set * 4)
                                                      : (const void *)(h->d_tap_refit + (size_t)set * 9);
    ORBFE_HIP(hipMemcpy(dst, srcp, need, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_homography_kat(int32_t what, int32_t n, const void *in, void *out)
{
    if (n < 0 || !out || (!in && n > 0) || what < ORBFE_HOMO_KAT_RNG || what > ORBFE_HOMO_KAT_JACOBI8) return ORBFE_ERR_ARG;
    if (n == 0) return ORBFE_OK;
    size_t in_b = 0, out_b = 0;
    switch (what) {
    case ORBFE_HOMO_KAT_RNG: in_b = sizeof(uint64_t); out_b = (size_t)n * 4; break;
    case ORBFE_HOMO_KAT_HYPOT: in_b = (size_t)n * 16; out_b = (size_t)n * 8; break;
    case ORBFE_HOMO_KAT_NUMITERS: in_b = (size_t)n * 24; out_b = (size_t)n * 4; break;
    case ORBFE_HOMO_KAT_JACOBI9: in_b = (size_t)n * 81 * 8; out_b = (size_t)n * 90 * 8; break;
    default: in_b = (size_t)n * 64 * 8; out_b = (size_t)n * 72 * 8; break;
    }
    return orb_kat_run("orbfe_homography_kat", in, in_b, out, out_b, 0, [&](void *d_in, void *d_out, void *) {
        const unsigned T = 128, B = (unsigned)((n + T - 1) / T);
        switch (what) {
        case ORBFE_HOMO_KAT_RNG: k_homo_kat_rng<<<1, 64>>>(*(const uint64_t *)in, n, (uint32_t *)d_out); break;
        case ORBFE_HOMO_KAT_HYPOT: k_homo_kat_hypot<<<B, T>>>(n, (const double *)d_in, (double *)d_out); break;
        case ORBFE_HOMO_KAT_NUMITERS: k_homo_kat_iters<<<B, T>>>(n, (const double *)d_in, (int32_t *)d_out); break;
        case ORBFE_HOMO_KAT_JACOBI9: k_homo_kat_jacobi<9><<<B, T>>>(n, (double *)d_in, (double *)d_out); break;
        default: k_homo_kat_jacobi<8><<<B, T>>>(n, (double *)d_in, (double *)d_out); break;
        }
    });
}
