// orbfe_epnp.h -- the reference's EPnP (src/PnPsolver.cc: compute_pose and everything under it) as plain C++ on doubles, one
// operation at a time in the reference's order, for host and device alike (-ffp-contract=off).  Restated by tests/pnp_oracle.py.
// The OpenCV calls are those of csrc/orbfe_svd.h; cvMulTransposed is the ordered sum of oracle P4.
#pragma once
#include <stddef.h>

#include "orbfe_svd.h"

// qr_solve on A (nr x nc row-major, overwritten) and b (overwritten): X is written unless a column is found all zero (P6, P7)
ORBFE_HD inline void epnp_qr_solve(double *pA, double *pb, int nr, int nc, double *pX)
{
    double A1[SVD_MAX], A2[SVD_MAX];
    double *ppAkk = pA;
    for (int k = 0; k < nc; k++) {
        double *ppAik = ppAkk, eta = fabs(*ppAik);
        for (int i = k + 1; i < nr; i++) {
            const double elt = fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) return;
        ppAik = ppAkk;
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) {
            *ppAik *= inv_eta;
            sum += *ppAik * *ppAik;
            ppAik += nc;
        }
        double sigma = sqrt(sum);
        if (*ppAkk < 0) sigma = -sigma;
        *ppAkk += sigma;
        A1[k] = sigma * *ppAkk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            ppAik = ppAkk;
            sum = 0;
            for (int i = k; i < nr; i++) {
                sum += *ppAik * ppAik[j - k];
                ppAik += nc;
            }
            const double tau = sum / A1[k];
            ppAik = ppAkk;
            for (int i = k; i < nr; i++) {
                ppAik[j - k] -= tau * *ppAik;
                ppAik += nc;
            }
        }
        ppAkk += nc + 1;
    }
    double *ppAjj = pA;
    for (int j = 0; j < nc; j++) {
        double *ppAij = ppAjj, tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; i++) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        const double *ppAij = pA + i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; j++) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

ORBFE_HD inline double epnp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

ORBFE_HD inline double epnp_dist2(const double *p1, const double *p2)
{
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// cvSolve(L_6xk, Rho, x, CV_SVD) on the columns `cols` of l_6x10
ORBFE_HD inline void epnp_solve_6xk(const double *l_6x10, const int *cols, int k, const double *rho, double *x)
{
    double At[6 * 5], W[5], Vt[5 * 5];
    for (int i = 0; i < k; i++)
        for (int r = 0; r < 6; r++) At[i * 6 + r] = l_6x10[10 * r + cols[i]];
    jacobi_svd(At, W, Vt, 6, k);
    svbksb_solve(At, W, Vt, 6, k, rho, x);
}

ORBFE_HD inline void epnp_betas_1(const double *l, const double *rho, double *betas)
{
    const int cols[4] = {0, 1, 3, 6};
    double b4[4];
    epnp_solve_6xk(l, cols, 4, rho, b4);
    if (b4[0] < 0) {
        betas[0] = sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0];
        betas[2] = -b4[2] / betas[0];
        betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = sqrt(b4[0]);
        betas[1] = b4[1] / betas[0];
        betas[2] = b4[2] / betas[0];
        betas[3] = b4[3] / betas[0];
    }
}

// find_betas_approx_2 (k = 3) and _3 (k = 5)
ORBFE_HD inline void epnp_betas_23(const double *l, const double *rho, int k, double *betas)
{
    const int cols[5] = {0, 1, 2, 3, 4};
    double b[5];
    epnp_solve_6xk(l, cols, k, rho, b);
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = k == 5 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

ORBFE_HD inline void epnp_gauss_newton(const double *l_6x10, const double *rho, double *betas)
{
    double a[6 * 4], b[6], x[4] = {0, 0, 0, 0};   // x at zeros: the library's decision where the reference reads an uninitialised array (P6)
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double *rowL = l_6x10 + i * 10;
            double *rowA = a + i * 4;
            rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
            rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
            rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
            rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
            b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                             rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                             rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                             rowL[9] * betas[3] * betas[3]);
        }
        epnp_qr_solve(a, b, 6, 4, x);
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// element (row, col) of fill_M's matrix, from the alphas
ORBFE_HD inline double epnp_m_at(const double *alphas, const double *us, const double *K, int row, int col)
{
    const int p = row >> 1, c = col % 3;
    const double as = alphas[4 * p + col / 3];
    if (row & 1) return c == 0 ? 0.0 : c == 1 ? as * K[1] : as * (K[3] - us[2 * p + 1]);
    return c == 0 ? as * K[0] : c == 1 ? 0.0 : as * (K[2] - us[2 * p]);
}

// ---- compute_pose in pieces ---------------------------------------------------------------------------------------------------------
// Each piece is one lane's share when a workgroup runs Refine (one point, or one entry of a sum walked in index order);
// epnp_compute_pose strings the same pieces together serially, so both give the same bits.
// pws [n][3], us [n][2], alphas [n][4], pcs [n][3]; K = (fu, fv, uc, vc).

// 0.0 + a[j] + a[stride + j] + ... over n rows
ORBFE_HD inline double epnp_col_sum(int n, const double *a, int stride, int j)
{
    double s = 0.0;
    for (int i = 0; i < n; i++) s += a[(size_t)stride * i + j];
    return s;
}

// entry (i, j) of PW0^T PW0 (cvMulTransposed, P4); c0 the centroid
ORBFE_HD inline double epnp_pw0_entry(int n, const double *pws, const double *c0, int i, int j)
{
    double s0 = 0;
    for (int k = 0; k < n; k++) s0 += (pws[3 * (size_t)k + i] - c0[i]) * (pws[3 * (size_t)k + j] - c0[j]);
    return s0;
}

// the rest of choose_control_points and the inverse of compute_barycentric_coordinates: cws[0] holds the centroid, s3 PW0^T PW0
ORBFE_HD inline void epnp_control_points(int n, const double *s3, double (*cws)[3], double *ci)
{
    double at3[9], dc[3], vt3[9], cc[9];
    svd_compute(s3, 3, 3, at3, dc, vt3);
    for (int i = 1; i < 4; i++) {
        const double k = sqrt(dc[i - 1] / n);
        for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * at3[3 * (i - 1) + j];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
    svd_compute(cc, 3, 3, at3, dc, vt3);
    svbksb_invert(at3, dc, vt3, 3, ci);
}

ORBFE_HD inline void epnp_alpha_point(const double *pi, const double *c0, const double *ci, double *a)
{
    for (int j = 0; j < 3; j++) a[1 + j] = ci[3 * j] * (pi[0] - c0[0]) + ci[3 * j + 1] * (pi[1] - c0[1]) + ci[3 * j + 2] * (pi[2] - c0[2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// entry (i, j) of M^T M in the order of MulTransposedR: the rows in order from 0.0, no product left out (0 * inf is a NaN)
ORBFE_HD inline double epnp_mtm_entry(int n, const double *alphas, const double *us, const double *K, int i, int j)
{
    double s0 = 0;
    for (int k = 0; k < 2 * n; k++) s0 += epnp_m_at(alphas, us, K, k, i) * epnp_m_at(alphas, us, K, k, j);
    return s0;
}

// mtm holds M^T M, both triangles (symmetric: its own transpose for the SVD); afterwards its rows are ut.  compute_L_6x10, compute_rho
ORBFE_HD inline void epnp_nullspace(double *mtm, double *vtw, const double (*cws)[3], double *l_6x10, double *rho)
{
    double d[12];
    jacobi_svd(mtm, d, vtw, 12, 12);
    const double *ut = mtm;
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
        const double *v = ut + 12 * (11 - i);
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            dv[i][j][0] = v[3 * a] - v[3 * b];
            dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
            dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
            b++;
            if (b > 3) {
                a++;
                b = a + 1;
            }
        }
    }
    for (int i = 0; i < 6; i++) {
        double *row = l_6x10 + 10 * i;
        row[0] = epnp_dot(dv[0][i], dv[0][i]);
        row[1] = 2.0 * epnp_dot(dv[0][i], dv[1][i]);
        row[2] = epnp_dot(dv[1][i], dv[1][i]);
        row[3] = 2.0 * epnp_dot(dv[0][i], dv[2][i]);
        row[4] = 2.0 * epnp_dot(dv[1][i], dv[2][i]);
        row[5] = epnp_dot(dv[2][i], dv[2][i]);
        row[6] = 2.0 * epnp_dot(dv[0][i], dv[3][i]);
        row[7] = 2.0 * epnp_dot(dv[1][i], dv[3][i]);
        row[8] = 2.0 * epnp_dot(dv[2][i], dv[3][i]);
        row[9] = epnp_dot(dv[3][i], dv[3][i]);
    }
    rho[0] = epnp_dist2(cws[0], cws[1]);
    rho[1] = epnp_dist2(cws[0], cws[2]);
    rho[2] = epnp_dist2(cws[0], cws[3]);
    rho[3] = epnp_dist2(cws[1], cws[2]);
    rho[4] = epnp_dist2(cws[1], cws[3]);
    rho[5] = epnp_dist2(cws[2], cws[3]);
}

// find_betas_approx_k, gauss_newton, compute_ccs
ORBFE_HD inline void epnp_betas_ccs(int k, const double *l_6x10, const double *rho, const double *ut, double (*ccs)[3])
{
    double betas[4];
    if (k == 1)
        epnp_betas_1(l_6x10, rho, betas);
    else
        epnp_betas_23(l_6x10, rho, k == 2 ? 3 : 5, betas);
    epnp_gauss_newton(l_6x10, rho, betas);
    for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0;
    for (int i = 0; i < 4; i++) {
        const double *v = ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
            for (int c = 0; c < 3; c++) ccs[j][c] += betas[i] * v[3 * j + c];
    }
}

ORBFE_HD inline void epnp_pc_point(const double *a, const double (*ccs)[3], double *pc)
{
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
}

// entry (j, c) of estimate_R_and_t's ABt
ORBFE_HD inline double epnp_abt_entry(int n, const double *pcs, const double *pws, const double *pc0, const double *pw0, int j, int c)
{
    double s = 0;
    for (int i = 0; i < n; i++) s += (pcs[3 * (size_t)i + j] - pc0[j]) * (pws[3 * (size_t)i + c] - pw0[c]);
    return s;
}

// the rest of estimate_R_and_t: the full 3x3 SVD, U * V^T by rows, the determinant fix on row 2, t
ORBFE_HD inline void epnp_R_t_from_abt(const double *abt, const double *pc0, const double *pw0, double *R, double *t)
{
    double at[9], w[3], vt[9];
    svd_compute(abt, 3, 3, at, w, vt);
    // U[i][k] = at[k][i], V[j][k] = vt[k][j] (P2)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = at[i] * vt[j] + at[3 + i] * vt[3 + j] + at[6 + i] * vt[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                       R[0] * R[5] * R[7];
    if (det < 0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
    t[0] = pc0[0] - epnp_dot(R, pw0);
    t[1] = pc0[1] - epnp_dot(R + 3, pw0);
    t[2] = pc0[2] - epnp_dot(R + 6, pw0);
}

// one point's term of reprojection_error
ORBFE_HD inline double epnp_reproj_term(const double *pw, double u, double v, const double *K, const double *R, const double *t)
{
    const double Xc = epnp_dot(R, pw) + t[0];
    const double Yc = epnp_dot(R + 3, pw) + t[1];
    const double inv_Zc = 1.0 / (epnp_dot(R + 6, pw) + t[2]);
    const double ue = K[2] + K[0] * Xc * inv_Zc;
    const double ve = K[3] + K[1] * Yc * inv_Zc;
    return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// the rep_errors choice with plain <: a NaN never wins
ORBFE_HD inline int epnp_choose(const double *rep_errors /* [1 .. 3] */)
{
    int N = 1;
    if (rep_errors[2] < rep_errors[1]) N = 2;
    if (rep_errors[3] < rep_errors[N]) N = 3;
    return N;
}

// compute_pose on n correspondences; mtm [144], vtw [144] are workspace.  -> rep_errors[N]; R row-major, t, the chosen N of 1 .. 3,
// the three errors
ORBFE_HD inline double epnp_compute_pose(int n, const double *pws, const double *us, double *alphas, double *pcs, const double *K,
                                         double *mtm, double *vtw, double *R, double *t, int *N_out, double *rep)
{
    double cws[4][3], s3[9], ci[9];
    for (int j = 0; j < 3; j++) cws[0][j] = epnp_col_sum(n, pws, 3, j) / n;
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) s3[3 * i + j] = s3[3 * j + i] = epnp_pw0_entry(n, pws, cws[0], i, j);
    epnp_control_points(n, s3, cws, ci);
    for (int i = 0; i < n; i++) epnp_alpha_point(pws + 3 * (size_t)i, cws[0], ci, alphas + 4 * (size_t)i);
    for (int i = 0; i < 12; i++)
        for (int j = i; j < 12; j++) mtm[12 * i + j] = mtm[12 * j + i] = epnp_mtm_entry(n, alphas, us, K, i, j);
    double l_6x10[60], rho[6];
    epnp_nullspace(mtm, vtw, cws, l_6x10, rho);
    double Rs[4][9], ts[4][3], rep_errors[4];
    for (int k = 1; k <= 3; k++) {
        double ccs[4][3], pc0[3], pw0[3], abt[9];
        epnp_betas_ccs(k, l_6x10, rho, mtm, ccs);
        for (int i = 0; i < n; i++) epnp_pc_point(alphas + 4 * (size_t)i, ccs, pcs + 3 * (size_t)i);
        if (pcs[2] < 0.0)   // solve_for_sign reads the first point only
            for (size_t i = 0; i < 3 * (size_t)n; i++) pcs[i] = -pcs[i];
        for (int j = 0; j < 3; j++) {
            pc0[j] = epnp_col_sum(n, pcs, 3, j) / n;
            pw0[j] = epnp_col_sum(n, pws, 3, j) / n;
        }
        for (int e = 0; e < 9; e++) abt[e] = epnp_abt_entry(n, pcs, pws, pc0, pw0, e / 3, e % 3);
        epnp_R_t_from_abt(abt, pc0, pw0, Rs[k], ts[k]);
        double sum2 = 0.0;
        for (int i = 0; i < n; i++) sum2 += epnp_reproj_term(pws + 3 * (size_t)i, us[2 * (size_t)i], us[2 * (size_t)i + 1], K, Rs[k], ts[k]);
        rep_errors[k] = sum2 / n;
    }
    const int N = epnp_choose(rep_errors);
    for (int e = 0; e < 9; e++) R[e] = Rs[N][e];
    for (int e = 0; e < 3; e++) t[e] = ts[N][e];
    *N_out = N;
    for (int k = 0; k < 3; k++) rep[k] = rep_errors[k + 1];
    return rep_errors[N];
}

// ---- known-answer entry points (orbfe_pnp_kat): item i of a batch, doubles in and out ----------------------------------------------
enum {
    EPNP_KAT_SVD3 = 0, EPNP_KAT_SVD12 = 1, EPNP_KAT_SVD6X3 = 2, EPNP_KAT_SVD6X4 = 3, EPNP_KAT_SVD6X5 = 4, EPNP_KAT_SOLVE6X3 = 5,
    EPNP_KAT_SOLVE6X4 = 6, EPNP_KAT_SOLVE6X5 = 7, EPNP_KAT_INVERT3 = 8, EPNP_KAT_QR_SOLVE = 9, EPNP_KAT_COMPUTE_POSE = 10
};

ORBFE_HD inline void epnp_kat_shape(int what, int *m, int *n)
{
    *m = what == EPNP_KAT_SVD3 || what == EPNP_KAT_INVERT3 ? 3 : what == EPNP_KAT_SVD12 ? 12 : 6;
    *n = what == EPNP_KAT_SVD3 || what == EPNP_KAT_INVERT3 ? 3 : what == EPNP_KAT_SVD12 ? 12 :
         what == EPNP_KAT_SVD6X3 || what == EPNP_KAT_SOLVE6X3 ? 3 : what == EPNP_KAT_SVD6X5 || what == EPNP_KAT_SOLVE6X5 ? 5 : 4;
}

// doubles per item: in / out
ORBFE_HD inline void epnp_kat_sizes(int what, int *in_d, int *out_d)
{
    int m, n;
    epnp_kat_shape(what, &m, &n);
    if (what <= EPNP_KAT_SVD6X5) {
        *in_d = m * n;
        *out_d = n + n * m + n * n;
    } else if (what <= EPNP_KAT_SOLVE6X5 || what == EPNP_KAT_QR_SOLVE) {
        *in_d = m * n + m;
        *out_d = n;
    } else {
        *in_d = 9;
        *out_d = 9;
    }
}

// `ws` holds 300 doubles of workspace for the item
ORBFE_HD inline void epnp_kat_item(int what, const double *in, double *out, double *ws)
{
    int m, n;
    epnp_kat_shape(what, &m, &n);
    double *At = ws, *Vt = ws + 144, *W = ws + 288;
    if (what == EPNP_KAT_QR_SOLVE) {
        double x[4] = {0, 0, 0, 0};
        for (int e = 0; e < 24; e++) At[e] = in[e];
        for (int e = 0; e < 6; e++) Vt[e] = in[24 + e];
        epnp_qr_solve(At, Vt, 6, 4, x);
        for (int e = 0; e < 4; e++) out[e] = x[e];
        return;
    }
    svd_compute(in, m, n, At, W, Vt);
    if (what <= EPNP_KAT_SVD6X5) {
        for (int e = 0; e < n; e++) out[e] = W[e];
        for (int e = 0; e < n * m; e++) out[n + e] = At[e];
        for (int e = 0; e < n * n; e++) out[n + n * m + e] = Vt[e];
    } else if (what == EPNP_KAT_INVERT3) {
        svbksb_invert(At, W, Vt, 3, out);
    } else {
        svbksb_solve(At, W, Vt, m, n, in + m * n, out);
    }
}
